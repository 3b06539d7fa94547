"""csrc/pairing_consts.hip.h against tools/pairing_constants.py and against constants recomputed here with Python integers:
the Frobenius coefficients xi^(k (q^j - 1)/6), the hard part of the final exponent, the loop counts, the twist constants."""
import pathlib, re, sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import pairing_constants as pc  # noqa: E402

HDR = ROOT / "eigen-zkvm_amd" / "csrc" / "pairing_consts.hip.h"


def _sections():
    text = HDR.read_text()
    return {C.ns: text.split("namespace %s {" % C.ns)[1].split("}  // namespace %s" % C.ns)[0] for C in pc.CURVES}


def _array(sec, name):
    body = re.search(r"%s(?:\[\d+\])+ = \{(.*?)\};" % name, sec, re.S).group(1)
    return [int(x, 16) for x in re.findall(r"0x([0-9a-f]+)u", body)]


def _scalar(sec, name):
    return int(re.search(r"%s = (0x[0-9a-f]+|\d+)" % name, sec).group(1), 0)


def _unmont(C, limbs):
    v = sum(x << (29 * i) for i, x in enumerate(limbs))
    assert all(x < 1 << 29 for x in limbs)
    return v * pow(1 << (29 * C.nr), -1, C.q) % C.q


def _f2mul(q, a, b): return ((a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q)


def _f2pow(q, a, e):
    r = (1, 0)
    while e:
        if e & 1: r = _f2mul(q, r, a)
        a = _f2mul(q, a, a); e >>= 1
    return r


def test_header_is_what_the_tool_emits():
    assert HDR.read_text() == pc.render()


def test_constants_recomputed():
    secs = _sections()
    for C in pc.CURVES:
        s, q, r = secs[C.ns], C.q, C.r
        t = 4965661367192848881 if C.bn else 0xd201000000010000
        loop = _scalar(s, "PAIR_LOOP_LO") | (_scalar(s, "PAIR_LOOP_HI") << 64)
        assert loop == (6 * t + 2 if C.bn else t) and _scalar(s, "PAIR_LOOP_BITS") == loop.bit_length()
        if C.bn:                                            # the BN family: q and r as polynomials in t
            assert q == 36 * t**4 + 36 * t**3 + 24 * t**2 + 6 * t + 1 and r == 36 * t**4 + 36 * t**3 + 18 * t**2 + 6 * t + 1
        else:                                               # BLS12: r = x^4 - x^2 + 1, q = (x - 1)^2 r / 3 + x with x = -t
            x = -t
            assert r == x**4 - x**2 + 1 and q == (x - 1)**2 * r // 3 + x
        assert sum(w << (32 * i) for i, w in enumerate(_array(s, "PAIR_R"))) == r
        xi = (_scalar(s, "PAIR_XI0"), 1)
        for j in (1, 2, 3):
            g = _array(s, "PAIR_GAMMA%d" % j)
            assert len(g) == 12 * C.nr
            vals = [(_unmont(C, g[2 * k * C.nr:(2 * k + 1) * C.nr]), _unmont(C, g[(2 * k + 1) * C.nr:(2 * k + 2) * C.nr])) for k in range(6)]
            for k in range(6):
                assert vals[k] == _f2pow(q, xi, k * (q**j - 1) // 6), (C.name, j, k)
            # gamma_j[1]^6 = xi^(q^j - 1) = xi^(q^j) / xi
            assert _f2mul(q, _f2pow(q, vals[1], 6), xi) == _f2pow(q, xi, q**j)
        nd = _scalar(s, "PAIR_HARD_DIGITS")
        wds = _array(s, "PAIR_HARD")
        digits = [(wds[e >> 3] >> (4 * (e & 7))) & 15 for e in range(nd)]
        e = 0
        for d in digits: e = e * 16 + d
        assert digits[0] != 0 and e * r == q**4 - q**2 + 1
        assert (q**12 - 1) // r == (q**6 - 1) * (q**2 + 1) * e
        bt = _array(s, "PAIR_TWIST_B")
        bt = (_unmont(C, bt[:C.nr]), _unmont(C, bt[C.nr:]))
        b = _unmont(C, _array(s, "PAIR_G1_B"))
        assert b == C.b and (C.g1[1]**2 - C.g1[0]**3 - b) % q == 0
        assert (_f2mul(q, bt, xi) == (b, 0)) if C.dtype else (bt == _f2mul(q, (b, 0), xi))
        assert ("PAIR_DTYPE = true" in s) == C.dtype and ("PAIR_BN = true" in s) == C.bn


def test_model_pairing_is_bilinear_on_bn254():
    C = pc.BN254; M = pc.Model(C)
    e = M.pairing(C.g1, C.g2)
    assert e != M.one() and M.pairing(C.g1_mul(5, C.g1), C.g2_mul(7, C.g2)) == M.pow(e, 35)
