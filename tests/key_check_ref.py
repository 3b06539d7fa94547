"""TEST INFRASTRUCTURE ONLY.  A plain-Python check of a Groth16 proving key that gives the report of zk_groth16_key_check
(include/zkgpu.h, "groth16_key_check"), written from bellman's Parameters layout (groth16/src/api.rs:545-550, pairing_ce's
uncompressed points) and the curves' published parameters.  Curve arithmetic on Python integers -- Fq2 = Fq[u]/(u^2 + 1) as pairs,
G1 embedded as c1 = 0 --, membership by the definition ([r]P = O, never an endomorphism), section lengths from the .r1cs, and the
G1 / G2 pairs tied by the oracle's pairing (oracle/pairing.py, pinned by tests/test_oracle_pairing.py) one element at a time.
Serial and slow; nothing here touches the GPU or the product."""
import json
import pathlib
import struct
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
import pairing as PG  # noqa: E402

CLASSES = ("infinity", "coordinate_range", "not_on_curve", "not_in_subgroup")
G1_SECTIONS = ("ic", "h", "l", "a", "b_g1")
VK_POINTS = (("alpha_g1", 0), ("beta_g1", 0), ("beta_g2", 1), ("gamma_g2", 1), ("delta_g1", 0), ("delta_g2", 1))


class Curve:
    def __init__(self, name, pg, x, b, twist_b, g1, g2, h1, h2):
        self.name, self.pg, self.q, self.r, self.x = name, pg, pg.Q, pg.R, x
        self.b = ((b, 0), twist_b)                                        # by group
        self.gen = (((g1[0], 0), (g1[1], 0)), ((g2[0], g2[1]), (g2[2], g2[3])))
        self.cofactor = (h1, h2)
        self.coord_bytes = (self.q.bit_length() + 63) // 64 * 8
        self._seen, self._pairs = {}, {}

    # ---- Fq2 ----
    def fadd(self, a, b): return ((a[0] + b[0]) % self.q, (a[1] + b[1]) % self.q)
    def fsub(self, a, b): return ((a[0] - b[0]) % self.q, (a[1] - b[1]) % self.q)
    def fmul(self, a, b): return ((a[0] * b[0] - a[1] * b[1]) % self.q, (a[0] * b[1] + a[1] * b[0]) % self.q)
    def finv(self, a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, self.q)
        return (a[0] * n % self.q, -a[1] * n % self.q)
    def fpow(self, a, e):
        r = (1, 0)
        while e:
            if e & 1: r = self.fmul(r, a)
            a = self.fmul(a, a); e >>= 1
        return r
    def fsqrt(self, a):
        """a square root in Fq2 (q = 3 mod 4: Adj-Rodriguez-Henriquez, algorithm 9), or None"""
        q = self.q
        if a == (0, 0): return a
        a1 = self.fpow(a, (q - 3) // 4)
        al = self.fmul(self.fmul(a1, a1), a)
        a0 = self.fmul((al[0], -al[1] % q), al)                           # alpha^(q + 1)
        if a0 == (q - 1, 0): return None
        x0 = self.fmul(a1, a)
        if al == (q - 1, 0): return self.fmul((0, 1), x0)
        return self.fmul(self.fpow(self.fadd((1, 0), al), (q - 1) // 2), x0)

    # ---- points: None = infinity, else (x, y) over Fq2 ----
    def on_curve(self, p, g): return self.fmul(p[1], p[1]) == self.fadd(self.fmul(self.fmul(p[0], p[0]), p[0]), self.b[g])
    def neg(self, p): return None if p is None else (p[0], self.fsub((0, 0), p[1]))
    def add(self, p, s):
        if p is None: return s
        if s is None: return p
        if p[0] == s[0]:
            if self.fadd(p[1], s[1]) == (0, 0): return None
            xx = self.fmul(p[0], p[0])
            m = self.fmul(self.fadd(self.fadd(xx, xx), xx), self.finv(self.fadd(p[1], p[1])))
        else:
            m = self.fmul(self.fsub(s[1], p[1]), self.finv(self.fsub(s[0], p[0])))
        x3 = self.fsub(self.fsub(self.fmul(m, m), p[0]), s[0])
        return (x3, self.fsub(self.fmul(m, self.fsub(p[0], x3)), p[1]))
    def mul(self, p, k):
        if k < 0: p, k = self.neg(p), -k
        acc = None
        while k:
            if k & 1: acc = self.add(acc, p)
            p = self.add(p, p); k >>= 1
        return acc
    def lift_x(self, x, g):
        """a curve point of the group's curve with this x (an Fq2 pair; c1 = 0 for G1), or None"""
        y = self.fsqrt(self.fadd(self.fmul(self.fmul(x, x), x), self.b[g]))
        if y is None or (g == 0 and y[1] != 0): return None
        return (x, y)
    def order(self, g): return self.r * self.cofactor[g]

    # ---- coordinates as a key file and the device hold them ----
    def coords(self, p, g):
        """point -> the integer coordinates (G1: x, y; G2: x.c0, x.c1, y.c0, y.c1); infinity = all zero"""
        if p is None: return (0,) * (4 if g else 2)
        return (p[0][0], p[0][1], p[1][0], p[1][1]) if g else (p[0][0], p[1][0])
    def classify(self, c, g):
        """integer coordinates -> the first class that applies, or None (remembered: a key is classified once, a damaged copy costs its
        damaged points)"""
        key = (g, tuple(c))
        if key not in self._seen: self._seen[key] = self._classify(c, g)
        return self._seen[key]
    def _classify(self, c, g):
        if not any(c): return "infinity"
        if any(v >= self.q for v in c): return "coordinate_range"
        p = ((c[0], c[1]), (c[2], c[3])) if g else ((c[0], 0), (c[1], 0))
        if not self.on_curve(p, g): return "not_on_curve"
        if self.mul(p, self.r) is not None: return "not_in_subgroup"
        return None
    def pair_ok(self, c1, c2):
        """e(P1, G2) = e(G1, P2) for finite points given by their coordinates: e(P1, G2) e(-G1, P2) = 1 with the oracle's Miller loop
        and final exponent (remembered, seconds each)"""
        key = (tuple(c1), tuple(c2))
        if key not in self._pairs:
            pg, F = self.pg, self.pg.F12
            g1, g2 = self.coords(self.neg(self.gen[0]), 0), self.coords(self.gen[1], 1)
            f = pg.miller_loop(pg.twist(g2), (F([c1[0]]), F([c1[1]]))) * pg.miller_loop(pg.twist(tuple(c2)), (F([g1[0]]), F([g1[1]])))
            self._pairs[key] = f ** pg.final_exp == F.one()
        return self._pairs[key]


_X_BLS = -0xd201000000010000
_X_BN = 4965661367192848881
_Q_BN = PG.BN254.Q
BN128 = Curve("BN128", PG.BN254, _X_BN, 3,
              # 3 / (9 + u)
              (19485874751759354771024239261021720505790618469301721065564631296452457478373, 266929791119991161246907387137283842545076965332900288569378510910307636690),
              (1, 2),
              (10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634,
               8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531),
              1, 2 * _Q_BN - PG.BN254.R)
_Q_BLS = PG.BLS12_381.Q
BLS12381 = Curve("BLS12381", PG.BLS12_381, _X_BLS, 4, (4, 4),
                 (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
                  0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1),
                 (0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
                  0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e,
                  0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
                  0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be),
                 (_X_BLS - 1) ** 2 // 3,
                 (_X_BLS ** 8 - 4 * _X_BLS ** 7 + 5 * _X_BLS ** 6 - 4 * _X_BLS ** 4 + 6 * _X_BLS ** 3 - 4 * _X_BLS ** 2 - 4 * _X_BLS + 13) // 9)
CURVES = {"BN128": BN128, "BLS12381": BLS12381}


# ---- the key file -------------------------------------------------------------------------------------------------------------
def parse_key(cv, b):
    """bellman's Parameters::read layout -> {"vk": {name: coords}, section: [coords]}; the texts of g16::parse_params on a file
    that cannot be read"""
    cb, o = cv.coord_bytes, 0

    def point(g):
        nonlocal o
        n = (4 if g else 2) * cb
        if n > len(b) - o: raise ValueError("proving key: truncated file")
        p = b[o:o + n]; o += n
        if p[0] & 0x80: raise ValueError("proving key: compressed point where an uncompressed one is expected")
        if p[0] & 0x40: return (0,) * (4 if g else 2)
        v = [int.from_bytes(p[i * cb:(i + 1) * cb], "big") for i in range(4 if g else 2)]
        return (v[1], v[0], v[3], v[2]) if g else tuple(v)

    def section(g):
        nonlocal o
        if 4 > len(b) - o: raise ValueError("proving key: truncated file")
        n = struct.unpack(">I", b[o:o + 4])[0]; o += 4
        return [point(g) for _ in range(n)]                                # point by point, as the library reads: the first fault is the one reported
    key = {"vk": {name: point(g) for name, g in VK_POINTS}}
    for name in ("ic", "h", "l", "a", "b_g1"): key[name] = section(0)
    key["b_g2"] = section(1)
    if o != len(b): raise ValueError("proving key: trailing bytes")
    return key


def wanted_sizes(r1cs):
    """the section lengths the circuit of an .r1cs dict (oracle/groth16.read_r1cs) fixes"""
    ni = 1 + r1cs["n_pub_out"] + r1cs["n_pub_in"]
    rows = [(a, b, c) for a, b, c in r1cs["constraints"] if not ((len(a) == 0 or len(b) == 0) and len(c) == 0)]
    log_m = 0
    while (1 << log_m) < len(rows) + ni: log_m += 1
    a_aux = {j for a, _b, _c in rows for j, _ in a if j >= ni}
    b_any = {j for _a, b, _c in rows for j, _ in b}
    nb = len(b_any)
    return dict(ni=ni, log_m=log_m, want={"ic": ni, "h": (1 << log_m) - 1, "l": r1cs["n_wires"] - ni, "a": ni + len(a_aux), "b_g1": nb, "b_g2": nb})


def _vk_fields(vk_json):
    v = json.loads(vk_json) if isinstance(vk_json, str) else vk_json
    i = lambda s: int(s, 0)
    g1 = lambda p: (i(p["x"]), i(p["y"]))
    g2 = lambda p: (i(p["x"][0]), i(p["x"][1]), i(p["y"][0]), i(p["y"][1]))
    out = [("vk_alpha_1", g1(v["vk_alpha_1"]))]
    if "vk_beta_1" in v: out.append(("vk_beta_1", g1(v["vk_beta_1"])))
    out += [("vk_beta_2", g2(v["vk_beta_2"])), ("vk_gamma_2", g2(v["vk_gamma_2"]))]
    if "vk_delta_1" in v: out.append(("vk_delta_1", g1(v["vk_delta_1"])))
    out += [("vk_delta_2", g2(v["vk_delta_2"])), ("IC", [g1(p) for p in v["IC"]])]
    return out


def _json_zero(c):
    """pairing_ce's zero (0, 1) of a JSON file is the all-zero encoding of a key file"""
    half = len(c) // 2
    return tuple(0 for _ in c) if c[half] == 1 and not any(v for k, v in enumerate(c) if k != half) else tuple(c)


def report(curve, r1cs_bytes, params_bytes, vk_json=None, max_findings=16, b_indices=None, classify_sections=None):
    """The report of groth16_key_check as a dict.  b_indices: the elements of the b sections whose G1 / G2 pair is compared with the
    pairing (None: all of them -- seconds each).  classify_sections: the sections whose points are classified (None: all; a key of
    thousands of points takes minutes here, so a test of the sums names the few sections it touched and the rest count as valid)."""
    cv = CURVES[curve]
    prime, r1cs = G.read_r1cs(r1cs_bytes)
    if prime != cv.r: raise ValueError("r1cs: the file's prime is not the scalar field of the selected curve")
    key = parse_key(cv, params_bytes)
    w = wanted_sizes(r1cs)
    sections = {s: len(key[s]) for s in G1_SECTIONS + ("b_g2",)}
    found = {k: [] for k in ("size",) + CLASSES + ("g1_g2_mismatch", "vk_mismatch")}
    for s in G1_SECTIONS + ("b_g2",):
        if sections[s] != w["want"][s]: found["size"].append(dict(kind="size", section=s, have=sections[s], want=w["want"][s]))
    bad = {}                                                              # section -> {class: [indices]}
    todo = [(name, g, [key["vk"][name]]) for name, g in VK_POINTS] + [(s, 0, key[s]) for s in G1_SECTIONS] + [("b_g2", 1, key["b_g2"])]
    for name, g, pts in todo:
        per = {}
        for i, c in enumerate(pts if classify_sections is None or name in classify_sections else []):
            k = cv.classify(c, g)
            if k: per.setdefault(k, []).append(i)
        bad[name] = per
        for k in CLASSES:
            if k in per: found[k].append(dict(kind=k, section=name, n_points=len(per[k]), first_index=per[k][0]))
    skipped, pairs = [], 0
    for what, n1, n2 in (("beta", "beta_g1", "beta_g2"), ("delta", "delta_g1", "delta_g2")):
        if bad[n1] or bad[n2]:
            skipped.append(dict(check="g1_g2_mismatch", section=what, reason="an invalid point")); continue
        pairs += 1
        if not cv.pair_ok(key["vk"][n1], key["vk"][n2]): found["g1_g2_mismatch"].append(dict(kind="g1_g2_mismatch", section=what, first_index=0))
    if sections["b_g1"] != sections["b_g2"]:
        skipped.append(dict(check="g1_g2_mismatch", section="b", reason="b_g1 and b_g2 differ in length"))
    elif bad["b_g1"] or bad["b_g2"]:
        skipped.append(dict(check="g1_g2_mismatch", section="b", reason="an invalid point"))
    else:
        pairs += sections["b_g1"]
        for i in (range(sections["b_g1"]) if b_indices is None else sorted(b_indices)):
            if not cv.pair_ok(key["b_g1"][i], key["b_g2"][i]):
                found["g1_g2_mismatch"].append(dict(kind="g1_g2_mismatch", section="b", first_index=i)); break
    if vk_json is not None:
        own = dict(vk_alpha_1=key["vk"]["alpha_g1"], vk_beta_1=key["vk"]["beta_g1"], vk_beta_2=key["vk"]["beta_g2"], vk_gamma_2=key["vk"]["gamma_g2"],
                   vk_delta_1=key["vk"]["delta_g1"], vk_delta_2=key["vk"]["delta_g2"])
        for name, val in _vk_fields(vk_json):
            if name == "IC":
                if len(val) != len(key["ic"]): found["vk_mismatch"].append(dict(kind="vk_mismatch", field="IC")); continue
                for i, (a, b) in enumerate(zip(val, key["ic"])):
                    if _json_zero(a) != tuple(b): found["vk_mismatch"].append(dict(kind="vk_mismatch", field="IC[%d]" % i))
            elif _json_zero(val) != tuple(own[name]): found["vk_mismatch"].append(dict(kind="vk_mismatch", field=name))
    n1 = 3 + sum(sections[s] for s in G1_SECTIONS)
    return dict(curve=curve, n_wires=r1cs["n_wires"], n_public=w["ni"] - 1, domain_log=w["log_m"], sections=sections,
                checked=dict(g1_points=n1, g2_points=3 + sections["b_g2"], pairs=pairs), skipped=skipped,
                counts={k: len(v) for k, v in found.items()},
                findings=[f for k in found for f in found[k][:max_findings]])


def finding_line(f):
    """the line tools/zkgpu_prove.py groth16_key_check prints for one finding"""
    k = f["kind"]
    if k == "size": return "size: section %s has %d points, the circuit needs %d (the key of another circuit?)" % (f["section"], f["have"], f["want"])
    if k in CLASSES: return "%s: section %s: %d point%s, first at index %d" % (k, f["section"], f["n_points"], "" if f["n_points"] == 1 else "s", f["first_index"])
    if k == "g1_g2_mismatch": return "g1_g2_mismatch: %s: the G1 and G2 halves differ, first at index %d" % (f["section"], f["first_index"])
    return "vk_mismatch: %s differs from the key's embedded copy" % f["field"]


def skipped_line(s):
    """the line the tool prints for one entry of "skipped" """
    return "skipped: %s of %s: %s" % (s["check"], s["section"], s["reason"])
