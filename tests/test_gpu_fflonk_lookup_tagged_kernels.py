"""The kernel of the fflonk prover with tagged lookups (csrc/fflonk_lookup_tagged_impl.hip.h) word for word against Python
integers, in the form of test_gpu_fflonk_lookup_kernels.py: the four numerators from ONE launch at log_n = 3 (32 coset points: half a wave,
the (i + 4) mod m wrap inside it) and log_n = 7 (512 points: two workgroups), every operand word at 2^256 - 1 with every scalar at r - 1,
k_1, k_2 = 2, 3 (additions) and 5, 7 (products: both paths of pk_times_k), q_K and Tg up to 65535, both fields; with Tg = 0 and q_K in
{0, 1} the same words as zk_fflonk_<curve>_lookup_quotients_dev on the 21 shared columns (output 3 where q_K = 0: eta^3 q_K enters f where
q_K = 1); output 3 against zk_plonk_<curve>_lookup_tagged_quotient_dev with alpha = 1 on a zero accumulator; every pattern of outputs left
out; the refusals.  An input element is the 256-bit integer its words are (any value below 2^256, not only below r) and stands for
words / 2^256 mod r; every output word vector must be the canonical Montgomery representative.  Exact: no tolerance anywhere."""
import importlib, itertools, random

import numpy as np
import pytest

import plonk_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")
SHARED = ("a", "b", "c", "Z", "qL", "qR", "qO", "qM", "qC", "S1", "S2", "S3", "PI", "L1", "X", "qK", "T1", "T2", "T3", "M", "Phi")
NAMES = SHARED + ("Tg",)
TAGGED_NAMES = ("a", "b", "c", "qK", "T1", "T2", "T3", "Tg", "M", "Phi")                   # the order of zk_plonk_<curve>_lookup_tagged_quotient_dev


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def flt(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk_lookup_tagged")


def _dev(zk, words):
    """integers below 2^256, taken as the words themselves"""
    a = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in words), dtype="<u8").astype(np.uint64)
    return zk.DevArray.from_host(a)


def _host(d, n):
    b = d.to_host()[:4 * n].astype("<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _want(r, cols, m, beta, gamma, k1, k2, eta, delta):
    """the four numerators at every index from the columns' words, as Montgomery words"""
    rinv = pow(1 << 256, -1, r)
    v = {k: [w * rinv % r for w in cols[k]] for k in NAMES}
    out = [[], [], [], []]
    for i in range(m):
        a, b, c, z, x = v["a"][i], v["b"][i], v["c"][i], v["Z"][i], v["X"][i]
        zw, phiw = v["Z"][(i + 4) % m], v["Phi"][(i + 4) % m]
        gate = a * b * v["qM"][i] + a * v["qL"][i] + b * v["qR"][i] + c * v["qO"][i] + v["qC"][i] + v["PI"][i]
        p1 = (a + beta * x + gamma) * (b + beta * k1 * x + gamma) * (c + beta * k2 * x + gamma) * z
        p2 = (a + beta * v["S1"][i] + gamma) * (b + beta * v["S2"][i] + gamma) * (c + beta * v["S3"][i] + gamma) * zw
        f = delta + a + eta * b + eta * eta * c + eta ** 3 * v["qK"][i]
        t = delta + v["T1"][i] + eta * v["T2"][i] + eta * eta * v["T3"][i] + eta ** 3 * v["Tg"][i]
        look = (phiw - v["Phi"][i]) * f * t - v["qK"][i] * t + v["M"][i] * f
        for j, val in enumerate((gate, v["L1"][i] * (z - 1), p1 - p2, look)):
            out[j].append((val % r << 256) % r)
    return out


def _take(outs, m):
    try:
        return [None if o is None else _host(o, m) for o in outs]
    finally:
        for o in outs:
            if o is not None:
                o.free()


def _run(zk, flt, cv, log_n, cols, sc, want=(True, True, True, True)):
    ds = [_dev(zk, cols[k]) for k in NAMES]
    try:
        return _take(flt.quotients(ds, log_n, *sc, cv, want=want), 4 << log_n)
    finally:
        for d in ds:
            d.free()


def _cases(r, m, rng):
    mont = lambda v: (v << 256) % r
    rand = lambda: {k: [mont(rng.randrange(r)) for _ in range(m)] for k in NAMES}
    const = lambda w: {k: [w] * m for k in NAMES}
    wide = {k: [rng.randrange(r, 1 << 256) for _ in range(m)] for k in NAMES}             # words >= r but < 2^256
    for k in NAMES:
        wide[k][0], wide[k][1], wide[k][m - 1] = (1 << 256) - 1, r, (1 << 256) - 1
    wrap = const(mont(1))                                              # Z and Phi alone distinct: indices 4n - 4 .. 4n - 1 read them at 0 .. 3
    wrap["Z"] = [mont(i + 2) for i in range(m)]
    wrap["Phi"] = [mont(3 * i + 5) for i in range(m)]
    tags = rand()                                                      # q_K and Tg as the protocol has them on H: integers 0 .. 65535, the ends included
    tags["qK"] = [mont(v) for v in [0, 1, 65535, 65534] + [rng.randrange(65536) for _ in range(m - 4)]]
    tags["Tg"] = [mont(v) for v in [65535, 1, 65535, 2] + [rng.randrange(1, 65536) for _ in range(m - 4)]]
    sc = lambda k1, k2: [rng.randrange(r), rng.randrange(r), k1, k2, rng.randrange(r), rng.randrange(r)]
    top = lambda k1, k2: [r - 1, r - 1, k1, k2, r - 1, r - 1]
    return [("random, k = 2, 3", rand(), sc(2, 3)),
            ("random, k = 5, 7", rand(), sc(5, 7)),
            ("random, k = 3, r - 1", rand(), sc(3, r - 1)),
            ("all zero", const(0), sc(2, 3)),
            ("all r - 1, every scalar r - 1", const(mont(r - 1)), top(r - 1, r - 1)),
            ("every word 2^256 - 1, every scalar r - 1, k = 2, 3", const((1 << 256) - 1), top(2, 3)),
            ("every word 2^256 - 1, every scalar r - 1, k = 5, 7", const((1 << 256) - 1), top(5, 7)),
            ("words >= r, k = 2, 3", wide, sc(2, 3)),
            ("words >= r, k = 5, 7, scalars r - 1", wide, top(5, 7)),
            ("the wrap of Z(wX) and Phi(wX)", wrap, sc(2, 3)),
            ("every scalar 0", rand(), [0, 0, 2, 3, 0, 0]),
            ("q_K and Tg up to 65535, k = 2, 3", tags, sc(2, 3)),
            ("q_K and Tg up to 65535, every scalar r - 1, k = 5, 7", tags, top(5, 7))]


@pytest.mark.parametrize("log_n", (3, 7))
@pytest.mark.parametrize("cv", CURVES)
def test_the_four_numerators_word_for_word(zk, flt, cv, log_n):
    r, m, rng = ref.R[cv], 4 << log_n, random.Random(0x27 + log_n + len(cv))
    if log_n == 7:
        assert m > 256                                                                     # more than one workgroup of 256 lanes
    for name, cols, sc in _cases(r, m, rng):
        got = _run(zk, flt, cv, log_n, cols, sc)
        want = _want(r, cols, m, *sc)
        for j in range(4):
            assert all(w < r for w in got[j]), (name, j)                                   # canonical
            assert got[j][m - 4:] == want[j][m - 4:], (name, j)                            # the wrap
            assert got[j] == want[j], (name, j)


@pytest.mark.parametrize("log_n", (3, 7))
@pytest.mark.parametrize("cv", CURVES)
def test_without_tags_it_is_the_single_table_kernel(zk, flt, cv, log_n):
    """Tg = 0 and q_K in {0, 1}: outputs 0 .. 2 are zk_fflonk_<curve>_lookup_quotients_dev's for any inputs, output 3 where q_K = 0"""
    fl = importlib.import_module("eigen_zkvm_amd.fflonk_lookup")
    r, m, rng = ref.R[cv], 4 << log_n, random.Random(0x28 + log_n + len(cv))
    mont = lambda v: (v << 256) % r
    for name, cols, sc in _cases(r, m, rng)[1:9:3]:                                        # random k = 5, 7; all r - 1; words >= r
        cols = dict(cols, Tg=[0] * m, qK=[mont(rng.randrange(2)) for _ in range(m)])
        cols["qK"][0], cols["qK"][1] = 0, mont(1)
        ds = {k: _dev(zk, cols[k]) for k in NAMES}
        try:
            tagged = _take(flt.quotients([ds[k] for k in NAMES], log_n, *sc, cv), m)
            single = _take(fl.quotients([ds[k] for k in SHARED], log_n, *sc, cv), m)
            assert tagged[:3] == single[:3], name
            off = [i for i in range(m) if cols["qK"][i] == 0]
            assert 0 < len(off) < m and [tagged[3][i] for i in off] == [single[3][i] for i in off], name
            if sc[4] and name.startswith("random"):                                        # eta^3 q_K is in f where q_K = 1
                assert any(tagged[3][i] != single[3][i] for i in range(m) if cols["qK"][i]), name
        finally:
            for d in ds.values():
                d.free()


@pytest.mark.parametrize("log_n", (3, 7))
@pytest.mark.parametrize("cv", CURVES)
def test_output_3_is_the_tagged_quotient_of_plonk_lookup(zk, flt, cv, log_n):
    pl = importlib.import_module("eigen_zkvm_amd.plonk_lookup")
    r, m, rng = ref.R[cv], 4 << log_n, random.Random(0x29 + log_n + len(cv))
    cases = _cases(r, m, rng)
    for name, cols, sc in cases[1:9:3] + cases[-1:]:
        ds = {k: _dev(zk, cols[k]) for k in NAMES}
        acc = zk.DevArray(4 * m, zero=True)
        try:
            fused = _take(flt.quotients([ds[k] for k in NAMES], log_n, *sc, cv, want=(False, False, False, True)), m)
            pl.lookup_quotient([ds[k] for k in TAGGED_NAMES], log_n, 1, sc[4], sc[5], acc, cv, tagged=True)
            assert fused[3] == _host(acc, m), name
        finally:
            acc.free()
            for d in ds.values():
                d.free()


@pytest.mark.parametrize("cv", CURVES)
def test_every_pattern_of_outputs_left_out(zk, flt, cv):
    r, log_n, rng = ref.R[cv], 3, random.Random(0x2a + len(cv))
    m = 4 << log_n
    cols = {k: [rng.randrange(1 << 256) for _ in range(m)] for k in NAMES}
    sc = [rng.randrange(r), rng.randrange(r), 2, 3, rng.randrange(r), rng.randrange(r)]
    want = _want(r, cols, m, *sc)
    ds = [_dev(zk, cols[k]) for k in NAMES]
    try:
        for pattern in itertools.product((False, True), repeat=4):
            if any(pattern):
                got = _take(flt.quotients(ds, log_n, *sc, cv, want=pattern), m)
                assert got == [w if p else None for w, p in zip(want, pattern)], pattern
    finally:
        for d in ds:
            d.free()


@pytest.mark.parametrize("cv", CURVES)
def test_refusals(zk, flt, cv):
    r = ref.R[cv]
    cols = [_dev(zk, [0] * 32) for _ in range(22)]
    outs = [zk.DevArray(4 * 32) for _ in range(4)]
    ok = [2, 3, 2, 3, 5, 7]
    try:
        with pytest.raises(flt.ZkError, match="fflonk lookup tagged: quotients: output 1 overlaps column 17"):
            flt.quotients(cols, 3, *ok, cv, outs=[outs[0], cols[17], outs[2], outs[3]])
        with pytest.raises(flt.ZkError, match="output 3 overlaps column 21"):
            flt.quotients(cols, 3, *ok, cv, outs=[outs[0], outs[1], outs[2], cols[21]])
        with pytest.raises(flt.ZkError, match="output 3 overlaps output 0"):
            flt.quotients(cols, 3, *ok, cv, outs=[outs[0], outs[1], outs[2], outs[0]])
        with pytest.raises(flt.ZkError, match="every output is null"):
            flt.quotients(cols, 3, *ok, cv, want=(False, False, False, False))
        for at, name in enumerate(("beta", "gamma", "k1", "k2", "eta", "delta")):
            sc = list(ok)
            sc[at] = r
            with pytest.raises(flt.ZkError, match="%s is not below" % name):
                flt.quotients(cols, 3, *sc, cv)
        with pytest.raises(flt.ZkError, match="every column of the quotients holds 4n = 64"):
            flt.quotients(cols, 4, *ok, cv)
        with pytest.raises(flt.ZkError, match="every output of the quotients holds 4n = 32"):
            flt.quotients(cols, 3, *ok, cv, outs=[zk.DevArray(4 * 16), None, None, None])
        with pytest.raises(flt.ZkError, match="take 22 columns"):
            flt.quotients(cols[:21], 3, *ok, cv)
        # the library's own refusals, decided on the host before any device work
        lib = zk.lib()
        fn = getattr(lib, "zk_fflonk_%s_lookup_tagged_quotients_dev" % {"BN128": "bn254", "BLS12381": "bls12_381"}[cv])
        big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
        one = np.array([1, 0, 0, 0], dtype=np.uint64)
        ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
        op = [o.ptr for o in outs]
        assert fn(zk._ptr(ptrs), 3, *[zk._ptr(one)] * 5, zk._ptr(big), *op, None) != 0
        assert "fflonk lookup tagged: delta is not below the scalar field's modulus" in lib.zk_last_error().decode()
        s = flt.pa.TWO_ADICITY[cv]
        assert fn(zk._ptr(ptrs), s - 1, *[zk._ptr(one)] * 6, *op, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
        ptrs[21] = 0
        assert fn(zk._ptr(ptrs), 3, *[zk._ptr(one)] * 6, *op, None) != 0 and "column 21 is null" in lib.zk_last_error().decode()
    finally:
        for d in cols + outs:
            d.free()
