"""The kernel of the fflonk prover (csrc/fflonk_impl.hip.h) word for word against Python integers: the three numerators from
ONE launch at log_n = 3 (32 coset points: half a wave, the (i + 4) mod m wrap inside it) and log_n = 7 (512 points: two workgroups), every
operand word at 2^256 - 1 with every scalar at r - 1, k_1, k_2 = 2, 3 (additions) and 5, 7 (products: both paths of pk_times_k), both fields;
then the launches the prover makes, with outputs left out, and the refusals.  An input element is the 256-bit integer its words are (any
value below 2^256, not only below r) and stands for words / 2^256 mod r; every output word vector must be the canonical Montgomery
representative.  Exact: no tolerance anywhere."""
import importlib, random

import numpy as np
import pytest

import plonk_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")
NAMES = ("a", "b", "c", "Z", "qL", "qR", "qO", "qM", "qC", "S1", "S2", "S3", "PI", "L1", "X")      # the order of zk_plonk_<curve>_quotient_dev


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def fflonk(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk")


def _dev(zk, words):
    """integers below 2^256, taken as the words themselves"""
    a = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in words), dtype="<u8").astype(np.uint64)
    return zk.DevArray.from_host(a)


def _host(d, n):
    b = d.to_host()[:4 * n].astype("<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _want(r, cols, m, beta, gamma, k1, k2):
    """the three numerators at every index from the columns' words, as Montgomery words"""
    rinv = pow(1 << 256, -1, r)
    v = {k: [w * rinv % r for w in cols[k]] for k in NAMES}
    out = [[], [], []]
    for i in range(m):
        a, b, c, z, x = v["a"][i], v["b"][i], v["c"][i], v["Z"][i], v["X"][i]
        zw = v["Z"][(i + 4) % m]
        gate = a * b * v["qM"][i] + a * v["qL"][i] + b * v["qR"][i] + c * v["qO"][i] + v["qC"][i] + v["PI"][i]
        p1 = (a + beta * x + gamma) * (b + beta * k1 * x + gamma) * (c + beta * k2 * x + gamma) * z
        p2 = (a + beta * v["S1"][i] + gamma) * (b + beta * v["S2"][i] + gamma) * (c + beta * v["S3"][i] + gamma) * zw
        for j, val in enumerate((gate, v["L1"][i] * (z - 1), p1 - p2)):
            out[j].append((val % r << 256) % r)
    return out


def _run(zk, fflonk, cv, log_n, cols, beta, gamma, k1, k2, want=(True, True, True)):
    m = 4 << log_n
    ds = [_dev(zk, cols[k]) for k in NAMES]
    try:
        outs = fflonk.quotients(ds, log_n, beta, gamma, k1, k2, cv, want=want)
        try:
            return [None if o is None else _host(o, m) for o in outs]
        finally:
            for o in outs:
                if o is not None:
                    o.free()
    finally:
        for d in ds:
            d.free()


@pytest.mark.parametrize("log_n", (3, 7))
@pytest.mark.parametrize("cv", CURVES)
def test_the_three_numerators_word_for_word(zk, fflonk, cv, log_n):
    r, m, rng = ref.R[cv], 4 << log_n, random.Random(0x23 + log_n + len(cv))
    if log_n == 7:
        assert m > 256                                                                     # more than one workgroup of 256 lanes
    mont = lambda v: (v << 256) % r
    rand = lambda: {k: [mont(rng.randrange(r)) for _ in range(m)] for k in NAMES}
    const = lambda w: {k: [w] * m for k in NAMES}
    wide = {k: [rng.randrange(r, 1 << 256) for _ in range(m)] for k in NAMES}             # words >= r but < 2^256
    for k in NAMES:
        wide[k][0], wide[k][1], wide[k][m - 1] = (1 << 256) - 1, r, (1 << 256) - 1
    wrap = const(mont(1))                                                                  # Z alone distinct: indices 4n - 4 .. 4n - 1 read Z at 0 .. 3
    wrap["Z"] = [mont(i + 2) for i in range(m)]
    sc = lambda: [rng.randrange(r) for _ in range(2)]
    cases = [("random, k = 2, 3", rand(), sc(), (2, 3)),
             ("random, k = 5, 7", rand(), sc(), (5, 7)),
             ("random, k = 3, r - 1", rand(), sc(), (3, r - 1)),
             ("all zero", const(0), sc(), (2, 3)),
             ("all r - 1, every scalar r - 1", const(mont(r - 1)), [r - 1] * 2, (r - 1, r - 1)),
             ("every word 2^256 - 1, every scalar r - 1, k = 2, 3", const((1 << 256) - 1), [r - 1] * 2, (2, 3)),
             ("every word 2^256 - 1, every scalar r - 1, k = 5, 7", const((1 << 256) - 1), [r - 1] * 2, (5, 7)),
             ("words >= r, k = 2, 3", wide, sc(), (2, 3)),
             ("words >= r, k = 5, 7, scalars r - 1", wide, [r - 1] * 2, (5, 7)),
             ("the wrap of Z(wX)", wrap, sc(), (2, 3)),
             ("beta = gamma = 0", rand(), [0, 0], (2, 3))]
    for name, cols, (beta, gamma), (k1, k2) in cases:
        got = _run(zk, fflonk, cv, log_n, cols, beta, gamma, k1, k2)
        want = _want(r, cols, m, beta, gamma, k1, k2)
        for j in range(3):
            assert all(w < r for w in got[j]), (name, j)                                   # canonical
            assert got[j][m - 4:] == want[j][m - 4:], (name, j)                            # the wrap
            assert got[j] == want[j], (name, j)


@pytest.mark.parametrize("cv", CURVES)
def test_the_launches_the_prover_makes_leave_outputs_out(zk, fflonk, cv):
    r, log_n, rng = ref.R[cv], 3, random.Random(0x24 + len(cv))
    m = 4 << log_n
    cols = {k: [rng.randrange(1 << 256) for _ in range(m)] for k in NAMES}
    beta, gamma = rng.randrange(r), rng.randrange(r)
    want = _want(r, cols, m, beta, gamma, 2, 3)
    first = dict(cols, Z=cols["a"])                                                        # round 1: no Z, no beta, no gamma yet
    assert _run(zk, fflonk, cv, log_n, first, 0, 0, 2, 3, want=(True, False, False)) == [want[0], None, None]
    assert _run(zk, fflonk, cv, log_n, cols, beta, gamma, 2, 3, want=(False, True, True)) == [None, want[1], want[2]]
    assert _run(zk, fflonk, cv, log_n, cols, beta, gamma, 2, 3, want=(False, True, False)) == [None, want[1], None]
    assert _run(zk, fflonk, cv, log_n, cols, beta, gamma, 2, 3, want=(False, False, True)) == [None, None, want[2]]


@pytest.mark.parametrize("cv", CURVES)
def test_refusals(zk, fflonk, cv):
    r = ref.R[cv]
    cols = [_dev(zk, [0] * 32) for _ in range(15)]
    outs = [zk.DevArray(4 * 32) for _ in range(3)]
    try:
        with pytest.raises(fflonk.ZkError, match="output 1 overlaps column 7"):
            fflonk.quotients(cols, 3, 2, 3, 2, 3, cv, outs=[outs[0], cols[7], outs[2]])
        with pytest.raises(fflonk.ZkError, match="output 2 overlaps output 0"):
            fflonk.quotients(cols, 3, 2, 3, 2, 3, cv, outs=[outs[0], outs[1], outs[0]])
        with pytest.raises(fflonk.ZkError, match="every output is null"):
            fflonk.quotients(cols, 3, 2, 3, 2, 3, cv, want=(False, False, False))
        for at, name in enumerate(("beta", "gamma", "k1", "k2")):
            sc = [2, 3, 2, 3]
            sc[at] = r
            with pytest.raises(fflonk.ZkError, match="%s is not below" % name):
                fflonk.quotients(cols, 3, *sc, cv)
        with pytest.raises(fflonk.ZkError, match="every column of the quotients holds 4n = 64"):
            fflonk.quotients(cols, 4, 2, 3, 2, 3, cv)
        with pytest.raises(fflonk.ZkError, match="every output of the quotients holds 4n = 32"):
            fflonk.quotients(cols, 3, 2, 3, 2, 3, cv, outs=[zk.DevArray(4 * 16), None, None])
        with pytest.raises(fflonk.ZkError, match="take 15 columns"):
            fflonk.quotients(cols[:14], 3, 2, 3, 2, 3, cv)
        # the library's own refusals of a scalar and of the size, decided on the host before any device work
        lib = zk.lib()
        fn = getattr(lib, "zk_fflonk_%s_quotients_dev" % {"BN128": "bn254", "BLS12381": "bls12_381"}[cv])
        big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
        one = np.array([1, 0, 0, 0], dtype=np.uint64)
        ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
        assert fn(zk._ptr(ptrs), 3, zk._ptr(one), zk._ptr(big), zk._ptr(one), zk._ptr(one), outs[0].ptr, outs[1].ptr, outs[2].ptr, None) != 0
        assert "fflonk: gamma is not below the scalar field's modulus" in lib.zk_last_error().decode()
        s = fflonk.TWO_ADICITY[cv]
        assert fn(zk._ptr(ptrs), s - 1, *[zk._ptr(one)] * 4, outs[0].ptr, outs[1].ptr, outs[2].ptr, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
    finally:
        for d in cols + outs:
            d.free()
