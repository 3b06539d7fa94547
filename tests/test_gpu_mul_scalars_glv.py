"""The per-point scalar product through the endomorphism split (csrc/ecntt_impl.hip.h ecn_mul_scalars_glv_kernel, glv_split.hip.h;
zk_g1_<curve>_mul_scalars_glv_dev, mul_scalars(..., glv=True)): G1 of both curves, byte for byte against the bit walk of mul_scalars,
which tests/test_gpu_groth16_verify_aggregate.py pins to the CPU reference -- affine canonical output, so there is no tolerance -- and a
dozen products directly against the reference.
Sizes: the walk launches 64 lanes a block (63, 64, 65), the way out 256 (257).  Points: the multiples of the generator of mul_cases in
tests/test_gpu_group_ntt.py (restated: a fixture of another module), infinities among them.  Scalars: the ends of the range, the
neighbourhood of lambda and of 2^128 where the halves change length, scalars with an empty half, with equal halves, and 240 random ones
of full width; within a launch every lane has a scalar of its own."""
import importlib, pathlib, random, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
# (beta x, y) = [lambda](x, y) on G1 (tools/glv_constants.py)
LAMBDA = {"bn254": 4407920970296243842393367215006156084916469457145843978461, "bls12_381": 0xac45a4010001a40200000000ffffffff}
MUL_N = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def g16(orc):
    return {cv: G.Groth16Oracle(orc, cv) for cv, _ in CURVES}


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


@pytest.fixture(scope="module")
def cases(g16):
    """per curve: the multipliers of the generator behind the points (as mul_cases has them) and 257 distinct scalars"""
    out = {}
    for cv, _ in CURVES:
        r = g16[cv].r; lam = LAMBDA[cv]; rng = random.Random(31)
        assert (lam * lam + lam + 1) % r == 0
        a = [rng.randrange(1, r) for _ in range(max(MUL_N))]
        for i in (0, 5, 62, 63, 64, 200, 256):
            a[i] = 0
        a[1] = 1; a[2] = r - 1
        m = rng.randrange(2**100, 2**120)
        edge = [0, 1, 2, 3, r - 1, lam, lam - 1, lam + 1, 2 * lam + 2, 2**127, 2**128 - 1, 2**128,
                5 * lam % r, m * lam % r,                                 # k1 = 0
                2**100 + 3, m,                                            # k2 = 0
                m * (lam + 1) % r]                                        # equal halves
        ks = edge + [rng.randrange(2**250, r) for _ in range(max(MUL_N) - len(edge))]
        assert len(set(ks)) == max(MUL_N)
        out[cv] = (a, ks)
    return out


def _points(zk, g, cv, ks):
    return zk.mul_generator_fr(zk.DevArray.from_host(g.fr_array(ks).reshape(-1)), cv, group="g1")


@pytest.mark.parametrize("n,start", [(1, 0), (1, 1), (63, 0), (64, 0), (65, 0), (257, 0)])
@pytest.mark.parametrize("cv,tag", CURVES)
def test_glv_walk_equals_the_bit_walk(zk, g16, dev, cases, cv, tag, n, start):
    g = g16[cv]
    a, ks = cases[cv]
    a = a[start:start + n]
    d = _points(zk, g, cv, a)
    src = d.to_host().copy()
    for shift in (0, 1, 16):                                              # every edge scalar meets finite points and an infinity
        k = [ks[(i + shift) % len(ks)] for i in range(n)]
        want = dev.mul_scalars(d, k, tag, "g1").to_host().reshape(n, -1)
        got = dev.mul_scalars(d, k, tag, "g1", glv=True).to_host().reshape(n, -1)
        bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
        assert not bad, (tag, n, shift, [(i, hex(k[i]), a[i] == 0) for i in bad[:4]])
        for i in range(n):                                                # the all-zero encoding where the contract says so
            assert got[i].any() == (a[i] != 0 and k[i] != 0), (tag, n, shift, i)
    assert d.to_host().tobytes() == src.tobytes()                         # the input is left alone


@pytest.mark.parametrize("cv,tag", CURVES)
def test_glv_walk_against_the_reference(zk, g16, dev, cases, cv, tag):
    g = g16[cv]
    a, ks = cases[cv]
    lanes = [1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14]                  # finite points; the scalars 5 .. 18 of the list and r - 1
    k = [ks[i + 4] for i in range(65)]
    d = _points(zk, g, cv, a[:65])
    src = d.to_host().reshape(65, -1)
    got = dev.mul_scalars(d, k, tag, "g1", glv=True).to_host().reshape(65, -1)
    for i in lanes:
        exp = g.mul(g.g1, src[i], k[i])
        assert np.array_equal(got[i], np.zeros_like(got[i]) if exp is None else exp), (tag, i, hex(k[i]))


@pytest.mark.parametrize("cv,tag", CURVES)
def test_glv_walk_in_place(zk, g16, dev, cases, cv, tag):
    """d_out == d_points: the products go through a work buffer of their own"""
    g = g16[cv]
    a, ks = cases[cv]
    n = 65
    k = [ks[(i + 9) % len(ks)] for i in range(n)]
    d = _points(zk, g, cv, a[:n])
    want = dev.mul_scalars(d, k, tag, "g1").to_host().copy()
    kw = np.array([(v >> (64 * j)) & (2**64 - 1) for v in k for j in range(4)], dtype=np.uint64)
    dk = zk.DevArray.from_host(kw)
    assert getattr(zk.lib(), "zk_g1_%s_mul_scalars_glv_dev" % cv)(d.ptr, n, dk.ptr, d.ptr, 0) == 0, zk.lib().zk_last_error()
    assert d.to_host().tobytes() == want.tobytes()


def test_no_split_for_g2(zk, dev):
    with pytest.raises(zk.ZkError):
        dev.mul_scalars(zk.DevArray(32), [1], "BN128", "g2", glv=True)
