"""Transforms and scalar products whose elements are curve points (csrc/ecntt.hip, ecntt_impl.hip.h; zk_<g1|g2>_<curve>_ntt_dev and
_mul_scalar_dev through the C ABI), both curves and both groups, byte for byte -- points are affine and canonical, so there is no
tolerance.  A transform of [k_i]G must be [NTT(k)_i]G: NTT(k) comes from the CPU reference's scalar-field transform, the points on both
sides from the fixed-base kernel that tests/test_gpu_groth16_keygen.py holds to the reference's scalar product.
Sizes: a butterfly launch is 64 lanes a block (n / 2 = 32, 64, 128 at log_n 6, 7, 8), a wave shares its twiddle while a stage has 64
groups or more (first at log_n 7), the way out is 256 lanes a block (n = 128, 256, 512 at log_n 7, 8, 9)."""
import importlib, pathlib, random, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
GROUPS = ("g1", "g2")
LOGS = (0, 1, 2, 3, 6, 7, 8, 9)


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


def _points(zk, g, cv, group, ks):
    """[k_i]G on the device; zero gives the all-zero encoding"""
    return zk.mul_generator_fr(zk.DevArray.from_host(g.fr_array(ks).reshape(-1)), cv, group=group)


def _ntt_ints(g, ks, inverse=False):
    return g.fr_ints(g.from_mont(g.ntt(g.to_mont(g.fr_array(ks)), inverse=inverse)))


def _check_transform(zk, dev, g, cv, tag, group, ks):
    d = _points(zk, g, cv, group, ks)
    before = d.to_host().copy()
    want = _points(zk, g, cv, group, _ntt_ints(g, ks)).to_host()
    dev.group_ntt(d, tag, group)
    got = d.to_host()
    assert got.tobytes() == want.tobytes(), [i for i in range(len(ks)) if got.reshape(len(ks), -1)[i].tobytes() != want.reshape(len(ks), -1)[i].tobytes()][:8]
    dev.group_ntt(d, tag, group, inverse=True)
    assert d.to_host().tobytes() == before.tobytes()
    return got.reshape(len(ks), -1)


@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("cv,tag", CURVES)
def test_transform_of_multiples_of_the_generator(zk, g16, dev, cv, tag, group, log_n):
    g = g16[cv]; rng = random.Random(1000 + log_n)
    ks = [rng.randrange(g.r) for _ in range(1 << log_n)]
    _check_transform(zk, dev, g, cv, tag, group, ks)
    # the inverse on its own, against the reference's inverse transform (1 / n included)
    d = _points(zk, g, cv, group, ks)
    dev.group_ntt(d, tag, group, inverse=True)
    assert d.to_host().tobytes() == _points(zk, g, cv, group, _ntt_ints(g, ks, inverse=True)).to_host().tobytes()


@pytest.mark.parametrize("log_n", (3, 7))
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("cv,tag", CURVES)
def test_transform_directed_inputs(zk, g16, dev, cv, tag, group, log_n):
    """what add-2008-s alone gets wrong (P + P, P - P in the very first butterflies) and infinity on either side"""
    g = g16[cv]; r = g.r; n = 1 << log_n; rng = random.Random(77 + log_n)
    c = rng.randrange(1, r)
    out = _check_transform(zk, dev, g, cv, tag, group, [c] * n)                       # all equal: [n c]G, then infinity
    assert out[0].any() and not out[1:].any()
    out = _check_transform(zk, dev, g, cv, tag, group, [c, r - c] * (n // 2))         # P, -P alternating: only index n / 2 survives
    assert out[n // 2].any() and not np.delete(out, n // 2, axis=0).any()
    out = _check_transform(zk, dev, g, cv, tag, group, [0] * n)                       # all infinity
    assert not out.any()
    out = _check_transform(zk, dev, g, cv, tag, group, [c] + [0] * (n - 1))           # one finite point at index 0: a constant column
    assert all(row.tobytes() == out[0].tobytes() for row in out) and out[0].any()
    out = _check_transform(zk, dev, g, cv, tag, group, [0] * (n - 1) + [c])           # one finite point at index n - 1
    assert all(row.any() for row in out)
    sparse = [rng.randrange(1, r) if i % 3 == 0 else 0 for i in range(n)]             # NTT(k) with zeros: infinity appears in the output
    out = _check_transform(zk, dev, g, cv, tag, group, _ntt_ints(g, sparse, inverse=True))
    assert [bool(row.any()) for row in out] == [v != 0 for v in sparse]


MUL_N = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def mul_cases(g16):
    """per curve: the multipliers of the generator behind the points (zeros = infinities among them) and the scalars"""
    out = {}
    for cv, _ in CURVES:
        r = g16[cv].r; rng = random.Random(31)
        a = [rng.randrange(1, r) for _ in range(max(MUL_N))]
        for i in (0, 5, 62, 63, 64, 200, 256):
            a[i] = 0
        a[1] = 1; a[2] = r - 1
        out[cv] = (a, [1, 2, r - 1, rng.randrange(3, r - 1)])
    return out


@pytest.mark.parametrize("n", MUL_N)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("cv,tag", CURVES)
def test_mul_scalar_matches_oracle(zk, g16, dev, mul_cases, cv, tag, group, n):
    g = g16[cv]; cur = g.g2 if group == "g2" else g.g1
    a, ks = mul_cases[cv]
    d = _points(zk, g, cv, group, a[:n])
    src = d.to_host().copy().reshape(n, -1)
    Gen = cur.generator()
    for k in ks:
        got = dev.mul_scalar(d, k, tag, group).to_host().reshape(n, -1)
        for i in range(n):
            exp = g.mul(cur, None if a[i] == 0 else src[i], k)                         # the CPU reference's scalar product of the point itself
            assert np.array_equal(got[i], np.zeros_like(got[i]) if exp is None else exp), (hex(k), i)
        if n == 65:                                                                    # and the same through the generator: [a_i k]G
            for i in (1, 2, 64):
                exp = g.mul(cur, Gen, a[i] * k)
                assert np.array_equal(got[i], np.zeros_like(got[i]) if exp is None else exp)
    assert d.to_host().tobytes() == src.tobytes()                                      # the input is left alone
