"""out = acc + w q with q = (p - p(z)) / (X - z) on the device (the accumulating last phase of csrc/kzg_impl.hip.h through
zk_kzg_<curve>_divide_acc_dev) and the interleaving of k polynomials (zk_kzg_<curve>_interleave_dev), word for word against plain Python:
everything is an exact integer mod r, so there is no tolerance.  No powers-of-tau file is needed.
Lengths come from the exported constants as in test_gpu_kzg_divide.py: T = zk_kzg_tile_elems(), S = zk_kzg_aggregate_span().  The entry point
updates the running sum in place, so acc and out are always the same buffer here; the sum is zero, random, or -- kept on the device across
calls -- the result of the previous division."""
import random
import pytest

import kzg_ref as ref
import kzg_multi_ref as mref

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def kzg():
    import importlib
    return importlib.import_module("eigen_zkvm_amd.kzg")


@pytest.fixture(scope="module")
def consts(zk):
    return int(zk.lib().zk_kzg_tile_elems()), int(zk.lib().zk_kzg_aggregate_span())


def _want(coeffs, z, w, acc, r):
    q, y = ref.divide(coeffs, z, r)
    return [(a + w * q[j]) % r if j < len(q) else a for j, a in enumerate(acc)], y


def _check(kzg, curve, coeffs, z, w, acc):
    r = ref.R[curve]
    want, want_y = _want(coeffs, z, w, acc, r)
    got, y = kzg.divide_acc(coeffs, z, w, acc, curve)
    assert y == want_y
    assert got == want, (len(coeffs), [j for j in range(len(want)) if got[j] != want[j]][:8])


@pytest.mark.parametrize("curve", CURVES)
def test_every_length_random_operands(kzg, consts, curve):
    T = consts[0]
    rng = random.Random(0x1A + len(curve))
    r = ref.R[curve]
    for n in (1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        coeffs = [rng.randrange(r) for _ in range(n)]
        _check(kzg, curve, coeffs, rng.randrange(r), rng.randrange(r), [rng.randrange(r) for _ in range(n - 1)])
        _check(kzg, curve, coeffs, rng.randrange(r), rng.randrange(r), [0] * (n - 1))


@pytest.mark.parametrize("curve", CURVES)
def test_edge_points_and_weights(kzg, consts, curve):
    """z in {0, 1, r - 1, a root of unity, random} x w in {0, 1, r - 1, random}, on both sides of a tile border; acc = r - 1 everywhere makes
    every sum wrap"""
    T = consts[0]
    rng = random.Random(0x1B + len(curve))
    r = ref.R[curve]
    for n in (3, 65, T + 1):
        coeffs = [rng.randrange(r) for _ in range(n)]
        acc = [rng.randrange(r) for _ in range(n - 1)]
        for z in (0, 1, r - 1, ref.root_of_unity(curve, 5), rng.randrange(r)):
            for w in (0, 1, r - 1, rng.randrange(r)):
                _check(kzg, curve, coeffs, z, w, acc)
        _check(kzg, curve, [r - 1] * n, r - 1, r - 1, [r - 1] * (n - 1))


@pytest.mark.parametrize("curve", CURVES)
def test_running_sum_on_the_device(kzg, consts, curve):
    """three divisions of different polynomials at different points into ONE device buffer, each reading what the one before wrote: the
    quotient by Z_S as the library forms it, here against the reference's successive division"""
    T = consts[0]
    rng = random.Random(0x1C + len(curve))
    r = ref.R[curve]
    n = T + 5
    f = [rng.randrange(r) for _ in range(n)]
    pts = [rng.randrange(r) for _ in range(3)]
    d = kzg.DevArray.from_host(kzg.to_mont([0] * (n - 1), curve).reshape(-1))
    try:
        for j, s in enumerate(pts):
            den = 1
            for j2, s2 in enumerate(pts):
                if j2 != j:
                    den = den * (s - s2) % r
            _, y = kzg.divide_acc(f, s, pow(den, -1, r), d, curve)
            assert y == ref.horner(f, s, r)
        got = kzg.from_mont(d.to_host(), curve)
    finally:
        d.free()
    q, _ = mref.quotient_by_successive_division(f, pts, r)
    assert got[:len(q)] == q and not any(got[len(q):])


@pytest.mark.parametrize("curve", CURVES)
def test_a_shorter_polynomial_leaves_the_tail(kzg, consts, curve):
    T = consts[0]
    rng = random.Random(0x1D + len(curve))
    r = ref.R[curve]
    for n, n_acc in ((1, 5), (2, 5), (65, 200), (T, 2 * T + 3), (T + 1, T + 2)):
        _check(kzg, curve, [rng.randrange(r) for _ in range(n)], rng.randrange(r), rng.randrange(r), [rng.randrange(r) for _ in range(n_acc)])


@pytest.mark.parametrize("n_of", (lambda T, S: T * S, lambda T, S: T * S + T + 1), ids=("TS", "TS+T+1"))
def test_past_one_step_of_the_combining_workgroup(kzg, consts, n_of):
    """the two large cases, on one curve: S tile aggregates exactly, and S + 2 of them"""
    T, S = consts
    n = n_of(T, S)
    rng = random.Random(0x1E + n % 7)
    r = ref.R["BN128"]
    _check(kzg, "BN128", [rng.randrange(r) for _ in range(n)], rng.randrange(r), rng.randrange(r), [rng.randrange(r) for _ in range(n - 1)])


def test_refusals(kzg):
    r = ref.R["BN128"]
    with pytest.raises(kzg.ZkError, match="w is not below the scalar field's modulus"):
        kzg.divide_acc([1, 2, 3], 1, r, [0, 0], "BN128")
    with pytest.raises(kzg.ZkError, match="z is not below the scalar field's modulus"):
        kzg.divide_acc([1, 2, 3], r, 1, [0, 0], "BN128")
    with pytest.raises(kzg.ZkError, match="running sum holds 1 elements"):
        kzg.divide_acc([1, 2, 3], 1, 1, [0], "BN128")
    assert kzg.divide_acc([], 5, 7, [], "BN128") == ([], 0)
    assert kzg.divide_acc([9], 5, 7, [4], "BN128") == ([4], 9)


@pytest.mark.parametrize("curve", CURVES)
def test_interleave(kzg, consts, curve):
    """k in {1, 2, 3, 8}, ragged lengths (an empty polynomial among them), more than one workgroup of output"""
    rng = random.Random(0x1F + len(curve))
    r = ref.R[curve]
    for lens in ((5,), (300,), (7, 4), (257, 300), (3, 0, 130), (90, 1, 77, 0, 64, 65, 100, 2)):
        polys = [[rng.randrange(r) for _ in range(n)] for n in lens]
        assert kzg.interleave(polys, curve) == mref.interleave(polys), lens
    assert kzg.interleave([[], []], curve) == []
