"""y = p(z) and q = (p - y) / (X - z) on the device (csrc/kzg_impl.hip.h through zk_kzg_<curve>_divide_dev) against tests/kzg_ref.py, word for
word: everything is an exact integer mod r, so there is no tolerance.  No powers-of-tau file is needed.
Lengths come from the exported constants: T = zk_kzg_tile_elems() coefficients per workgroup (8 per lane), S = zk_kzg_aggregate_span() tile
aggregates per step of the combining workgroup.  1, 2, 3: lanes without a full run; 63 .. 65: the 8-coefficient runs of one wave; T - 1 .. 3T - 1:
one, two and three tiles with the border inside a lane's run; past T S: the combining workgroup takes a second step (q checked in full)."""
import random
import numpy as np
import pytest

import kzg_ref as ref

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


def _lengths(T):
    return [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1]


def _check(kzg, curve, coeffs, z):
    r = ref.R[curve]
    want_q, want_y = ref.divide(coeffs, z, r)
    d = kzg.DevArray.from_host(kzg.to_mont(coeffs, curve).reshape(-1))       # one upload serves the division and the evaluation
    try:
        q, y = kzg.divide(d, z, curve)
        assert y == want_y
        assert q == want_q, [j for j in range(len(want_q)) if q[j] != want_q[j]][:8]
        assert kzg.evaluate(d, z, curve) == want_y                          # evaluation alone: the same y, no q
    finally:
        d.free()


def test_exported_constants(consts):
    T, S = consts
    assert T >= 64 and T & (T - 1) == 0 and S >= 2


@pytest.mark.parametrize("curve", CURVES)
def test_random_polynomials_at_every_length(kzg, consts, curve):
    rng = random.Random(0xD1 + len(curve))
    r = ref.R[curve]
    for n in _lengths(consts[0]):
        _check(kzg, curve, [rng.randrange(r) for _ in range(n)], rng.randrange(r))


@pytest.mark.parametrize("curve", CURVES)
def test_edge_points(kzg, consts, curve):
    """z = 0 (no inverse anywhere), 1, r - 1, at lengths on both sides of a tile border"""
    rng = random.Random(0xE0 + len(curve))
    r = ref.R[curve]
    T = consts[0]
    for n in (1, 2, 65, T + 1, 2 * T + 1):
        coeffs = [rng.randrange(r) for _ in range(n)]
        for z in (0, 1, r - 1):
            _check(kzg, curve, coeffs, z)


@pytest.mark.parametrize("curve", CURVES)
def test_root_of_unity(kzg, consts, curve):
    """p = X^(2^k) - 1 at a primitive 2^k-th root w: y = 0 and q_j = w^(2^k - 1 - j); 2^k = 2T spans two tiles exactly"""
    r = ref.R[curve]
    for n in (64, 2 * consts[0]):
        w = ref.root_of_unity(curve, n.bit_length() - 1)
        coeffs = [r - 1] + [0] * (n - 1) + [1]
        q, y = kzg.divide(coeffs, w, curve)
        assert y == 0
        assert q == [pow(w, n - 1 - j, r) for j in range(n)]
        _check(kzg, curve, coeffs, w)


@pytest.mark.parametrize("curve", CURVES)
def test_edge_polynomials(kzg, consts, curve):
    rng = random.Random(0xE1 + len(curve))
    r = ref.R[curve]
    T = consts[0]
    for n in (3, 65, T + 1, 3 * T - 1):
        z = rng.randrange(r)
        _check(kzg, curve, [0] * n, z)                                                   # all zero
        _check(kzg, curve, [0] * (n - 1) + [rng.randrange(1, r)], z)                     # a single non-zero top coefficient
        _check(kzg, curve, [rng.randrange(r) for _ in range(n - n // 2)] + [0] * (n // 2), z)   # the top half all zero
        _check(kzg, curve, [r - 1] * n, z)                                               # every coefficient r - 1
        _check(kzg, curve, [r - 1] * n, r - 1)


@pytest.mark.parametrize("curve", CURVES)
def test_past_one_step_of_the_combining_workgroup(kzg, consts, curve):
    """T S + T + 1 coefficients: S + 2 tile aggregates, so the combining workgroup carries h from its second step into its first"""
    T, S = consts
    n = T * S + T + 1
    rng = random.Random(0xA6 + len(curve))
    r = ref.R[curve]
    _check(kzg, curve, [rng.randrange(r) for _ in range(n)], rng.randrange(r))


@pytest.mark.parametrize("off", (-1, 0))
@pytest.mark.parametrize("curve", CURVES)
def test_tile_count_a_multiple_of_the_span(kzg, consts, curve, off):
    """T S and T S - 1 coefficients: exactly S tile aggregates, so the last tile's carry is the one entry no lane of the combining workgroup
    meets as a neighbour from a higher step (it is h past the end: zero).  Divided twice, q checked in full both times: the second call's
    scratch is the first call's, recycled and dirty."""
    T, S = consts
    n = T * S + off
    rng = random.Random(0xB7 + len(curve) + off)
    r = ref.R[curve]
    coeffs, z = [rng.randrange(r) for _ in range(n)], rng.randrange(r)
    want_q, want_y = ref.divide(coeffs, z, r)
    d = kzg.DevArray.from_host(kzg.to_mont(coeffs, curve).reshape(-1))
    try:
        for _ in range(2):
            q, y = kzg.divide(d, z, curve)
            assert y == want_y
            assert q == want_q, [j for j in range(len(want_q)) if q[j] != want_q[j]][:8]
    finally:
        d.free()


def test_refusals(kzg):
    r = ref.R["BN128"]
    with pytest.raises(kzg.ZkError, match="below the scalar field's modulus"):
        kzg.divide([1, 2, 3], r, "BN128")
    assert kzg.divide([], 5, "BN128") == ([], 0)


@pytest.mark.parametrize("curve", CURVES)
def test_linear_combination(kzg, consts, curve):
    """sum gamma^i p_i over unequal lengths, one and several polynomials, gamma = 0 and 1 included"""
    rng = random.Random(0xC0 + len(curve))
    r = ref.R[curve]
    for lens in ((5,), (3, 300), (257, 1, 64, 0, 256)):
        polys = [[rng.randrange(r) for _ in range(n)] for n in lens]
        for gamma in (0, 1, r - 1, rng.randrange(r)):
            assert kzg.lincomb(polys, gamma, curve) == ref.fold_polys(polys, gamma, r)
