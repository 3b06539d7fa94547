"""Products of polynomials and quotients by X^N - 1 on the device (csrc/frpoly_impl.hip.h through eigen_zkvm_amd.frpoly) against
tests/frpoly_ref.py: the schoolbook product, long division, the coset factors from their definition.  Exact integers mod r, no tolerance.
The last test reaches one quotient by two routes -- coefficients (poly_mul, divmod_zh) and the coset of twice the size (the existing
transforms, pointwise, divide_zh_coset) -- and asks for the same words from both, from the reference, and from the identity at a random point."""
import importlib
import random

import numpy as np
import pytest

import frpoly_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def fp():
    return importlib.import_module("eigen_zkvm_amd.frpoly")


@pytest.fixture(scope="module")
def g16():
    return importlib.import_module("eigen_zkvm_amd.groth16")


@pytest.fixture(scope="module")
def T(zk):
    return int(zk.lib().zk_frpoly_tile_elems())


def _mul_words(zk, fp, curve, a, b):
    """a b on the device -> the output's words"""
    r = ref.R[curve]
    da, db = zk.DevArray.from_host(ref.mont_words(a, r)), zk.DevArray.from_host(ref.mont_words(b, r))
    try:
        out = fp.poly_mul(da, db, curve)
        try:
            assert out.n == 4 * (len(a) + len(b) - 1)
            return out.to_host()
        finally:
            out.free()
    finally:
        da.free(); db.free()


@pytest.mark.parametrize("shape", ("1x1", "1x5", "2x3", "64x65", "TxT+1", "4097x4096"))
@pytest.mark.parametrize("curve", CURVES)
def test_poly_mul_against_the_schoolbook_product(zk, fp, T, curve, shape):
    r = ref.R[curve]
    na, nb = {"TxT+1": (T, T + 1)}.get(shape) or tuple(int(x) for x in shape.split("x"))
    rng = random.Random(0xD1 + len(curve) + na)
    a, b = [rng.randrange(r) for _ in range(na)], [rng.randrange(r) for _ in range(nb)]
    got = _mul_words(zk, fp, curve, a, b)
    assert np.array_equal(got, ref.mont_words(ref.poly_mul(a, b, r), r))
    assert np.array_equal(_mul_words(zk, fp, curve, b, a), got)                        # commutes, word for word


@pytest.mark.parametrize("curve", CURVES)
def test_poly_mul_edge_polynomials(fp, curve):
    r = ref.R[curve]
    rng = random.Random(0xD2 + len(curve))
    a = [rng.randrange(r) for _ in range(37)]
    assert fp.poly_mul([0] * 5, a, curve) == [0] * 41 and fp.poly_mul(a, [0], curve) == [0] * 37       # zero polynomials, leading zeros kept
    assert fp.poly_mul([0] * 3, [0] * 4, curve) == [0] * 6
    assert fp.poly_mul(a + [0, 0], [1, 0], curve) == a + [0, 0, 0]
    m1 = [r - 1] * 70
    assert fp.poly_mul(m1, m1, curve) == ref.poly_mul(m1, m1, r)                                         # every coefficient r - 1
    assert fp.poly_mul(m1, a, curve) == ref.poly_mul(m1, a, r)
    with pytest.raises(fp.ZkError, match="no coefficients"):
        fp.poly_mul([], a, curve)


@pytest.mark.parametrize("log_n", (0, 1, 6, 11))
@pytest.mark.parametrize("curve", CURVES)
def test_divmod_zh(fp, curve, log_n):
    r = ref.R[curve]
    N = 1 << log_n
    rng = random.Random(0xD3 + len(curve) + log_n)
    for n_p in sorted({N - 1, N // 2, N, N + 1, 3 * N - 1, 4 * N}):                    # below N, N, N + 1, 3N - 1, 4N
        p = [rng.randrange(r) for _ in range(n_p)]
        q, rem, bad = fp.divmod_zh(p, log_n, curve)
        want_q, want_rem = ref.divmod_zh(p, log_n, r)
        assert (q, rem) == (want_q, want_rem), n_p
        assert bad == sum(1 for x in want_rem if x) and len(rem) == N and len(q) == max(n_p - N, 0)
        assert fp.divmod_zh(p, log_n, curve, want_q=False) == (None, want_rem, bad)
        assert fp.divmod_zh(p, log_n, curve, want_rem=False) == (want_q, None, bad)
    a = [rng.randrange(r) for _ in range(2 * N + 3)]                                    # a (X^N - 1): p_i = a_(i-N) - a_i
    p = [((a[i - N] if i >= N else 0) - (a[i] if i < len(a) else 0)) % r for i in range(len(a) + N)]
    q, rem, bad = fp.divmod_zh(p, log_n, curve)
    assert bad == 0 and not any(rem) and q == a
    p[N // 2] = (p[N // 2] + 1) % r                                                     # one coefficient off: exactly one remainder coefficient
    q, rem, bad = fp.divmod_zh(p, log_n, curve)
    assert bad == 1 and rem[N // 2] == 1 and q == a


def test_divmod_zh_refuses_a_long_chain(zk, fp):
    d = zk.DevArray(4 * 4097, zero=True)
    try:
        with pytest.raises(fp.ZkError, match="ZK_FRPOLY_MAX_RATIO.*zk_kzg_bn254_divide_dev"):
            fp.divmod_zh(d, 0, "BN128")
        q, rem, bad = fp.divmod_zh([5] * 4096, 0, "BN128")                              # the longest chain that is taken
        assert bad == 1 and rem == [5 * 4096] and q == [5 * (4095 - j) for j in range(4095)]
    finally:
        d.free()


@pytest.mark.parametrize("logs", ((3, 3), (4, 2), (12, 10), (12, 12)))
@pytest.mark.parametrize("curve", CURVES)
def test_divide_zh_coset_against_the_definition(zk, fp, curve, logs):
    r = ref.R[curve]
    log_m, log_n = logs
    rng = random.Random(0xD4 + len(curve) + 16 * log_m + log_n)
    e = [rng.randrange(r) for _ in range(1 << log_m)]
    e[0] = 0; e[1] = r - 1
    f = ref.coset_factors(curve, log_m, log_n)
    want = [x * y % r for x, y in zip(e, f)]
    d = zk.DevArray.from_host(ref.mont_words(e, r))
    try:
        assert fp.divide_zh_coset(d, log_m, log_n, curve) is d
        assert np.array_equal(d.to_host(), ref.mont_words(want, r))
    finally:
        d.free()
    if log_m <= 4:
        assert fp.divide_zh_coset(e, log_m, log_n, curve) == want
    with pytest.raises(fp.ZkError, match="exceeds the domain"):
        fp.divide_zh_coset([1, 2], 1, 2, curve)


@pytest.mark.parametrize("k", (1, 6, 11))
@pytest.mark.parametrize("curve", CURVES)
def test_divide_zh_coset_is_the_division_step_of_the_groth16_quotient(zk, fp, g16, curve, k):
    """log_m == log_n: (a 1 - 0) / Z through zk_fr_<curve>_quotient_dev against the same four steps with divide_zh_coset in the middle"""
    r = ref.R[curve]
    n = 1 << k
    rng = random.Random(0xD5 + len(curve) + k)
    a = ref.mont_words([rng.randrange(r) for _ in range(n)], r)
    d1, d2 = zk.DevArray.from_host(a), zk.DevArray.from_host(a)
    ones, zeros = zk.DevArray.from_host(ref.mont_words([1] * n, r)), zk.DevArray(4 * n, zero=True)
    try:
        g16.fr_quotient(d1, ones, zeros, curve)
        g16.fr_ntt(d2, curve, inverse=True)
        g16.fr_ntt(d2, curve, coset=True)
        fp.divide_zh_coset(d2, k, k, curve)
        g16.fr_ntt(d2, curve, inverse=True, coset=True)
        assert np.array_equal(d2.to_host(), d1.to_host())
    finally:
        for d in (d1, d2, ones, zeros):
            d.free()


@pytest.mark.parametrize("curve", CURVES)
def test_two_routes_to_one_quotient(zk, fp, g16, curve):
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    r = ref.R[curve]
    k = 8
    N = 1 << k
    rng = random.Random(0xD6 + len(curve))
    a_ev, b_ev = [rng.randrange(r) for _ in range(N)], [rng.randrange(r) for _ in range(N)]
    c_ev = ref.pointwise("mul", a_ev, b_ev, r)

    def coeffs(ev):                                                                     # values on H_N -> coefficients, the existing inverse transform
        return kzg.from_mont(g16.fr_ntt(ref.mont_words(ev, r), curve, inverse=True), curve)
    a, b, c = coeffs(a_ev), coeffs(b_ev), coeffs(c_ev)
    # route one: coefficients
    ab = fp.poly_mul(a, b, curve)
    t = fp.pointwise("sub", ab, c + [0] * (N - 1), curve)
    q, rem, bad = fp.divmod_zh(t, k, curve)
    assert bad == 0 and not any(rem) and len(q) == N - 1
    # the reference
    want_t = [(x - y) % r for x, y in zip(ref.poly_mul(a, b, r), c + [0] * (N - 1))]
    want_q, want_rem = ref.divmod_zh(want_t, k, r)
    assert t == want_t and q == want_q and not any(want_rem)
    # route two: the coset of twice the size
    devs = [zk.DevArray.from_host(ref.mont_words(p + [0] * N, r)) for p in (a, b, c)]
    try:
        for d in devs:
            g16.fr_ntt(d, curve, coset=True)
        fp.pointwise("mul", devs[0], devs[1], curve, out=devs[0])
        fp.pointwise("sub", devs[0], devs[2], curve, out=devs[0])
        fp.divide_zh_coset(devs[0], k + 1, k, curve)
        g16.fr_ntt(devs[0], curve, inverse=True, coset=True)
        assert np.array_equal(devs[0].to_host(), ref.mont_words(q + [0] * (N + 1), r))   # the same q, word for word, zeros above it
    finally:
        for d in devs:
            d.free()
    # the identity at a random point, by the evaluation of the KZG layer
    z = rng.randrange(r)
    ev = lambda p: kzg.evaluate(p, z, curve)
    assert (ev(a) * ev(b) - ev(c)) % r == ev(q) * (pow(z, N, r) - 1) % r
