"""Running products and batch inversion on the device (csrc/frpoly_impl.hip.h through zk_fr_<curve>_prefix_product_dev and
zk_fr_<curve>_batch_inverse_dev) against tests/frpoly_ref.py, word for word: every output vector is compared as the Montgomery words of the
canonical representative, so a value that is right mod r but not below r fails.  There is no tolerance.
Lengths come from the exported constants, T = zk_frpoly_tile_elems() elements per workgroup (8 per lane) and S = zk_frpoly_span() tile
aggregates per step of the combining workgroup: 1, 2, 3: lanes without a full run; 63 .. 65: the runs of one wave; T - 1 .. 3T - 1: one, two
and three tiles with the border inside a lane's run; T S: exactly one step of the combining workgroup (run twice: the second call's scratch is
the first call's, recycled); T S + T + 1: the smallest length at which it takes a second step.
One random vector per (curve, length) is made once and shared, with its inverses by pow(x, -1, r) (inversion is element by element, so a
vector with one element zeroed reuses them)."""
import functools
import random

import numpy as np
import pytest

import frpoly_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")
LENGTHS = ("1", "2", "3", "63", "64", "65", "T-1", "T", "T+1", "2T+1", "3T-1", "TS", "TS+T+1")
PATTERNS = ("random", "ones", "minus_ones", "zero@0", "zero@7", "zero@8", "zero@T-1", "zero@T", "zero@n-1", "zeros")


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def fp():
    import importlib
    return importlib.import_module("eigen_zkvm_amd.frpoly")


@pytest.fixture(scope="module")
def consts(zk):
    return int(zk.lib().zk_frpoly_tile_elems()), int(zk.lib().zk_frpoly_span())


def _length(name, T, S):
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "3T-1": 3 * T - 1, "TS": T * S, "TS+T+1": T * S + T + 1}.get(name) or int(name)


@functools.lru_cache(maxsize=4)
def _base(curve, n):
    """the shared random vector of a (curve, length): non-zero elements, their words, the words of their inverses.  Every element is a
    uniform draw, with repetition, from a pool of 4099 random field elements, so that the 2^20 inversions by pow(x, -1, r) of a long vector
    are 4099: inversion is element by element, and no two running products are alike for it."""
    r = ref.R[curve]
    rng = random.Random(0x5CA0 + 31 * n + len(curve))
    pool = [rng.randrange(1, r) for _ in range(4099)]
    pool_inv = ref.inverses(pool, r)[0]
    pick = [rng.randrange(4099) for _ in range(n)]
    v = [pool[i] for i in pick]
    return v, ref.mont_words(v, r), ref.mont_words([pool_inv[i] for i in pick], r)


def _vector(curve, n, pattern, T):
    """-> (elements, their words, the words of the inverses with zeros left zero), or None when the pattern's position is outside the vector"""
    r = ref.R[curve]
    if pattern in ("ones", "minus_ones", "zeros"):
        x = {"ones": 1, "minus_ones": r - 1, "zeros": 0}[pattern]
        w = np.tile(ref.mont_words([x], r), n)                           # 1 / 1 = 1, 1 / (r - 1) = r - 1, and a zero stays zero
        assert x * x % r == (1 if x else 0) and ref.inverses([x], r)[0] == [x]
        return [x] * n, w, w
    v, vw, iw = _base(curve, n)
    if pattern == "random":
        return v, vw, iw
    pos = {"0": 0, "7": 7, "8": 8, "T-1": T - 1, "T": T, "n-1": n - 1}[pattern.split("@")[1]]
    if pos >= n:
        return None
    v, vw, iw = list(v), vw.copy(), iw.copy()
    v[pos] = 0; vw[4 * pos:4 * pos + 4] = 0; iw[4 * pos:4 * pos + 4] = 0
    return v, vw, iw


def _words(d, n):
    return d.to_host()[:4 * n]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_products_and_inverses(zk, fp, consts, curve, length, pattern):
    T, S = consts
    n = _length(length, T, S)
    made = _vector(curve, n, pattern, T)
    if made is None:
        return                                                           # the zero's position lies past this length: nothing to run
    v, v_words, want_inv = made
    r = ref.R[curve]
    assert np.array_equal(want_inv[:4 * 64], ref.mont_words(ref.inverses(v[:64], r)[0], r))
    excl, total = ref.prefix_products(v, r)
    want_excl = ref.mont_words(excl, r)
    want_incl = np.concatenate([want_excl[4:], ref.mont_words([total], r)])      # inclusive[i] = exclusive[i + 1]
    assert ref.prefix_products(v[:70], r, inclusive=True)[0] == excl[1:71] + ([total] if n <= 70 else [])
    zeros = [i for i, x in enumerate(v) if x == 0]
    d = zk.DevArray.from_host(v_words)
    o = zk.DevArray(4 * n)
    try:
        for _ in range(2 if length == "TS" else 1):
            got, t = fp.prefix_product(d, curve, out=o)
            assert got is o and t == total
            assert np.array_equal(_words(o, n), want_excl)
            _, t = fp.prefix_product(d, curve, inclusive=True, out=o)
            assert t == total and np.array_equal(_words(o, n), want_incl)
            assert fp.prefix_product(d, curve, total_only=True) == (None, total)
            _, nz, first = fp.batch_inverse(d, curve, out=o)
            assert (nz, first) == (len(zeros), zeros[0] if zeros else None)
            assert np.array_equal(_words(o, n), want_inv)
        # in place, both entry points: the input is its own output
        _, t = fp.prefix_product(d, curve, inclusive=True, out=d)
        assert t == total and np.array_equal(_words(d, n), want_incl)
        fp.batch_inverse(o, curve, out=o)                                # o holds the inverses: back to the elements, zeros where they were
        assert np.array_equal(_words(o, n), v_words)
    finally:
        d.free(); o.free()


@pytest.mark.parametrize("curve", CURVES)
def test_outputs_are_below_r_as_words(fp, consts, curve):
    """the plain integers the output words spell, not their residues: each is below r"""
    T, _ = consts
    r = ref.R[curve]
    rng = random.Random(0xB1 + len(curve))
    v = [rng.randrange(r) for _ in range(T + 65)]
    d = fp.DevArray.from_host(ref.mont_words(v, r))
    try:
        for out in (fp.prefix_product(d, curve)[0], fp.prefix_product(d, curve, inclusive=True)[0], fp.batch_inverse(d, curve)[0]):
            try:
                assert max(ref.words_ints(out.to_host())) < r
            finally:
                out.free()
    finally:
        d.free()


@pytest.mark.parametrize("curve", CURVES)
def test_integers_in_integers_out_and_the_empty_vector(fp, curve):
    r = ref.R[curve]
    rng = random.Random(0xB2 + len(curve))
    v = [rng.randrange(r) for _ in range(67)]
    assert fp.prefix_product(v, curve) == ref.prefix_products(v, r)
    assert fp.prefix_product(v, curve, inclusive=True) == ref.prefix_products(v, r, inclusive=True)
    assert fp.batch_inverse(v, curve) == ref.inverses(v, r)
    assert fp.prefix_product([], curve) == ([], 1)
    assert fp.prefix_product([], curve, total_only=True) == (None, 1)
    assert fp.batch_inverse([], curve) == ([], 0, None)


@pytest.mark.parametrize("curve", CURVES)
def test_a_vector_the_transform_has_just_written(zk, fp, curve):
    """the words zk_fr_<curve>_ntt_dev leaves, fed in without conversion"""
    import importlib
    g16 = importlib.import_module("eigen_zkvm_amd.groth16")
    r = ref.R[curve]
    rng = random.Random(0xB3 + len(curve))
    d = zk.DevArray.from_host(ref.mont_words([rng.randrange(r) for _ in range(128)], r))
    try:
        g16.fr_ntt(d, curve)
        rinv = pow(1 << 256, -1, r)
        v = [w * rinv % r for w in ref.words_ints(d.to_host())]
        out, total = fp.prefix_product(d, curve)
        try:
            want, want_total = ref.prefix_products(v, r)
            assert total == want_total and np.array_equal(out.to_host(), ref.mont_words(want, r))
        finally:
            out.free()
        out, nz, first = fp.batch_inverse(d, curve)
        try:
            want, want_nz, want_first = ref.inverses(v, r)
            assert (nz, first) == (want_nz, want_first) and np.array_equal(out.to_host(), ref.mont_words(want, r))
        finally:
            out.free()
    finally:
        d.free()
