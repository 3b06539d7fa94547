"""Pointwise work, powers, the terms of a grand product and the grand product itself on the device (csrc/frpoly_impl.hip.h through
eigen_zkvm_amd.frpoly) against tests/frpoly_ref.py: exact integers mod r, no tolerance.  T = zk_frpoly_tile_elems(); lengths sit on both
sides of a tile border where a kernel is tiled, and past one block of 256 lanes where it is not.  The last tests build the grand product of
a permutation argument from these parts alone -- three columns, labels from `powers`, numerator and denominator from `terms` -- and check
that it closes exactly when the values respect the permutation."""
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
    import importlib
    return importlib.import_module("eigen_zkvm_amd.frpoly")


@pytest.fixture(scope="module")
def T(zk):
    return int(zk.lib().zk_frpoly_tile_elems())


@pytest.mark.parametrize("curve", CURVES)
def test_pointwise(zk, fp, curve):
    r = ref.R[curve]
    rng = random.Random(0xC1 + len(curve))
    edge = [0, 1, r - 1]
    a = [x for x in edge for _ in edge] + [rng.randrange(r) for _ in range(300)]        # every pair of 0 / 1 / r - 1, then random, past one block
    b = [y for _ in edge for y in edge] + [rng.randrange(r) for _ in range(300)]
    for op in ("mul", "add", "sub"):
        assert fp.pointwise(op, a, b, curve) == ref.pointwise(op, a, b, r), op
    assert fp.pointwise(fp.SUB, a, b, curve) == ref.pointwise("sub", a, b, r)
    n = len(a)
    for op in ("mul", "add", "sub"):                                                    # aliasing: the output is the first, the second, both operands
        want = ref.mont_words(ref.pointwise(op, a, b, r), r)
        for alias in ("a", "b"):
            da, db = zk.DevArray.from_host(ref.mont_words(a, r)), zk.DevArray.from_host(ref.mont_words(b, r))
            try:
                out = da if alias == "a" else db
                assert fp.pointwise(op, da, db, curve, out=out) is out
                assert np.array_equal(out.to_host(), want), (op, alias)
            finally:
                da.free(); db.free()
        da = zk.DevArray.from_host(ref.mont_words(a, r))
        try:
            fp.pointwise(op, da, da, curve, out=da)
            assert np.array_equal(da.to_host(), ref.mont_words(ref.pointwise(op, a, a, r), r)), op
        finally:
            da.free()
    with pytest.raises(fp.ZkError, match="unknown pointwise operation"):
        fp.pointwise(3, a, b, curve)
    assert fp.pointwise("mul", [], [], curve) == []


@pytest.mark.parametrize("curve", CURVES)
def test_powers(fp, T, curve):
    r = ref.R[curve]
    rng = random.Random(0xC2 + len(curve))
    w8 = ref.root_of_unity(curve, 3)
    for base in (0, 1, r - 1, w8, rng.randrange(r)):
        for scale in (1, rng.randrange(r)):
            for n in (1, 9, T + 3):                                                     # T + 3: across a tile border, exponents of 12 bits
                assert fp.powers(base, scale, n, curve) == ref.powers(base, scale, n, r), (base, scale, n)
    assert fp.powers(0, 5, 3, curve) == [5, 0, 0] and fp.powers(7, 0, 3, curve) == [0, 0, 0] and fp.powers(3, 1, 0, curve) == []
    got = fp.powers(w8, 1, 17, curve)
    assert got[8] == 1 and got[16] == 1 and got[4] == r - 1
    for bad in ((r, 1), (1, r)):
        with pytest.raises(fp.ZkError, match="is not below the scalar field's modulus"):
            fp.powers(bad[0], bad[1], 4, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_terms(fp, curve):
    r = ref.R[curve]
    rng = random.Random(0xC3 + len(curve))
    n = 259
    cols = [[rng.randrange(r) for _ in range(n)] for _ in range(16)]
    labs = [[rng.randrange(r) for _ in range(n)] for _ in range(16)]
    cols[0][:3] = [0, 1, r - 1]; labs[0][:3] = [r - 1, 0, 1]
    for k in (1, 3, 16):
        for beta, gamma in ((rng.randrange(r), rng.randrange(r)), (0, rng.randrange(r)), (rng.randrange(r), 0), (0, 0), (r - 1, r - 1)):
            assert fp.terms(cols[:k], labs[:k], beta, gamma, curve) == ref.terms(cols[:k], labs[:k], beta, gamma, r), (k, beta, gamma)
            assert fp.terms(cols[:k], None, beta, gamma, curve) == ref.terms(cols[:k], None, beta, gamma, r), (k, gamma)
    for k in (0, 17):
        with pytest.raises(fp.ZkError, match="a term takes 1 to 16"):
            fp.terms((cols + cols)[:k], None, 1, 1, curve)
    with pytest.raises(fp.ZkError, match="gamma is not below"):
        fp.terms(cols[:1], None, 1, r, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_grand_product(zk, fp, T, curve):
    r = ref.R[curve]
    rng = random.Random(0xC4 + len(curve))
    for n in (1, 65, T + 1, 2 * T + 1):
        num = [rng.randrange(1, r) for _ in range(n)]
        den = list(num); rng.shuffle(den)                                               # a permutation of each other: closes
        z, last = fp.grand_product(num, den, curve)
        assert last == 1 and (z, last) == ref.grand_product(num, den, r)
        num[n // 2] = (num[n // 2] + 1) % r or 1                                        # one element changed: it does not close ...
        z, last = fp.grand_product(num, den, curve)
        assert last != 1 and (z, last) == ref.grand_product(num, den, r)
        zz = z + [last]                                                                 # ... and the recurrence still holds row by row
        assert zz[0] == 1 and all(zz[i + 1] * den[i] % r == zz[i] * num[i] % r for i in range(n))
    assert fp.grand_product([], [], curve) == ([], 1)
    # z may be the numerator's own buffer
    n = T + 1
    num = [rng.randrange(1, r) for _ in range(n)]; den = [rng.randrange(1, r) for _ in range(n)]
    dn, dd = zk.DevArray.from_host(ref.mont_words(num, r)), zk.DevArray.from_host(ref.mont_words(den, r))
    try:
        z, last = fp.grand_product(dn, dd, curve, out=dn)
        want_z, want_last = ref.grand_product(num, den, r)
        assert z is dn and last == want_last and np.array_equal(dn.to_host(), ref.mont_words(want_z, r))
    finally:
        dn.free(); dd.free()


@pytest.mark.parametrize("curve", CURVES)
def test_grand_product_refuses_a_zero_denominator(zk, fp, T, curve):
    """at row T (and again at a later row: the first is named), with z left as it was"""
    r = ref.R[curve]
    rng = random.Random(0xC5 + len(curve))
    n = 2 * T + 5
    num = [rng.randrange(1, r) for _ in range(n)]; den = [rng.randrange(1, r) for _ in range(n)]
    den[T] = 0; den[T + 70] = 0
    mark = ref.mont_words([rng.randrange(r) for _ in range(n)], r)
    dn, dd, dz = zk.DevArray.from_host(ref.mont_words(num, r)), zk.DevArray.from_host(ref.mont_words(den, r)), zk.DevArray.from_host(mark)
    try:
        with pytest.raises(fp.ZkError, match=r"the denominator of row %d is zero \(2 zero denominators" % T):
            fp.grand_product(dn, dd, curve, out=dz)
        assert np.array_equal(dz.to_host(), mark)
    finally:
        dn.free(); dd.free(); dz.free()


def _cycles_of(perm):
    seen, out = [False] * len(perm), []
    for s in range(len(perm)):
        if not seen[s]:
            c, j = [], s
            while not seen[j]:
                seen[j] = True; c.append(j); j = perm[j]
            out.append(c)
    return out


@pytest.mark.parametrize("which", ("64", "T+1"))
@pytest.mark.parametrize("curve", CURVES)
def test_the_shape_of_a_permutation_argument(fp, T, curve, which):
    """3 columns x n rows; the values are constant on the cycles of a random permutation sigma of the 3n cells; the label of cell (c, i)
    is (c + 1) w^i.  num = terms(cols, ids), den = terms(cols, sigma labels): the product closes; with one cell changed it does not."""
    r = ref.R[curve]
    n = 64 if which == "64" else 1 << T.bit_length()                                   # T + 1 rounded up to the domain's power of two
    assert n >= (64 if which == "64" else T + 1) and n & (n - 1) == 0
    rng = random.Random(0xC6 + len(curve) + n)
    w = ref.root_of_unity(curve, n.bit_length() - 1)
    ids = [fp.powers(w, scale, n, curve) for scale in (1, 2, 3)]
    flat = [x for col in ids for x in col]
    assert len(set(flat)) == 3 * n                                                      # the 3n labels are distinct
    assert ids[1][:5] == ref.powers(w, 2, 5, r)
    sigma = list(range(3 * n)); rng.shuffle(sigma)
    vals = [0] * (3 * n)
    for cyc in _cycles_of(sigma):
        x = rng.randrange(r)
        for cell in cyc:
            vals[cell] = x
    cols = [vals[c * n:(c + 1) * n] for c in range(3)]
    sig = [[flat[sigma[c * n + i]] for i in range(n)] for c in range(3)]
    beta, gamma = rng.randrange(1, r), rng.randrange(r)
    num, den = fp.terms(cols, ids, beta, gamma, curve), fp.terms(cols, sig, beta, gamma, curve)
    assert num[:4] == ref.terms([c[:4] for c in cols], [c[:4] for c in ids], beta, gamma, r)
    z, last = fp.grand_product(num, den, curve)
    assert last == 1 and z[0] == 1
    row = n // 3
    assert z[row + 1] * den[row] % r == z[row] * num[row] % r
    cell = next(c for c in range(3 * n) if sigma[c] != c)                               # a cell that sigma ties to another one
    cols[cell // n][cell % n] = (cols[cell // n][cell % n] + 1) % r
    num, den = fp.terms(cols, ids, beta, gamma, curve), fp.terms(cols, sig, beta, gamma, curve)
    assert fp.grand_product(num, den, curve)[1] != 1
