"""The copy-constraint wiring kernels on their own (zk_c12_sigma_dev: the S identity, the stable radix sort, the rotation
of every run) against the serial chain of swaps of plonk_setup.rs:665-728 as restated in tests/c12_setup_ref.py: exact."""
import importlib, random
import numpy as np
import pytest

import c12_setup_ref as REF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)
    return importlib.import_module("eigen_zkvm_amd.compressor12")


def check(dev, s_map, n_bits):
    got = dev.sigma(s_map, n_bits).to_host().reshape(1 << n_bits, 12)
    want = np.array(REF.sigma([list(map(int, r)) for r in s_map], n_bits), dtype=np.uint64)
    assert np.array_equal(got, want)
    return got


def identity(n_bits):
    return np.array(REF.sigma([], n_bits), dtype=np.uint64)


def test_small_shapes(zk, dev):
    """n_bits 4, n_used 16: nothing moves / one signal in 2 cells / one signal in 3 cells of one row / zeros scattered"""
    base = np.arange(1, 16 * 12 + 1, dtype=np.uint32).reshape(16, 12)
    assert np.array_equal(check(dev, base, 4), identity(4))                       # every cell distinct
    m = base.copy(); m[11, 7] = m[2, 3]
    got = check(dev, m, 4); ident = identity(4)
    assert got[2, 3] == ident[11, 7] and got[11, 7] == ident[2, 3] and (got != ident).sum() == 2
    m = base.copy(); m[5, 1] = m[5, 4] = m[5, 10] = 999
    got = check(dev, m, 4)
    assert (got[5, 4], got[5, 10], got[5, 1]) == (ident[5, 1], ident[5, 4], ident[5, 10])   # the rotation, in walk order
    rng = random.Random(3)
    m = np.array([[rng.choice([0, 0, rng.randrange(1, 30)]) for _ in range(12)] for _ in range(16)], dtype=np.uint32)
    check(dev, m, 4)


def test_long_run_and_partial_use(zk, dev):
    """n_used 1000 < N = 1024: one signal in 3000 cells (longer than any workgroup and tile), the rest from a pool of 200"""
    rng = random.Random(5)
    cells = [rng.randrange(1, 201) for _ in range(12000)]
    for p in rng.sample(range(12000), 3000): cells[p] = 7777
    got = check(dev, np.array(cells, dtype=np.uint32).reshape(1000, 12), 10)
    assert np.array_equal(got[1000:], identity(10)[1000:])                        # rows >= n_used keep the identity


def test_every_radix_digit_and_stability(zk, dev):
    """ids that differ only in one radix digit each, mixed with small ones: a pass that mis-orders or is not stable breaks
    the rotation order"""
    rng = random.Random(7)
    ids = [1, 1 << 8, 1 << 16, 1 << 24, 0xFFFFFFFF, 2, 3, 0x01010101, 0xFF00FF00, 0x00FF00FF]
    m = np.array([[rng.choice(ids) for _ in range(12)] for _ in range(200)], dtype=np.uint32)
    check(dev, m, 8)


@pytest.mark.parametrize("n_used,n_bits", [(64, 6), (1, 5), (0, 3)])
def test_edges(zk, dev, n_used, n_bits):
    """n_used == N, n_used == 1, no row at all"""
    rng = random.Random(n_used)
    check(dev, np.array([[rng.randrange(0, 20) for _ in range(12)] for _ in range(n_used)], dtype=np.uint32).reshape(n_used, 12), n_bits)


def test_all_zero_map(zk, dev):
    assert np.array_equal(check(dev, np.zeros((40, 12), np.uint32), 6), identity(6))


def test_other_columns_are_left_alone(zk, dev):
    """S at column offset 2 of a 17-column matrix: the 12 columns are written, the other 5 keep what they held"""
    rng = random.Random(11)
    m = np.array([[rng.randrange(0, 9) for _ in range(12)] for _ in range(30)], dtype=np.uint32)
    out = zk.DevArray.from_host(np.full(32 * 17, 5, np.uint64))
    got = dev.sigma(m, 5, n_const=17, col0=2, out=out).to_host().reshape(32, 17)
    assert np.array_equal(got[:, 2:14], np.array(REF.sigma(m.tolist(), 5), dtype=np.uint64))
    assert (got[:, :2] == 5).all() and (got[:, 14:] == 5).all()


def test_wide_wire_id_is_a_named_error(zk, dev):
    """a custom-gate signal >= 2^32 through the handle: refused when the circuit is read, before anything is launched"""
    import c12_setup_circuits as CC
    sig = list(range(1, 13)); sig[4] = 1 << 32
    b = REF.write_r1cs(20, 0, 2, 17, [([(1, 1)], [(2, 1)], [(3, 1)])], list(CC.ALL_TEMPLATES), [(0, sig)])
    with pytest.raises(zk.ZkError, match="does not fit 32 bits"):
        dev.Compressor12Setup.from_r1cs(b)
    with pytest.raises(zk.ZkError, match="more rows than the trace"):
        dev.sigma(np.ones((9, 12), np.uint32), 3)
