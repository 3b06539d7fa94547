"""The factored output factors of an NTT pass (A_ka * S_kb: S once per workgroup through LDS, no running product) and the 32-bit lane
addressing, on every path that uses them, against the CPU oracle.  Bit-exact everywhere (integer field).

The plan splits nbits evenly into passes of at most 8 bits:
  22 -> 8 + 7 + 7, 23 -> 8 + 8 + 7: the smallest sizes whose first pass is the <4,4> tile in its one-column form with the table factors
        (L > 2^16); 23 also has a <4,4> middle pass on the direct table;
  17 -> 6 + 6 + 5: first pass <3,3>, 64 lanes per tile; three columns make the tiles ragged and take the division branch; sixteen columns
        switch the one-column thread order off;
  extension 16 -> 17 and 17 -> 19: the last pass of the inverse transform takes its c g^row from the same factoring, and the first forward
        pass reads a zero-padded input.
Inputs: seeded random canonical words, all p - 1, all zero -- as whole inputs for one column, as columns beside each other otherwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)


def _input(kind, n, n_pols, seed):
    rng = np.random.default_rng(seed)
    if n_pols == 1:
        if kind == "random":
            x = rng.integers(0, P, size=n, dtype=np.uint64)
            x[:4] = [0, 1, P - 1, 0xFFFFFFFF]
            return x
        return np.full(n, P - 1 if kind == "allp1" else 0, np.uint64)
    x = rng.integers(0, P, size=(n, n_pols), dtype=np.uint64)      # several columns: column 0 all p - 1, column 1 all zero, the rest random
    x[:, 0] = P - 1
    x[:, 1] = 0
    return np.ascontiguousarray(x).reshape(-1)


@pytest.mark.parametrize("kind", ["random", "allp1", "zero"])
@pytest.mark.parametrize("nbits", [22, 23])
def test_one_column_first_pass_matches_oracle(zk, orc, nbits, kind):
    x = _input(kind, 1 << nbits, 1, 8100 + nbits)
    assert np.array_equal(zk.fft(x, 1, nbits), orc.ntt_blocked(x, nbits, False)), "forward"
    assert np.array_equal(zk.ifft(x, 1, nbits), orc.ntt_blocked(x, nbits, True)), "inverse"


@pytest.mark.parametrize("kind", ["random", "allp1", "zero"])
def test_narrow_one_column_matches_oracle(zk, orc, kind):
    x = _input(kind, 1 << 17, 1, 8217)
    assert np.array_equal(zk.fft(x, 1, 17), orc.ntt_blocked(x, 17, False)), "forward"
    assert np.array_equal(zk.ifft(x, 1, 17), orc.ntt_blocked(x, 17, True)), "inverse"


@pytest.mark.parametrize("n_pols", [3, 16], ids=["narrow3", "wide16"])
def test_several_columns_match_oracle(zk, orc, n_pols):
    """each column against the one-column oracle"""
    n = 1 << 17
    x = _input("columns", n, n_pols, 8300 + n_pols)
    X = zk.fft(x, n_pols, 17).reshape(n, n_pols)
    Xi = zk.ifft(x, n_pols, 17).reshape(n, n_pols)
    cols = x.reshape(n, n_pols)
    for c in range(n_pols):
        col = np.ascontiguousarray(cols[:, c])
        assert np.array_equal(X[:, c], orc.ntt_blocked(col, 17, False)), f"forward, column {c}"
        assert np.array_equal(Xi[:, c], orc.ntt_blocked(col, 17, True)), f"inverse, column {c}"


@pytest.mark.parametrize("kind", ["random", "allp1", "zero"])
@pytest.mark.parametrize("nbits,ext", [(16, 17), (17, 19)])
def test_extension_one_column_matches_oracle(zk, orc, nbits, ext, kind):
    x = _input(kind, 1 << nbits, 1, 8400 + ext)
    assert np.array_equal(zk.interpolate(x, 1, nbits, ext), orc.lde(x, 1, nbits, ext))


@pytest.mark.parametrize("nbits,ext", [(16, 17), (17, 19)])
def test_extension_three_columns_matches_oracle(zk, orc, nbits, ext):
    x = _input("columns", 1 << nbits, 3, 8500 + ext)
    assert np.array_equal(zk.interpolate(x, 3, nbits, ext), orc.lde(x, 3, nbits, ext))


def test_round_trip_2p22(zk):
    x = _input("random", 1 << 22, 1, 8622)
    assert np.array_equal(zk.ifft(zk.fft(x, 1, 22), 1, 22), x)
