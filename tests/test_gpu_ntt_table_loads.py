"""The NTT pass with every table load of a tile requested at kernel entry: each transform path against the CPU oracle, bit for bit.

What moved (eigen-zkvm_amd/csrc/ntt.hip): the 16 entries of w256 a 16-lane row needs in sub-step A, and -- where the row shares p -- its
16 entries of the direct inter-pass table, are fetched one per lane and handed round by a DPP row broadcast; where p differs inside a
row the per-lane loads go out in front of the barrier; the two-level look-ups of a first pass (L > 2^16) and of an extension's scaled
last pass go out in front of the data loads.  The cases are the smallest shapes at which each of these can go wrong:

  (9, 19)            s n_pols = 19: not the one-column order, p changes inside a row -> the per-lane form
  (10, 16)           s n_pols = 16: p shared by a row but not by the tile
  (10, 3) (12, 1) (16, 1)   one-column thread order on the direct table
  (8, 3)             a single pass with a partly dead row: the w256 broadcast runs with dead lanes
  (9, 7) (12, 7)     whole dead rows in the last tile
  (13, 1)            <4,3> + <3,3>, two sub-transforms per thread in sub-step A
  (17, 1) (20, 1)    two-level look-up at entry, a shift-twiddle middle pass
  (23, 1)            the smallest size whose first pass is <4,4> one-column on the chain and whose middle pass is <4,4> on the
                     row-shared table (64 MiB; the oracle takes a few seconds for both directions)
  extensions 8 -> 9, 12 -> 14, 16 -> 17 with 1 and 3 columns: the scaled last pass's look-up at entry; the zero-padded first
                     forward pass"""
import numpy as np
import pytest

P = 0xFFFFFFFF00000001
CASES = [(9, 19), (10, 16), (10, 3), (12, 1), (16, 1), (8, 3), (9, 7), (12, 7), (13, 1), (17, 1), (20, 1), (23, 1)]


@pytest.fixture(scope="module")
def gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)
    return zk


def _matrix(n, n_pols, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, P, size=(n, n_pols), dtype=np.uint64)
    x[:4, 0] = [0, 1, P - 1, 0xFFFFFFFF][:min(4, n)]
    if n_pols > 1:
        x[:, 1] = P - 1
    return np.ascontiguousarray(x)


@pytest.mark.gpu
@pytest.mark.parametrize("nbits,n_pols", CASES, ids=["%d-%d" % c for c in CASES])
def test_transform_matches_oracle(gpu, orc, nbits, n_pols):
    n = 1 << nbits
    cols = _matrix(n, n_pols, 32000 + 32 * nbits + n_pols)
    x = cols.reshape(-1)
    X = gpu.fft(x, n_pols, nbits).reshape(n, n_pols)
    Xi = gpu.ifft(x, n_pols, nbits).reshape(n, n_pols)
    for c in range(n_pols):
        col = np.ascontiguousarray(cols[:, c])
        assert np.array_equal(X[:, c], orc.ntt_blocked(col, nbits, False)), f"forward, column {c}"
        assert np.array_equal(Xi[:, c], orc.ntt_blocked(col, nbits, True)), f"inverse, column {c}"


@pytest.mark.gpu
@pytest.mark.parametrize("n_pols", [1, 3])
@pytest.mark.parametrize("nbits,ext", [(8, 9), (12, 14), (16, 17)])
def test_extension_matches_oracle(gpu, orc, nbits, ext, n_pols):
    x = _matrix(1 << nbits, n_pols, 32500 + 32 * ext + n_pols).reshape(-1)
    assert np.array_equal(gpu.interpolate(x, n_pols, nbits, ext), orc.lde(x, n_pols, nbits, ext))
