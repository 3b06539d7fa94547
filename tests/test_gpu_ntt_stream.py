"""The NTT pass with non-temporal data loads: every transform path against the CPU oracle, bit for bit (integer field).

Sizes: the plan splits nbits evenly into passes of at most 8 bits, so 4 ... 8 are one pass, 9 ... 16 two, 17 ... 24 three; 4, 5, 8, 9, 12, 13,
16, 17 and 20 take every tile shape, the direct inter-pass table (L <= 2^16) and the two-level table (L > 2^16: the first pass of 17 and
20), and both thread orders of a first pass.  Columns: 1, 3 (ragged last tiles, whose loads of absent words are redirected to word 0, and
the 32-bit division) and 16 (the one-column thread order is off).  Extensions 8 -> 9, 12 -> 14, 16 -> 17 run the scaled last pass and a
zero-padded first forward pass.  Grids of 1, 7, 8, 9, 15 and 17 workgroups surround the number of XCDs the workgroups are dealt to: the
sizes at which a block -> tile remapping (tools/experiments/ntt_stream_rejected.patch, which adds its host check to this file) can go
wrong, kept as cases of the shipped identity order."""
import numpy as np
import pytest

P = 0xFFFFFFFF00000001
NTT_TILE = 4096
SIZES = [4, 5, 8, 9, 12, 13, 16, 17, 20]


def plan(nbits):
    """radices of the passes of a 2^nbits transform, as ntt.hip's plan()"""
    if nbits < 4:
        return []
    np_ = (nbits + 7) // 8
    base, extra = divmod(nbits, np_)
    return [base + (1 if i < extra else 0) for i in range(np_)]


def grid_sizes(nbits, n_pols):
    """workgroups of each pass: ceil((N >> logr) * n_pols / C), C = NTT_TILE >> logr lanes per tile"""
    return [-(-((1 << nbits >> logr) * n_pols) // (NTT_TILE >> logr)) for logr in plan(nbits)]


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


def _check_transform(zk, orc, nbits, n_pols, seed):
    n = 1 << nbits
    cols = _matrix(n, n_pols, seed)
    x = cols.reshape(-1)
    X = zk.fft(x, n_pols, nbits).reshape(n, n_pols)
    Xi = zk.ifft(x, n_pols, nbits).reshape(n, n_pols)
    for c in range(n_pols):
        col = np.ascontiguousarray(cols[:, c])
        assert np.array_equal(X[:, c], orc.ntt_blocked(col, nbits, False)), f"forward, column {c}"
        assert np.array_equal(Xi[:, c], orc.ntt_blocked(col, nbits, True)), f"inverse, column {c}"


@pytest.mark.gpu
@pytest.mark.parametrize("n_pols", [1, 3, 16])
@pytest.mark.parametrize("nbits", SIZES)
def test_transform_matches_oracle(gpu, orc, nbits, n_pols):
    assert gpu.lib().zk_gl_ntt_passes(nbits) == len(plan(nbits)) == (nbits + 7) // 8
    _check_transform(gpu, orc, nbits, n_pols, 9000 + 32 * nbits + n_pols)


@pytest.mark.gpu
@pytest.mark.parametrize("n_pols", [1, 3])
@pytest.mark.parametrize("nbits,ext", [(8, 9), (12, 14), (16, 17)])
def test_extension_matches_oracle(gpu, orc, nbits, ext, n_pols):
    x = _matrix(1 << nbits, n_pols, 9500 + 32 * ext + n_pols).reshape(-1)
    assert np.array_equal(gpu.interpolate(x, n_pols, nbits, ext), orc.lde(x, n_pols, nbits, ext))


# (nbits, n_pols) -> workgroups of every pass of the transform
GRIDS = [(12, 1, 1), (12, 7, 7), (15, 1, 8), (12, 9, 9), (12, 15, 15), (12, 17, 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("nbits,n_pols,blocks", GRIDS, ids=["blocks%d" % g[2] for g in GRIDS])
def test_grid_sizes_around_the_tile_map(gpu, orc, nbits, n_pols, blocks):
    assert gpu.lib().zk_gl_ntt_passes(nbits) == len(plan(nbits)), "the plan changed: recompute the grid sizes of this test"
    assert grid_sizes(nbits, n_pols) == [blocks] * len(plan(nbits))
    _check_transform(gpu, orc, nbits, n_pols, 9700 + blocks)

