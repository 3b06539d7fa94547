"""The NTT passes' lean field arithmetic: the twiddle product gl::mul_tw and its non-canonical form against Python integers, and every
code path of the transform that uses them against the CPU oracle.  Bit-exact everywhere (integer field)."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)


def _probe(zk, a, b):
    fn = zk.lib().zk_gl_twmul_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    a = np.ascontiguousarray(a, np.uint64); b = np.ascontiguousarray(b, np.uint64)
    out = np.empty(3 * len(a), np.uint64)
    rc = fn(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(a))
    assert rc == 0, zk.lib().zk_last_error()
    return out.reshape(3, len(a))


def _operand_pairs(n, top):
    """n pairs below `top`: the edge values against each other, the pairs where a borrow or a fix-up can go wrong, then seeded random"""
    edge = [0, 1, P - 1, 0xFFFFFFFF, 1 << 32, (1 << 64) - (1 << 32), P - (1 << 32), 2, P - 2, (1 << 32) + 1, 0xFFFFFFFE00000001]
    if top > P:
        edge += [M64, M64 - 1, P, P + 1, 1 << 63]
    pairs = [(x, y) for x in edge for y in edge]
    rng = np.random.default_rng(20240)
    for _ in range(64):
        # r2 = 2^32 - 1 and r3 = 0: a b = (2^32 - 1) 2^64 + lo with lo < 2^64 (b solved for from a random a; the excess is below a < 2^62)
        a = int(rng.integers(1 << 33, 1 << 62))
        b = ((0xFFFFFFFF << 64) + int(rng.integers(0, 1 << 63))) // a + 1
        assert a < top and b < top and ((a * b) >> 64) == 0xFFFFFFFF
        pairs.append((a, b))
        # r3 > w1:w0: both low halves zero, so a b = a1 b1 2^64 has w1:w0 = 0 and r3 = a1 b1 >> 32 > 0
        a1, b1 = int(rng.integers(1 << 16, 0xFFFFFFFF)), int(rng.integers(1 << 16, 0xFFFFFFFF))
        assert (a1 * b1) >> 32 > 0
        pairs.append((a1 << 32, b1 << 32))
    m = n - len(pairs)
    if top > P:
        ra = rng.integers(0, 1 << 64, size=m, dtype=np.uint64, endpoint=False); rb = rng.integers(0, 1 << 64, size=m, dtype=np.uint64, endpoint=False)
    else:
        ra = rng.integers(0, P, size=m, dtype=np.uint64); rb = rng.integers(0, P, size=m, dtype=np.uint64)
    a = np.concatenate([np.array([p[0] for p in pairs], np.uint64), ra])
    b = np.concatenate([np.array([p[1] for p in pairs], np.uint64), rb])
    return a, b


def _expect(a, b):
    ao, bo = a.astype(object), b.astype(object)
    ab = (ao * bo) % P
    return ab.astype(np.uint64), ((ab * bo % P) * bo % P).astype(np.uint64)


@pytest.mark.parametrize("top", [P, 1 << 64], ids=["canonical", "any_u64"])
def test_twiddle_product_matches_python_integers(zk, top):
    """2^16 pairs.  Row 0: mul_tw; row 1: mul_tw_nc canonicalised once; row 2: two non-canonical products multiplied (a b^3)."""
    a, b = _operand_pairs(1 << 16, top)
    got = _probe(zk, a, b)
    ab, ab3 = _expect(a, b)
    assert np.array_equal(got[0], ab), "mul_tw"
    assert np.array_equal(got[1], ab), "mul_tw_nc, canonicalised"
    assert np.array_equal(got[2], ab3), "mul_tw of two mul_tw_nc results"


def _cols(rng, n, n_pols):
    """column 0 all p - 1, the last column seeded random with the edge values sprinkled in; one column alone is the random one"""
    x = rng.integers(0, P, size=(n, n_pols), dtype=np.uint64)
    x[:4, -1] = [0, 1, P - 1, 0xFFFFFFFF]
    if n_pols > 1:
        x[:, 0] = P - 1
    return np.ascontiguousarray(x).reshape(-1)


# The plan splits nbits evenly into passes of at most 8 bits.  12: two 6-bit passes, shift twiddles; 16: two 8-bit passes, the first-pass
# chain and then the last pass; 17: three passes (6 + 6 + 5), the middle one through the direct table; 20: three passes (7 + 7 + 6) --
# with three columns the first pass is the row-major form at s n_pols = 3 and its last tile is ragged.  n_pols = 1 is a seeded random
# column, n_pols > 1 an all-(p - 1) column beside random ones; "allp1" is the all-(p - 1) column alone.
@pytest.mark.parametrize("nbits,n_pols,allp1", [(12, 1, False), (12, 1, True), (16, 1, False), (16, 1, True), (17, 1, False), (17, 2, False),
                                                (20, 1, False), (20, 3, False)])
def test_transform_paths_match_oracle(zk, orc, nbits, n_pols, allp1):
    rng = np.random.default_rng(7000 + nbits * 13 + n_pols)
    x = np.full(1 << nbits, P - 1, np.uint64) if allp1 else _cols(rng, 1 << nbits, n_pols)
    X = zk.fft(x, n_pols, nbits)
    assert np.array_equal(X, orc.ntt(x, n_pols, nbits, False)), "forward"
    assert np.array_equal(zk.ifft(x, n_pols, nbits), orc.ntt(x, n_pols, nbits, True)), "inverse"
    assert np.array_equal(zk.ifft(X, n_pols, nbits), x), "round trip"


def test_shift_twiddles_match_python_integers(zk):
    """gl::mul_pow2<E>, every 0 <= E < 96.  The operands include what the 32 < E < 64 branch can get wrong: multiples of 2^(64 - r)
    (E = 32 + r), for which both low words of x 2^r vanish and the result is p - t2 through the second step of the fold."""
    xs = [0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - (1 << 32), P - (1 << 32)]
    xs += [1 << k for k in range(64)]
    for r in range(1, 32):
        xs += [k << (64 - r) for k in {1, 2, 3, (1 << r) - 1, (1 << r) // 2, (1 << r) // 3} if 0 < k < (1 << r)]
        xs += [(k << (64 - r)) + 1 for k in (1, (1 << r) - 1)] + [(1 << (32 - r)) * 5, ((1 << r) - 1) << (32 - r)]
    xs = sorted({v for v in xs if v < P})
    rng = np.random.default_rng(4242)
    x = np.concatenate([np.array(xs, np.uint64), rng.integers(0, P, size=4096 - len(xs), dtype=np.uint64)])
    fn = zk.lib().zk_gl_pow2_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]
    out = np.empty(96 * len(x), np.uint64)
    assert fn(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(x)) == 0, zk.lib().zk_last_error()
    out = out.reshape(96, len(x)); xo = x.astype(object)
    for e in range(96):
        assert np.array_equal(out[e], ((xo << e) % P).astype(np.uint64)), f"mul_pow2<{e}>"


def test_lde_scaled_last_pass_and_padded_first_pass(zk, orc):
    rng = np.random.default_rng(7777)
    x = _cols(rng, 1 << 12, 3)
    assert np.array_equal(zk.interpolate(x, 3, 12, 13), orc.lde(x, 3, 12, 13))
