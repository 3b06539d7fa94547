"""The NTT passes' multiply-add forms of the Goldilocks sum, difference and canonicalising tail (gl::add_m, gl::sub_m, gl::mad_eps_m, the
fold of gl::mul_fold96) beside gl::sub and gl::add_nc, against Python integers through the probe of csrc/gl_probe.hip, and every plan shape
of the transform that runs them against the CPU oracle.  Bit-exact everywhere (integer field); a result is reduced mod p by the test only
where the primitive is documented to return "some u64 congruent to the value" (add_nc)."""
import ctypes as C
import functools
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
EPS = 0xFFFFFFFF
EDGE = [0, 1, EPS, 1 << 32, P - (1 << 32), P - 1, P - 2]
ROWS = ["add_m", "sub_m", "sub", "add_nc", "mul_tw(add_nc)", "mad_eps_m", "mul_tw"]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)


@functools.lru_cache(maxsize=None)
def _operands():
    """Canonical pairs (a, b) and a factor w (any u64): all pairs of the edge values, a == b, a == b - 1, the sums and differences next
    to p and 2^64, then 2^12 seeded random pairs."""
    rng = np.random.default_rng(20260)
    tr = [(x, y) for x in EDGE for y in EDGE]
    for _ in range(64):
        b = int(rng.integers(1, P, dtype=np.uint64))
        tr += [(b, b), (b - 1, b)]
        for s in (P - 1, P, P + 1, M64, 1 << 64, (1 << 64) + 1):        # a + b on either side of p and of 2^64
            a = int(rng.integers(max(0, s - (P - 1)), min(s, P - 1) + 1, dtype=np.uint64))
            tr.append((a, s - a))
        k, m = int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 16))
        tr += [(k, P - 1 - m), (EPS, int(rng.integers(1, EPS)) << 32)]  # a - b + 2^64 next to 2^32, and with a low word of 2^32 - 1
    tr += [(b - 1, b) for b in EDGE if b > 0] + [(b, b) for b in EDGE]
    a = np.concatenate([np.array([t[0] for t in tr], np.uint64), rng.integers(0, P, size=1 << 12, dtype=np.uint64)])
    b = np.concatenate([np.array([t[1] for t in tr], np.uint64), rng.integers(0, P, size=1 << 12, dtype=np.uint64)])
    assert int(a.max()) < P and int(b.max()) < P
    w = rng.integers(0, 1 << 64, size=len(a), dtype=np.uint64, endpoint=False)
    w[:8] = [0, 1, EPS, 1 << 32, P - 1, P, M64, M64 - 1]
    return a, b, w


@functools.lru_cache(maxsize=None)
def _probe_rows(zk):
    a, b, w = _operands()
    fn = zk.lib().zk_gl_ntt_arith_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    out = np.empty(len(ROWS) * len(a), np.uint64)
    rc = fn(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(a))
    assert rc == 0, zk.lib().zk_last_error()
    return dict(zip(ROWS, out.reshape(len(ROWS), len(a))))


def _u64(x):
    return np.asarray(x, dtype=object).astype(np.uint64)


@pytest.mark.parametrize("row", ["add_m", "sub_m", "sub"])
def test_sum_and_difference_forms_are_canonical_and_exact(zk, row):
    a, b, _ = _operands()
    ao, bo = a.astype(object), b.astype(object)
    want = (ao + bo) % P if row == "add_m" else (ao - bo) % P
    assert np.array_equal(_probe_rows(zk)[row], _u64(want)), row


def test_add_nc_is_congruent_and_feeds_a_twiddle_product(zk):
    """add_nc returns some u64 congruent to a + b; the twiddle product of it is the canonical (a + b) w"""
    a, b, w = _operands()
    ao, bo, wo = a.astype(object), b.astype(object), w.astype(object)
    got = _probe_rows(zk)
    assert np.array_equal(_u64(got["add_nc"].astype(object) % P), _u64((ao + bo) % P)), "add_nc mod p"
    assert np.array_equal(got["mul_tw(add_nc)"], _u64((ao + bo) * wo % P)), "mul_tw(add_nc(a, b), w)"


def test_canonicalising_tail_and_twiddle_product(zk):
    """mad_eps_m(r2, t) = t + r2 (2^32 - 1) mod p for any u64 t (here the canonical a and the factor's low word), and mul_tw through it"""
    a, _, w = _operands()
    ao, wo = a.astype(object), w.astype(object)
    got = _probe_rows(zk)
    assert np.array_equal(got["mad_eps_m"], _u64((ao + (wo & EPS) * EPS) % P)), "mad_eps_m"
    assert np.array_equal(got["mul_tw"], _u64(ao * wo % P)), "mul_tw"


def _cols(rng, n, n_pols):
    """column 0 all p - 1, the last column seeded random with the edge values at its head; one column alone is the random one"""
    x = rng.integers(0, P, size=(n, n_pols), dtype=np.uint64)
    x[:len(EDGE), -1] = EDGE
    if n_pols > 1:
        x[:, 0] = P - 1
    return np.ascontiguousarray(x).reshape(-1)


# 8: one pass; 12: two passes of 6 bits, shift twiddles between the halves of a pass; 17: the smallest three-pass plan; 16 x 3: two 8-bit
# passes, three columns
@pytest.mark.parametrize("nbits,n_pols", [(8, 1), (12, 1), (17, 1), (16, 3)])
def test_plain_transforms_match_oracle(zk, orc, nbits, n_pols):
    x = _cols(np.random.default_rng(9100 + nbits * 7 + n_pols), 1 << nbits, n_pols)
    X = zk.fft(x, n_pols, nbits)
    assert np.array_equal(X, orc.ntt(x, n_pols, nbits, False)), "forward"
    assert np.array_equal(zk.ifft(x, n_pols, nbits), orc.ntt(x, n_pols, nbits, True)), "inverse"
    assert np.array_equal(zk.ifft(X, n_pols, nbits), x), "round trip"


# the scaled last pass of the inverse half and the zero-padded first pass of the forward half
@pytest.mark.parametrize("nbits,n_pols", [(10, 3), (16, 1)])
def test_extension_matches_oracle(zk, orc, nbits, n_pols):
    x = _cols(np.random.default_rng(9200 + nbits), 1 << nbits, n_pols)
    assert np.array_equal(zk.interpolate(x, n_pols, nbits, nbits + 1), orc.lde(x, n_pols, nbits, nbits + 1))
