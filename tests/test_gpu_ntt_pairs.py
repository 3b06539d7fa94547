"""The paired forms of the NTT passes' field primitives (gl::bfly_m, gl::bfly2_m, gl::sub2_m, gl::mul_tw2, gl::mul_tw2_nc, gl::mul_tw2_m_nc,
gl::mad_eps2_m, gl::mul_pow2_2: two or four carry chains alternating inside one asm block) against Python integers mod p through
zk_gl_ntt_pair_probe of csrc/gl_probe.hip, and the transforms that run them against the CPU oracle, bit for bit.

The chains of a block can only go wrong together where they share a register, a mask or a flag, so the two slots of a pair always hold
DIFFERENT operands (an edge pair beside a seeded random pair), and every case runs a second time with the slots swapped: the results
must swap too.  A result is reduced mod p by the test only where the primitive returns "some u64 congruent to the value" (the _nc forms)."""
import ctypes as C
import functools
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
EPS = 0xFFFFFFFF
E = [0, 1, 2, EPS - 1, EPS, 1 << 32, (1 << 32) + 1, 1 << 63, P - (1 << 32), P - 2, P - 1]
NC = [P, P + 1, M64]                      # the products take any u64
N_ROWS = 16 + 4 * 96


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)


@functools.lru_cache(maxsize=None)
def _operands():
    """(p0, q0, p1, q1): slot 0 = every ordered pair of E, then every ordered pair with a non-canonical word in it, then 2^12
    seeded random pairs; slot 1 = seeded random pairs throughout."""
    rng = np.random.default_rng(20261)
    canon = [(x, y) for x in E for y in E]
    nc = [(x, y) for x in E + NC for y in E + NC if x >= P or y >= P]
    nr = 1 << 12
    p0 = np.concatenate([np.array([t[0] for t in canon + nc], np.uint64), rng.integers(0, P, size=nr, dtype=np.uint64)])
    q0 = np.concatenate([np.array([t[1] for t in canon + nc], np.uint64), rng.integers(0, P, size=nr, dtype=np.uint64)])
    p1 = rng.integers(0, P, size=len(p0), dtype=np.uint64)
    q1 = rng.integers(0, P, size=len(p0), dtype=np.uint64)
    # random words beyond p for the products of the random tail
    p1[-64:] = rng.integers(P, 1 << 64, size=64, dtype=np.uint64, endpoint=False)
    q1[-64:-32] = rng.integers(P, 1 << 64, size=32, dtype=np.uint64, endpoint=False)
    return p0, q0, p1, q1


def _run(zk, p0, q0, p1, q1):
    fn = zk.lib().zk_gl_ntt_pair_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 5 + [C.c_size_t]
    out = np.empty(N_ROWS * len(p0), np.uint64)
    rc = fn(*(v.ctypes.data_as(C.c_void_p) for v in (p0, q0, p1, q1, out)), len(p0))
    assert rc == 0, zk.lib().zk_last_error()
    return out.reshape(N_ROWS, len(p0))


@functools.lru_cache(maxsize=None)
def _rows(zk):
    """the probe's rows for (slot 0, slot 1) and for the slots swapped: computed once, shared by every test below"""
    p0, q0, p1, q1 = _operands()
    return _run(zk, p0, q0, p1, q1), _run(zk, p1, q1, p0, q0)


def _u64(x):
    return np.asarray(x, dtype=object).astype(np.uint64)


def _obj():
    return [v.astype(object) for v in _operands()]


def _both(zk, r_slot0, r_slot1, want0, want1, what, mod_p=(False, False)):
    """rows r_slot0 / r_slot1 hold slot 0's / slot 1's result, in the swapped run the other's; mod_p goes with the row"""
    plain, swapped = _rows(zk)
    for name, rows, w0, w1 in (("", plain, want0, want1), (" (slots swapped)", swapped, want1, want0)):
        for r, w, m in ((r_slot0, w0, mod_p[0]), (r_slot1, w1, mod_p[1])):
            got = rows[r]
            if m:
                got = _u64(got.astype(object) % P)
            bad = np.nonzero(got != _u64(w))[0]
            assert bad.size == 0, f"{what}{name}: row {r}, first case {bad[:4]}"


def test_butterflies_sum_and_difference(zk):
    p0, q0, p1, q1 = _obj()
    a, b, c, d = p0 % P, q0 % P, p1 % P, q1 % P          # the probe hands the sums and differences the operands mod p
    plain, swapped = _rows(zk)
    assert np.array_equal(plain[0], _u64((a + b) % P)) and np.array_equal(plain[1], _u64((a - b) % P)), "bfly_m"
    assert np.array_equal(swapped[0], _u64((c + d) % P)) and np.array_equal(swapped[1], _u64((c - d) % P)), "bfly_m (other slot)"
    _both(zk, 2, 4, (a + b) % P, (c + d) % P, "bfly2_m sum")
    _both(zk, 3, 5, (a - b) % P, (c - d) % P, "bfly2_m difference")
    _both(zk, 6, 7, (a - b) % P, (c - d) % P, "sub2_m")


def test_twiddle_products(zk):
    """any u64 operands; mul_tw2 and the first result of mul_tw2_m_nc are canonical, the _nc results congruent"""
    p0, q0, p1, q1 = _obj()
    w0, w1 = p0 * q0 % P, p1 * q1 % P
    _both(zk, 8, 9, w0, w1, "mul_tw2")
    _both(zk, 10, 11, w0, w1, "mul_tw2_nc", mod_p=(True, True))
    _both(zk, 12, 13, w0, w1, "mul_tw2_m_nc", mod_p=(False, True))


def test_canonicalising_tail(zk):
    """mad_eps2_m(r2, t) = t + r2 (2^32 - 1) mod p for any u64 t"""
    p0, q0, p1, q1 = _obj()
    _both(zk, 14, 15, (p0 + (q0 & EPS) * EPS) % P, (p1 + (q1 & EPS) * EPS) % P, "mad_eps2_m")


@pytest.mark.parametrize("lo", [0, 32, 64])
def test_paired_shifts(zk, lo):
    """x 2^e for every e of 0 ... 95 (32 exponents per case) on canonical x: both slots the same exponent, then e beside 95 - e"""
    p0, _, p1, _ = _obj()
    a, c = p0 % P, p1 % P
    for e in range(lo, lo + 32):
        _both(zk, 16 + 4 * e, 17 + 4 * e, (a << e) % P, (c << e) % P, f"mul_pow2_2<{e}, {e}>")
        plain = _rows(zk)[0]               # unequal exponents: the swapped run is no mirror image, the test below has it
        assert np.array_equal(plain[18 + 4 * e], _u64((a << e) % P)) and np.array_equal(plain[19 + 4 * e], _u64((c << (95 - e)) % P)), f"mul_pow2_2<{e}, {95 - e}>"


def test_paired_shifts_swapped_exponents(zk):
    """the second run hands slot 1's words to exponent e and slot 0's to 95 - e: covered by the swap above only for equal exponents"""
    p0, _, p1, _ = _obj()
    a, c = p0 % P, p1 % P
    _, swapped = _rows(zk)
    for e in range(96):
        assert np.array_equal(swapped[18 + 4 * e], _u64((c << e) % P)) and np.array_equal(swapped[19 + 4 * e], _u64((a << (95 - e)) % P)), e


def _cols(rng, n, n_pols):
    """column 0 all p - 1, the last column seeded random with the edge values at its head; one column alone is the random one"""
    x = rng.integers(0, P, size=(n, n_pols), dtype=np.uint64)
    x[:len(E), -1] = E
    if n_pols > 1:
        x[:, 0] = P - 1
    return np.ascontiguousarray(x).reshape(-1)


# 4 ... 8: one pass of every <LOGA, LOGB>; 12: 6 + 6, the shift twiddles of sub-step A; 16: 8 + 8, a one-column first pass and a last pass;
# 17: 6 + 6 + 5; 20: 7 + 7 + 6.  Columns: 1 (the one-column thread order), 3 (per-lane direct table), 16 (row-shared table).
SHAPES = [(nb, k) for nb in (4, 5, 6, 7, 8, 12, 16, 17, 20) for k in (1, 3, 16)]


@pytest.mark.parametrize("nbits,n_pols", SHAPES)
def test_transforms_match_oracle(zk, orc, nbits, n_pols):
    x = _cols(np.random.default_rng(9300 + nbits * 17 + n_pols), 1 << nbits, n_pols)
    assert np.array_equal(zk.fft(x, n_pols, nbits), orc.ntt(x, n_pols, nbits, False)), "forward"
    assert np.array_equal(zk.ifft(x, n_pols, nbits), orc.ntt(x, n_pols, nbits, True)), "inverse"


def test_ragged_last_tile(zk, orc):
    x = _cols(np.random.default_rng(9399), 1 << 9, 3)
    assert np.array_equal(zk.fft(x, 3, 9), orc.ntt(x, 3, 9, False)), "forward"
    assert np.array_equal(zk.ifft(x, 3, 9), orc.ntt(x, 3, 9, True)), "inverse"


# the scaled last pass of the inverse half, the zero-padded first pass of the forward half and the chain path
@pytest.mark.parametrize("nbits", [10, 16])
def test_extension_matches_oracle(zk, orc, nbits):
    x = _cols(np.random.default_rng(9400 + nbits), 1 << nbits, 2)
    assert np.array_equal(zk.interpolate(x, 2, nbits, nbits + 1), orc.lde(x, 2, nbits, nbits + 1))
