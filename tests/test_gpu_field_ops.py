"""Every Goldilocks device primitive on chosen operands, by name: the scalar operations of csrc/gl.hip.h, the cubic extension, the carry-free
accumulators of csrc/acc6.hip.h, the matrix-pipe product of csrc/gl_mfma.hip.h (through the probes of csrc/gl_probe.hip) and `evals` with its
accumulators filled to the fold.  The reference is Python integers; every comparison is exact.  A result is reduced mod p by the test only
where the primitive is documented to return "some u64 congruent to the value".

The operand generators are checked without a GPU (the unmarked tests): a Python model of each primitive's carry code -- which also has to
give the right value, and in which the "cannot borrow again" / "cannot carry again" steps are assertions -- sorts the operands into the
classes listed in _required(), and every class must be non-empty."""
import ctypes as C
import functools
import numpy as np
import pytest

gpu = pytest.mark.gpu
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
EPS = 0xFFFFFFFF
Q = 0xFFFFFFFEFFFFFFFF                      # p - 2: the canonical word with the most one-bits
EDGE = [0, 1, 2, P - 1, P - 2, M32, 1 << 32, (1 << 32) + 1, (1 << 64) - (1 << 32), P - (1 << 32), 0xFFFFFFFE00000001, Q]
EDGE_ANY = EDGE + [P, P + 1, 1 << 63, M64 - 1, M64]
N_SCALAR = 1 << 16
ROWS = ["add", "sub", "neg", "mul", "mul_add", "sqr", "inv", "pow", "reduce128", "mul_nc", "sqr_nc", "mul_add_nc", "add_nc", "add_word",
        "mad_eps_nc", "pow7", "nc_chain"]


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def _u64(a):
    return np.asarray(a, dtype=object).astype(np.uint64)


def _b(x):
    return np.asarray(x, dtype=object).astype(bool)


# ---- operands of the scalar probe ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scalar_operands(top):
    """N_SCALAR triples below `top` (p: canonical operands, 2^64: any u64): the cube of the edge set, the solved-for families that force
    each branch, then seeded random.  Returns a, b, c and the indices whose inv / pow rows are compared (at most 4096: the edge pairs,
    the families and a random rest)."""
    edge = EDGE_ANY if top > P else EDGE
    tr = [(x, y, z) for x in edge for y in edge for z in edge]
    pair_idx = [i for i in range(len(tr)) if i % len(edge) == 0]          # one triple per pair (x, y)
    rng = np.random.default_rng(20251)
    r64 = lambda: int(rng.integers(0, top, dtype=np.uint64))              # noqa: E731
    fam0 = len(tr)
    tr += [(1 << 48, 1 << 48, 0), (M32 + 2, M32, 0), (M32, M32, 0), (0, P - 1, 0), (M32, 1 << 32, 0), (M32, P - 1, 0)]
    # a b = 2^96: w1:w0 = 0, r3 = 1, so the first step leaves 2^64 - 1 and the second step's low subtraction does not borrow
    tr += [(1 << (32 + k), 1 << (64 - k), 0) for k in range(1, 32)]
    if top > P:
        tr += [(M64, M64, M64), (M32, M64, M64), ((1 << 63) | M32, M64, M64), (M64, M32, 0), (1 << 32, M64, 0), (M64, 1, 0), (M64, P - 1, 0)]
    for _ in range(64):
        # r2 = 2^32 - 1 and r3 = 0: a b = (2^32 - 1) 2^64 + lo (b solved for from a random a; the excess is below a < 2^62)
        a = int(rng.integers(1 << 33, 1 << 62)); b = ((M32 << 64) + int(rng.integers(0, 1 << 63))) // a + 1
        assert a < top and b < top and ((a * b) >> 64) == M32
        tr.append((a, b, 0)); tr.append((a, b, r64()))
        # r3 > w1:w0: both low halves zero, so a b = a1 b1 2^64 has w1:w0 = 0 and r3 = a1 b1 >> 32 > 0
        a1, b1 = int(rng.integers(1 << 16, M32)), int(rng.integers(1 << 16, M32))
        tr.append((a1 << 32, b1 << 32, 0)); tr.append((a1 << 32, b1 << 32, int(rng.integers(0, 1 << 32))))
        # the folded value lands in [p, 2^64): a b in [p, 2^64) itself (r2 = r3 = 0)
        a = int(rng.integers(1 << 20, 1 << 32)); v = int(rng.integers(P, (1 << 64) - a, dtype=np.uint64)); b = -(-v // a)
        assert P <= a * b < 1 << 64
        tr.append((a, b, 0)); tr.append((b, a, 0))
        # ... and a b + c in [p, 2^64) with a small product
        a, b = int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 16))
        if top > P:
            tr.append((a, b, int(rng.integers(P, 1 << 64, dtype=np.uint64)) - a * b))
            # mul_add: p1 = a0 b1 + (p0 >> 32) + (c >> 32) reaches 2^64 - 1 (a0 = b0 = b1 = 2^32 - 1, c = 2^64 - 1; a1 free)
            tr.append(((int(rng.integers(0, 1 << 32)) << 32) | M32, M64, M64))
        # sums a + b in {p - 1, p, 2^64 - 1, 2^64} of canonical a, b
        for s in (P - 1, P, M64, 1 << 64):
            a = int(rng.integers(max(0, s - (P - 1)), min(s, P - 1) + 1, dtype=np.uint64))
            assert 0 <= a < P and 0 <= s - a < P
            tr.append((a, s - a, r64()))
        # differences a < b: the smallest a - b + 2^64 two canonical words reach is 2^32 (0 - (p - 1)); a - b + 2^64 < 2^32 - 1 would make
        # the + p fix-up borrow again and needs b >= p, which sub excludes (the model asserts it never happens).  The family is the
        # differences next to that boundary, and those whose low word is 2^32 - 1 (the fix-up's low subtraction then does not borrow).
        k, m = int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 16))
        tr.append((k, P - 1 - m, r64()))
        tr.append((M32, int(rng.integers(1, M32)) << 32, r64()))
        # add_nc: any a + canonical b in {2^64 - 1, 2^64, 2^64 + small}
        if top > P:
            b = int(rng.integers(1, P, dtype=np.uint64))
            for s in (M64, 1 << 64, (1 << 64) + k):
                if 0 <= s - b <= M64:
                    tr.append((s - b, b, r64()))
    n_dir = len(tr)
    assert n_dir < 16384
    m = N_SCALAR - n_dir
    a = np.concatenate([np.array([t[0] for t in tr], np.uint64), rng.integers(0, top, size=m, dtype=np.uint64)])
    b = np.concatenate([np.array([t[1] for t in tr], np.uint64), rng.integers(0, top, size=m, dtype=np.uint64)])
    c = np.concatenate([np.array([t[2] for t in tr], np.uint64), rng.integers(0, top, size=m, dtype=np.uint64)])
    slow = pair_idx + list(range(fam0, n_dir))
    slow = np.array(slow + list(range(n_dir, n_dir + 4096 - len(slow))))
    assert len(slow) == 4096 and slow.max() < N_SCALAR
    return a, b, c, slow


# ---- the carry code in Python integers -------------------------------------------------------------------------------------------
def _model_fold(X, canonical):
    """reduce_words / reduce_words_nc on the 128-bit X = lo + r2 2^64 + r3 2^96 (gl.hip.h sub_word_fold, then mad_eps or mad_eps_nc)"""
    lo, r2, r3 = X & M64, (X >> 64) & M32, X >> 96
    borrow1 = _b(lo < r3)                                               # first step of sub_word_fold: (w1:w0) - r3 borrows
    t1 = (lo - r3) & M64
    low2 = borrow1 & _b((t1 & M32) != M32)                              # second step taken AND its low subtraction borrows into the high word
    nolow2 = borrow1 & ~low2                                            # second step taken, low word 2^32 - 1: no borrow inside it
    t = t1 - EPS * borrow1.astype(object)
    assert (t >= 0).all(), "sub_word_fold: the second step borrowed out of the 64 bits"
    s = t + r2 * EPS
    carry = _b(s >= 1 << 64)                                            # the carry of mad_eps' multiply-add
    u = (s & M64) + EPS * carry.astype(object)
    assert (u <= M64).all(), "mad_eps: the + 2^32 - 1 fix-up carried again"
    cls = {"fold_borrow1": borrow1, "fold_no_borrow1": ~borrow1, "fold_step2_low_borrow": low2, "fold_step2_no_low_borrow": nolow2,
           "mad_eps_carry": carry, "mad_eps_no_carry": ~carry, "r3_gt_w": _b(r3 > lo), "r2_max_r3_0": _b(r2 == M32) & _b(r3 == 0)}
    if canonical:
        final = _b(u >= P)
        cls.update(final_sub_taken=final, final_sub_not_taken=~final)
        u = u - P * final.astype(object)
        assert (u < P).all()
    assert ((u - X) % P == 0).all(), "the model of the fold does not give X mod p"
    return cls


def _classes(top):
    a, b, c, _ = _scalar_operands(top)
    a, b, c = _obj(a), _obj(b), _obj(c)
    ca, cb = a % P, b % P
    out = {}
    for name, X, canonical in (("mul", a * b, True), ("sqr", a * a, True), ("mul_add", a * b + c, True), ("mul_nc", a * b, False),
                               ("sqr_nc", a * a, False), ("mul_add_nc", a * b + c, False)):
        out[name] = _model_fold(X, canonical)
    p0 = (a & M32) * (b & M32) + (c & M32)
    p1 = (a & M32) * (b >> 32) + (p0 >> 32) + (c >> 32)
    assert (p1 <= M64).all()
    for name in ("mul_add", "mul_add_nc"):
        out[name]["p1_is_2^64-1"] = _b(p1 == M64)
    # add (canonical operands): c1 = the carry of a + b, d1 = the carry of s + 2^32 - 1, i.e. s >= p
    s = ca + cb
    c1, d1 = _b(s >= 1 << 64), _b((s & M64) >= P)
    out["add"] = {"c1": c1, "d1_without_c1": ~c1 & d1, "neither": ~c1 & ~d1, "sum_p-1": _b(s == P - 1), "sum_p": _b(s == P), "sum_2^64-1": _b(s == M64),
                  "sum_2^64": _b(s == 1 << 64)}
    assert ((np.where(c1 | d1, (s + EPS) & M64, s) - s) % P == 0).all() and (np.where(c1 | d1, (s + EPS) & M64, s) < P).all()
    # sub: borrow -> minus 2^32 - 1
    brw = _b(ca < cb)
    d = (ca - cb) & M64
    assert (d[brw] >= EPS).all(), "sub: the fix-up borrowed again"
    out["sub"] = {"borrow": brw, "no_borrow": ~brw, "borrow_fixup_low_borrow": brw & _b((d & M32) != M32), "borrow_fixup_no_low_borrow": brw & _b((d & M32) == M32),
                  "borrow_smallest_2^32": brw & _b(d == 1 << 32)}
    out["neg"] = {"zero": _b(ca == 0), "nonzero": _b(ca != 0)}
    # add_nc (any a, canonical b): carry -> plus 2^32 - 1, which must not carry again
    s = a + cb
    cy = _b(s >= 1 << 64)
    assert ((s & M64)[cy] + EPS <= M64).all(), "add_nc: the fix-up carried again"
    out["add_nc"] = {"carry": cy, "no_carry": ~cy, "carry_fixup_low_carry": cy & _b((s & M32) != 0), "carry_fixup_no_low_carry": cy & _b((s & M32) == 0)}
    # mad_eps_nc(r2 = (u32)b, t = a) on its own
    s = a + (b & M32) * EPS
    cy = _b(s >= 1 << 64)
    assert ((s & M64)[cy] + EPS <= M64).all(), "mad_eps_nc: the fix-up carried again"
    out["mad_eps_nc"] = {"carry": cy, "no_carry": ~cy}
    s = a + (b & M32)
    out["add_word"] = {"wraps": _b(s > M64), "no_wrap": _b(s <= M64)}
    # reduce128(lo = a, hi = b)
    t0b = _b(a < (b >> 32))
    t0 = (a - (b >> 32) - EPS * t0b.astype(object)) & M64
    t1 = (b & M32) * EPS
    t2c = _b(t0 + t1 > M64)
    t2 = ((t0 + t1) & M64) + EPS * t2c.astype(object)
    assert (t2 <= M64).all() and ((t2 - (a + (b << 64))) % P == 0).all()
    out["reduce128"] = {"t0_borrow": t0b, "t0_no_borrow": ~t0b, "t2_carry": t2c, "t2_no_carry": ~t2c, "final_sub_taken": _b(t2 >= P), "final_sub_not_taken": _b(t2 < P)}
    return out


# the classes each operand set must reach.  Only non-canonical words reach "p1_is_2^64-1" (b = c = 2^64 - 1), a wrapping add_word
# (a canonical word plus 2^32 - 1 stays below 2^64) and add_nc's carry with a zero low word (a + b = 2^64 + k 2^32 is above the family
# of canonical sums); a squaring never has r2 = 2^32 - 1 with r3 = 0 on these operands.
def _required(top):
    fold = ["fold_borrow1", "fold_no_borrow1", "fold_step2_low_borrow", "fold_step2_no_low_borrow", "mad_eps_carry", "mad_eps_no_carry", "r3_gt_w", "r2_max_r3_0"]
    final = ["final_sub_taken", "final_sub_not_taken"]
    req = {"mul": fold + final, "sqr": [f for f in fold if f != "r2_max_r3_0"] + final, "mul_add": fold + final, "mul_nc": fold,
           "sqr_nc": [f for f in fold if f != "r2_max_r3_0"], "mul_add_nc": fold,
           "add": ["c1", "d1_without_c1", "neither", "sum_p-1", "sum_p", "sum_2^64-1", "sum_2^64"],
           "sub": ["borrow", "no_borrow", "borrow_fixup_low_borrow", "borrow_fixup_no_low_borrow", "borrow_smallest_2^32"], "neg": ["zero", "nonzero"],
           "add_nc": ["carry", "no_carry", "carry_fixup_low_carry"], "mad_eps_nc": ["carry", "no_carry"], "add_word": ["no_wrap"],
           "reduce128": ["t0_borrow", "t0_no_borrow", "t2_carry", "t2_no_carry", "final_sub_taken", "final_sub_not_taken"]}
    if top > P:
        req["mul_add"] = req["mul_add"] + ["p1_is_2^64-1"]; req["mul_add_nc"] = req["mul_add_nc"] + ["p1_is_2^64-1"]
        req["add_nc"] = req["add_nc"] + ["carry_fixup_no_low_carry"]; req["add_word"] = req["add_word"] + ["wraps"]
    return req


@pytest.mark.parametrize("top", [P, 1 << 64], ids=["canonical", "any_u64"])
def test_scalar_operands_reach_every_branch(top):
    """No GPU: the generator against the Python model of the carry code.  Every class a primitive's code distinguishes is non-empty (the
    sizes are printed: -s), the model returns the right value for every operand, and its "cannot happen" steps never happen."""
    cls = _classes(top)
    for prim, names in _required(top).items():
        sizes = {k: int(cls[prim][k].sum()) for k in names}
        print(f"{'canonical' if top == P else 'any_u64'} {prim}: " + ", ".join(f"{k}={v}" for k, v in sizes.items()))
        for k, v in sizes.items():
            assert v > 0, f"{prim}: no operand of class {k}"


# ---- scalar primitives on the device -----------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)
    return zk


@gpu
@pytest.mark.parametrize("top", [P, 1 << 64], ids=["canonical", "any_u64"])
def test_scalar_primitives_match_python_integers(dev, top):
    """2^16 triples, one row per primitive (ROWS).  add, sub, neg get a mod p, b mod p and add_nc b mod p from the probe; the nc rows are
    reduced once here; add_word is a 64-bit addition and is compared as it is.  inv and pow are compared on 4096 of the triples."""
    a, b, c, slow = _scalar_operands(top)
    n = len(a)
    fn = dev.lib().zk_gl_scalar_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 4 + [C.c_size_t]
    out = np.empty(len(ROWS) * n, np.uint64)
    assert fn(_ptr(a), _ptr(b), _ptr(c), _ptr(out), n) == 0, dev.lib().zk_last_error()
    got = dict(zip(ROWS, out.reshape(len(ROWS), n)))
    ao, bo, co = _obj(a), _obj(b), _obj(c)
    ca, cb = ao % P, bo % P
    want = {"add": (ca + cb) % P, "sub": (ca - cb) % P, "neg": (-ca) % P, "mul": ao * bo % P, "mul_add": (ao * bo + co) % P, "sqr": ao * ao % P,
            "reduce128": (ao + (bo << 64)) % P, "mul_nc": ao * bo % P, "sqr_nc": ao * ao % P, "mul_add_nc": (ao * bo + co) % P, "add_nc": (ao + cb) % P,
            "add_word": (ao + (bo & M32)) & M64, "mad_eps_nc": (ao + (bo & M32) * EPS) % P, "pow7": ao ** 7 % P,
            "nc_chain": (ao * bo * co * co + ao * co + cb) % P}
    nc = {"mul_nc", "sqr_nc", "mul_add_nc", "add_nc", "mad_eps_nc", "pow7", "nc_chain"}
    bad = []
    for name, w in want.items():
        g = got[name]
        if name in nc:
            g = _u64(_obj(g) % P)
        w = _u64(w)
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            bad.append(f"{name}: {int((g != w).sum())} wrong, first at a={int(a[i]):#x} b={int(b[i]):#x} c={int(c[i]):#x}: got {int(got[name][i]):#x}, want {int(w[i]):#x}")
    for name, f in (("inv", lambda x, y: pow(x, P - 2, P)), ("pow", lambda x, y: pow(x, y, P))):
        for i in slow:
            w = f(int(a[i]), int(b[i]))
            if int(got[name][i]) != w:
                bad.append(f"{name}: a={int(a[i]):#x} b={int(b[i]):#x}: got {int(got[name][i]):#x}, want {w:#x}")
                break
    assert not bad, "\n".join(bad)


# ---- cubic extension -------------------------------------------------------------------------------------------------------------
def _f3_mul(x, y):
    """GF(p)[x] / (x^3 - x - 1), schoolbook: x^3 = x + 1, x^4 = x^2 + x.  x, y: (n, 3) object arrays"""
    c0 = x[:, 0] * y[:, 0]; c1 = x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0]; c2 = x[:, 0] * y[:, 2] + x[:, 1] * y[:, 1] + x[:, 2] * y[:, 0]
    c3 = x[:, 1] * y[:, 2] + x[:, 2] * y[:, 1]; c4 = x[:, 2] * y[:, 2]
    return np.stack([(c0 + c3) % P, (c1 + c3 + c4) % P, (c2 + c4) % P], axis=1)


def _f3_inv(x):
    """the solution y of M y = (1, 0, 0), M = the matrix of the multiplication by x (columns x, x X, x X^2), by Cramer's rule; 0 -> 0"""
    n = len(x)
    e = lambda k: np.tile(np.array([[int(i == k) for i in range(3)]], dtype=object), (n, 1))   # noqa: E731
    col = [_f3_mul(x, e(k)) for k in range(3)]                     # col[k][:, r] = M[r][k]
    m = lambda r, k: col[k][:, r]                                    # noqa: E731
    det = (m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) + m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0))) % P
    di = np.array([pow(int(d), P - 2, P) for d in det], dtype=object)
    y0 = (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) * di % P
    y1 = -(m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) * di % P
    y2 = (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)) * di % P
    return np.stack([y0, y1, y2], axis=1)


@functools.lru_cache(maxsize=None)
def _f3_operands():
    """4096 (x, y, s): every edge word in every coordinate of x (the cube) against rotated edge words, base-field-valued elements
    (v, 0, 0) on either side, pairs with x y = 1, then seeded random; s runs through the any-u64 edge words, then random"""
    rng = np.random.default_rng(3303)
    E = EDGE
    xs = [(u, v, w) for u in E for v in E for w in E]
    ys = [(E[(i * 5 + 1) % 12], E[(i // 12 + 7) % 12], E[(i // 7) % 12]) for i in range(len(xs))]
    for v in E:
        for w in E:
            xs.append((v, 0, 0)); ys.append((w, 0, 0))
            xs.append((v, 0, 0)); ys.append((w, E[3], E[11]))
            xs.append((E[4], v, E[9])); ys.append((w, 0, 0))
    n_inv = 512
    n = 4096
    m = n - len(xs) - n_inv
    x = np.concatenate([np.array(xs, dtype=np.uint64), rng.integers(0, P, size=(m + n_inv, 3), dtype=np.uint64)])
    y = np.concatenate([np.array(ys, dtype=np.uint64), rng.integers(0, P, size=(m + n_inv, 3), dtype=np.uint64)])
    x[-n_inv:-n_inv + 144] = np.array(xs[:1728:12], dtype=np.uint64)               # edge-word elements among the inverse pairs; (0, 0, 0) stays (y = 0)
    y[-n_inv:] = _u64(_f3_inv(_obj(x[-n_inv:])))                                   # x y = 1
    s = np.concatenate([np.array([EDGE_ANY[i % 17] for i in range(len(xs))], np.uint64), rng.integers(0, 1 << 64, size=n - len(xs), dtype=np.uint64, endpoint=False)])
    return x, y, s


def test_f3_reference_inverts():
    """No GPU: the reference inverse against the reference product, and the operand families are what they claim to be"""
    x, y, s = _f3_operands()
    xo = _obj(x)
    prod = _f3_mul(xo, _f3_inv(xo))
    nz = (x != 0).any(axis=1)
    assert (prod[nz] == np.array([1, 0, 0], dtype=object)).all() and (prod[~nz] == 0).all() and (~nz).sum() >= 1
    one = (_f3_mul(_obj(x[-512:]), _obj(y[-512:])) == np.array([1, 0, 0], dtype=object)).all(axis=1)
    assert one.sum() >= 500 and (x < P).all() and (y < P).all()
    assert ((x[:, 1:] == 0).all(axis=1) & (y[:, 1:] == 0).all(axis=1)).sum() >= 144


def _f3_probe(dev, x, y, s):
    fn = dev.lib().zk_gl_f3_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 4 + [C.c_size_t]
    n = len(s)
    out = np.empty(15 * n, np.uint64)
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert fn(_ptr(x), _ptr(y), _ptr(s), _ptr(out), n) == 0, dev.lib().zk_last_error()
    return dict(zip(["f3_add", "f3_sub", "f3_mul", "f3_muls", "f3_inv"], out.reshape(5, n, 3)))


@gpu
def test_extension_matches_python_integers(dev):
    x, y, s = _f3_operands()
    got = _f3_probe(dev, x, y, s)
    xo, yo, so = _obj(x), _obj(y), _obj(s)
    want = {"f3_add": (xo + yo) % P, "f3_sub": (xo - yo) % P, "f3_mul": _f3_mul(xo, yo), "f3_muls": xo * so[:, None] % P, "f3_inv": _f3_inv(xo)}
    for name, w in want.items():
        w = _u64(w)
        ok = (got[name] == w).all(axis=1)
        i = int(np.flatnonzero(~ok)[0]) if not ok.all() else 0
        assert ok.all(), f"{name}: {int((~ok).sum())} wrong, first x={[hex(int(v)) for v in x[i]]} y={[hex(int(v)) for v in y[i]]} s={int(s[i]):#x}: got {[hex(int(v)) for v in got[name][i]]}, want {[hex(int(v)) for v in w[i]]}"
    # without the reference: the device's product of x and the device's own inverse of x is one
    again = _f3_probe(dev, x, got["f3_inv"], s)["f3_mul"]
    nz = (x != 0).any(axis=1)
    assert (again[nz] == np.array([1, 0, 0], np.uint64)).all() and (again[~nz] == 0).all()


# ---- Acc6 ------------------------------------------------------------------------------------------------------------------------
ACC_N = [1, 12, 256, 512]           # one term, dot12, EV_FLUSH, the limit stated in acc6.hip.h
ACC_LANES = 300                     # more than one block, the last one ragged


@functools.lru_cache(maxsize=None)
def _acc_operands(n):
    """lanes x n constants (canonical) and words (any u64) and a start word per lane.  Lane l: constant pattern l % 5 against word pattern
    (l // 5) % 5; pattern 4 is seeded random, and from lane 25 on every term draws its own pattern.  Constant patterns: p - 2 (limbs
    0x3FFFFF, 0x3FFBFF, 0xFFFFF: the most ones a canonical word has), p - 1, 0xFFFFEFFFFFFFFFFF (limbs 0 and 1 all ones), 0xFFFFF7FFFFFFFFFF;
    word patterns 2^64 - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF, 0xFFFFFFFEFFFFFFFF."""
    rng = np.random.default_rng(600 + n)
    cpat = np.array([Q, P - 1, 0xFFFFEFFFFFFFFFFF, 0xFFFFF7FFFFFFFFFF], np.uint64)
    wpat = np.array([M64, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF, Q], np.uint64)
    L = ACC_LANES
    rc = rng.integers(0, P, size=(L, n), dtype=np.uint64); rw = rng.integers(0, 1 << 64, size=(L, n), dtype=np.uint64, endpoint=False)
    ci = rng.integers(0, 5, size=(L, n)); wi = rng.integers(0, 5, size=(L, n))
    for l in range(25):
        ci[l, :] = l % 5; wi[l, :] = (l // 5) % 5
    c = np.where(ci < 4, cpat[np.minimum(ci, 3)], rc)
    w = np.where(wi < 4, wpat[np.minimum(wi, 3)], rw)
    start = rng.integers(0, 1 << 64, size=L, dtype=np.uint64, endpoint=False)
    start[:25:3] = M64; start[1:25:3] = P - 1; start[2:25:6] = 0
    assert (c < P).all()
    return np.ascontiguousarray(c), np.ascontiguousarray(w), start


def _acc_model(c, w, start):
    """the six accumulators and acc_finish's columns as integers: (largest accumulator, largest column Z or Y1 / Y2, largest Y3, value mod p)"""
    co, wo = _obj(c), _obj(w)
    l = [co & 0x3FFFFF, (co >> 22) & 0x3FFFFF, co >> 44]
    x = [wo & M32, wo >> 32]
    a = {(i, h): (l[i] * x[h]).sum(axis=1) for i in range(3) for h in range(2)}
    if start is not None:
        so = _obj(start)
        a[0, 0] = a[0, 0] + (so & M32); a[0, 1] = a[0, 1] + (so >> 32)
    amax = max(int(v.max()) for v in a.values())
    lo, hi = (lambda v: v & M32), (lambda v: v >> 32)
    Z0 = lo(a[1, 0]) * (1 << 22) + a[0, 0]
    Z1 = hi(a[1, 0]) * (1 << 22) + a[0, 1] + lo(a[1, 1]) * (1 << 22) + lo(a[2, 0]) * (1 << 12)
    Z2 = hi(a[1, 1]) * (1 << 22) + hi(a[2, 0]) * (1 << 12) + lo(a[2, 1]) * (1 << 12)
    Z3 = hi(a[2, 1]) * (1 << 12)
    Y1 = Z1 + hi(Z0); Y2 = Z2 + hi(Y1); Y3 = Z3 + hi(Y2)
    val = (lo(Z0) + (lo(Y1) << 32) + (lo(Y2) << 64) + (Y3 << 96))
    full = sum(a[i, h] << (22 * i + 32 * h) for i in range(3) for h in range(2))
    assert (val == full).all(), "the model of acc_finish's columns does not add up to the accumulators' value"
    colmax = max(int(v.max()) for v in (Z0, Z1, Z2, Z3, Y1, Y2))
    return amax, colmax, int(Y3.max()), full % P


@pytest.mark.parametrize("n", ACC_N)
def test_acc6_inputs_stay_inside_the_accumulators(n):
    """No GPU.  What acc6.hip.h assumes about n <= 512 terms, on these inputs: no accumulator and no column of acc_finish reaches 2^64, and
    Y3 (the words above 2^96) stays below 2^42.  At n = 512 the inputs come within a factor 1.01 of the largest sum there is."""
    c, w, start = _acc_operands(n)
    for st in (None, start):
        amax, colmax, y3, val = _acc_model(c, w, st)
        print(f"n={n} start={'word' if st is not None else 'zero'}: largest accumulator 2^{np.log2(amax):.3f}, largest column 2^{np.log2(colmax):.3f}, largest Y3 2^{np.log2(max(y3, 1)):.3f}")
        assert amax < 1 << 64 and colmax < 1 << 64 and y3 < 1 << 42
        dot = (_obj(c) * _obj(w)).sum(axis=1) + (0 if st is None else _obj(st))
        assert (dot % P == val).all()
        if n == 512:
            assert amax * 1.01 > 512 * 0x3FFFFF * M32


@gpu
@pytest.mark.parametrize("n", ACC_N)
def test_acc6_dot_products_match_python_integers(dev, n):
    c, w, start = _acc_operands(n)
    fn = dev.lib().zk_gl_acc6_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 4 + [C.c_size_t] * 2
    for st in (None, start):
        out = np.empty(ACC_LANES, np.uint64)
        assert fn(_ptr(c), _ptr(w), _ptr(st) if st is not None else None, _ptr(out), ACC_LANES, n) == 0, dev.lib().zk_last_error()
        want = _u64(((_obj(c) * _obj(w)).sum(axis=1) + (0 if st is None else _obj(st))) % P)
        got = _u64(_obj(out) % P)                                   # acc_finish: nc out
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"n={n}, start={'acc_word' if st is not None else 'acc_zero'}: lanes {bad[:8].tolist()} wrong; lane {bad[0]}: got {int(out[bad[0]]):#x}, want {int(want[bad[0]]):#x}"


# ---- matrix pipe -------------------------------------------------------------------------------------------------------------------
N_VEC = 1024
BIG = 0x7F807F807F807F80            # every c 2^(8 b) mod p of it has digits of magnitude 127 / 128: the digit-column sums come within 0.3 % of 12 * 8 * 128


def _digits(v):
    """the balanced base-256 digits of c 2^(8 b) mod p, b < 8, as gl_mfma.hip.h build_tables writes them: [b][d]"""
    S = M64 // 255
    out = []
    for _ in range(8):
        s = v - P if v > 127 * S else v
        row = []
        for _ in range(8):
            dg = ((s + 128) % 256) - 128
            row.append(dg); s = (s - dg) // 256
        assert s == 0
        out.append(row); v = (v << 8) % P
    return out


def _poseidon_matrix(zk):
    m = np.empty(144, np.uint64)
    fn = zk.lib().zk_gl_poseidon_matrix_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    assert fn(_ptr(m)) == 0
    return m.reshape(12, 12)


def _coef_sets(zk):
    """the fixed list: (name, coefficients [n_out][n_in], the table's addend or None).  12 x 12, and 11 x 11 as Poseidon's partial-round
    blocks use the product: 11 words in, 12 outputs computed, the first PR_B = 11 kept (the twelfth is an empty row: 0)."""
    rng = np.random.default_rng(808)
    pm = _poseidon_matrix(zk)
    rnd = rng.integers(0, P, size=(12, 12), dtype=np.uint64)
    mixed = np.array([[(BIG, P - 1, 1, Q, 0x8080808080808080 % P, 0x7F7F7F7F7F7F7F7F)[(3 * o + j) % 6] for j in range(12)] for o in range(12)], np.uint64)
    base = [("ones", np.ones((12, 12), np.uint64)), ("p-1", np.full((12, 12), P - 1, np.uint64)), ("identity", np.eye(12, dtype=np.uint64)),
            ("big_columns", np.full((12, 12), BIG, np.uint64)), ("mixed_extremes", mixed), ("random", rnd), ("poseidon_P", pm)]
    tab_add = np.array([P - 1, 0, 1, Q] * 3, np.uint64)
    sets = []
    for name, m in base:
        sets.append((name + "_12x12", np.ascontiguousarray(m), None))
        sets.append((name + "_11x11", np.ascontiguousarray(m[:11, :11]), None))
    sets.append(("random_12x12_table_addend", np.ascontiguousarray(rnd), tab_add))
    sets.append(("big_columns_11x11_table_addend", np.ascontiguousarray(np.full((11, 11), BIG, np.uint64)), np.ascontiguousarray(tab_add[:11])))
    return sets


def _vectors(coef):
    """N_VEC vectors of 12 words.  The patterns repeat with an odd period, so lanes l and l + 32 of a wave (which trade halves through
    permlane32_swap) never hold the same one; the second half of the vectors is seeded random."""
    rng = np.random.default_rng(909)
    n_in = coef.shape[1]
    byte = lambda v: int.from_bytes(bytes([v]) * 8, "little")      # noqa: E731
    pats = [[byte(v)] * 12 for v in (0x00, 0x7F, 0x80, 0xFF)]
    pats += [[0x807F807F807F807F] * 12, [0x7F807F807F807F80] * 12, [0x7F7F7F7F80808080, 0x808080807F7F7F7F] * 6, [M64] * 12, [P - 1] * 12, [Q] * 12]
    for j in range(12):
        for v in (M64, 1, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F):
            pats.append([v if k == j else 0 for k in range(12)])
    # the vectors that drive one digit column of output 0 as far as it goes: byte (j, b) = 0xFF (+127) where the digit is positive and
    # 0x00 (-128) where it is negative, and the other way round
    dg = [_digits(int(coef[0, j])) for j in range(n_in)]
    for d in range(8):
        for sign in (1, -1):
            vec = []
            for j in range(12):
                word = 0
                for b in range(8):
                    if j < n_in and dg[j][b][d] * sign > 0:
                        word |= 0xFF << (8 * b)
                vec.append(word)
            pats.append(vec)
    if len(pats) % 2 == 0:
        pats.append([0x0123456789ABCDEF] * 12)
    pats = np.array(pats, np.uint64)
    assert len(pats) % 2 == 1 and len(pats) < N_VEC // 2
    x = rng.integers(0, 1 << 64, size=(N_VEC, 12), dtype=np.uint64, endpoint=False)
    half = N_VEC // 2
    x[:half] = pats[np.arange(half) % len(pats)]
    assert all((x[l] != x[l + 32]).any() for l in range(half - 32))
    ad = rng.integers(0, 1 << 64, size=(N_VEC, 12), dtype=np.uint64, endpoint=False)
    sel = (np.arange(N_VEC)[:, None] + np.arange(12)[None, :]) % 4
    ad = np.where(sel == 0, np.uint64(0), np.where(sel == 1, np.uint64(P - 1), np.where(sel == 2, np.uint64(M64), ad)))
    return np.ascontiguousarray(x), np.ascontiguousarray(ad)


def test_matrix_pipe_coefficient_sets_all_build(zk):
    """No GPU: build_tables accepts and check_tables passes every set of the list, so none is left out on the device; the set chosen for
    large digit columns has them (128 x the column's sum of digit magnitudes is what build_tables bounds by 2^21)."""
    fn = zk.lib().zk_gl_mfma_tables_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    sets = _coef_sets(zk)
    assert len(sets) == 16
    for name, coef, tab_add in sets:
        assert fn(_ptr(coef), coef.shape[0], coef.shape[1], _ptr(tab_add) if tab_add is not None else None) == 0, (name, zk.lib().zk_last_error())
    dg = _digits(BIG)
    worst = max(sum(abs(dg[b][d]) for b in range(8)) for d in range(8)) * 12 * 128
    print(f"big_columns: 128 x largest digit-column sum = {worst} = 2^{np.log2(worst):.3f}")
    assert 0.99 * 12 * 8 * 128 * 128 < worst <= 1 << 21


@gpu
def test_matrix_pipe_products_match_python_integers(dev):
    """product<3> and product_add<3> behind make_b<12> / make_b<11>, one vector per lane, for every coefficient set; the outputs past
    n_out are empty rows (0, or the lane's addend)"""
    fn = dev.lib().zk_gl_mfma_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t]
    bad = []
    for name, coef, tab_add in _coef_sets(dev):
        n_out, n_in = coef.shape
        x, ad = _vectors(coef)
        out = np.empty(2 * N_VEC * 12, np.uint64)
        rc = fn(_ptr(coef), n_out, n_in, _ptr(tab_add) if tab_add is not None else None, _ptr(x), _ptr(ad), _ptr(out), N_VEC)
        assert rc == 0, (name, dev.lib().zk_last_error())
        got = _obj(out.reshape(2, N_VEC, 12)) % P                  # recombine / recombine_add: nc out
        full = np.zeros((12, 12), dtype=object); full[:n_out, :n_in] = _obj(coef)
        ta = np.zeros(12, dtype=object)
        if tab_add is not None:
            ta[:n_out] = _obj(tab_add)
        want = (_obj(x).dot(full.T) + ta[None, :]) % P
        for k, (form, w) in enumerate((("product", want), ("product_add", (want + _obj(ad)) % P))):
            ne = got[k] != w
            if ne.any():
                v, o = [int(i) for i in np.argwhere(ne)[0]]
                bad.append(f"{name} {form}: {int(ne.sum())} wrong, first vector {v} (lane {v % 64}) output {o}: got {int(got[k][v, o]):#x}, want {int(w[v, o]):#x}, x={[hex(int(t)) for t in x[v]]}")
    assert not bad, "\n".join(bad)


# ---- evals with full accumulators --------------------------------------------------------------------------------------------------
EV_NBITS, EV_EXT = 23, 0


@gpu
def test_evals_at_the_accumulator_bound(dev, orc):
    """zk.evals against the oracle's dot product with every operand word p - 1 or 0xFFFFFFFEFFFFFFFF, at the smallest size at which a lane
    folds full accumulators.  evals_partial_kernel runs n_row_blocks = min(4096, 2^nbits / 32) blocks of 8 rows x 32 columns; a lane takes
    the rows k = 8 block + row (mod 8 n_row_blocks), that is 2^nbits / (8 n_row_blocks) terms: 4 for nbits <= 17, 2^(nbits - 15) above.
    It folds when EV_FLUSH = 256 terms are pending, so nbits = 23 (ext = 0: nbits + ext = 23) is the first size with a fold of 256 terms
    (at 22 a lane's only fold takes 128).  Each of the three Acc6 of a lane then holds 256 products of a 22-bit limb of the column
    word with a 32-bit half of a weight: dim-1 and dim-3 columns, LEv and LpEv (prime), the tables handed over as they are."""
    n = 1 << EV_NBITS
    sec = np.empty((n << EV_EXT, 4), np.uint64)
    sec[:, 0] = P - 1; sec[:, 1] = Q; sec[:, 2] = P - 1; sec[:, 3] = Q
    sec = sec.reshape(-1)
    L = np.tile(np.array([P - 1, Q, P - 1], np.uint64), n)
    Lp = np.tile(np.array([Q, P - 1, Q], np.uint64), n)
    d_sec = dev.DevArray.from_host(sec)
    descs = [(d_sec, 4, 0, 1, False), (d_sec, 4, 1, 1, True), (d_sec, 4, 1, 3, False), (d_sec, 4, 0, 3, True), (d_sec, 4, 1, 1, False), (d_sec, 4, 0, 1, True)]
    got = dev.evals(descs, EV_NBITS, EV_EXT, dev.DevArray.from_host(L), dev.DevArray.from_host(Lp)).to_host().reshape(-1, 3)
    for e, (_, w, off, dim, prime) in enumerate(descs):
        exp = orc.eval_dot(sec, w, off, dim, EV_NBITS, EV_EXT, Lp if prime else L)
        assert np.array_equal(got[e], exp), (e, off, dim, prime, [hex(int(v)) for v in got[e]], [hex(int(v)) for v in exp])
        # the oracle's loop of field operations against one integer sum (constant columns: the dot product is n times one product)
        col = np.array([[int(sec[off + j]) for j in range(dim)] + [0] * (3 - dim)], dtype=object)
        lw = _obj((Lp if prime else L)[:3]).reshape(1, 3)
        assert [int(v) for v in exp] == [int(v) * n % P for v in _f3_mul(col, lw)[0]]
