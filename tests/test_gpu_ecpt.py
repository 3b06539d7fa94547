"""The coordinate field `cf` and the XYZZ point formulas of csrc/ecpt_impl.hip.h on chosen operands, for G1 and G2 of BN254 and BLS12-381,
through the probes of csrc/ecpt_probe.hip (compiled as msm.hip compiles the formulas).  Points cross as raw XYZZ limbs, so the test
chooses the lazy representative of every coordinate: X = x + kq for k = 0..7, Y up to exactly 4q, ZZ and ZZZ up to 2q - 1, ZZ != 1.

Two references.  (1) Plain affine arithmetic in Python integers on multiples of the generator (tests/key_check_ref.py's Curve): every
device result must be that point (X / ZZ, Y / ZZZ, the infinity flag, pt_to_std's external Montgomery words).  (2) tests/fe29_model.py's
replay of each formula's sequence of field operations, which checks from the operands' bounds, at every cf_mul / cf_sqr / fe_mul2, the
A B <= floor(R'/q) condition (per component for Fq2, with the 8q - b1 operand that makes it A (B + 8)), at every cf_sub<M> that the
subtrahend is <= M q, and on every result the stored-point invariants; the device must equal it limb for limb.  The unmarked test
runs (2) without a GPU: a swapped operand order at a call site fails there (on the device it would not, on these operands: products
rarely come out far above q, so the subtrahend that may reach 10q stays below 8q).  0.06 to 0.23 s per group on an MI355X."""
import ctypes as C
import functools
import numpy as np
import pytest

from fe29_model import FIELDS, Curve, _b, _flat, _sat, _stack, _val
import key_check_ref as KR

gpu = pytest.mark.gpu
GROUPS = [("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2)]
IDS = [f"{c}_g{g}" for c, g in GROUPS]
E_CFMUL, E_CFSQR, E_CFINV, E_RENORM, E_DBL_AFF, E_DBL, E_MADD, E_ADD, E_NEG, E_TO_STD, E_DBL4, E_ADD4 = range(12)
COORDS = ("X", "Y", "ZZ", "ZZZ")


class Ctx:
    def __init__(self, curve, group):
        self.curve, self.group, self.g2 = curve, group, group == 2
        self.F = FIELDS[curve + "_fq"]
        self.cv = KR.CURVES["BN128" if curve == "bn254" else "BLS12381"]
        self.nc = 2 if self.g2 else 1
        self.model = Curve(self.F, self.g2)
        self.q = self.F.q
        self.mults = [None] + [self.cv.mul(self.cv.gen[group - 1], k) for k in range(1, 14)]       # mults[k] = [k]G, affine over Fq2

    # one coordinate = a list of nc integers (the internal Montgomery value plus a multiple of q)
    def coord(self, x, ks):
        return [x[c] * self.F.Rp % self.q + ks[c] * self.q for c in range(self.nc)]

    def lift(self, P, z, kx, ky, kz):
        """affine P -> X, Y, ZZ, ZZZ with ZZ = z^2: lazy representatives + k q, k per coordinate (a pair per Fq2 coordinate)"""
        cv = self.cv
        zz = cv.fmul(z, z); zzz = cv.fmul(zz, z)
        return [self.coord(cv.fmul(P[0], zz), kx), self.coord(cv.fmul(P[1], zzz), ky), self.coord(zz, kz), self.coord(zzz, kz[::-1])]

    def batch(self, elems, k):
        """coordinate k of a list of elements -> cf of (NR, n) limb batches (one per component)"""
        return [self.F.limbs([e[k][c] for e in elems]) for c in range(self.nc)]

    def cf_V(self, comps, ub):
        vs = [self.model.B.new(l, ub) for l in comps]
        return tuple(vs) if self.g2 else vs[0]

    def point_V(self, elems):
        q = self.q
        return {n: self.cf_V(self.batch(elems, k), ub) for k, (n, ub) in enumerate(zip(COORDS, (8 * q - 1, 4 * q, 2 * q - 1, 2 * q - 1)))}

    def aff_V(self, elems):
        return tuple(self.cf_V(self.batch(elems, k), 2 * self.q - 1) for k in (0, 1))

    def comps(self, cf):
        return [v.l for v in (cf if self.g2 else (cf,))]

    def residue(self, comps, i):
        """element i of a cf given as limb batches -> the Fq2 element it stands for"""
        inv = pow(self.F.Rp, -1, self.q)
        v = [int(self.F.val(l[:, i:i + 1])[0]) * inv % self.q for l in comps]
        return (v[0], v[1] if len(v) > 1 else 0)

    def affine_of(self, pt, i):
        """element i of a point given as {coordinate: [component limb batches]} -> None or the affine point"""
        zz = self.residue(pt["ZZ"], i)
        if zz == (0, 0):
            return None
        cv = self.cv
        return (cv.fmul(self.residue(pt["X"], i), cv.finv(zz)), cv.fmul(self.residue(pt["Y"], i), cv.finv(self.residue(pt["ZZZ"], i))))


@functools.lru_cache(maxsize=None)
def _ctx(curve, group):
    return Ctx(curve, group)


@functools.lru_cache(maxsize=None)
def _cases(curve, group):
    """{label: (family, [operand element lists], [reference affine results])}; every label takes one branch of its formula"""
    cx = _ctx(curve, group)
    cv, q, nc = cx.cv, cx.q, cx.nc
    rng = np.random.default_rng(3810 + 2 * (curve == "bls12_381") + group)
    rnd = lambda: int.from_bytes(rng.bytes(64), "little") % (q - 2) + 2            # noqa: E731
    rz = lambda: (rnd(), rnd() if cx.g2 else 0)                                    # noqa: E731
    kk = lambda i, top: [(i + 3 * c) % top for c in range(nc)]                     # noqa: E731

    def lifted(P, i):
        """representative i of P: X + (i mod 8) q (7: just under 8q), Y + (i mod 4) q, ZZ / ZZZ + (0 or 1) q"""
        return cx.lift(P, rz(), kk(i, 8), kk(i + 1, 4), kk(i, 2))

    def aff(P, i):
        return [cx.coord(P[0], kk(i, 2)), cx.coord(P[1], kk(i + 1, 2))]

    zero = [0] * nc
    infs = [[zero, zero, zero, zero]]                                               # pt_inf(), then ZZ = 0 spelled with q
    for pat in ([q] * nc, [q, 0][:nc], [0, q][:nc]):
        e = lifted(cx.mults[3], len(infs)); e[2] = list(pat); e[3] = list(pat)
        infs.append(e)
    G = cx.mults
    out = {}
    N = 8
    pairs = [(1 + i % 5, 7 + i % 6) for i in range(N)]
    out["add_generic"] = (E_ADD, [[lifted(G[a], i) for i, (a, b) in enumerate(pairs)], [lifted(G[b], i + 5) for i, (a, b) in enumerate(pairs)]],
                          [cv.add(G[a], G[b]) for a, b in pairs])
    same = [2 + i % 4 for i in range(N)]
    out["add_same_point"] = (E_ADD, [[lifted(G[a], i) for i, a in enumerate(same)], [lifted(G[a], i + 3) for i, a in enumerate(same)]], [cv.add(G[a], G[a]) for a in same])
    out["add_opposite"] = (E_ADD, [[lifted(G[a], i) for i, a in enumerate(same)], [lifted(cv.neg(G[a]), i + 3) for i, a in enumerate(same)]], [None] * N)
    out["add_inf_p"] = (E_ADD, [[infs[i % 4] for i in range(N)], [lifted(G[a], i) for i, a in enumerate(same)]], [G[a] for a in same])
    out["add_p_inf"] = (E_ADD, [[lifted(G[a], i) for i, a in enumerate(same)], [infs[i % 4] for i in range(N)]], [G[a] for a in same])
    out["add_inf_inf"] = (E_ADD, [[infs[i % 4] for i in range(N)], [infs[(i + i // 4) % 4] for i in range(N)]], [None] * N)
    out["dbl_generic"] = (E_DBL, [[lifted(G[a], i) for i, a in enumerate(same)]], [cv.add(G[a], G[a]) for a in same])
    out["dbl_inf"] = (E_DBL, [[infs[i % 4] for i in range(4)]], [None] * 4)
    out["dbl_aff"] = (E_DBL_AFF, [[aff(G[a], i) for i, a in enumerate(same)]], [cv.add(G[a], G[a]) for a in same])
    out["madd_generic"] = (E_MADD, [[lifted(G[a], i) for i, (a, b) in enumerate(pairs)], [aff(G[b], i) for i, (a, b) in enumerate(pairs)]], [cv.add(G[a], G[b]) for a, b in pairs])
    out["madd_same_point"] = (E_MADD, [[lifted(G[a], i) for i, a in enumerate(same)], [aff(G[a], i + 1) for i, a in enumerate(same)]], [cv.add(G[a], G[a]) for a in same])
    out["madd_opposite"] = (E_MADD, [[lifted(G[a], i) for i, a in enumerate(same)], [aff(cv.neg(G[a]), i + 1) for i, a in enumerate(same)]], [None] * N)
    out["madd_onto_inf"] = (E_MADD, [[infs[i % 4] for i in range(N)], [aff(G[a], i) for i, a in enumerate(same)]], [G[a] for a in same])
    out["neg_generic"] = (E_NEG, [[lifted(G[a], i) for i, a in enumerate(same)]], [cv.neg(G[a]) for a in same])
    y0 = []
    for i in range(5 if nc == 1 else 10):                                           # Y = 0 spelled 0, q, 2q, 3q, 4q (per component)
        e = lifted(G[2], i); e[1] = [(i % 5) * q, ((i * 2 + i // 5) % 5) * q][:nc]
        y0.append(e)
    out["neg_y_zero"] = (E_NEG, [y0], [None] * len(y0))                            # (no such point on the curve: compared on Y alone)
    return out


def _point_dict(cx, elems):
    return {n: cx.batch(elems, k) for k, n in enumerate(COORDS)}


@functools.lru_cache(maxsize=None)
def _model_results(curve, group):
    """the model's replay of every case: {label: result point as {coordinate: [component limb batches]}}"""
    cx = _ctx(curve, group)
    m = cx.model
    res = {}
    for label, (fam, ops, want) in _cases(curve, group).items():
        if fam == E_ADD:
            r = m.pt_add(cx.point_V(ops[0]), cx.point_V(ops[1]))
        elif fam == E_DBL:
            r = m.pt_dbl(cx.point_V(ops[0]))
        elif fam == E_DBL_AFF:
            r = m.pt_dbl_aff(cx.aff_V(ops[0]))
        elif fam == E_MADD:
            r = m.pt_madd(cx.point_V(ops[0]), cx.aff_V(ops[1]))
        else:
            r = m.pt_neg(cx.point_V(ops[0]))
        m.stored(r, label)
        res[label] = {n: cx.comps(r[n]) for n in COORDS}
    return res


def _check_against_affine(cx, label, pt, want):
    q = cx.q
    F = cx.F
    for n, ub in zip(COORDS, (8 * q - 1, 4 * q, 2 * q - 1, 2 * q - 1)):
        for l in pt[n]:
            assert F.normalised(l) and _b(F.val(l) <= ub).all(), f"{label}: {n} breaks the stored-point invariant"
    for i, w in enumerate(want):
        if label == "neg_y_zero":
            assert cx.residue(pt["Y"], i) == (0, 0)
            continue
        got = cx.affine_of(pt, i)
        assert got == w, f"{label}[{i}]: not the reference's point"
        if w is not None:
            zz, zzz = cx.residue(pt["ZZ"], i), cx.residue(pt["ZZZ"], i)
            assert cx.cv.fmul(cx.cv.fmul(zz, zz), zz) == cx.cv.fmul(zzz, zzz), f"{label}[{i}]: ZZ^3 != ZZZ^2"


# ---- cf operands ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cf_cases(curve, group):
    """{label: (family, [cf operands as lists of component limb batches], [bounds per operand component])}"""
    cx = _ctx(curve, group)
    F, q, nc = cx.F, cx.q, cx.nc
    rng = np.random.default_rng(77 + group)
    rnd = lambda top: int.from_bytes(rng.bytes(64), "little") % top                # noqa: E731

    def forms(ub, n_rand=6):
        f = [F.split(ub), F.split(ub - 1), _sat(F, ub), _flat(F, ub), F.split(0), F.split(q)] + [F.split(rnd(ub + 1)) for _ in range(n_rand)]
        return [x for x in f if x is not None and _val(x) <= ub]

    def cf(ubs):
        """a batch per component cycling through the forms under its own bound, the components out of step"""
        fs = [forms(u) for u in ubs]
        n = 12
        return [_stack(F, [fs[c][(i + 5 * c * (i // 4)) % len(fs[c])] for i in range(n)]) for c in range(nc)]

    out = {}
    if cx.g2:
        out["cf_mul_10q_x_6q_c1_at_8q"] = (E_CFMUL, [cf([10 * q - 1, 10 * q - 1]), cf([6 * q - 1, 8 * q])], [[10 * q - 1] * 2, [6 * q - 1, 8 * q]])
        out["cf_mul_8q_x_2q"] = (E_CFMUL, [cf([8 * q - 1, 8 * q - 1]), cf([2 * q - 1, 2 * q - 1])], [[8 * q - 1] * 2, [2 * q - 1] * 2])
        out["cf_sqr_c0_under_10q_c1_under_2q"] = (E_CFSQR, [cf([10 * q - 1, 2 * q - 1])], [[10 * q - 1, 2 * q - 1]])
        out["cf_sqr_8q"] = (E_CFSQR, [cf([8 * q, 8 * q])], [[8 * q, 8 * q]])
        out["fe_renorm"] = (E_RENORM, [[_stack(F, forms(min(F.limit, 168) * q, 20))]], [[min(F.limit, 168) * q]])
    else:
        out["cf_mul_10q_x_6q"] = (E_CFMUL, [cf([10 * q - 1]), cf([6 * q - 1])], [[10 * q - 1], [6 * q - 1]])
        out["cf_sqr_under_10q"] = (E_CFSQR, [cf([10 * q - 1])], [[10 * q - 1]])
    inv = []
    for i in range(24):
        e = [rnd(2 * q) for _ in range(nc)]
        if i < 8:
            e[i % nc] = (i // 2 % 2) * q                                            # c0 = 0 or c1 = 0 (G1: zero itself), spelled 0 or q
        inv.append([F.split(v) for v in e])
    out["cf_inv"] = (E_CFINV, [[_stack(F, [e[c] for e in inv]) for c in range(nc)]], [[2 * q - 1] * nc])
    return out


def _cf_reference(cx, label, fam, ops, ubs):
    """the model's result (component limb batches) -- None for cf_inv, whose ladder the model does not replay here"""
    m = cx.model
    def mk(o, ub):
        parts = [m.B.new(l, u) for l, u in zip(o, ub)]
        return tuple(parts) if cx.g2 and fam != E_RENORM else parts[0]
    a = [mk(o, ub) for o, ub in zip(ops, ubs)]
    if fam == E_CFMUL:
        return cx.comps(m.cf_mul(a[0], a[1], label + ": "))
    if fam == E_CFSQR:
        return cx.comps(m.cf_sqr(a[0], label + ": "))
    if fam == E_RENORM:
        return [m.B.renorm(a[0]).l]
    m.cf_inv(a[0])
    return None


def _cf_math(cx, fam, ops, i):
    cv = cx.cv
    x = cx.residue(ops[0], i)
    if fam == E_CFMUL:
        return cv.fmul(x, cx.residue(ops[1], i))
    if fam == E_CFSQR:
        return cv.fmul(x, x)
    if fam == E_RENORM:
        return x
    return cv.finv(x) if x != (0, 0) else (0, 0)


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_point_formulas_keep_their_bounds_in_the_model(curve, group):
    """No GPU: the replay of every formula on every case -- the A B condition at every product, b <= M q at every difference, the
    stored-point invariants on every result -- and the results are the reference's affine points.  Case sizes printed (-s)."""
    cx = _ctx(curve, group)
    cases = _cases(curve, group)
    res = _model_results(curve, group)
    for label, (fam, ops, want) in cases.items():
        print(f"{curve} g{group} {label}: {len(want)} elements")
        assert len(want) > 0
        _check_against_affine(cx, label, res[label], want)
    # representatives the cases must contain: X just under 8q, Y at exactly 4q, infinity spelled with q
    xs = [e[0][0] // cx.q for label, (fam, ops, want) in cases.items() if fam in (E_ADD, E_DBL, E_MADD, E_NEG) for e in ops[0]]
    assert max(xs) == 7 and min(xs) == 0
    assert any(e[1][0] == 4 * cx.q for e in cases["neg_y_zero"][1][0])
    assert any(e[2][0] == cx.q for e in cases["add_inf_p"][1][0])
    # pt_to_std's call sites on every finite input and result
    for label, (fam, ops, want) in cases.items():
        if fam in (E_ADD, E_DBL, E_NEG) and want[0] is not None and "inf" not in label:
            cx.model.pt_to_std_bounds(cx.point_V(ops[0]))
    for label, r in res.items():
        if cases[label][2][0] is not None and label != "neg_y_zero":
            pv = {n: cx.cf_V(r[n], ub) for n, ub in zip(COORDS, (8 * cx.q - 1, 4 * cx.q, 2 * cx.q - 1, 2 * cx.q - 1))}
            cx.model.pt_to_std_bounds(pv)


@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_cf_operands_keep_their_bounds_in_the_model(curve, group):
    """No GPU: cf_mul / cf_sqr / cf_inv / fe_renorm at the bounds their call sites reach, replayed by the model, against Fq2 arithmetic"""
    cx = _ctx(curve, group)
    F, m = cx.F, cx.model.B.m
    for label, (fam, ops, ubs) in _cf_cases(curve, group).items():
        r = _cf_reference(cx, label, fam, ops, ubs)
        n = ops[0][0].shape[1]
        print(f"{curve} g{group} {label}: {n} elements")
        if r is not None:
            for i in range(n):
                assert cx.residue(r, i) == _cf_math(cx, fam, ops, i), f"{label}[{i}]"
    if cx.g2:                                                    # cf_inv: the norm a0^2 + a1^2 before fe_renorm, as the lazy sum of two products
        a = _cf_cases(curve, group)["cf_inv"][1][0]
        nrm = F.val(m.add(m.mul(a[0], a[0]), m.mul(a[1], a[1])))
        sizes = {f"norm_in_[{k}q,{k + 1}q)": int((_b(nrm >= k * F.q) & _b(nrm < (k + 1) * F.q)).sum()) for k in range(4)}
        print(f"{curve} g2 cf_inv: " + ", ".join(f"{k}={v}" for k, v in sizes.items()))
        assert sizes["norm_in_[0q,1q)"] > 0 and sum(v for k, v in sizes.items() if k != "norm_in_[0q,1q)") > 0
        zc = [cx.residue(a, i) for i in range(a[0].shape[1])]
        assert any(z[0] == 0 and z[1] != 0 for z in zc) and any(z[1] == 0 and z[0] != 0 for z in zc)


# ---- on the device -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)
    return zk


def _call(dev, cx, fam, inp, out_words):
    fn = dev.lib().zk_ecpt_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    out = np.zeros((inp.shape[0], out_words), np.uint32)
    assert fn(0 if cx.curve == "bn254" else 1, cx.group, fam, inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), inp.shape[0]) == 0, dev.lib().zk_last_error()
    return out


def _cf_words(comps):
    return np.concatenate([l.T.astype(np.uint32) for l in comps], axis=1)


def _pt_words(cx, elems):
    return np.concatenate([_cf_words(cx.batch(elems, k)) for k in range(len(elems[0]))], axis=1)


def _pt_from_words(cx, w):
    NR, nc = cx.F.NR, cx.nc
    return {n: [w[:, (k * nc + c) * NR:(k * nc + c + 1) * NR].T.astype(object) for c in range(nc)] for k, n in enumerate(COORDS)}


def _ragged(rows):
    """one ragged final block: pad with copies of the first row to a count that is no multiple of the block of 64 lanes (16 quads)"""
    return np.concatenate([rows, rows[:1]], axis=0) if rows.shape[0] % 16 == 0 else rows


@gpu
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_points_match_the_affine_reference_and_the_model(dev, curve, group):
    """pt_add, pt_dbl, pt_dbl_aff, pt_madd, pt_neg: the reference's affine point, the infinity flag, the stored-point invariants and
    ZZ^3 = ZZZ^2 on every output, and limb for limb the model's replay; pt_add4 / pt_dbl4 bit for bit pt_add / pt_dbl with the four lanes
    agreeing; pt_to_std of every finite operand and result = the reference's external Montgomery words."""
    cx = _ctx(curve, group)
    F, NR, nc = cx.F, cx.F.NR, cx.nc
    PW = 4 * nc * NR
    cases, model = _cases(curve, group), _model_results(curve, group)
    finite, finite_want = [], []
    for fam in (E_ADD, E_DBL, E_DBL_AFF, E_MADD, E_NEG):
        labels = [l for l, c in cases.items() if c[0] == fam]
        rows = _ragged(np.concatenate([np.concatenate([_pt_words(cx, o) for o in cases[l][1]], axis=1) for l in labels], axis=0))
        assert rows.shape[0] % 64 and rows.shape[0] % 16
        out = _call(dev, cx, fam, rows, PW)
        quad = _call(dev, cx, {E_ADD: E_ADD4, E_DBL: E_DBL4}[fam], rows, PW + 1) if fam in (E_ADD, E_DBL) else None
        if quad is not None:
            assert (quad[:, PW] == 1).all(), "the four lanes of a quad disagree"
            assert np.array_equal(quad[:, :PW], out), "pt_add4 / pt_dbl4 is not bit for bit pt_add / pt_dbl"
        o = 0
        for l in labels:
            n = len(cases[l][2])
            got = _pt_from_words(cx, out[o:o + n]); o += n
            _check_against_affine(cx, l, got, cases[l][2])
            for name in COORDS:
                for c in range(nc):
                    assert _b(got[name][c] == model[l][name][c]).all(), f"{l}: {name} differs from the model's limbs"
            if l != "neg_y_zero":
                for i, w in enumerate(cases[l][2]):
                    if w is not None:
                        finite.append(out[o - n + i]); finite_want.append(w)
            if fam in (E_ADD, E_DBL, E_NEG) and "inf" not in l and l != "neg_y_zero":
                src = _pt_words(cx, cases[l][1][0])
                ref_in = [cx.affine_of(_pt_from_words(cx, src), i) for i in range(n)]
                finite += list(src); finite_want += ref_in
    rows = _ragged(np.stack(finite))
    std = _call(dev, cx, E_TO_STD, rows, 2 * nc * F.NL)
    for i, w in enumerate(finite_want):
        want_words = []
        for coord in w:
            for c in range(nc):
                v = coord[c] * F.R % F.q
                want_words += [(v >> (32 * k)) & 0xFFFFFFFF for k in range(F.NL)]
        assert [int(x) for x in std[i]] == want_words, f"pt_to_std[{i}]"


@gpu
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_cf_matches_fq2_arithmetic_and_the_model(dev, curve, group):
    """cf_mul, cf_sqr, fe_renorm: the model's limbs, the mathematical product, components below 2q and normalised; cf_inv: the inverse
    (0 -> 0), components below 2q and normalised"""
    cx = _ctx(curve, group)
    F, NR, nc = cx.F, cx.F.NR, cx.nc
    for label, (fam, ops, ubs) in _cf_cases(curve, group).items():
        rows = np.concatenate([_cf_words(o) for o in ops], axis=1)
        assert rows.shape[0] % 64
        k = 1 if fam == E_RENORM else nc
        out = _call(dev, cx, fam, rows, k * NR)
        got = [out[:, c * NR:(c + 1) * NR].T.astype(object) for c in range(k)]
        ref = _cf_reference(cx, label, fam, ops, ubs)
        for c in range(k):
            assert F.normalised(got[c]) and _b(F.val(got[c]) < 2 * F.q).all(), f"{label}: component {c} is no normalised value below 2q"
            if ref is not None:
                assert _b(got[c] == ref[c]).all(), f"{label}: component {c} differs from the model's limbs"
        for i in range(rows.shape[0]):
            assert cx.residue(got, i) == _cf_math(cx, fam, ops, i), f"{label}[{i}]"
