"""The pairing tower of csrc/pairing_impl.hip.h on chosen operands, for BN254 and BLS12-381, through the probes of csrc/pairing_probe.hip
(compiled as pairing.hip compiles the tower): the Fq2 operations as pairing.o builds them, cf_mul_xi / cf_red / cf_neg, the Jacobian line
steps, the whole line table of g2_lines_kernel, the Fq12 primitives on groups of eight lanes, fe_to_canon_words and final_exp_dev.  Operands
cross as raw internal limbs, so the test chooses the lazy representative r + kq of every Fq component up to the bound its call site declares.

Two references.  (1) tests/pairing_tower_model.py replays each function operation by operation on fe29_model's bounded values: the device
must return its limbs exactly, and from the operands' declared bounds it checks A B (+ 8q) <= floor(R'/q) at every product and the
subtrahend <= M q at every cf_sub<M>.  (2) tools/pairing_constants.py's `Model` and `Curve` on Python integers: every device result
stands for the value the plain tower arithmetic gives, a line vanishes at the points it passes through, a cyclotomic squaring is the square,
and final_exp_dev's canonical words are Model.final_exp's.  The unmarked tests run the model without a GPU: the operand classes, every
call site of the three kernels at its worst-case bounds, and two deliberately wrong replays that must be rejected.

Wall time on an MI355X per GPU test (BN254 / BLS12-381), the model's replay shared with the unmarked tests that ran before: Fq2 0.22 (with the
first call's start-up) / 0.08 s, line steps 0.03 / 0.04 s, line table 0.03 / 0.02 s, each Fq12 primitive 0.01 to 0.02 s, canonical words
under 0.005 s, final exponentiation 0.15 / 0.34 s.  The replay itself (no GPU): 2.6 / 3.8 s for all cases, 0.6 / 0.9 s for the call sites.
A record, not a limit."""
import ctypes as C
import functools
import pathlib
import sys
import numpy as np
import pytest

from fe29_model import FIELDS, LB, LMASK, ModelError, _b
from pairing_tower_model import Tower, contract, replay_sites

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tools"))
import pairing_constants as pc  # noqa: E402

gpu = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
T_CF, T_XI, T_LINE_DBL, T_LINE_ADD, T_LINES, T_F12_MUL, T_F12_TAB, T_F12_LINE, T_F12_CYC, T_F12_MAPS, T_CANON, T_FINAL_EXP = range(12)
F12_COUNTS = (1, 7, 8, 9, 67)                      # a lone group, a workgroup less one, a full one, one group past it, nine workgroups with idle groups
RES_CLASSES = {"0", "1", "q-1", "R'", "q-R'", "ones", "limb", "rand"}


class Ctx:
    def __init__(self, name):
        self.name, self.idx = name, CURVES.index(name)
        self.F, self.C = FIELDS[name + "_fq"], (pc.BN254, pc.BLS12_381)[self.idx]
        self.M, self.tw = pc.Model(self.C), Tower(self.F, self.C)
        self.q, self.Rp, self.NR, self.NL = self.F.q, self.F.Rp, self.F.NR, self.F.NL
        self.Rinv = pow(self.Rp, -1, self.q)
        self.W = 2 * self.NR
        self.ct = contract(self.q)
        rng = np.random.default_rng(2950 + self.idx)
        self.rnd = lambda top: int.from_bytes(rng.bytes(64), "little") % top
        # residues: (class, value) -- raw internal values below q
        q, top = self.q, self.q.bit_length()
        res = [("0", 0), ("1", 1), ("q-1", q - 1), ("R'", self.Rp % q), ("q-R'", q - self.Rp % q), ("ones", (1 << (top - 1)) - 1)]
        res += [("limb", 1 << (LB * i)) for i in range(1, self.NR) if (1 << (LB * i)) < q]
        res += [("ones", LMASK << (LB * i)) for i in range(self.NR) if (LMASK << (LB * i)) < q]
        res += [("rand", self.rnd(q)) for _ in range(6)]
        self.res_class = {v: c for c, v in reversed(res)}
        self.RES = [v for _, v in res]

    def mont(self, x): return x * self.Rp % self.q
    def res(self, v): return int(v) * self.Rinv % self.q
    def res2(self, v): return (self.res(v[0]), self.res(v[1]))
    def mont2(self, x, k=(0, 0)): return (self.mont(x[0]) + k[0] * self.q, self.mont(x[1]) + k[1] * self.q)

    def draw(self, ub, n, salt=0):
        """n representatives r + kq <= ub: k runs through 0 .. ub // q (the top one is the bound itself when it is a multiple of q), r
        through the residues, the two out of step"""
        q, R = self.q, self.RES
        K = ub // q + 1
        out = []
        for i in range(n):
            v = R[(i // K + i + 5 * salt) % len(R)] + ((i + salt) % K) * q
            out.append(v if v <= ub else ub)
        return out

    def rand2(self): return (self.rnd(self.q), self.rnd(self.q))


@functools.lru_cache(maxsize=None)
def _ctx(name):
    return Ctx(name)


class Case:
    """vals: (n, S, 2) internal integers (S Fq2 slots per element); ubs: per slot one bound or a pair; ops: which results the call site's
    bounds cover (None: all); info: per element, what the value checks need; classes: the operand classes the case stands for"""
    def __init__(self, label, fam, elems, ubs, ops=None, info=None, classes=()):
        self.label, self.fam, self.ubs, self.ops, self.info, self.classes = label, fam, ubs, ops, info, set(classes)
        self.vals = np.empty((len(elems), len(ubs), 2), dtype=object)
        for i, e in enumerate(elems):
            assert len(e) == len(ubs), label
            for s, v in enumerate(e):
                self.vals[i, s, 0], self.vals[i, s, 1] = int(v[0]), int(v[1])
        self.n = len(elems)

    def ub(self, s, c):
        u = self.ubs[s]
        return u[c] if isinstance(u, (tuple, list)) else u


def _slots(cx, n, ubs, salt=0):
    """n elements of len(ubs) slots drawn from the pool under each slot's bound"""
    cols = []
    for s, u in enumerate(ubs):
        pair = u if isinstance(u, (tuple, list)) else (u, u)
        cols.append([cx.draw(pair[c], n, salt + 2 * s + c) for c in (0, 1)])
    return [[(cols[s][0][i], cols[s][1][i]) for s in range(len(ubs))] for i in range(n)]


# ---- Fq12 operands ------------------------------------------------------------------------------------------------------------------
def _zero(cx, i): return ((i % 2) * cx.q, ((i // 2) % 2) * cx.q)              # zero spelled 0 or q per component


def _f12_operands(cx, ub, salt):
    """{class: [elements]}; an element is six (c0, c1) internal values"""
    q = cx.q
    one = (cx.Rp % q, 0)
    d = lambda i: tuple(cx.draw(ub, 2, salt + i))                             # noqa: E731
    out = {"one": [[one] + [(0, 0)] * 5, [(one[0] + q, q)] + [_zero(cx, j) for j in range(5)]]}
    for k in range(6):
        out[f"w^{k}"] = [[d(7 * k + j) if j == k else _zero(cx, j + k) for j in range(6)]]
    out["Fq2"] = out["w^0"]
    out["Fq6"] = [[d(50 + j) if j % 2 == 0 else _zero(cx, j) for j in range(6)]]
    out["2q-1"] = [[(2 * q - 1, 2 * q - 1)] * 6]
    vals = cx.draw(ub, 12 * 24, salt + 9)
    out["random"] = [[(vals[12 * e + 2 * j], vals[12 * e + 2 * j + 1]) for j in range(6)] for e in range(24)]
    return out


F12_CLASSES = {"one", "Fq2", "Fq6", "2q-1", "random"} | {f"w^{k}" for k in range(6)}


def _fill(elems, n):
    return [elems[i % len(elems)] for i in range(n)]


def _cyclotomic(cx, f):
    M = cx.M
    g = M.mul(M.conj6(f), M.inv(f))
    return M.mul(M.frob2(g), g)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases(name):
    cx = _ctx(name)
    q, Cv, ct = cx.q, cx.C, cx.ct
    f2 = Cv.f2mul
    cases = []
    # -- CF: cf_mul / cf_sqr / cf_inv at the bounds of the tower's call sites
    cases.append(Case("cf_10q_x_6q", T_CF, _slots(cx, 260, [10 * q - 1, 6 * q - 1]), [10 * q - 1, 6 * q - 1], ops={"mul"}))      # (S - X3) M
    cases.append(Case("cf_8q_x_2q", T_CF, _slots(cx, 210, [8 * q - 1, 2 * q], 1), [8 * q - 1, 2 * q], ops={"mul"}))              # xi b times a
    cases.append(Case("cf_6q_x_10q_c1_8q", T_CF, _slots(cx, 260, [6 * q - 1, (10 * q - 1, 8 * q)], 2), [6 * q - 1, (10 * q - 1, 8 * q)], ops={"mul", "sqr"}))   # cf_sqr at M; a second operand with c1 at exactly 8q
    cases.append(Case("cf_4q_x_4q", T_CF, _slots(cx, 110, [4 * q - 1, 4 * q - 1], 3), [4 * q - 1, 4 * q - 1], ops={"mul", "sqr"}))  # Z^2, H^2, (V - X3) R
    el = _slots(cx, 60, [2 * q - 1, 2 * q - 1], 4)
    for i in range(8):                                                          # c0 = 0 or c1 = 0, spelled 0 or q; zero itself
        z = (i // 2 % 2) * q
        el[i][0] = (z, el[i][0][1]) if i % 2 == 0 else (el[i][0][0], z)
    el[8][0] = (0, 0); el[9][0] = (q, q)
    cases.append(Case("cf_2q_inverse", T_CF, el, [2 * q - 1, 2 * q - 1], ops={"mul", "sqr", "inv"}))
    # -- XI: cf_mul_xi takes < 4q, cf_neg <= 2q, cf_red whatever a product with one admits below the largest sum the tower forms (40q)
    cases.append(Case("xi_4q", T_XI, _slots(cx, 110, [4 * q - 1]), [4 * q - 1], ops={"xi", "red"}))
    cases.append(Case("neg_2q", T_XI, _slots(cx, 90, [2 * q], 1), [2 * q], ops={"xi", "red", "neg"}))
    cases.append(Case("red_40q", T_XI, _slots(cx, 200, [40 * q - 1], 2), [40 * q - 1], ops={"red"}))
    # -- the line steps on points: T = [k]Q lifted with Z = 1, random Z, Z at 4q - 1
    Q = Cv.g2
    ks = [1, 2, 3, 5, 7] + [cx.rnd(Cv.r - 1) + 1 for _ in range(3)]
    pts = [Cv.g2_mul(k, Q) for k in ks]
    one = cx.Rp % q

    def lift(P, Z, i):
        Zr = cx.res2(Z)
        ZZ = f2(Zr, Zr)
        return [cx.mont2(f2(P[0], ZZ), (i % 2, (i + 1) % 2)), cx.mont2(f2(P[1], f2(ZZ, Zr)), ((i // 2) % 2, (i + 1) // 2 % 2)), Z]

    def zs(i):
        return [("Z=1", (one, 0)), ("Z=1", (one + q, q)), ("Z=4q-1", (4 * q - 1, 4 * q - 1)),
                ("Z random", (cx.rnd(q) + (i % 4) * q, cx.rnd(q) + ((i + 1) % 4) * q)), ("Z random", (cx.rnd(q) + ((i + 2) % 4) * q, cx.rnd(q) + ((i + 3) % 4) * q))]
    el, info, cl = [], [], set()
    for i, P in enumerate(pts):
        for j, (zl, Z) in enumerate(zs(i)):
            el.append(lift(P, Z, i + j)); info.append({"T": P}); cl |= {zl, "small k" if ks[i] < 8 else "random k"}
    tb = [ct["T.X"], ct["T.Y"], ct["T.Z"]]
    cases.append(Case("line_dbl_points", T_LINE_DBL, el, tb, info=info, classes=cl))
    cases.append(Case("line_dbl_pool", T_LINE_DBL, _slots(cx, 80, tb, 3), tb))               # the formulas do not need the curve equation
    el, info, cl = [], [], set()
    for i, P in enumerate(pts):
        for j, (zl, Z) in enumerate(zs(i + 1)):
            P2 = pts[(i + 1 + j % 3) % len(pts)]
            el.append(lift(P, Z, i + j) + [cx.mont2(P2[0], (j % 2, i % 2)), cx.mont2(P2[1], ((i + j) % 2, (j + 1) % 2))])
            info.append({"T": P, "P2": P2}); cl |= {zl, "small k" if ks[i] < 8 else "random k"}
    ab = tb + [ct["x2"], ct["y2"]]
    cases.append(Case("line_add_points", T_LINE_ADD, el, ab, info=info, classes=cl))
    cases.append(Case("line_add_pool", T_LINE_ADD, _slots(cx, 80, ab, 5), ab))               # reaches y2 at exactly 2q
    # -- Fq12
    n = F12_COUNTS[-1]
    A, Bo = _f12_operands(cx, 2 * q, 0), _f12_operands(cx, 2 * q, 11)                        # f12_conj6 hands on <= 2q
    mono = [(A[f"w^{i}"][0], Bo[f"w^{j}"][0]) for i in range(6) for j in range(6)]
    mixed = [(A["one"][0], Bo["random"][0]), (A["random"][0], Bo["one"][1]), (A["Fq2"][0], Bo["Fq6"][0]), (A["Fq6"][0], Bo["Fq2"][0]), (A["2q-1"][0], Bo["2q-1"][0])]
    pairs = mono + mixed + [(A["random"][i], Bo["random"][i + 1]) for i in range(1, 23)]
    cases.append(Case("f12_mul", T_F12_MUL, _fill([a + b for a, b in pairs], n), [2 * q] * 12, classes=F12_CLASSES))
    # a table entry: g below 2q and xi g as cf_mul_xi leaves it (BN254: renormalised; BLS12-381: g0 - g1 + 4q, g0 + g1)
    xb = (2 * q - 1, 2 * q - 1) if cx.tw.xi0 == 9 else (6 * q - 1, 4 * q - 1)
    G, A1 = _f12_operands(cx, 2 * q - 1, 23), _f12_operands(cx, 2 * q - 1, 5)
    gl = [G[f"w^{j}"][0] for j in range(6)] + [G["one"][0], G["Fq6"][0], G["2q-1"][0]] + G["random"][:8]

    def with_xi(g, i):
        out = []
        for j, v in enumerate(g):
            x = f2(Cv.xi, cx.res2(v))
            out.append(tuple(cx.mont(x[c]) + ((i + j + c) % ((xb[c] + 1) // q)) * q for c in (0, 1)))
        return g + out
    al = [A1[f"w^{i}"][0] for i in range(6)]
    tabs = [al[i] + with_xi(gl[j], i + j) for i in range(6) for j in range(6)] + [A1["random"][i] + with_xi(gl[i % len(gl)], i) for i in range(17)]
    tabs += [A1["one"][0] + with_xi(gl[7], 1), A1["2q-1"][0] + with_xi(gl[8], 2), A1["Fq6"][0] + with_xi(gl[6], 3)]
    cases.append(Case("f12_mul_tab", T_F12_TAB, _fill(tabs, n), [2 * q - 1] * 12 + [xb] * 6, classes=F12_CLASSES))
    # a line: (vy, vx, c0) in the order of the curve's twist type, and the skip form
    worst = [max(a, b) for a, b in zip(ct["dbl"], ct["add"])]
    vb = [2 * q - 1, 2 * q - 1, worst[2]] if Cv.dtype else [worst[2], 2 * q - 1, 2 * q - 1]
    fl = [A1["one"][0], A1["one"][1], A1["Fq6"][0], A1["2q-1"][0]] + [A1[f"w^{i}"][0] for i in range(6)] + A1["random"][:12]
    vs = _slots(cx, 40, vb, 7)
    skip = [(one, 0), (0, 0), (0, 0)]
    ln = [fl[i % len(fl)] + vs[i] for i in range(40)] + [fl[i] + skip for i in range(len(fl))]
    cases.append(Case("f12_mul_line", T_F12_LINE, _fill(ln, n), [2 * q - 1] * 6 + vb, classes=F12_CLASSES | {"skip", "D-type" if Cv.dtype else "M-type"}))
    cyc, info = [], []
    for i in range(7):
        g = _cyclotomic(cx, [cx.rand2() for _ in range(6)])
        cyc.append([cx.mont2(v, ((i + j) % 2, (i + j // 2) % 2)) for j, v in enumerate(g)]); info.append("cyclotomic")
    cyc += [A["one"][0], A["one"][1]]; info += ["cyclotomic"] * 2                              # (-1 is not: the subgroup's order q^4 - q^2 + 1 is odd)
    C2 = _f12_operands(cx, 2 * q - 1, 31)
    other = [C2[f"w^{i}"][0] for i in range(6)] + [C2["Fq6"][0], C2["2q-1"][0]] + C2["random"]
    cases.append(Case("f12_cyc_sqr", T_F12_CYC, _fill(cyc + other, n), [2 * q - 1] * 6, info=_fill(info + [None] * len(other), n), classes=F12_CLASSES | {"cyclotomic"}))
    maps = A["one"] + [A[f"w^{i}"][0] for i in range(6)] + [A["Fq6"][0], A["2q-1"][0]] + A["random"]
    cases.append(Case("f12_maps", T_F12_MAPS, _fill(maps, n), [2 * q] * 6, classes=F12_CLASSES))
    return cases


def _coverage(cx, cases, fam):
    """per family: the residue classes reached; per case and declared bound, the k of r + kq that are missing (and the bound itself where
    it is a multiple of q, the comment's <=)"""
    classes, gaps = set(), []
    for c in cases:
        if c.fam != fam:
            continue
        ks = {}
        for s in range(len(c.ubs)):
            for comp in (0, 1):
                v = [int(x) for x in c.vals[:, s, comp]]
                classes |= {cx.res_class.get(x % cx.q, "other") for x in v}
                ks.setdefault(c.ub(s, comp), set()).update((x // cx.q, x) for x in v)
        for ub, seen in ks.items():
            missing = set(range(ub // cx.q + 1)) - {k for k, _ in seen}
            on_curve = c.info is not None and c.fam in (T_LINE_DBL, T_LINE_ADD)        # a point's coordinate is no multiple of q: the pool case has it
            if on_curve:
                missing.discard(ub // cx.q if ub % cx.q == 0 else -1)
            if missing or (ub % cx.q == 0 and not on_curve and ub not in {x for _, x in seen}):
                gaps.append((c.label, ub // cx.q, sorted(missing)))
    return classes, gaps


# ---- LINES, CANON, FINAL_EXP: operands that are not Fq2 slots ---------------------------------------------------------------------------
def _f2sqrt(Cv, a):
    """a square root in Fq2 = Fq[u]/(u^2 + 1), q = 3 mod 4, or None"""
    q = Cv.q
    if a == (0, 0):
        return a
    s = pow((a[0] * a[0] + a[1] * a[1]) % q, (q + 1) // 4, q)
    for sg in (s, q - s):
        h = (a[0] + sg) * pow(2, -1, q) % q
        x0 = pow(h, (q + 1) // 4, q)
        if x0 * x0 % q == h and x0:
            r = (x0, a[1] * pow(2 * x0, -1, q) % q)
            if Cv.f2mul(r, r) == a:
                return r
    return None


@functools.lru_cache(maxsize=None)
def _lines_points(name):
    """[(class, (x, y) as Fq2 residues)]"""
    cx = _ctx(name)
    Cv, q = cx.C, cx.q
    out = [("subgroup", Cv.g2), ("subgroup", Cv.g2_mul(cx.rnd(Cv.r - 1) + 1, Cv.g2))]
    while len(out) < 3:
        x = cx.rand2()
        y = _f2sqrt(Cv, Cv.f2add(Cv.f2mul(x, Cv.f2mul(x, x)), Cv.bt))
        if y is not None and Cv.g2_mul(Cv.r, (x, y)) is not None:
            out.append(("twist point outside the subgroup", (x, y)))
    if Cv.bn:
        out += [("x.c1 = 0", ((cx.rnd(q), 0), cx.rand2())), ("y.c1 = 0", (cx.rand2(), (cx.rnd(q), 0)))]
    out.append(("all-zero encoding", ((0, 0), (0, 0))))
    return out


def _std_words(cx, vals):
    """Fq residues -> (n, NL) external Montgomery words"""
    return np.array([[((v * cx.F.R % cx.q) >> (32 * k)) & 0xFFFFFFFF for k in range(cx.NL)] for v in vals], dtype=np.uint32)


def _canon_words(cx, v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(cx.NL)]


@functools.lru_cache(maxsize=None)
def _lines_model(name):
    """(input rows, the model's table as limb batches per step and coefficient, the value reference per point)"""
    cx = _ctx(name)
    pts = [P for _, P in _lines_points(name)]
    rows = np.concatenate([_std_words(cx, [P[0][0] for P in pts]), _std_words(cx, [P[0][1] for P in pts]),
                           _std_words(cx, [P[1][0] for P in pts]), _std_words(cx, [P[1][1] for P in pts])], axis=1)
    w = [rows[:, k * cx.NL:(k + 1) * cx.NL].T.astype(object) for k in range(4)]
    qx, qy = cx.tw.cf_from_std((w[0], w[1])), cx.tw.cf_from_std((w[2], w[3]))
    ct = cx.ct

    def promised(kind, T, ln):
        for nm in "XYZ": cx.tw.within(T[nm], ct["T." + nm], f"{kind} T.{nm}")
        for c, ub, nm in zip(ln, ct[kind], ("cY", "cX", "c0")): cx.tw.within(c, ub, f"{kind} {nm}")
    table = cx.tw.lines(qx, qy, on_step=promised)
    return rows, table, [cx.M.lines(P) for P in pts]


@functools.lru_cache(maxsize=None)
def _canon_values(name):
    """[(class, internal value)]: the residue x the words must spell, as x R' mod q + kq"""
    cx = _ctx(name)
    q = cx.q
    xs = [("0", 0), ("1", 1), ("q-1", q - 1)]
    xs += [("word boundary", 1 << b) for j in range(1, cx.NL) for b in (32 * j - 1, 32 * j) if (1 << b) < q]
    xs += [("limb boundary", 1 << b) for i in range(1, cx.NR) for b in (LB * i - 1, LB * i) if (1 << b) < q]
    xs += [("random", cx.rnd(q)) for _ in range(8)]
    out = [(c, cx.mont(x) + (i % 2) * q) for i, (c, x) in enumerate(xs)] + [(c, cx.mont(x) + ((i + 1) % 2) * q) for i, (c, x) in enumerate(xs)]
    return out + [("pool", v) for v in cx.draw(2 * q - 1, 60)]


@functools.lru_cache(maxsize=None)
def _final_exp_values(name):
    """[(class, f as six internal Fq2 values)]"""
    cx = _ctx(name)
    Cv, M, q = cx.C, cx.M, cx.q
    z = (0, 0)
    mil = M.miller([(Cv.g1_mul(5, Cv.g1), Cv.g2_mul(7, Cv.g2))])
    unit = [cx.rand2() for _ in range(6)]
    out = [("1", [cx.mont2((1, 0))] + [z] * 5), ("1", [cx.mont2((1, 0), (1, 1))] + [(q, 0), (0, q), z, (q, q), z]),
           ("-1", [cx.mont2((q - 1, 0))] + [z] * 5), ("Fq2", [cx.mont2(cx.rand2(), (0, 1))] + [z] * 5),
           ("unit in [q, 2q)", [cx.mont2(v, (1, 1)) for v in unit]), ("Miller value", [cx.mont2(v) for v in mil]),
           ("Miller value", [cx.mont2(v, (j % 2, (j + 1) % 2)) for j, v in enumerate(mil)])]
    if not Cv.bn:                                                               # as miller_kernel's closing f12_conj6 leaves it: 2q - a
        out.append(("Miller value", [v if j % 2 == 0 else tuple((2 * q - cx.mont(c)) for c in Cv.f2neg(cx.res2(v))) for j, v in enumerate(out[5][1])]))
    return out


# ---- the model's replay of a case -----------------------------------------------------------------------------------------------------
def _limbs(cx, case, s):
    return (cx.F.limbs(case.vals[:, s, 0]), cx.F.limbs(case.vals[:, s, 1]))


@functools.lru_cache(maxsize=None)
def _model(name, label):
    """per output slot the model's cf (a pair of bounded values), or None where the case's bounds do not cover the operation"""
    cx = _ctx(name)
    case = {c.label: c for c in _cases(name)}[label]
    tw, cv, ct = cx.tw, cx.tw.cv, cx.ct
    a = [tw.cf_new(_limbs(cx, case, s), case.ubs[s], f"{label} slot {s}") for s in range(len(case.ubs))]
    ops, fam = case.ops, case.fam
    if fam == T_CF:
        return [cv.cf_mul(a[0], a[1], label + ": ") if "mul" in ops else None, cv.cf_sqr(a[0], label + ": ") if "sqr" in ops else None,
                cv.cf_inv(a[0], replay=True) if "inv" in ops else None]
    if fam == T_XI:
        return [tw.cf_mul_xi(a[0], label + ": ") if "xi" in ops else None, cv.cf_red(a[0]) if "red" in ops else None,
                cv.cf_neg(a[0], label + ": ") if "neg" in ops else None]
    if fam in (T_LINE_DBL, T_LINE_ADD):
        T = {"X": a[0], "Y": a[1], "Z": a[2]}
        kind = "dbl" if fam == T_LINE_DBL else "add"
        T2, ln = tw.line_dbl(T) if fam == T_LINE_DBL else tw.line_add(T, a[3], a[4])
        for nm in "XYZ": tw.within(T2[nm], ct["T." + nm], f"{label} T.{nm}")
        for c, ub, nm in zip(ln, ct[kind], ("cY", "cX", "c0")): tw.within(c, ub, f"{label} {nm}")
        return [T2["X"], T2["Y"], T2["Z"], *ln]
    if fam == T_F12_MAPS:
        r0, r1 = tw.f12_conj6(a), tw.f12_frob2(a)
        for x in r0: tw.within(x, ct["f12_conj6"], label + " conj6")
        for x in r1: tw.within(x, ct["f12"], label + " frob2")
        return r0 + r1
    r = {T_F12_MUL: lambda: tw.f12_mul(a[:6], a[6:]), T_F12_TAB: lambda: tw.f12_mul_tab(a[:6], a[6:12], a[12:]),
         T_F12_LINE: lambda: tw.f12_mul_line(a[:6], a[6], a[7], a[8]), T_F12_CYC: lambda: tw.f12_cyc_sqr(a)}[fam]()
    for x in r: tw.within(x, ct["f12"], label)
    return r


def _values(cx, case, r):
    """the plain tower arithmetic on the residues r of one element's slots: the residues of the result slots"""
    Cv, M, fam = cx.C, cx.M, case.fam
    if fam == T_CF:
        return [Cv.f2mul(r[0], r[1]), Cv.f2mul(r[0], r[0]), Cv.f2inv(r[0]) if r[0] != (0, 0) else (0, 0)]
    if fam == T_XI:
        return [Cv.f2mul(Cv.xi, r[0]), r[0], Cv.f2neg(r[0])]
    if fam == T_LINE_DBL:
        T, ln = M.line_dbl(tuple(r))
        return [*T, *ln]
    if fam == T_LINE_ADD:
        T, ln = M.line_add(tuple(r[:3]), r[3], r[4])
        return [*T, *ln]
    if fam == T_F12_MUL:
        return M.mul(r[:6], r[6:])
    if fam == T_F12_TAB:
        assert r[12:] == [Cv.f2mul(Cv.xi, g) for g in r[6:12]]
        return M.mul(r[:6], r[6:12])
    if fam == T_F12_LINE:
        ln = (r[6], r[7], r[8]) if Cv.dtype else (r[8], r[7], r[6])          # Model.line_mul takes (cY yP, cX xP, c0) at P = (1, 1)
        return M.line_mul(r[:6], ln, (1, 1))
    if fam == T_F12_CYC:
        return M.cyc_sqr(r)
    return M.conj6(r) + M.frob2(r)


def _line_geometry(cx, case, i, r_in, r_out):
    """element i of a line case on points: T' is the reference's point and the line vanishes where it must"""
    Cv = cx.C
    inf = case.info[i]
    P, P2 = inf["T"], inf.get("P2")
    want = Cv.g2_add(P, P2 if P2 is not None else P)
    X3, Y3, Z3, cY, cX, c0 = r_out
    zi = Cv.f2inv(Z3); zi2 = Cv.f2mul(zi, zi)
    assert (Cv.f2mul(X3, zi2), Cv.f2mul(Y3, Cv.f2mul(zi2, zi))) == want, f"{case.label}[{i}]: T' is not the reference's point"
    at = lambda p: Cv.f2add(Cv.f2add(Cv.f2mul(cY, p[1]), Cv.f2mul(cX, p[0])), c0)      # noqa: E731
    for p in (P, P2 if P2 is not None else P, (want[0], Cv.f2neg(want[1]))):
        assert at(p) == (0, 0), f"{case.label}[{i}]: the line does not vanish at a point it passes through"
    assert at(want) != (0, 0)


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_operand_generator_reaches_every_class(name):
    cx = _ctx(name)
    cases = _cases(name)
    for fam in (T_CF, T_XI, T_LINE_DBL, T_LINE_ADD, T_F12_MUL, T_F12_TAB, T_F12_LINE, T_F12_CYC, T_F12_MAPS):
        classes, gaps = _coverage(cx, cases, fam)
        assert RES_CLASSES <= classes, (fam, RES_CLASSES - classes)
        assert not gaps, gaps
    by = {c.label: c for c in cases}
    for label in ("line_dbl_points", "line_add_points"):
        assert by[label].classes == {"Z=1", "Z random", "Z=4q-1", "small k", "random k"}
        assert any(int(v) == 4 * cx.q - 1 for v in by[label].vals[:, 2, 0])
    assert any(int(v) == 2 * cx.q for v in by["line_add_pool"].vals[:, 4, 1])                      # y2 at the bound the comment gives with <=
    for label in ("f12_mul", "f12_mul_tab", "f12_mul_line", "f12_cyc_sqr", "f12_maps"):
        assert F12_CLASSES <= by[label].classes and by[label].n == F12_COUNTS[-1]
    assert {"skip", "D-type" if cx.C.dtype else "M-type"} <= by["f12_mul_line"].classes
    mono = by["f12_mul"].vals[:36]                                              # every w^i times every w^j: each wrap through xi for each output lane
    for e in range(36):
        nz = lambda s0: {s - s0 for s in range(s0, s0 + 6) if any(int(mono[e, s, c]) % cx.q for c in (0, 1))}   # noqa: E731
        assert nz(0) <= {e // 6} and nz(6) <= {e % 6}
    want = {"subgroup", "twist point outside the subgroup", "all-zero encoding"} | ({"x.c1 = 0", "y.c1 = 0"} if cx.C.bn else set())
    assert {c for c, _ in _lines_points(name)} == want
    assert {c for c, _ in _canon_values(name)} == {"0", "1", "q-1", "word boundary", "limb boundary", "random", "pool"}
    assert sum(c == "word boundary" for c, _ in _canon_values(name)) >= 4 * (cx.NL - 2) and sum(c == "limb boundary" for c, _ in _canon_values(name)) >= 4 * (cx.NR - 2)
    assert {c for c, _ in _final_exp_values(name)} == {"1", "-1", "Fq2", "unit in [q, 2q)", "Miller value"}
    unit = dict(_final_exp_values(name))["unit in [q, 2q)"]
    assert all(cx.q <= v < 2 * cx.q for p in unit for v in p)
    assert _cyclotomic(cx, [cx.res2(v) for v in unit]) != [cx.res2(v) for v in unit]
    cyc = by["f12_cyc_sqr"]
    assert sum(x == "cyclotomic" for x in cyc.info[:17]) == 9


@pytest.mark.parametrize("name", CURVES)
def test_every_call_site_holds_at_its_worst_case_bounds(name):
    """No GPU.  g2_lines_kernel, miller_kernel and final_exp_kernel site by site, operands declared at the bounds the header's comments give:
    every product within floor(R'/q), every subtrahend within its bias, every result within what the next site is promised."""
    cx = _ctx(name)
    replay_sites(cx.tw)
    assert cx.F.limit == cx.F.Rp // cx.q and (name != "bn254" or cx.F.limit == 169)


@pytest.mark.parametrize("name", CURVES)
def test_model_rejects_wrong_replays(name):
    """No GPU.  A swapped operand order at (S - X3) M and cf_mul_xi on a value declared below 8q pass every value test; the bounds refuse them."""
    cx = _ctx(name)
    with pytest.raises(ModelError, match="subtrahend may reach 10"):
        replay_sites(cx.tw, swap_y3=True)
    with pytest.raises(ModelError, match="cf_mul_xi"):
        replay_sites(cx.tw, xi_at=8)


@pytest.mark.parametrize("name", CURVES)
def test_model_of_every_case_is_the_plain_tower_arithmetic(name):
    """No GPU.  The replay of every case keeps its bounds, and its limbs stand for the values pairing_constants.Model computes."""
    cx = _ctx(name)
    for case in _cases(name):
        ref = _model(name, case.label)
        _check_values(cx, case, [None if v is None else (v[0].l, v[1].l) for v in ref], range(0, case.n, 3))
    rows, table, want = _lines_model(name)
    for e in range(rows.shape[0]):
        for step, ln in enumerate(table):
            assert tuple(_residue(cx, (c[0].l, c[1].l), e) for c in ln) == want[e][step], f"lines[{e}] step {step}"


def _residue(cx, comps, i):
    return (cx.res(cx.F.val(comps[0][:, i:i + 1])[0]), cx.res(cx.F.val(comps[1][:, i:i + 1])[0]))


def _check_values(cx, case, out, elems):
    """out: per result slot a pair of limb batches or None"""
    for i in elems:
        r_in = [cx.res2(case.vals[i, s]) for s in range(len(case.ubs))]
        want = _values(cx, case, r_in)
        got = [None if o is None else _residue(cx, o, i) for o in out]
        for s, (g, w) in enumerate(zip(got, want)):
            assert g is None or g == w, f"{case.label}[{i}] result {s}: not the plain arithmetic's value"
        if case.fam in (T_LINE_DBL, T_LINE_ADD) and case.info:
            _line_geometry(cx, case, i, r_in, got)
        if case.fam == T_F12_CYC and case.info[i] == "cyclotomic":
            assert got == cx.M.mul(r_in, r_in), f"{case.label}[{i}]: not the square"


# ---- on the device -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)
    return zk


def _call(dev, cx, fam, inp, out_words):
    fn = dev.lib().zk_pairing_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    out = np.zeros((inp.shape[0], out_words), np.uint32)
    assert fn(cx.idx, fam, inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), inp.shape[0]) == 0, dev.lib().zk_last_error()
    return out


def _case_words(cx, case):
    return np.concatenate([l.T.astype(np.uint32) for s in range(len(case.ubs)) for l in _limbs(cx, case, s)], axis=1)


def _out_slots(cx, out, n_slots):
    NR = cx.NR
    return [(out[:, 2 * s * NR:(2 * s + 1) * NR].T.astype(object), out[:, (2 * s + 1) * NR:(2 * s + 2) * NR].T.astype(object)) for s in range(n_slots)]


OUT_SLOTS = {T_CF: 3, T_XI: 3, T_LINE_DBL: 6, T_LINE_ADD: 6, T_F12_MUL: 6, T_F12_TAB: 6, T_F12_LINE: 6, T_F12_CYC: 6, T_F12_MAPS: 12}


def _run_family(dev, name, fam):
    cx = _ctx(name)
    for case in (c for c in _cases(name) if c.fam == fam):
        rows = _case_words(cx, case)
        ns = OUT_SLOTS[fam]
        out = _call(dev, cx, fam, rows, ns * cx.W)
        ref = _model(name, case.label)
        got = _out_slots(cx, out, ns)
        for s, v in enumerate(ref):
            if v is None:
                got[s] = None
                continue
            for c in (0, 1):
                assert _b(got[s][c] == v[c].l).all(), f"{case.label}: result {s} component {c} differs from the model's limbs"
        _check_values(cx, case, got, range(case.n))
        if fam >= T_F12_MUL:                                                     # the same elements as a lone group, around one workgroup, and whole
            for n in F12_COUNTS[:-1]:
                assert np.array_equal(_call(dev, cx, fam, rows[:n], ns * cx.W), out[:n]), f"{case.label}: {n} elements differ from the first {n} of {case.n}"


@gpu
@pytest.mark.parametrize("name", CURVES)
def test_fq2_as_the_pairing_builds_it(dev, name):
    """cf_mul, cf_sqr, cf_inv (the ladder replayed), cf_mul_xi, cf_red, cf_neg: the model's limbs and the Fq2 value."""
    _run_family(dev, name, T_CF)
    _run_family(dev, name, T_XI)


@gpu
@pytest.mark.parametrize("name", CURVES)
def test_line_steps(dev, name):
    """line_dbl, line_add on lifted multiples of the generator and on pool operands: the model's limbs, Model.line_dbl / line_add's values,
    T' the affine sum, the line zero at T, at the second point and at minus the sum."""
    _run_family(dev, name, T_LINE_DBL)
    _run_family(dev, name, T_LINE_ADD)


@gpu
@pytest.mark.parametrize("name", CURVES)
def test_line_table(dev, name):
    """g2_lines_kernel's whole table and infinity word: the model's limbs step by step, Model.lines' values."""
    cx = _ctx(name)
    rows, table, want = _lines_model(name)
    n, W = rows.shape[0], cx.W
    out = _call(dev, cx, T_LINES, rows, cx.tw.steps * 3 * W + 1)
    assert [int(x) for x in out[:, -1]] == [1 if c == "all-zero encoding" else 0 for c, _ in _lines_points(name)]
    got = _out_slots(cx, out[:, :-1], cx.tw.steps * 3)
    for step, ln in enumerate(table):
        for j, c in enumerate(ln):
            for comp in (0, 1):
                assert _b(got[3 * step + j][comp] == c[comp].l).all(), f"step {step} coefficient {j}: differs from the model's limbs"
        for e in range(n):
            assert tuple(_residue(cx, got[3 * step + j], e) for j in range(3)) == want[e][step], f"lines[{e}] step {step}"


@gpu
@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("fam", [T_F12_MUL, T_F12_TAB, T_F12_LINE, T_F12_CYC, T_F12_MAPS], ids=["mul", "mul_tab", "mul_line", "cyc_sqr", "maps"])
def test_fq12_primitives(dev, name, fam):
    """f12_mul, f12_mul_tab, f12_mul_line, f12_cyc_sqr, f12_conj6 / f12_frob2 at 1, 7, 8, 9 and 67 elements: the model's limbs, Model's
    values, a cyclotomic squaring the square."""
    _run_family(dev, name, fam)


@gpu
@pytest.mark.parametrize("name", CURVES)
def test_canonical_words(dev, name):
    """fe_to_canon_words: the model's words and the residue's."""
    cx = _ctx(name)
    vals = [v for _, v in _canon_values(name)]
    l = cx.F.limbs(vals)
    out = _call(dev, cx, T_CANON, l.T.astype(np.uint32), cx.NL)
    ref = cx.tw.cv.to_canon_words(cx.tw.B.new(l, 2 * cx.q - 1))
    assert _b(out.T.astype(object) == ref).all(), "differs from the model's words"
    for i, v in enumerate(vals):
        assert [int(x) for x in out[i]] == _canon_words(cx, cx.res(v)), f"canon[{i}]"


@gpu
@pytest.mark.parametrize("name", CURVES)
def test_final_exponentiation(dev, name):
    """final_exp_dev on Fq12 values in miller_kernel's layout, 1, 7, 8, 9 and 67 of them: Model.final_exp's canonical words, and without the
    exponentiation the value itself."""
    cx = _ctx(name)
    fs = [f for _, f in _final_exp_values(name)]
    want = []
    for f in fs:
        r = [cx.res2(v) for v in f]
        want.append(sum((_canon_words(cx, c) for p in cx.M.final_exp(r) for c in p), []) + sum((_canon_words(cx, c) for p in r for c in p), []))
    case = Case("final_exp", T_FINAL_EXP, _fill(fs, F12_COUNTS[-1]), [2 * cx.q] * 6)
    rows = _case_words(cx, case)
    out = _call(dev, cx, T_FINAL_EXP, rows, 24 * cx.NL)
    for i in range(case.n):
        assert [int(x) for x in out[i]] == want[i % len(fs)], f"final_exp[{i}] ({_final_exp_values(name)[i % len(fs)][0]})"
    for n in F12_COUNTS[:-1]:
        assert np.array_equal(_call(dev, cx, T_FINAL_EXP, rows[:n], 24 * cx.NL), out[:n]), f"{n} elements differ from the first {n}"
