"""TEST INFRASTRUCTURE ONLY.  Python-integer model of the pairing tower of csrc/pairing_impl.hip.h on top of tests/fe29_model.py's
Curve(F, g2=True): cf_mul_xi, the Jacobian line steps, the line table of g2_lines_kernel, the Fq12 primitives on six Fq2 coefficients,
the canonical words -- each replayed operation by operation in the order the header writes them, on fe29_model's bounded values.  So every
replay yields the exact limbs the device must return and, from the bounds declared for its operands, the checks fe29_model makes at every
step: A B (+ the 8q operand of an Fq2 product) <= floor(R'/q) at every product, subtrahend <= M q at every cf_sub<M>, limbs that the
products admit.  `contract` holds the bounds the header's comments promise between the primitives; `replay_sites` runs every call site
of g2_lines_kernel, miller_kernel and final_exp_kernel once with operands declared at those bounds and requires every result to be within
what the next primitive is promised, which closes the analysis by induction (the exponentiation is not replayed limb by limb).

An Fq2 value is a pair of fe29_model.V, an Fq12 value a list of six of them.  Bounds are inclusive: "< 2q" is 2q - 1, "<= 2q" is 2q."""
from fe29_model import Curve, V, need, _all


class Tower:
    def __init__(self, F, C):
        """F: fe29_model field; C: tools/pairing_constants.py curve (xi, twist type, loop count, gamma)"""
        self.F, self.C, self.q = F, C, F.q
        self.cv = Curve(F, g2=True)
        self.B = self.cv.B
        self.xi0, self.dtype, self.bn = C.xi[0], C.dtype, C.bn
        assert C.xi[1] == 1 and self.xi0 in (1, 9)
        bits = [(C.loop >> b) & 1 for b in range(C.loop.bit_length() - 2, -1, -1)]
        self.loop_bits = bits
        self.steps = len(bits) + sum(bits) + (2 if C.bn else 0)

    # ---- constants and conversions ----
    def fe_const(self, x, n):
        """the Fq integer x as the device's constant: canonical Montgomery limbs"""
        return V(self.B.m.const(self.F.split(self.F.to_mont(x % self.q)), n), self.q - 1)

    def cf_const(self, x, n): return (self.fe_const(x[0], n), self.fe_const(x[1], n))

    def cf_new(self, comps, ub, what="operand"):
        """(c0, c1) limb batches with one declared bound (or a pair of bounds)"""
        ubs = ub if isinstance(ub, (tuple, list)) else (ub, ub)
        return tuple(self.B.new(l, u, what) for l, u in zip(comps, ubs))

    def within(self, a, ub, what):
        """a result keeps the bound the header promises for it, normalised"""
        for c in a:
            need(c.ub <= ub, f"{what}: may reach {c.ub / self.q:.3f}q, promised {ub / self.q:.3f}q")
            need(self.F.normalised(c.l) and _all(self.F.val(c.l) <= c.ub), f"{what}: breaks its bound")
        return a

    # ---- cf_mul_xi ----
    def cf_mul_xi(self, a, site=""):
        B, cv = self.B, self.cv
        if self.xi0 == 1:
            return (B.sub(4, a[0], a[1], site + "cf_mul_xi: "), B.add(a[0], a[1]))
        a8 = cv.cf_dbl(cv.cf_dbl(cv.cf_dbl(a)))
        a9 = cv.cf_add(a8, a)
        return (B.mul(B.sub(4, a9[0], a[1], site + "cf_mul_xi: "), B.one(cv.n_of(a)), site + "cf_mul_xi c0 renorm: "),
                B.mul(B.add(a9[1], a[0]), B.one(cv.n_of(a)), site + "cf_mul_xi c1 renorm: "))

    # ---- the line steps: T = {"X", "Y", "Z"}; returns T', (cY, cX, c0) ----
    def line_dbl(self, T, swap_y3=False):
        cv = self.cv
        X, Y, Z = T["X"], T["Y"], T["Z"]
        A, Bq, ZZ = cv.cf_sqr(X, "line_dbl A: "), cv.cf_sqr(Y, "line_dbl B: "), cv.cf_sqr(Z, "line_dbl ZZ: ")
        S = cv.cf_dbl(cv.cf_dbl(cv.cf_mul(X, Bq, "line_dbl S: ")))
        M = cv.cf_add(cv.cf_dbl(A), A)
        X3 = cv.cf_red(cv.cf_sub(8, cv.cf_sub(8, cv.cf_sqr(M, "line_dbl M^2: "), S, "line_dbl X3: "), S, "line_dbl X3: "))
        Z3 = cv.cf_dbl(cv.cf_mul(Y, Z, "line_dbl Z3: "))
        B4 = cv.cf_dbl(cv.cf_dbl(cv.cf_sqr(Bq, "line_dbl B^2: ")))
        d = cv.cf_sub(2, S, X3, "line_dbl S - X3: ")
        t = cv.cf_mul(M, d, "line_dbl M (S - X3), swapped: ") if swap_y3 else cv.cf_mul(d, M, "line_dbl (S - X3) M: ")
        Y3 = cv.cf_red(cv.cf_sub(8, cv.cf_sub(8, t, B4, "line_dbl Y3: "), B4, "line_dbl Y3: "))
        cY = cv.cf_mul(Z3, ZZ, "line_dbl cY: ")
        cX = cv.cf_neg(cv.cf_mul(M, ZZ, "line_dbl cX: "), "line_dbl cX: ")
        c0 = cv.cf_sub(4, cv.cf_mul(M, X, "line_dbl c0: "), cv.cf_dbl(Bq), "line_dbl c0: ")
        return {"X": X3, "Y": Y3, "Z": Z3}, (cY, cX, c0)

    def line_add(self, T, x2, y2):
        cv = self.cv
        X, Y, Z = T["X"], T["Y"], T["Z"]
        ZZ = cv.cf_sqr(Z, "line_add ZZ: "); ZZZ = cv.cf_mul(Z, ZZ, "line_add ZZZ: ")
        H = cv.cf_sub(2, cv.cf_mul(x2, ZZ, "line_add x2 ZZ: "), X, "line_add H: ")
        Rr = cv.cf_sub(2, cv.cf_mul(y2, ZZZ, "line_add y2 ZZZ: "), Y, "line_add R: ")
        HH = cv.cf_sqr(H, "line_add HH: "); HHH = cv.cf_mul(H, HH, "line_add HHH: "); Vv = cv.cf_mul(X, HH, "line_add V: ")
        X3 = cv.cf_red(cv.cf_sub(4, cv.cf_sub(2, cv.cf_sqr(Rr, "line_add R^2: "), HHH, "line_add X3: "), cv.cf_dbl(Vv), "line_add X3: "))
        Z3 = cv.cf_mul(Z, H, "line_add Z3: ")
        Y3 = cv.cf_red(cv.cf_sub(2, cv.cf_mul(cv.cf_sub(2, Vv, X3, "line_add V - X3: "), Rr, "line_add (V - X3) R: "),
                                 cv.cf_mul(Y, HHH, "line_add Y HHH: "), "line_add Y3: "))
        cX = cv.cf_sub(4, cv.cf_zero(cv.n_of(Rr)), Rr, "line_add cX: ")
        c0 = cv.cf_sub(2, cv.cf_mul(Rr, x2, "line_add R x2: "), cv.cf_mul(y2, Z3, "line_add y2 Z3: "), "line_add c0: ")
        return {"X": X3, "Y": Y3, "Z": Z3}, (Z3, cX, c0)

    # ---- g2_lines_kernel ----
    def cf_from_std(self, w):
        """w: a pair of (NL, n) external word batches"""
        return tuple(self.B._prod(self.B.m.from_std(x), "fe_from_std") for x in w)

    def frobenius_points(self, qx, qy):
        """the operands of the two closing additions of the BN loop: pi(Q), then -pi^2(Q)"""
        B, cv, C = self.B, self.cv, self.C
        n = cv.n_of(qx)
        cx = (qx[0], B.sub(2, B.zero(n), qx[1], "pi(Q) x: ")); cy = (qy[0], B.sub(2, B.zero(n), qy[1], "pi(Q) y: "))
        p1 = (cv.cf_mul(cx, self.cf_const(C.gamma[1][2], n), "pi(Q) x: "), cv.cf_mul(cy, self.cf_const(C.gamma[1][3], n), "pi(Q) y: "))
        p2 = (cv.cf_scale(qx, self.fe_const(C.gamma[2][2][0], n), "pi^2(Q) x: "),
              cv.cf_neg(cv.cf_scale(qy, self.fe_const(C.gamma[2][3][0], n), "pi^2(Q) y: "), "pi^2(Q) y: "))
        return p1, p2

    def lines(self, qx, qy, on_step=None):
        """the table of g2_lines_kernel for affine (qx, qy) (cf, below 2q): a list of (cY, cX, c0) per step"""
        cv = self.cv
        T = {"X": qx, "Y": qy, "Z": cv.cf_one(cv.n_of(qx))}
        out = []

        def keep(kind, T2, ln):
            if on_step:
                on_step(kind, T2, ln)
            out.append(ln)
            return T2
        for b in self.loop_bits:
            T = keep("dbl", *self.line_dbl(T))
            if b:
                T = keep("add", *self.line_add(T, qx, qy))
        if self.bn:
            p1, p2 = self.frobenius_points(qx, qy)
            T = keep("add", *self.line_add(T, *p1))
            T = keep("add", *self.line_add(T, *p2))
        assert len(out) == self.steps
        return out

    # ---- Fq12 on six coefficients ----
    def f12_dot(self, A, Bc, BX, k, site):
        cv = self.cv
        acc = cv.cf_zero(cv.n_of(A[0]))
        for i in range(6):
            j = k - i
            b = BX[j + 6] if j < 0 else Bc[j]
            acc = cv.cf_add(acc, cv.cf_mul(b, A[i], f"{site} k={k} i={i}: "))
        return cv.cf_red(acc)

    def f12_mul(self, a, b, site="f12_mul"):
        bx = [self.cf_mul_xi(x, site + " xi b: ") for x in b]
        return [self.f12_dot(a, b, bx, k, site) for k in range(6)]

    def f12_mul_tab(self, a, g, gx, site="f12_mul_tab"):
        return [self.f12_dot(a, g, gx, k, site) for k in range(6)]

    def f12_mul_line(self, f, v0, v1, v2, site="f12_mul_line"):
        cv = self.cv
        P1 = 1 if self.dtype else 2
        fx = [self.cf_mul_xi(x, site + " xi f: ") for x in f]
        out = []
        for k in range(6):
            j1, j2 = k - P1, k - 3
            acc = cv.cf_mul(v0, f[k], f"{site} k={k} v0: ")
            acc = cv.cf_add(acc, cv.cf_mul(fx[j1 + 6] if j1 < 0 else f[j1], v1, f"{site} k={k} v1: "))
            acc = cv.cf_add(acc, cv.cf_mul(fx[j2 + 6] if j2 < 0 else f[j2], v2, f"{site} k={k} v2: "))
            out.append(cv.cf_red(acc))
        return out

    def f12_cyc_sqr(self, a, site="f12_cyc_sqr"):
        cv = self.cv
        ax = [self.cf_mul_xi(x, site + " xi a: ") for x in a]
        t = []
        for k in range(6):
            lo = k < 3
            pk = k + 3 if lo else k - 3
            p, xp = a[pk], ax[pk]
            X, Y = (a[k], xp) if lo else (p, a[k])
            t.append(cv.cf_add(cv.cf_mul(X, a[k], f"{site} k={k} X a: "), cv.cf_mul(Y, p, f"{site} k={k} Y p: ")))
        tx = [self.cf_mul_xi(x, site + " xi t: ") for x in t]
        out = []
        for k in range(6):
            src = (0, 5, 1, 3, 2, 4)[k]
            s = (tx if k == 1 else t)[src]
            s3, a2 = cv.cf_add(cv.cf_dbl(s), s), cv.cf_dbl(a[k])
            out.append(cv.cf_red(cv.cf_add(s3, a2) if k & 1 else cv.cf_sub(4, s3, a2, f"{site} k={k}: ")))
        return out

    def f12_conj6(self, a): return [self.cv.cf_neg(a[k], "f12_conj6: ") if k & 1 else a[k] for k in range(6)]

    def f12_frob2(self, a):
        n = self.cv.n_of(a[0])
        return [self.cv.cf_scale(a[k], self.fe_const(self.C.gamma[2][k][0], n), "f12_frob2: ") for k in range(6)]

    def f12_one(self, n): return [self.cv.cf_one(n)] + [self.cv.cf_zero(n) for _ in range(5)]

    def line_values(self, ln, xp, yp, skip=False):
        """miller_kernel's lines_in up to the call: the (v0, v1, v2) f12_mul_line gets for the stored coefficients ln and the point (xp, yp)"""
        cv = self.cv
        n = cv.n_of(ln[0])
        vy, vx, v0 = cv.cf_scale(ln[0], yp, "lines_in vy: "), cv.cf_scale(ln[1], xp, "lines_in vx: "), ln[2]
        if skip:
            vy, vx, v0 = cv.cf_zero(n), cv.cf_zero(n), cv.cf_zero(n)
            if self.dtype: vy = cv.cf_one(n)
            else: v0 = cv.cf_one(n)
        return (vy, vx, v0) if self.dtype else (v0, vx, vy)


def contract(q):
    """the bounds the comments of pairing_impl.hip.h promise (inclusive)"""
    return {"T.X": 2 * q - 1, "T.Y": 2 * q - 1, "T.Z": 4 * q - 1,
            "dbl": (2 * q - 1, 2 * q, 6 * q - 1), "add": (2 * q - 1, 4 * q, 4 * q - 1),           # cY, cX, c0
            "x2": 2 * q - 1, "y2": 2 * q,                                                          # line_add's second point (y2 = 2q: -pi^2(Q))
            "f12": 2 * q - 1, "f12_conj6": 2 * q, "xi_in": 4 * q - 1, "xi_out": 8 * q - 1}


def replay_sites(tw, swap_y3=False, xi_at=None):
    """Every call site of g2_lines_kernel, miller_kernel and final_exp_kernel once, operands at their declared worst-case bound (the
    values themselves at the bound and just below it), every result within what the next site is promised.  swap_y3 / xi_at: the two
    deliberately wrong replays (the operands of line_dbl's (S - X3) M swapped; cf_mul_xi on a value declared below xi_at q)."""
    F, q, cv, B = tw.F, tw.q, tw.cv, tw.B
    ct = contract(q)

    def at(ub):
        """a two-element batch: the bound itself and a value just under a multiple of q below it"""
        return F.limbs([ub, ub - (ub % q) - 1 if ub >= q else 0])

    def cf(ub): return tw.cf_new((at(ub), at(ub)), ub)
    def f12(ub): return [cf(ub) for _ in range(6)]
    if xi_at is not None:
        tw.cf_mul_xi(cf(xi_at * q - 1), "wrong replay: ")
        return
    # -- g2_lines_kernel --
    T = {"X": cf(ct["T.X"]), "Y": cf(ct["T.Y"]), "Z": cf(ct["T.Z"])}
    T2, ln = tw.line_dbl(T, swap_y3=swap_y3)
    for name in "XYZ": tw.within(T2[name], ct["T." + name], "line_dbl T." + name)
    for c, ub, name in zip(ln, ct["dbl"], ("cY", "cX", "c0")): tw.within(c, ub, "line_dbl " + name)
    qa = cf(2 * q - 1)                                                      # what cf_from_std returns
    ops = [(qa, qa)]
    if tw.bn:
        ops += list(tw.frobenius_points(qa, qa))
        tw.within(ops[1][0], ct["x2"], "pi(Q) x"); tw.within(ops[1][1], ct["x2"], "pi(Q) y")
        tw.within(ops[2][0], ct["x2"], "pi^2(Q) x"); tw.within(ops[2][1], ct["y2"], "-pi^2(Q) y")
    for x2, y2 in ops + [(cf(ct["x2"]), cf(ct["y2"]))]:
        T2, ln = tw.line_add(T, x2, y2)
        for name in "XYZ": tw.within(T2[name], ct["T." + name], "line_add T." + name)
        for c, ub, name in zip(ln, ct["add"], ("cY", "cX", "c0")): tw.within(c, ub, "line_add " + name)
    # -- miller_kernel --
    f = f12(ct["f12"])
    tw.within(sum((list(x) for x in tw.f12_mul(f, f, "miller f^2")), []), ct["f12"], "miller f^2")
    xp = B.new(at(2 * q - 1), 2 * q - 1); yp = B.new(at(2 * q - 1), 2 * q - 1)
    worst = tuple(cf(max(a, b)) for a, b in zip(ct["dbl"], ct["add"]))
    for skip in (False, True):
        r = tw.f12_mul_line(f, *tw.line_values(worst, xp, yp, skip), site="miller line" + (" (skip)" if skip else ""))
        for x in r: tw.within(x, ct["f12"], "f12_mul_line")
    fc = tw.f12_conj6(f)
    for x in fc: tw.within(x, ct["f12_conj6"], "f12_conj6")
    # -- final_exp_kernel: f as miller_kernel stores it (conjugated on BLS12-381) --
    f = f12(ct["f12"] if tw.bn else ct["f12_conj6"])
    fbar = tw.f12_conj6(f)
    p = f12(ct["f12"])                                                       # any product
    for a, b, what in ((f, fbar, "f fbar"), (p, tw.f12_frob2(p), "a a^(q^2)"), (p, p, "product of products"), (fbar, p, "fbar ab"), (tw.f12_frob2(p), p, "g^(q^2) g")):
        for x in tw.f12_mul(a, b, "final_exp " + what): tw.within(x, ct["f12"], "final_exp " + what)
    for x in tw.f12_frob2(p): tw.within(x, ct["f12"], "f12_frob2")
    ti = cv.cf_inv(p[0])
    tw.within(ti, ct["f12"], "cf_inv")
    finv = [cv.cf_mul(x, ti, "final_exp finv: ") for x in p]
    for x in tw.f12_mul(fbar, finv, "final_exp fbar finv"): tw.within(x, ct["f12"], "final_exp fbar finv")
    gx = [tw.within(tw.cf_mul_xi(x, "final_exp table: "), ct["xi_out"], "final_exp table xi g") for x in p]
    for x in tw.f12_mul_tab(p, p, gx, "final_exp r tab"): tw.within(x, ct["f12"], "f12_mul_tab")
    for x in tw.f12_cyc_sqr(p, "final_exp cyc_sqr"): tw.within(x, ct["f12"], "f12_cyc_sqr")
    for x in p:
        cv.to_canon_words(x[0], "final_exp: "); cv.to_canon_words(x[1], "final_exp: ")
    # -- cf_mul_xi at its own promise --
    tw.within(tw.cf_mul_xi(cf(ct["xi_in"]), "cf_mul_xi at 4q - 1: "), ct["xi_out"], "cf_mul_xi")
