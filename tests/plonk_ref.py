"""The yardstick of the PLONK prover in plain Python integers and hashlib, over a powers-of-tau file whose tau is KNOWN: a
commitment is then the scalar p(tau) and a proof's points are [scalar] G.  It shares no algorithm with the device and no code with the
package's plonk.py: no transform and no polynomial product anywhere.  Everything is an evaluation at one point x in O(n):
  a polynomial given by its values on H      sum_i v_i L_i(x), L_i(x) = w^i (x^n - 1) / (n (x - w^i)), the n inverses by one batch inversion
  the blinding                               + (b_1 x + b_2) Z_H(x), for Z + (b_7 x^2 + b_8 x + b_9) Z_H(x)
  the quotient                               t(x) = bracket(x) / Z_H(x)
  W1, W2                                     the opening's quotients evaluated at tau by division in the field (kzg_multi_ref's Lagrange and
                                             vanishing evaluations)
sigma is built by walking the positions of each variable (no sort), the transcript is written from the issue's table.  No test."""
import hashlib

import kzg_multi_ref as mref

R = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
TWO_ADICITY = {"BN128": 28, "BLS12381": 32}
SELECTORS = ("qL", "qR", "qO", "qM", "qC")


def omega(curve, log_n):
    r = R[curve]
    return pow(7, (r - 1) >> log_n, r)


def ks_by_definition(curve, n):
    """(k_1, k_2) straight from the definition: every candidate pair in order"""
    r = R[curve]
    k1 = next(k for k in range(2, 1000) if pow(k, n, r) != 1)
    k2 = next(k for k in range(k1 + 1, 1000) if pow(k, n, r) != 1 and pow(k, n, r) != pow(k1, n, r))
    return k1, k2


def chain(steps, r, x0=3):
    """x^3 + x + 5 = y, `steps` times, each y the next x: -> (n_vars, public, gates, witness).  Variable 0 pads; variable 1 is the constant 5,
    pinned by a constant gate; x_0 is used in all three columns of one gate (x + x - 2x = 0); the public input is the last y.
    2 + 4 steps gates, 1 public row."""
    gates = {k: [] for k in SELECTORS + ("a", "b", "c")}
    wit = [0, 5, x0 % r]

    def gate(a, b, c, qL=0, qR=0, qO=0, qM=0, qC=0):
        for k, v in (("qL", qL), ("qR", qR), ("qO", qO), ("qM", qM), ("qC", qC)):
            gates[k].append(v % r)
        gates["a"].append(a); gates["b"].append(b); gates["c"].append(c)

    def var(v):
        wit.append(v % r)
        return len(wit) - 1
    five, x = 1, 2
    gate(five, 0, 0, qL=1, qC=-5)
    gate(x, x, x, qL=1, qR=1, qO=-2)
    for _ in range(steps):
        sq = var(wit[x] * wit[x]); gate(x, x, sq, qM=1, qO=-1)
        cu = var(wit[sq] * wit[x]); gate(sq, x, cu, qM=1, qO=-1)
        s1 = var(wit[cu] + wit[x]); gate(cu, x, s1, qL=1, qR=1, qO=-1)
        y = var(wit[s1] + 5); gate(s1, five, y, qL=1, qR=1, qO=-1)
        x = y
    return len(wit), [x], gates, wit


class Table:
    """the padded gate table: the public rows in front, then the gates, then rows of zeros on variable 0"""

    def __init__(self, curve, n_vars, public, gates):
        self.curve, self.r = curve, R[curve]
        self.l = len(public)
        rows = self.l + len(gates["a"])
        self.log_n = max(3, (rows - 1).bit_length())
        self.n = n = 1 << self.log_n
        self.public = list(public)
        self.sel = {k: [0] * n for k in SELECTORS}
        self.wire = {k: [0] * n for k in "abc"}
        for i, v in enumerate(public):
            self.sel["qL"][i] = 1
            self.wire["a"][i] = v
        for g in range(len(gates["a"])):
            for k in SELECTORS:
                self.sel[k][self.l + g] = gates[k][g] % self.r
            for k in "abc":
                self.wire[k][self.l + g] = gates[k][g]
        self.w = omega(curve, self.log_n)
        self.k = (1,) + ks_by_definition(curve, n)
        self.wpow = [1] * n
        for i in range(1, n):
            self.wpow[i] = self.wpow[i - 1] * self.w % self.r

    def label(self, p):
        return self.k[p // self.n] * self.wpow[p % self.n] % self.r

    def sigma_labels(self):
        """per column, the labels of sigma(column, .): each variable's positions in (column, row) order, every one sent to the next"""
        n = self.n
        where = {}
        for j, k in enumerate("abc"):
            for i, v in enumerate(self.wire[k]):
                where.setdefault(v, []).append(j * n + i)
        sig = [0] * (3 * n)
        for ps in where.values():
            for q, p in enumerate(ps):
                sig[p] = ps[(q + 1) % len(ps)]
        return [[self.label(sig[j * n + i]) for i in range(n)] for j in range(3)]


def batch_inverse(vs, r):
    pre, acc = [], 1
    for v in vs:
        pre.append(acc)
        acc = acc * v % r
    inv = pow(acc, -1, r)
    out = [0] * len(vs)
    for i in range(len(vs) - 1, -1, -1):
        out[i] = inv * pre[i] % r
        inv = inv * vs[i] % r
    return out


def lagrange_weights(t, x):
    """L_i(x) for every i: x outside H"""
    r, n = t.r, t.n
    zh = (pow(x, n, r) - 1) % r
    assert zh != 0
    inv = batch_inverse([n * (x - wi) % r for wi in t.wpow], r)
    return [wi * zh % r * d % r for wi, d in zip(t.wpow, inv)]


def dot(vals, weights, r):
    return sum(v * w for v, w in zip(vals, weights)) % r


def bracket(r, v, x, pi_x, l1_x, beta, gamma, alpha, k1, k2):
    """the bracket of round 3 from the values v[name] at x (Zw: Z at w x)"""
    gate = v["a"] * v["b"] * v["qM"] + v["a"] * v["qL"] + v["b"] * v["qR"] + v["c"] * v["qO"] + v["qC"] + pi_x
    p1 = (v["a"] + beta * x + gamma) * (v["b"] + beta * k1 * x + gamma) * (v["c"] + beta * k2 * x + gamma) * v["Z"]
    p2 = (v["a"] + beta * v["S1"] + gamma) * (v["b"] + beta * v["S2"] + gamma) * (v["c"] + beta * v["S3"] + gamma) * v["Zw"]
    return (gate + alpha * (p1 - p2) + alpha * alpha * l1_x * (v["Z"] - 1)) % r


def draw(r, *parts):
    return int.from_bytes(hashlib.sha256(b"".join(parts)).digest(), "big") % r


def le(v):
    return v.to_bytes(32, "little")


FIXED = ("qL", "qR", "qO", "qM", "qC", "S1", "S2", "S3")
ORDER = FIXED + ("a", "b", "c", "t", "Z")          # the polynomials of the opening; Z on {zeta, zeta w}


class Reference:
    """everything the prover computes, as scalars.  point(scalar) -> the bytes of [scalar] G as the transcript hashes them."""

    def __init__(self, curve, n_vars, public, gates, tau, point):
        self.t = t = Table(curve, n_vars, public, gates)
        self.curve, self.r, self.tau, self.point = curve, t.r, tau % t.r, point
        self.fixed_vals = dict(t.sel)
        self.fixed_vals.update(zip(("S1", "S2", "S3"), t.sigma_labels()))
        self.lw_tau = lagrange_weights(t, self.tau)
        self.fixed_tau = {k: dot(self.fixed_vals[k], self.lw_tau, t.r) for k in FIXED}
        self.vk_points = [point(self.fixed_tau[k]) for k in FIXED]
        self.vkd = hashlib.sha256(curve.encode() + b"plonk-vk" + t.log_n.to_bytes(4, "little") + t.l.to_bytes(4, "little") + le(t.k[1]) + le(t.k[2]) +
                                  b"".join(self.vk_points)).digest()

    def wires_of(self, witness):
        return {k: [witness[v] % self.r for v in self.t.wire[k]] for k in "abc"}

    def gates_hold(self, wires, publics):
        t, r = self.t, self.r
        bad = []
        for i in range(t.n):
            a, b, c = wires["a"][i], wires["b"][i], wires["c"][i]
            pi = -publics[i] if i < t.l else 0
            if (t.sel["qL"][i] * a + t.sel["qR"][i] * b + t.sel["qO"][i] * c + t.sel["qM"][i] * a * b + t.sel["qC"][i] + pi) % r:
                bad.append(i)
        return bad

    def product(self, wires, beta, gamma):
        """z_0 .. z_(n-1) and z_n"""
        t, r = self.t, self.r
        sig = [self.fixed_vals[k] for k in ("S1", "S2", "S3")]
        num, den = [], []
        for i in range(t.n):
            a, b = 1, 1
            for j, k in enumerate("abc"):
                a = a * (wires[k][i] + beta * t.label(j * t.n + i) + gamma) % r
                b = b * (wires[k][i] + beta * sig[j][i] + gamma) % r
            num.append(a); den.append(b)
        inv = batch_inverse(den, r)
        z = [1]
        for i in range(t.n):
            z.append(z[-1] * num[i] % r * inv[i] % r)
        return z[:-1], z[-1]

    def evals_at(self, x, wires, z_vals, bs):
        """the values at x of the fixed polynomials, of the blinded a, b, c and of the blinded Z at x and at w x"""
        t, r = self.t, self.r
        zh = lambda y: (pow(y, t.n, r) - 1) % r
        lw = self.lw_tau if x == self.tau else lagrange_weights(t, x)
        xw = x * t.w % r
        lww = lagrange_weights(t, xw)
        v = {k: (self.fixed_tau[k] if x == self.tau else dot(self.fixed_vals[k], lw, r)) for k in FIXED}
        for j, k in enumerate("abc"):
            v[k] = (dot(wires[k], lw, r) + (bs[2 * j] * x + bs[2 * j + 1]) * zh(x)) % r
        blind = lambda y: (bs[6] * y * y + bs[7] * y + bs[8]) * zh(y)
        v["Z"] = (dot(z_vals, lw, r) + blind(x)) % r
        v["Zw"] = (dot(z_vals, lww, r) + blind(xw)) % r
        return v, lw

    def prove(self, witness, blinding):
        t, r, tau, point = self.t, self.r, self.tau, self.point
        bs = [b % r for b in blinding]
        publics = [witness[v] % r for v in t.public]
        wires = self.wires_of(witness)
        assert not self.gates_hold(wires, publics)
        out = {"publics": publics}
        pi_vals = [(-x) % r for x in publics] + [0] * (t.n - t.l)
        # round 1: only the commitments' scalars are needed to go on
        zh_tau = (pow(tau, t.n, r) - 1) % r
        sc = {}
        for j, k in enumerate("abc"):
            sc[k] = (dot(wires[k], self.lw_tau, r) + (bs[2 * j] * tau + bs[2 * j + 1]) * zh_tau) % r
        A, B, C = point(sc["a"]), point(sc["b"]), point(sc["c"])
        c0 = hashlib.sha256(self.curve.encode() + b"plonk-v1" + self.vkd + t.l.to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()
        c1 = hashlib.sha256(c0 + A + B + C).digest()
        beta, gamma = draw(r, c1, b"\x00"), draw(r, c1, b"\x01")
        # round 2
        z_vals, last = self.product(wires, beta, gamma)
        assert last == 1, "the product does not close"
        v_tau, lw_tau = self.evals_at(tau, wires, z_vals, bs)
        assert all(v_tau[k] == sc[k] for k in "abc")
        sc["Z"] = v_tau["Z"]
        Zp = point(sc["Z"])
        c2 = hashlib.sha256(c1 + Zp).digest()
        alpha = draw(r, c2, b"\x00")
        # round 3
        sc["t"] = bracket(r, v_tau, tau, dot(pi_vals, lw_tau, r), lw_tau[0], beta, gamma, alpha, t.k[1], t.k[2]) * pow(zh_tau, -1, r) % r
        T = point(sc["t"])
        c3 = hashlib.sha256(c2 + T).digest()
        ctr = 0
        while True:
            zeta = draw(r, c3, bytes([ctr]))
            if zeta != 0 and pow(zeta, t.n, r) != 1:
                break
            ctr += 1
        # rounds 4, 5
        v_z, lw_z = self.evals_at(zeta, wires, z_vals, bs)
        zh_z = (pow(zeta, t.n, r) - 1) % r
        v_z["t"] = bracket(r, v_z, zeta, dot(pi_vals, lw_z, r), lw_z[0], beta, gamma, alpha, t.k[1], t.k[2]) * pow(zh_z, -1, r) % r
        values = [v_z[k] for k in ORDER] + [v_z["Zw"]]
        c4 = hashlib.sha256(c3 + b"".join(le(v) for v in values)).digest()
        g = draw(r, c4, b"\x00")
        zw = zeta * t.w % r
        sets = [[zeta]] * 12 + [[zeta, zw]]
        ys = [[v] for v in values[:12]] + [values[12:]]
        f_tau = [self.fixed_tau[k] for k in FIXED] + [sc["a"], sc["b"], sc["c"], sc["t"], sc["Z"]]
        # W1: q(tau) = sum_i g^i (f_i(tau) - r_i(tau)) / Z_(S_i)(tau)
        w1 = 0
        for i, (f, s, y) in enumerate(zip(f_tau, sets, ys)):
            w1 = (w1 + pow(g, i, r) * (f - mref.lagrange_eval(s, y, tau, r)) % r * pow(mref.vanishing_at(s, tau, r), -1, r)) % r
        W1 = point(w1)
        ctr = 0
        while True:
            zq = draw(r, c4, b"\x01", W1, bytes([ctr]))
            if zq not in (zeta, zw):
                break
            ctr += 1
        # W2: L(tau) / (tau - z'), L = sum_i w_i (f_i - r_i(z')) - Z_T(z') q, w_i = g^i Z_(T \ S_i)(z')
        T_all = [zeta, zw]
        L = -mref.vanishing_at(T_all, zq, r) * w1
        for i, (f, s, y) in enumerate(zip(f_tau, sets, ys)):
            w = pow(g, i, r) * mref.vanishing_at([p for p in T_all if p not in s], zq, r) % r
            L += w * (f - mref.lagrange_eval(s, y, zq, r))
        w2 = L % r * pow(tau - zq, -1, r) % r
        out.update(scalars=sc, f_tau=f_tau, sets=sets, ys=ys, values=values, w1=w1, w2=w2,
                   challenges={"beta": beta, "gamma": gamma, "alpha": alpha, "zeta": zeta, "gamma_open": g, "z_open": zq},
                   proof={"A": A, "B": B, "C": C, "Z": Zp, "T": T, "values": values, "W1": W1, "W2": point(w2)})
        return out

    def identity_holds(self, publics, values, ch):
        """the verifier's identity at zeta, from the 14 values"""
        t, r = self.t, self.r
        zeta = ch["zeta"]
        v = dict(zip(ORDER, values[:13]))
        v["Zw"] = values[13]
        lw = lagrange_weights(t, zeta)
        pi = -sum(x * lw[i] for i, x in enumerate(publics)) % r
        zh = (pow(zeta, t.n, r) - 1) % r
        return (bracket(r, v, zeta, pi, lw[0], ch["beta"], ch["gamma"], ch["alpha"], t.k[1], t.k[2]) - v["t"] * zh) % r == 0

    def opening_holds(self, res, values=None, f_tau=None, w1=None, w2=None, gamma=None, z=None):
        """the opening equation in the exponent under the known tau (kzg_multi_ref.proof_holds), any part replaced"""
        vals = res["values"] if values is None else values
        ys = [[v] for v in vals[:12]] + [list(vals[12:])]
        ch = res["challenges"]
        return mref.proof_holds(res["f_tau"] if f_tau is None else f_tau, res["sets"], ys, ch["gamma_open"] if gamma is None else gamma, ch["z_open"] if z is None else z,
                                res["w1"] if w1 is None else w1, res["w2"] if w2 is None else w2, self.tau, self.r)
