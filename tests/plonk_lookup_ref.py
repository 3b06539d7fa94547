"""The yardstick of the PLONK prover with lookups in plain Python integers and hashlib, over a powers-of-tau file whose tau
is KNOWN, in the manner of plonk_ref.py, whose evaluation-only machinery it imports: a commitment is the scalar p(tau), every polynomial
is evaluated at one point from its values on H, the quotient is bracket / Z_H.  It shares no code with the package's plonk_lookup.py.  The
multiplicities come from a dictionary in which the first index of a row wins, phi is built with modular inverses one row at a time, the
transcript is written from the issue's table.  No test."""
import hashlib

import kzg_multi_ref as mref
import plonk_ref as ref
from plonk_ref import R, SELECTORS, batch_inverse, dot, draw, lagrange_weights, le

FIXED = ref.FIXED + ("qK", "T1", "T2", "T3")
ORDER = FIXED + ("a", "b", "c", "t", "M")          # opened on {zeta}; then Z and Phi on {zeta, zeta w}
N_VALUES = 21


def lookup_chain(steps, r, bits=1, x0=3, lookups=None):
    """plonk_ref.chain, then `lookups` (steps + 2 unless given) tuples of the AND table, every second one looked up twice: -> (n_vars, public,
    gates with qK, table, witness).  The table is the 2^bits x 2^bits AND table with its first row stored twice (a duplicated table row):
    5 rows for bits = 1.  steps = 0 gives n = 8, steps = 1 gives n = 16."""
    n_vars, public, gates, wit = ref.chain(steps, r, x0)
    gates["qK"] = [0] * len(gates["a"])
    size = 1 << bits
    table = [(0, 0, 0)] + [(x, y, x & y) for x in range(size) for y in range(size)]

    def var(v):
        wit.append(v % r)
        return len(wit) - 1
    for s in range(steps + 2 if lookups is None else lookups):
        x, y = (s * 7 + 1) % size, (s * 5 + 3) % size
        a, b, c = var(x), var(y), var(x & y)
        for _ in range(2 if s % 2 else 1):                                                 # duplicated lookups
            for k in SELECTORS:
                gates[k].append(0)
            gates["a"].append(a); gates["b"].append(b); gates["c"].append(c); gates["qK"].append(1)
    return len(wit), public, gates, table, wit


def lookup_term(r, v, eta, delta):
    f = delta + v["a"] + eta * v["b"] + eta * eta * v["c"]
    t = delta + v["T1"] + eta * v["T2"] + eta * eta * v["T3"]
    return ((v["Phiw"] - v["Phi"]) * f * t - v["qK"] * t + v["M"] * f) % r


class Reference(ref.Reference):
    """everything the prover computes, as scalars.  point(scalar) -> the bytes of [scalar] G as the transcript hashes them."""

    def __init__(self, curve, n_vars, public, gates, table, tau, point):
        r = R[curve]
        gates = {k: list(v) for k, v in gates.items()}
        short = len(table) - len(public) - len(gates["a"])                                 # n must hold the table: rows of zeros on variable 0, as padding is
        for k in gates:
            gates[k] += [0] * max(short, 0)
        super().__init__(curve, n_vars, public, {k: gates[k] for k in SELECTORS + ("a", "b", "c")}, tau, point)
        t = self.t
        assert all(q in (0, 1) for q in gates["qK"]) and len(table) >= 1 and t.n >= len(table)
        self.qk = [0] * t.l + [q % r for q in gates["qK"]] + [0] * (t.n - t.l - len(gates["qK"]))
        rows = [tuple(v % r for v in row) for row in table]
        self.rows = rows + [rows[-1]] * (t.n - len(rows))                                  # padded by repeating the last row
        self.fixed_vals["qK"] = self.qk
        for j, k in enumerate(("T1", "T2", "T3")):
            self.fixed_vals[k] = [row[j] for row in self.rows]
        self.fixed_tau = {k: dot(self.fixed_vals[k], self.lw_tau, r) for k in FIXED}
        self.vk_points = [point(self.fixed_tau[k]) for k in FIXED]
        self.vkd = hashlib.sha256(curve.encode() + b"plonkl-vk" + t.log_n.to_bytes(4, "little") + t.l.to_bytes(4, "little") + le(t.k[1]) + le(t.k[2]) +
                                  b"".join(self.vk_points)).digest()

    def multiplicities(self, wires):
        """m and the selected rows that are no row of the table: the first index of a row takes its whole count"""
        first = {}
        for j, row in enumerate(self.rows):
            first.setdefault(row, j)
        m, bad = [0] * self.t.n, []
        for i in range(self.t.n):
            if self.qk[i]:
                j = first.get((wires["a"][i], wires["b"][i], wires["c"][i]))
                if j is None:
                    bad.append(i)
                else:
                    m[j] += 1
        return m, bad

    def running_sum(self, wires, m, eta, delta):
        """phi_0 .. phi_(n-1) and phi_n, every step by two modular inverses"""
        r, phi = self.r, [0]
        for i in range(self.t.n):
            f = (delta + wires["a"][i] + eta * wires["b"][i] + eta * eta * wires["c"][i]) % r
            t = (delta + self.rows[i][0] + eta * self.rows[i][1] + eta * eta * self.rows[i][2]) % r
            phi.append((phi[-1] + self.qk[i] * pow(f, -1, r) - m[i] * pow(t, -1, r)) % r)
        return phi[:-1], phi[-1]

    def lookup_evals(self, v, x, lw, m, phi, bs):
        """adds to v the values at x of the four fixed lookup polynomials, of the blinded M and of the blinded Phi at x and at w x"""
        t, r = self.t, self.r
        zh = lambda y: (pow(y, t.n, r) - 1) % r
        xw = x * t.w % r
        for k in ("qK", "T1", "T2", "T3"):
            v[k] = self.fixed_tau[k] if x == self.tau else dot(self.fixed_vals[k], lw, r)
        v["M"] = (dot(m, lw, r) + (bs[9] * x + bs[10]) * zh(x)) % r
        blind = lambda y: (bs[11] * y * y + bs[12] * y + bs[13]) * zh(y)
        v["Phi"] = (dot(phi, lw, r) + blind(x)) % r
        v["Phiw"] = (dot(phi, lagrange_weights(t, xw), r) + blind(xw)) % r
        return v

    def bracket(self, v, x, pi_x, l1_x, ch):
        r = self.r
        return (ref.bracket(r, v, x, pi_x, l1_x, ch["beta"], ch["gamma"], ch["alpha"], self.t.k[1], self.t.k[2]) + pow(ch["alpha"], 3, r) * lookup_term(r, v, ch["eta"], ch["delta"])) % r

    def prove(self, witness, blinding, multiplicities=None):
        t, r, tau, point = self.t, self.r, self.tau, self.point
        bs = [b % r for b in blinding]
        assert len(bs) == 14
        publics = [witness[v] % r for v in t.public]
        wires = self.wires_of(witness)
        assert not self.gates_hold(wires, publics)
        m, bad = self.multiplicities(wires)
        assert not bad, "rows %s are no rows of the table" % bad
        if multiplicities is not None:
            m = list(multiplicities)
        out = {"publics": publics, "m": m}
        pi_vals = [(-x) % r for x in publics] + [0] * (t.n - t.l)
        zh_tau = (pow(tau, t.n, r) - 1) % r
        sc = {}
        for j, k in enumerate("abc"):
            sc[k] = (dot(wires[k], self.lw_tau, r) + (bs[2 * j] * tau + bs[2 * j + 1]) * zh_tau) % r
        sc["M"] = (dot(m, self.lw_tau, r) + (bs[9] * tau + bs[10]) * zh_tau) % r
        A, B, C, M = point(sc["a"]), point(sc["b"]), point(sc["c"]), point(sc["M"])
        c0 = hashlib.sha256(self.curve.encode() + b"plonkl-v1" + self.vkd + t.l.to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()
        c1 = hashlib.sha256(c0 + A + B + C + M).digest()
        ch = {"beta": draw(r, c1, b"\x00"), "gamma": draw(r, c1, b"\x01"), "eta": draw(r, c1, b"\x02"), "delta": draw(r, c1, b"\x03")}
        # round 2
        z_vals, last = self.product(wires, ch["beta"], ch["gamma"])
        assert last == 1, "the product does not close"
        phi, closes = self.running_sum(wires, m, ch["eta"], ch["delta"])
        assert closes == 0, "the lookup sum does not close"
        v_tau, lw_tau = self.evals_at(tau, wires, z_vals, bs)
        self.lookup_evals(v_tau, tau, lw_tau, m, phi, bs)
        assert all(v_tau[k] == sc[k] for k in ("a", "b", "c", "M"))
        sc["Z"], sc["Phi"] = v_tau["Z"], v_tau["Phi"]
        Zp, Php = point(sc["Z"]), point(sc["Phi"])
        c2 = hashlib.sha256(c1 + Zp + Php).digest()
        ch["alpha"] = draw(r, c2, b"\x00")
        # round 3
        sc["t"] = self.bracket(v_tau, tau, dot(pi_vals, lw_tau, r), lw_tau[0], ch) * pow(zh_tau, -1, r) % r
        T = point(sc["t"])
        c3 = hashlib.sha256(c2 + T).digest()
        ctr = 0
        while True:
            zeta = draw(r, c3, bytes([ctr]))
            if zeta != 0 and pow(zeta, t.n, r) != 1:
                break
            ctr += 1
        ch["zeta"] = zeta
        # rounds 4, 5
        v_z, lw_z = self.evals_at(zeta, wires, z_vals, bs)
        self.lookup_evals(v_z, zeta, lw_z, m, phi, bs)
        zh_z = (pow(zeta, t.n, r) - 1) % r
        v_z["t"] = self.bracket(v_z, zeta, dot(pi_vals, lw_z, r), lw_z[0], ch) * pow(zh_z, -1, r) % r
        values = [v_z[k] for k in ORDER] + [v_z["Z"], v_z["Zw"], v_z["Phi"], v_z["Phiw"]]
        c4 = hashlib.sha256(c3 + b"".join(le(v) for v in values)).digest()
        g = draw(r, c4, b"\x00")
        zw = zeta * t.w % r
        sets = [[zeta]] * 17 + [[zeta, zw]] * 2
        ys = [[v] for v in values[:17]] + [values[17:19], values[19:21]]
        f_tau = [self.fixed_tau[k] for k in FIXED] + [sc["a"], sc["b"], sc["c"], sc["t"], sc["M"], sc["Z"], sc["Phi"]]
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
        T_all = [zeta, zw]
        L = -mref.vanishing_at(T_all, zq, r) * w1
        for i, (f, s, y) in enumerate(zip(f_tau, sets, ys)):
            w = pow(g, i, r) * mref.vanishing_at([p for p in T_all if p not in s], zq, r) % r
            L += w * (f - mref.lagrange_eval(s, y, zq, r))
        w2 = L % r * pow(tau - zq, -1, r) % r
        ch.update(gamma_open=g, z_open=zq)
        out.update(scalars=sc, f_tau=f_tau, sets=sets, ys=ys, values=values, w1=w1, w2=w2, challenges=ch,
                   proof={"A": A, "B": B, "C": C, "M": M, "Z": Zp, "Phi": Php, "T": T, "values": values, "W1": W1, "W2": point(w2)})
        return out

    def identity_holds(self, publics, values, ch):
        """the verifier's identity at zeta, from the 21 values"""
        t, r = self.t, self.r
        zeta = ch["zeta"]
        v = dict(zip(ORDER + ("Z", "Zw", "Phi", "Phiw"), values))
        lw = lagrange_weights(t, zeta)
        pi = -sum(x * lw[i] for i, x in enumerate(publics)) % r
        zh = (pow(zeta, t.n, r) - 1) % r
        return (self.bracket(v, zeta, pi, lw[0], ch) - v["t"] * zh) % r == 0

    def opening_holds(self, res, values=None, f_tau=None, w1=None, w2=None, gamma=None, z=None):
        """the opening equation in the exponent under the known tau (kzg_multi_ref.proof_holds), any part replaced"""
        vals = res["values"] if values is None else values
        ys = [[v] for v in vals[:17]] + [list(vals[17:19]), list(vals[19:21])]
        ch = res["challenges"]
        return mref.proof_holds(res["f_tau"] if f_tau is None else f_tau, res["sets"], ys, ch["gamma_open"] if gamma is None else gamma, ch["z_open"] if z is None else z,
                                res["w1"] if w1 is None else w1, res["w2"] if w2 is None else w2, self.tau, self.r)
