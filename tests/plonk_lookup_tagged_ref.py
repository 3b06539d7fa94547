"""The yardstick of the TAGGED lookups of the PLONK prover in plain Python integers and hashlib, over a powers-of-tau file whose
tau is KNOWN, in the manner of plonk_lookup_ref.py, on whose evaluation-only machinery (and plonk_ref.py's) it stands: a commitment is the
scalar p(tau), every polynomial is evaluated at one point from its values on H.  It shares no code with the package's plonk_lookup.py.
Several tables, a row bound to its table by the tag T0 = k; q_K in 0 .. K is a row's tag and its weight; f and t carry eta^3 q_K and
eta^3 T0; m_j = T0_j x the count, the first index of a repeated tagged row taking the whole count; thirteen fixed polynomials, 22 values,
the domain strings "plonklt-vk" and "plonklt-v1".  No test."""
import hashlib

import kzg_multi_ref as mref
import plonk_lookup_ref as lref
import plonk_ref as ref
from plonk_ref import R, SELECTORS, dot, draw, lagrange_weights, le

FIXED = lref.FIXED + ("T0",)
ORDER = FIXED + ("a", "b", "c", "t", "M")          # opened on {zeta}; then Z and Phi on {zeta, zeta w}
N_VALUES = 22


def pad(row):
    """a row of one, two or three values, padded with zeros on the right"""
    row = tuple(row)
    assert 1 <= len(row) <= 3
    return row + (0,) * (3 - len(row))


def tagged_chain(steps, r, lookups=None, x0=3):
    """plonk_ref.chain, then `lookups` (steps + 3 unless given) lookups, by turns into table 1 -- the range rows (0,), (1,) -- and into
    table 2 -- the XOR rows of one bit with the first stored twice (a duplicated row), so that (0, 0, 0) is a row of BOTH tables; every
    second lookup is made twice: -> (n_vars, public, gates with qK in {0, 1, 2}, tables, witness).  steps = 0 gives n = 8, steps = 1
    gives n = 16; T = 2 + 5 = 7."""
    n_vars, public, gates, wit = ref.chain(steps, r, x0)
    gates["qK"] = [0] * len(gates["a"])
    tables = [[(0,), (1,)], [(0, 0, 0)] + [(x, y, x ^ y) for x in range(2) for y in range(2)]]

    def var(v):
        wit.append(v % r)
        return len(wit) - 1
    for s in range(steps + 3 if lookups is None else lookups):
        if s % 2 == 0:
            a, b, c, tag = var((s // 2) % 2), 0, 0, 1                                      # variable 0 pads and holds 0
        else:
            x, y = (s // 4) % 2, (s // 2) % 2                                              # s = 1 looks (0, 0, 0) up in table 2, s = 0 in table 1
            a, b, c, tag = var(x), var(y), var(x ^ y), 2
        for _ in range(2 if s % 2 else 1):
            for k in SELECTORS:
                gates[k].append(0)
            gates["a"].append(a); gates["b"].append(b); gates["c"].append(c); gates["qK"].append(tag)
    return len(wit), public, gates, tables, wit


def lookup_term(r, v, eta, delta):
    f = delta + v["a"] + eta * v["b"] + eta * eta * v["c"] + eta ** 3 * v["qK"]
    t = delta + v["T1"] + eta * v["T2"] + eta * eta * v["T3"] + eta ** 3 * v["T0"]
    return ((v["Phiw"] - v["Phi"]) * f * t - v["qK"] * t + v["M"] * f) % r


class Reference(lref.Reference):
    """everything the tagged prover computes, as scalars.  tables: K >= 2 lists of rows of one to three values."""

    def __init__(self, curve, n_vars, public, gates, tables, tau, point):
        r = R[curve]
        gates = {k: list(v) for k, v in gates.items()}
        rows = [(k + 1,) + tuple(v % r for v in pad(row)) for k, table in enumerate(tables) for row in table]
        assert 2 <= len(tables) <= 65535 and all(len(t) >= 1 for t in tables) and all(0 <= q <= len(tables) for q in gates["qK"])
        short = len(rows) - len(public) - len(gates["a"])                                  # n must hold the tables
        for k in gates:
            gates[k] += [0] * max(short, 0)
        ref.Reference.__init__(self, curve, n_vars, public, {k: gates[k] for k in SELECTORS + ("a", "b", "c")}, tau, point)
        t = self.t
        assert t.n >= len(rows)
        self.qk = [0] * t.l + list(gates["qK"]) + [0] * (t.n - t.l - len(gates["qK"]))
        self.rows = rows + [rows[-1]] * (t.n - len(rows))                                  # (T0, t1, t2, t3), padded by repeating the last row, tag included
        self.fixed_vals["qK"] = self.qk
        for j, k in enumerate(("T0", "T1", "T2", "T3")):
            self.fixed_vals[k] = [row[j] for row in self.rows]
        self.fixed_tau = {k: dot(self.fixed_vals[k], self.lw_tau, r) for k in FIXED}
        self.vk_points = [point(self.fixed_tau[k]) for k in FIXED]
        self.vkd = hashlib.sha256(curve.encode() + b"plonklt-vk" + t.log_n.to_bytes(4, "little") + t.l.to_bytes(4, "little") + le(t.k[1]) + le(t.k[2]) +
                                  b"".join(self.vk_points)).digest()

    def multiplicities(self, wires, weighted=True):
        """m and the selected rows that are no row of the table their q_K names: m_j = T0_j x the count (weighted=False: the count alone,
        which is NOT the protocol's m)"""
        first = {}
        for j, row in enumerate(self.rows):
            first.setdefault(row, j)
        m, bad = [0] * self.t.n, []
        for i in range(self.t.n):
            if self.qk[i]:
                j = first.get((self.qk[i], wires["a"][i], wires["b"][i], wires["c"][i]))
                if j is None:
                    bad.append(i)
                else:
                    m[j] += self.rows[j][0] if weighted else 1
        return m, bad

    def terms(self, wires, i, eta, delta):
        """(delta + f_i, delta + t_i)"""
        r, row = self.r, self.rows[i]
        return ((delta + wires["a"][i] + eta * wires["b"][i] + eta * eta * wires["c"][i] + eta ** 3 * self.qk[i]) % r,
                (delta + row[1] + eta * row[2] + eta * eta * row[3] + eta ** 3 * row[0]) % r)

    def running_sum(self, wires, m, eta, delta):
        r, phi = self.r, [0]
        for i in range(self.t.n):
            f, t = self.terms(wires, i, eta, delta)
            phi.append((phi[-1] + self.qk[i] * pow(f, -1, r) - m[i] * pow(t, -1, r)) % r)
        return phi[:-1], phi[-1]

    def lookup_evals(self, v, x, lw, m, phi, bs):
        super().lookup_evals(v, x, lw, m, phi, bs)
        v["T0"] = self.fixed_tau["T0"] if x == self.tau else dot(self.fixed_vals["T0"], lw, self.r)
        return v

    def bracket(self, v, x, pi_x, l1_x, ch):
        r = self.r
        return (ref.bracket(r, v, x, pi_x, l1_x, ch["beta"], ch["gamma"], ch["alpha"], self.t.k[1], self.t.k[2]) + pow(ch["alpha"], 3, r) * lookup_term(r, v, ch["eta"], ch["delta"])) % r

    def prove(self, witness, blinding, multiplicities=None, force=False):
        """force: the prover checks nothing.  Where the sum does not close, bracket is no multiple of Z_H; the best a prover can then commit
        to is the polynomial part t = (bracket - rho) / Z_H, rho the interpolant of bracket's values on H: zero everywhere but at the last
        row, where L = -phi_n (delta + f)(delta + t).  That t is what the forced proof carries, at tau and at zeta."""
        t, r, tau, point = self.t, self.r, self.tau, self.point
        bs = [b % r for b in blinding]
        assert len(bs) == 14
        publics = [witness[v] % r for v in t.public]
        wires = self.wires_of(witness)
        assert not self.gates_hold(wires, publics)
        m, bad = self.multiplicities(wires)
        assert force or not bad, "rows %s are no rows of the tables they name" % bad
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
        c0 = hashlib.sha256(self.curve.encode() + b"plonklt-v1" + self.vkd + t.l.to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()
        c1 = hashlib.sha256(c0 + A + B + C + M).digest()
        ch = {"beta": draw(r, c1, b"\x00"), "gamma": draw(r, c1, b"\x01"), "eta": draw(r, c1, b"\x02"), "delta": draw(r, c1, b"\x03")}
        # round 2
        z_vals, last = self.product(wires, ch["beta"], ch["gamma"])
        assert last == 1, "the product does not close"
        phi, closes = self.running_sum(wires, m, ch["eta"], ch["delta"])
        assert force or closes == 0, "the lookup sum does not close"
        v_tau, lw_tau = self.evals_at(tau, wires, z_vals, bs)
        self.lookup_evals(v_tau, tau, lw_tau, m, phi, bs)
        assert all(v_tau[k] == sc[k] for k in ("a", "b", "c", "M"))
        sc["Z"], sc["Phi"] = v_tau["Z"], v_tau["Phi"]
        Zp, Php = point(sc["Z"]), point(sc["Phi"])
        c2 = hashlib.sha256(c1 + Zp + Php).digest()
        ch["alpha"] = draw(r, c2, b"\x00")
        # round 3
        f_last, t_last = self.terms(wires, t.n - 1, ch["eta"], ch["delta"])
        rho_last = pow(ch["alpha"], 3, r) * (-closes) * f_last * t_last % r              # bracket at the last row of H; 0 when the sum closes
        sc["t"] = (self.bracket(v_tau, tau, dot(pi_vals, lw_tau, r), lw_tau[0], ch) - rho_last * lw_tau[-1]) * pow(zh_tau, -1, r) % r
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
        v_z["t"] = (self.bracket(v_z, zeta, dot(pi_vals, lw_z, r), lw_z[0], ch) - rho_last * lw_z[-1]) * pow(zh_z, -1, r) % r
        values = [v_z[k] for k in ORDER] + [v_z["Z"], v_z["Zw"], v_z["Phi"], v_z["Phiw"]]
        c4 = hashlib.sha256(c3 + b"".join(le(v) for v in values)).digest()
        g = draw(r, c4, b"\x00")
        zw = zeta * t.w % r
        sets = [[zeta]] * 18 + [[zeta, zw]] * 2
        ys = [[v] for v in values[:18]] + [values[18:20], values[20:22]]
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
        out.update(scalars=sc, f_tau=f_tau, sets=sets, ys=ys, values=values, w1=w1, w2=w2, challenges=ch, closes=closes,
                   proof={"A": A, "B": B, "C": C, "M": M, "Z": Zp, "Phi": Php, "T": T, "values": values, "W1": W1, "W2": point(w2)})
        return out

    def identity_holds(self, publics, values, ch):
        """the verifier's identity at zeta, from the 22 values"""
        t, r = self.t, self.r
        zeta = ch["zeta"]
        v = dict(zip(ORDER + ("Z", "Zw", "Phi", "Phiw"), values))
        lw = lagrange_weights(t, zeta)
        pi = -sum(x * lw[i] for i, x in enumerate(publics)) % r
        zh = (pow(zeta, t.n, r) - 1) % r
        return (self.bracket(v, zeta, pi, lw[0], ch) - v["t"] * zh) % r == 0

    def opening_holds(self, res, values=None, f_tau=None, w1=None, w2=None, gamma=None, z=None):
        vals = res["values"] if values is None else values
        ys = [[v] for v in vals[:18]] + [list(vals[18:20]), list(vals[20:22])]
        ch = res["challenges"]
        return mref.proof_holds(res["f_tau"] if f_tau is None else f_tau, res["sets"], ys, ch["gamma_open"] if gamma is None else gamma, ch["z_open"] if z is None else z,
                                res["w1"] if w1 is None else w1, res["w2"] if w2 is None else w2, self.tau, self.r)

    def verify(self, res, values=None):
        """the model's verifier: the identity at zeta and the opening equation, both"""
        vals = res["values"] if values is None else values
        return self.identity_holds(res["publics"], vals, res["challenges"]) and self.opening_holds(res, values=vals)
