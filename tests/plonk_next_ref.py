"""TEST INFRASTRUCTURE ONLY.  The yardstick of the PLONK prover with a next-row term in plain Python integers and hashlib.  It
stands on plonk_ref.py's known-tau machinery by import (Table, the Lagrange weights, the permutation product, the bracket without the new
term) and on kzg_multi_ref.py's opening equation; it shares no code with the package.  Two parts:
  Reference   the protocol as scalars: a commitment is p(tau), a point [scalar] G.  Row i satisfies
              qL a + qR b + qO c + qM a b + qC + qN c_(i+1 mod n) + PI_i = 0; c takes three blinders; 16 values; own domain strings.
  Compiled    the CHAIN rule of the R1CS import and the extension of a witness by it, written from the rule's text in include/zkgpu.h on
              plonk_r1cs_ref.py's reader and normalisation.
No test."""
import hashlib

import kzg_multi_ref as mref
import plonk_r1cs_ref as rr
import plonk_ref as pr
from plonk_ref import R, batch_inverse, dot, draw, lagrange_weights, le

FIXED = pr.FIXED + ("qN",)
ORDER = FIXED + ("a", "b", "c", "t", "Z")          # the polynomials of the opening, in its order; c and Z on {zeta, zeta w}
VALUE_NAMES = ORDER + ("Zw", "cw")                  # the proof's 16 values
SELECTORS = pr.SELECTORS + ("qN",)


def running_sums(terms, r, twice=True):
    """a hand-written circuit that uses qN in earnest.  terms: at least three (coefficient, value) pairs; S = sum c_i v_i.  Variable `one` is
    pinned to 1 by a constant gate, the public input is a variable sv that holds S.  A chain down column c sums the terms two a row and
    LANDS IN A CLOSING GATE: sv * one = S with the chain's value as that gate's c.  With twice, the same sum once more as a chain that
    lands in a row of its own (every selector zero), tied to sv by a gate of its own.  2 + ceil(m / 2) gates, or 4 + 2 ceil(m / 2); one
    public row.  -> (n_vars, public, gates, witness)"""
    assert len(terms) >= 3
    gates = {k: [] for k in SELECTORS + ("a", "b", "c")}
    wit = [0]

    def var(v):
        wit.append(v % r)
        return len(wit) - 1

    def gate(a, b, c, **q):
        for k in SELECTORS:
            gates[k].append(q.get(k, 0) % r)
        gates["a"].append(a); gates["b"].append(b); gates["c"].append(c)
    one = var(1)
    sig = [(c % r, var(v)) for c, v in terms]
    sv = var(sum(c * wit[s] for c, s in sig))

    def chain():
        acc, prev = 0, 0
        for j in range(0, len(sig), 2):
            (c1, s1), (c2, s2) = sig[j], sig[j + 1] if j + 1 < len(sig) else (0, 0)
            gate(s1, s2, prev, qL=c1, qR=c2, qO=1 if j else 0, qN=-1)
            acc = (acc + c1 * wit[s1] + c2 * wit[s2]) % r
            prev = var(acc)
        return prev
    gate(one, 0, 0, qL=1, qC=-1)
    gate(sv, one, chain(), qM=1, qO=-1)
    if twice:
        s2 = chain()
        gate(0, 0, s2)
        gate(s2, sv, 0, qL=1, qR=-1)
    return len(wit), [sv], gates, wit


class Table(pr.Table):
    def __init__(self, curve, n_vars, public, gates):
        super().__init__(curve, n_vars, public, gates)
        qn = gates.get("qN", [0] * len(gates["a"]))
        self.sel["qN"] = [0] * self.n
        for g, v in enumerate(qn):
            self.sel["qN"][self.l + g] = int(v) % self.r


def bracket(r, v, x, pi_x, l1_x, beta, gamma, alpha, k1, k2):
    """the bracket of round 3 from the values v[name] at x (Zw, cw: Z and c at w x)"""
    return (pr.bracket(r, v, x, pi_x, l1_x, beta, gamma, alpha, k1, k2) + v["qN"] * v["cw"]) % r


class Reference(pr.Reference):
    def __init__(self, curve, n_vars, public, gates, tau, point):
        self.t = t = Table(curve, n_vars, public, gates)
        self.curve, self.r, self.tau, self.point = curve, t.r, tau % t.r, point
        self.fixed_vals = dict(t.sel)
        self.fixed_vals.update(zip(("S1", "S2", "S3"), t.sigma_labels()))
        self.lw_tau = lagrange_weights(t, self.tau)
        self.fixed_tau = {k: dot(self.fixed_vals[k], self.lw_tau, t.r) for k in FIXED}
        self.vk_points = [point(self.fixed_tau[k]) for k in FIXED]
        self.vkd = hashlib.sha256(curve.encode() + b"plonk-next-vk" + t.log_n.to_bytes(4, "little") + t.l.to_bytes(4, "little") + le(t.k[1]) + le(t.k[2]) +
                                  b"".join(self.vk_points)).digest()

    def gates_hold(self, wires, publics):
        t, r = self.t, self.r
        bad = []
        for i in range(t.n):
            a, b, c, cn = wires["a"][i], wires["b"][i], wires["c"][i], wires["c"][(i + 1) % t.n]
            pi = -publics[i] if i < t.l else 0
            if (t.sel["qL"][i] * a + t.sel["qR"][i] * b + t.sel["qO"][i] * c + t.sel["qM"][i] * a * b + t.sel["qC"][i] + t.sel["qN"][i] * cn + pi) % r:
                bad.append(i)
        return bad

    def evals_at(self, x, wires, z_vals, bs):
        """the values at x of the 9 fixed polynomials, of the blinded a, b, c and Z, and of c and Z at w x"""
        t, r = self.t, self.r
        zh = lambda y: (pow(y, t.n, r) - 1) % r
        lw = self.lw_tau if x == self.tau else lagrange_weights(t, x)
        xw = x * t.w % r
        lww = lagrange_weights(t, xw)
        v = {k: (self.fixed_tau[k] if x == self.tau else dot(self.fixed_vals[k], lw, r)) for k in FIXED}
        v["a"] = (dot(wires["a"], lw, r) + (bs[0] * x + bs[1]) * zh(x)) % r
        v["b"] = (dot(wires["b"], lw, r) + (bs[2] * x + bs[3]) * zh(x)) % r
        blind_c = lambda y: (bs[4] * y * y + bs[5] * y + bs[6]) * zh(y)
        blind_z = lambda y: (bs[7] * y * y + bs[8] * y + bs[9]) * zh(y)
        v["c"] = (dot(wires["c"], lw, r) + blind_c(x)) % r
        v["cw"] = (dot(wires["c"], lww, r) + blind_c(xw)) % r
        v["Z"] = (dot(z_vals, lw, r) + blind_z(x)) % r
        v["Zw"] = (dot(z_vals, lww, r) + blind_z(xw)) % r
        return v, lw

    def sets_of(self, zeta):
        zw = zeta * self.t.w % self.r
        return [[zeta]] * 11 + [[zeta, zw], [zeta], [zeta, zw]]

    @staticmethod
    def ys_of(values):
        """the proof's 16 values -> per polynomial of the opening"""
        return [[v] for v in values[:11]] + [[values[11], values[15]], [values[12]], [values[13], values[14]]]

    def prove(self, witness, blinding):
        t, r, tau, point = self.t, self.r, self.tau, self.point
        bs = [b % r for b in blinding]
        assert len(bs) == 10
        publics = [witness[v] % r for v in t.public]
        wires = self.wires_of(witness)
        assert not self.gates_hold(wires, publics)
        out = {"publics": publics}
        pi_vals = [(-x) % r for x in publics] + [0] * (t.n - t.l)
        zh_tau = (pow(tau, t.n, r) - 1) % r
        # round 1: the wires' scalars need no challenge
        v0, _ = self.evals_at(tau, wires, [0] * t.n, bs)
        sc = {k: v0[k] for k in "abc"}
        A, B, C = point(sc["a"]), point(sc["b"]), point(sc["c"])
        c0 = hashlib.sha256(self.curve.encode() + b"plonk-next-v1" + self.vkd + t.l.to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()
        c1 = hashlib.sha256(c0 + A + B + C).digest()
        beta, gamma = draw(r, c1, b"\x00"), draw(r, c1, b"\x01")
        # round 2
        z_vals, last = self.product(wires, beta, gamma)
        assert last == 1, "the product does not close"
        v_tau, lw_tau = self.evals_at(tau, wires, z_vals, bs)
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
        values = [v_z[k] for k in VALUE_NAMES]
        c4 = hashlib.sha256(c3 + b"".join(le(v) for v in values)).digest()
        g = draw(r, c4, b"\x00")
        zw = zeta * t.w % r
        sets, ys = self.sets_of(zeta), self.ys_of(values)
        f_tau = [self.fixed_tau[k] for k in FIXED] + [sc["a"], sc["b"], sc["c"], sc["t"], sc["Z"]]
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
        out.update(scalars=sc, f_tau=f_tau, sets=sets, ys=ys, values=values, w1=w1, w2=w2,
                   challenges={"beta": beta, "gamma": gamma, "alpha": alpha, "zeta": zeta, "gamma_open": g, "z_open": zq},
                   proof={"A": A, "B": B, "C": C, "Z": Zp, "T": T, "values": values, "W1": W1, "W2": point(w2)})
        return out

    def identity_holds(self, publics, values, ch):
        """the verifier's identity at zeta, from the 16 values"""
        t, r = self.t, self.r
        zeta = ch["zeta"]
        v = dict(zip(VALUE_NAMES, values))
        lw = lagrange_weights(t, zeta)
        pi = -sum(x * lw[i] for i, x in enumerate(publics)) % r
        zh = (pow(zeta, t.n, r) - 1) % r
        return (bracket(r, v, zeta, pi, lw[0], ch["beta"], ch["gamma"], ch["alpha"], t.k[1], t.k[2]) - v["t"] * zh) % r == 0

    def opening_holds(self, res, values=None, f_tau=None, w1=None, w2=None, gamma=None, z=None):
        """the opening equation in the exponent under the known tau (kzg_multi_ref.proof_holds), any part replaced"""
        ch = res["challenges"]
        return mref.proof_holds(res["f_tau"] if f_tau is None else f_tau, res["sets"], self.ys_of(res["values"] if values is None else values),
                                ch["gamma_open"] if gamma is None else gamma, ch["z_open"] if z is None else z,
                                res["w1"] if w1 is None else w1, res["w2"] if w2 is None else w2, self.tau, self.r)


# ---- the chain rule ---------------------------------------------------------------------------------------------------------------------------
class Compiled:
    """an .r1cs under the chain rule.  n_wires, n_public, n_constraints, n_vars, n_aux, n_gates; gates: qL .. qC, qN and a, b, c; origin[g];
    public; segments: [(first auxiliary id, [(wire, coefficient)])] -- term t >= 1 of a segment of m terms defines variable first + t // 2
    when t is odd or t = m - 1"""

    def __init__(self, data, field):
        self.field, self.p = field, rr.R[field]
        p = self.p
        prime, self.n_wires, n_out, n_in, cons = rr.read_r1cs(data)
        if prime != p:
            raise rr.Refused("the file is over another field")
        self.n_public, self.n_constraints = n_out + n_in, len(cons)
        self.public = list(range(1, self.n_public + 1))
        self.gates = {k: [] for k in SELECTORS + rr.WIRES}
        self.origin, self.segments = [], []
        self.n_vars = self.n_wires
        self.pending = None                                    # a chain's value that must stand in c of the row emitted next
        for i, sides in enumerate(cons):
            for side in sides:
                for w, _ in side:
                    if w >= self.n_wires:
                        raise rr.Refused("constraint %d: wire %d of %d" % (i, w, self.n_wires))
            (A, kA), (B, kB), (C, kC) = (rr.normalise(s, p) for s in sides)
            k0 = (kA * kB - kC) % p
            if not A or not B:
                kk, S = (kA, B) if not A else (kB, A)
                L, _ = rr.normalise([(w, kk * c) for w, c in S] + [(w, -c) for w, c in C], p)
                if not L:
                    if k0:
                        raise rr.Refused("constraint %d is 0 = %d" % (i, k0))
                    continue
                if len(L) >= 4:
                    self._chain(i, L, closed=True, k0=k0)
                    continue
                L = L + [(0, 0)] * (3 - len(L))
                self._emit(i, L[0][0], L[1][0], L[2][0], qL=L[0][1], qR=L[1][1], qO=L[2][1], qC=k0)
                continue
            left = {}
            for name, sig in (("A", A), ("B", B), ("C", C)):          # what needs no chain: nothing, one signal, a fold of two
                if len(sig) == 0:
                    left[name] = (0, 0)
                elif len(sig) == 1:
                    left[name] = sig[0]
                elif len(sig) == 2:
                    x = self.n_vars
                    self.segments.append((x, list(sig)))
                    self._emit(i, sig[0][0], sig[1][0], x, qL=sig[0][1], qR=sig[1][1], qO=-1)
                    self.n_vars += 1
                    left[name] = (x, 1)
            for name, sig in (("A", A), ("B", B), ("C", C)):
                if len(sig) >= 3:
                    left[name] = (self._chain(i, sig), 1)
            (sA, fA), (sB, fB), (sC, fC) = left["A"], left["B"], left["C"]
            if self.pending is not None and self.pending != sC:
                self._emit(i, 0, 0, self.pending)                         # a landing row of its own
            self._emit(i, sA, sB, sC, qM=fA * fB, qL=fA * kB, qR=kA * fB, qO=-fC, qC=k0)
            assert self.pending is None
        if self.n_vars >= 1 << 32:
            raise rr.Refused("n_vars does not fit 32 bits")
        self.n_aux = self.n_vars - self.n_wires
        self.n_gates = len(self.origin)

    def _emit(self, i, a, b, c, **q):
        for k in SELECTORS:
            self.gates[k].append(q.get(k, 0) % self.p)
        for k, v in zip(rr.WIRES, (a, b, c)):
            self.gates[k].append(v)
        self.origin.append(i)
        self.pending = None

    def _chain(self, i, sig, closed=False, k0=0):
        m = len(sig)
        k = (m + 1) // 2
        first = self.n_vars
        self.segments.append((first, list(sig[:2 * (k - 1)] if closed else sig)))
        for j in range(k):
            s1, c1 = sig[2 * j]
            s2, c2 = sig[2 * j + 1] if 2 * j + 1 < m else (0, 0)
            c = first + j - 1 if j else (self.pending if self.pending is not None else 0)
            last = closed and j == k - 1
            self._emit(i, s1, s2, c, qL=c1, qR=c2, qO=1 if j else 0, qC=k0 if last else 0, qN=0 if last else -1)
        self.n_vars += k - 1 if closed else k
        if not closed:
            self.pending = first + k - 1
        return first + k - 1

    def extend(self, witness):
        assert len(witness) == self.n_wires
        out = [int(v) % self.p for v in witness] + [0] * self.n_aux
        for first, terms in self.segments:
            acc = 0
            for t, (s, c) in enumerate(terms):
                acc = (acc + c * out[s]) % self.p
                if t and (t % 2 == 1 or t == len(terms) - 1):
                    out[first + t // 2] = acc
        return out

    def failing_gates(self, values):
        """the gates the n_vars values do not satisfy, read as the table reads them: the gate after the last is taken as a row of zeros on
        variable 0 (by the rule the last gate has qN = 0)"""
        g, p, bad = self.gates, self.p, []
        for i in range(self.n_gates):
            a, b, c = values[g["a"][i]], values[g["b"][i]], values[g["c"][i]]
            cn = values[g["c"][i + 1]] if i + 1 < self.n_gates else values[0]
            if (g["qL"][i] * a + g["qR"][i] * b + g["qO"][i] * c + g["qM"][i] * a * b + g["qC"][i] + g["qN"][i] * cn) % p:
                bad.append(i)
        return bad

    def tables(self):
        ptr, wires, coefs = [0], [], []
        for _, terms in self.segments:
            wires += [s for s, _ in terms]
            coefs += [c for _, c in terms]
            ptr.append(len(wires))
        return {**self.gates, "origin": list(self.origin), "seg_first": [f for f, _ in self.segments], "seg_ptr": ptr, "seg_wire": wires, "seg_coef": coefs}
