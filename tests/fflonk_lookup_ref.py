"""The yardstick of the fflonk prover with lookups in plain Python integers and hashlib, over a powers-of-tau file whose tau
is KNOWN, on the evaluation-only machinery of fflonk_ref.py and plonk_lookup_ref.py: a commitment is the scalar
C(tau) = sum_m f_m(tau^t) tau^m and a proof's points are [scalar] G.  It shares no algorithm with the device and no code with the package's
fflonk_lookup.py: no transform, no polynomial product and no interleaved coefficient vector anywhere.  Everything is an evaluation at one
point x in O(n):
  a polynomial given by its values on H      sum_i v_i L_i(x), plonk_ref's barycentric weights, plus its blinding times Z_H(x)
  the multiplicities                         a dictionary in which the first index of a table row wins (plonk_lookup_ref)
  phi                                        two modular inverses per row (plonk_lookup_ref)
  T0 .. T3                                   numerator(x) / Z_H(x), pointwise: at tau^4 (T0, T1 inside C2), at tau^2 (T2, T3 inside C3), at xi
                                             and xi w for the values
  an opened value                            C(h) = sum_m f_m(h^t) h^m
  W1, W2                                     the opening's quotients evaluated at tau by division in the field (kzg_multi_ref)
The transcript is written from the issue's table.  No test."""
import hashlib

import kzg_multi_ref as mref
import plonk_lookup_ref as lref
import plonk_ref as pref

R, SELECTORS, lookup_chain = pref.R, pref.SELECTORS, lref.lookup_chain
draw, le, dot = pref.draw, pref.le, pref.dot
FIXED = lref.FIXED                                                  # the 8 of fflonk's C0, then qK, T1, T2, T3 of C0L
VALUE_NAMES = FIXED + ("a", "b", "c", "M", "Z", "Phi", "Zw", "Phiw", "T0w", "T1w")
N_VALUES = 22


def combine(parts, x, r):
    """sum_m parts[m] x^m"""
    return sum(v * pow(x, m, r) for m, v in enumerate(parts)) % r


def field_facts(curve, log_n):
    """what round 3 relies on, each as a boolean by name"""
    r, n = R[curve], 1 << log_n
    w, w4n = pref.omega(curve, log_n), pow(7, (r - 1) // (4 * n), r)
    return {"4n | r - 1": (r - 1) % (4 * n) == 0, "k + 2 within the 2-adicity": log_n + 2 <= pref.TWO_ADICITY[curve], "w_4n^4 = w": pow(w4n, 4, r) == w,
            "w_4n has order 4n": pow(w4n, 2 * n, r) == r - 1, "w_8 has order 8": pow(w, n // 8 * 4, r) == r - 1, "w_4 = w_8^2 has order 4": pow(w, n // 4 * 2, r) == r - 1}


def roots_of(curve, log_n, s):
    """the seed -> (xi, [S0, S1, S2, S3]), each root by its own definition"""
    r, n = R[curve], 1 << log_n
    w = pref.omega(curve, log_n)
    w8, w4n = pow(w, n // 8, r), pow(7, (r - 1) // (4 * n), r)
    w4 = pow(w, n // 4, r)
    h0, h1, h3 = s % r, s * s % r, s * s * s * s % r
    xi = h3 * h3 % r
    assert pow(h0, 8, r) == pow(h1, 4, r) == xi and pow(h1 * w4n, 4, r) == xi * w % r
    S0 = [h0 * pow(w8, j, r) % r for j in range(8)]
    S1 = [h1 * pow(w4, j, r) % r for j in range(4)]
    S2 = S1 + [h1 * w4n * pow(w4, j, r) % r for j in range(4)]
    return xi, [S0, S1, S2, [h3, -h3 % r]]


class Reference(lref.Reference):
    """everything the prover computes, as scalars.  point(scalar) -> the bytes of [scalar] G as the transcript hashes them."""

    def __init__(self, curve, n_vars, public, gates, table, tau, point):
        super().__init__(curve, n_vars, public, gates, table, tau, point)
        t, r = self.t, self.r
        lw8, lw4 = pref.lagrange_weights(t, pow(self.tau, 8, r)), pref.lagrange_weights(t, pow(self.tau, 4, r))
        self.c0 = combine([dot(self.fixed_vals[k], lw8, r) for k in FIXED[:8]], self.tau, r)
        self.c0l = combine([dot(self.fixed_vals[k], lw4, r) for k in FIXED[8:]], self.tau, r)
        self.C0, self.C0L = point(self.c0), point(self.c0l)
        self.vk_points = [self.C0, self.C0L]
        self.vkd = hashlib.sha256(curve.encode() + b"fflonkl-vk" + t.log_n.to_bytes(4, "little") + t.l.to_bytes(4, "little") + le(t.k[1]) + le(t.k[2]) + self.C0 + self.C0L).digest()

    def zh(self, x):
        return (pow(x, self.t.n, self.r) - 1) % self.r

    def round1_at(self, x, wires, m, bs):
        """the blinded a, b, c and M at x"""
        r, lw = self.r, pref.lagrange_weights(self.t, x)
        v = {k: (dot(wires[k], lw, r) + (bs[2 * j] * x + bs[2 * j + 1]) * self.zh(x)) % r for j, k in enumerate("abc")}
        v["M"] = (dot(m, lw, r) + (bs[9] * x + bs[10]) * self.zh(x)) % r
        return v

    def all_at(self, x, wires, pi_vals, z_vals, m, phi, bs, ch):
        """every polynomial of the protocol at x (Z and Phi at w x too), and the quotients T0 .. T3 as numerator / Z_H under the keys t0 .. t3
        (T1, T2, T3 are the table's columns)"""
        t, r = self.t, self.r
        v, lw = self.evals_at(x, wires, z_vals, bs)
        self.lookup_evals(v, x, lw, m, phi, bs)
        inv = pow(self.zh(x), -1, r)
        beta, gamma = ch["beta"], ch["gamma"]
        gate = v["a"] * v["b"] * v["qM"] + v["a"] * v["qL"] + v["b"] * v["qR"] + v["c"] * v["qO"] + v["qC"] + dot(pi_vals, lw, r)
        p1 = (v["a"] + beta * x + gamma) * (v["b"] + beta * t.k[1] * x + gamma) * (v["c"] + beta * t.k[2] * x + gamma) * v["Z"]
        p2 = (v["a"] + beta * v["S1"] + gamma) * (v["b"] + beta * v["S2"] + gamma) * (v["c"] + beta * v["S3"] + gamma) * v["Zw"]
        v["t0"] = gate % r * inv % r
        v["t1"] = lw[0] * (v["Z"] - 1) % r * inv % r
        v["t2"] = (p1 - p2) % r * inv % r
        v["t3"] = lref.lookup_term(r, v, ch["eta"], ch["delta"]) * inv % r
        return v

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
        pi_vals = [(-x) % r for x in publics] + [0] * (t.n - t.l)
        # round 1: C1(tau) from a, b, c, M at tau^4
        v1 = self.round1_at(pow(tau, 4, r), wires, m, bs)
        c1s = combine([v1["a"], v1["b"], v1["c"], v1["M"]], tau, r)
        C1 = point(c1s)
        c0 = hashlib.sha256(self.curve.encode() + b"fflonkl-v1" + self.vkd + t.l.to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()
        c1 = hashlib.sha256(c0 + C1).digest()
        ch = {"beta": draw(r, c1, b"\x00"), "gamma": draw(r, c1, b"\x01"), "eta": draw(r, c1, b"\x02"), "delta": draw(r, c1, b"\x03")}
        # round 2: C2(tau) from Z, Phi, T0, T1 at tau^4, C3(tau) from T2, T3 at tau^2
        z_vals, last = self.product(wires, ch["beta"], ch["gamma"])
        assert last == 1, "the product does not close"
        phi, closes = self.running_sum(wires, m, ch["eta"], ch["delta"])
        assert closes == 0, "the lookup sum does not close"
        v4 = self.all_at(pow(tau, 4, r), wires, pi_vals, z_vals, m, phi, bs, ch)
        v2 = self.all_at(pow(tau, 2, r), wires, pi_vals, z_vals, m, phi, bs, ch)
        assert all(v4[k] == v1[k] for k in ("a", "b", "c", "M"))
        c2s = combine([v4["Z"], v4["Phi"], v4["t0"], v4["t1"]], tau, r)
        c3s = combine([v2["t2"], v2["t3"]], tau, r)
        C2, C3 = point(c2s), point(c3s)
        c2 = hashlib.sha256(c1 + C2 + C3).digest()
        ctr = 0
        while True:
            s = draw(r, c2, bytes([ctr]))
            if s != 0 and pow(pow(s, 8, r), t.n, r) != 1:
                break
            ctr += 1
        # round 3
        xi, sets4 = roots_of(self.curve, t.log_n, s)
        sets = [sets4[0], sets4[1], sets4[1], sets4[2], sets4[3]]
        vx = self.all_at(xi, wires, pi_vals, z_vals, m, phi, bs, ch)
        vxw = self.all_at(xi * t.w % r, wires, pi_vals, z_vals, m, phi, bs, ch)
        assert vxw["Z"] == vx["Zw"] and vxw["Phi"] == vx["Phiw"]
        values = [vx[k] for k in FIXED] + [vx[k] for k in ("a", "b", "c", "M", "Z", "Phi")] + [vxw[k] for k in ("Z", "Phi", "t0", "t1")]
        at = lambda v, names, hs: [combine([v[k] for k in names], h, r) for h in hs]
        ys = [at(vx, FIXED[:8], sets[0]), at(vx, FIXED[8:], sets[1]), at(vx, ("a", "b", "c", "M"), sets[2]),
              at(vx, ("Z", "Phi", "t0", "t1"), sets[3][:4]) + at(vxw, ("Z", "Phi", "t0", "t1"), sets[3][4:]), at(vx, ("t2", "t3"), sets[4])]
        # round 4
        c3 = hashlib.sha256(c2 + b"".join(le(v) for v in values)).digest()
        g = draw(r, c3, b"\x00")
        f_tau = [self.c0, self.c0l, c1s, c2s, c3s]
        w1 = 0
        for i, (f, st, y) in enumerate(zip(f_tau, sets, ys)):
            w1 = (w1 + pow(g, i, r) * (f - mref.lagrange_eval(st, y, tau, r)) % r * pow(mref.vanishing_at(st, tau, r), -1, r)) % r
        W1 = point(w1)
        T_all = mref.union(sets)
        ctr = 0
        while True:
            zq = draw(r, c3, b"\x01", W1, bytes([ctr]))
            if zq not in T_all:
                break
            ctr += 1
        L = -mref.vanishing_at(T_all, zq, r) * w1
        for i, (f, st, y) in enumerate(zip(f_tau, sets, ys)):
            wt = pow(g, i, r) * mref.vanishing_at([p for p in T_all if p not in st], zq, r) % r
            L += wt * (f - mref.lagrange_eval(st, y, zq, r))
        w2 = L % r * pow(tau - zq, -1, r) % r
        ch.update(s=s, xi=xi, gamma_open=g, z_open=zq)
        return {"publics": publics, "m": m, "f_tau": f_tau, "sets": sets, "ys": ys, "values": values, "w1": w1, "w2": w2, "at_xi": vx, "challenges": ch,
                "proof": {"C1": C1, "C2": C2, "C3": C3, "W1": W1, "W2": point(w2), "values": values}}

    def opening_holds(self, res, ys=None, f_tau=None, sets=None, w1=None, w2=None, gamma=None, z=None):
        """the opening equation in the exponent under the known tau (kzg_multi_ref.proof_holds), any part replaced"""
        ch = res["challenges"]
        return mref.proof_holds(res["f_tau"] if f_tau is None else f_tau, res["sets"] if sets is None else sets, res["ys"] if ys is None else ys,
                                ch["gamma_open"] if gamma is None else gamma, ch["z_open"] if z is None else z, res["w1"] if w1 is None else w1,
                                res["w2"] if w2 is None else w2, self.tau, self.r)
