"""The yardstick of the fflonk prover in plain Python integers and hashlib, over a powers-of-tau file whose tau is KNOWN: a
commitment is then the scalar C_i(tau) = sum_m f_m(tau^t) tau^m and a proof's points are [scalar] G.  It shares no algorithm with the device
and no code with the package's fflonk.py: no transform, no polynomial product and no interleaved coefficient vector anywhere.  Everything is
an evaluation at one point x in O(n), by plonk_ref.py's table and barycentric sums:
  a polynomial given by its values on H      sum_i v_i L_i(x), L_i(x) = w^i (x^n - 1) / (n (x - w^i))
  the blinding                               + (b_1 x + b_2) Z_H(x), for Z + (b_7 x^2 + b_8 x + b_9) Z_H(x)
  T0, T1, T2                                 numerator(x) / Z_H(x), pointwise: at tau^4 for C1, at tau^3 for C2, at xi and xi w for the values
  an opened value                            C_i(h) = sum_m f_m(h^t) h^m
  W1, W2                                     the opening's quotients evaluated at tau by division in the field (kzg_multi_ref's Lagrange and
                                             vanishing evaluations)
The transcript is written from the issue's table.  No test."""
import hashlib

import kzg_multi_ref as mref
import plonk_ref as pref

R, FIXED, chain = pref.R, pref.FIXED, pref.chain
draw, le = pref.draw, pref.le
VALUE_NAMES = FIXED + ("a", "b", "c", "Z", "Zw", "T1w", "T2w")


def omega3(curve):
    r = R[curve]
    return pow(7, (r - 1) // 3, r)


def field_facts(curve, log_n):
    """what round 3 relies on, each as a boolean by name"""
    r, n = R[curve], 1 << log_n
    w = pref.omega(curve, log_n)
    e = next(e for e in range(n) if 3 * e % n == 1)
    return {"3 | r - 1": (r - 1) % 3 == 0, "24 | r - 1": (r - 1) % 24 == 0, "w_3 != 1": omega3(curve) != 1, "w_3^3 = 1": pow(omega3(curve), 3, r) == 1,
            "(w^e)^3 = w": pow(pow(w, e, r), 3, r) == w, "w_8 has order 8": pow(w, n // 8 * 4, r) == r - 1}


def roots_of(curve, log_n, s):
    """the seed -> (xi, [S0, S1, S2]), each root by its own definition"""
    r, n = R[curve], 1 << log_n
    w = pref.omega(curve, log_n)
    e = next(e for e in range(n) if 3 * e % n == 1)
    w8, w3 = pow(w, n // 8, r), omega3(curve)
    h0, h1, h2 = s * s * s % r, pow(s, 6, r), pow(s, 8, r)
    h3 = h2 * pow(w, e, r) % r
    xi = pow(h2, 3, r)
    assert pow(h0, 8, r) == pow(h1, 4, r) == xi and pow(h3, 3, r) == xi * w % r
    S0 = [h0 * pow(w8, j, r) % r for j in range(8)]
    S1 = [h1 * pow(w8, 2 * j, r) % r for j in range(4)]
    S2 = [h2, h2 * w3 % r, h2 * w3 * w3 % r, h3, h3 * w3 % r, h3 * w3 * w3 % r]
    return xi, [S0, S1, S2]


def combine(parts, x, r):
    """sum_m parts[m] x^m"""
    return sum(v * pow(x, m, r) for m, v in enumerate(parts)) % r


class Reference:
    """everything the prover computes, as scalars.  point(scalar) -> the bytes of [scalar] G as the transcript hashes them."""

    def __init__(self, curve, n_vars, public, gates, tau, point):
        self.t = t = pref.Table(curve, n_vars, public, gates)
        self.curve, self.r, self.tau, self.point = curve, t.r, tau % t.r, point
        self.fixed_vals = dict(t.sel)
        self.fixed_vals.update(zip(("S1", "S2", "S3"), t.sigma_labels()))
        r = t.r
        lw = pref.lagrange_weights(t, pow(self.tau, 8, r))
        self.c0 = combine([pref.dot(self.fixed_vals[k], lw, r) for k in FIXED], self.tau, r)
        self.C0 = point(self.c0)
        self.vkd = hashlib.sha256(curve.encode() + b"fflonk-vk" + t.log_n.to_bytes(4, "little") + t.l.to_bytes(4, "little") + le(t.k[1]) + le(t.k[2]) + self.C0).digest()

    def wires_of(self, witness):
        return {k: [witness[v] % self.r for v in self.t.wire[k]] for k in "abc"}

    gates_hold = pref.Reference.gates_hold
    product = pref.Reference.product

    def zh(self, x):
        return (pow(x, self.t.n, self.r) - 1) % self.r

    def round1_at(self, x, wires, pi_vals, bs):
        """the fixed polynomials, the blinded a, b, c and T0 at x"""
        t, r = self.t, self.r
        lw = pref.lagrange_weights(t, x)
        v = {k: pref.dot(self.fixed_vals[k], lw, r) for k in FIXED}
        for j, k in enumerate("abc"):
            v[k] = (pref.dot(wires[k], lw, r) + (bs[2 * j] * x + bs[2 * j + 1]) * self.zh(x)) % r
        gate = v["a"] * v["b"] * v["qM"] + v["a"] * v["qL"] + v["b"] * v["qR"] + v["c"] * v["qO"] + v["qC"] + pref.dot(pi_vals, lw, r)
        v["T0"] = gate % r * pow(self.zh(x), -1, r) % r
        return v, lw

    def round2_at(self, x, wires, pi_vals, z_vals, bs, beta, gamma):
        """everything at x: round 1's values, the blinded Z at x and at w x, T1 and T2"""
        t, r = self.t, self.r
        v, lw = self.round1_at(x, wires, pi_vals, bs)
        xw = x * t.w % r
        blind = lambda y: (bs[6] * y * y + bs[7] * y + bs[8]) * self.zh(y)
        v["Z"] = (pref.dot(z_vals, lw, r) + blind(x)) % r
        v["Zw"] = (pref.dot(z_vals, pref.lagrange_weights(t, xw), r) + blind(xw)) % r
        inv = pow(self.zh(x), -1, r)
        v["T1"] = lw[0] * (v["Z"] - 1) % r * inv % r
        p1 = (v["a"] + beta * x + gamma) * (v["b"] + beta * t.k[1] * x + gamma) * (v["c"] + beta * t.k[2] * x + gamma) * v["Z"]
        p2 = (v["a"] + beta * v["S1"] + gamma) * (v["b"] + beta * v["S2"] + gamma) * (v["c"] + beta * v["S3"] + gamma) * v["Zw"]
        v["T2"] = (p1 - p2) % r * inv % r
        return v

    def prove(self, witness, blinding):
        t, r, tau, point = self.t, self.r, self.tau, self.point
        bs = [b % r for b in blinding]
        publics = [witness[v] % r for v in t.public]
        wires = self.wires_of(witness)
        assert not self.gates_hold(wires, publics)
        pi_vals = [(-x) % r for x in publics] + [0] * (t.n - t.l)
        # round 1: C1(tau) from a, b, c, T0 at tau^4
        v4, _ = self.round1_at(pow(tau, 4, r), wires, pi_vals, bs)
        c1s = combine([v4["a"], v4["b"], v4["c"], v4["T0"]], tau, r)
        C1 = point(c1s)
        c0 = hashlib.sha256(self.curve.encode() + b"fflonk-v1" + self.vkd + t.l.to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()
        c1 = hashlib.sha256(c0 + C1).digest()
        beta, gamma = draw(r, c1, b"\x00"), draw(r, c1, b"\x01")
        # round 2: C2(tau) from Z, T1, T2 at tau^3
        z_vals, last = self.product(wires, beta, gamma)
        assert last == 1, "the product does not close"
        v3 = self.round2_at(pow(tau, 3, r), wires, pi_vals, z_vals, bs, beta, gamma)
        c2s = combine([v3["Z"], v3["T1"], v3["T2"]], tau, r)
        C2 = point(c2s)
        c2 = hashlib.sha256(c1 + C2).digest()
        ctr = 0
        while True:
            s = draw(r, c2, bytes([ctr]))
            if s != 0 and pow(pow(s, 24, r), t.n, r) != 1:
                break
            ctr += 1
        # round 3
        xi, sets = roots_of(self.curve, t.log_n, s)
        vx = self.round2_at(xi, wires, pi_vals, z_vals, bs, beta, gamma)
        vxw = self.round2_at(xi * t.w % r, wires, pi_vals, z_vals, bs, beta, gamma)
        assert vxw["Z"] == vx["Zw"]
        values = [vx[k] for k in FIXED] + [vx["a"], vx["b"], vx["c"], vx["Z"], vxw["Z"], vxw["T1"], vxw["T2"]]
        ys = [[combine([vx[k] for k in FIXED], h, r) for h in sets[0]], [combine([vx["a"], vx["b"], vx["c"], vx["T0"]], h, r) for h in sets[1]],
              [combine([vx["Z"], vx["T1"], vx["T2"]], h, r) for h in sets[2][:3]] + [combine([vxw["Z"], vxw["T1"], vxw["T2"]], h, r) for h in sets[2][3:]]]
        # round 4
        c3 = hashlib.sha256(c2 + b"".join(le(v) for v in values)).digest()
        g = draw(r, c3, b"\x00")
        f_tau = [self.c0, c1s, c2s]
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
        return {"publics": publics, "f_tau": f_tau, "sets": sets, "ys": ys, "values": values, "w1": w1, "w2": w2, "at_xi": vx,
                "challenges": {"beta": beta, "gamma": gamma, "s": s, "xi": xi, "gamma_open": g, "z_open": zq},
                "proof": {"C1": C1, "C2": C2, "W1": W1, "W2": point(w2), "values": values}}

    def opening_holds(self, res, ys=None, f_tau=None, sets=None, w1=None, w2=None, gamma=None, z=None):
        """the opening equation in the exponent under the known tau (kzg_multi_ref.proof_holds), any part replaced"""
        ch = res["challenges"]
        return mref.proof_holds(res["f_tau"] if f_tau is None else f_tau, res["sets"] if sets is None else sets, res["ys"] if ys is None else ys,
                                ch["gamma_open"] if gamma is None else gamma, ch["z_open"] if z is None else z, res["w1"] if w1 is None else w1,
                                res["w2"] if w2 is None else w2, self.tau, self.r)
