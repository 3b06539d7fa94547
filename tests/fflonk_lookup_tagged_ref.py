"""The yardstick of the fflonk prover with TAGGED lookups in plain Python integers and hashlib, over a powers-of-tau file
whose tau is KNOWN: fflonk_lookup_ref.Reference (the interleaved commitments as scalars, every polynomial evaluated at one point) with the
tables, the tag column, the weighted multiplicities, the running sum and lookup_term of plonk_lookup_tagged_ref.  It is evaluation-only and
shares no code with the package's fflonk_lookup_tagged.py.  What is its own: C0L = interleave_8(q_K, t1, t2, t3, Tg, 0, 0, 0) as the scalar
sum_m f_m(tau^8) tau^m, C0L opened on S0, the 23 values and the 30 opened ones, and the transcript, written from the issue: the domain strings
"fflonklt-vk" and "fflonklt-v1", c3 over the 23 values.  Among the values a bare T0 is the tag column (plonk_lookup_tagged_ref.FIXED ends in
it); the quotients at a point are under the lower-case keys t0 .. t3.  No test."""
import hashlib

import fflonk_lookup_ref as flref
import kzg_multi_ref as mref
import plonk_lookup_tagged_ref as tref
import plonk_ref as pref

R, tagged_chain, combine, roots_of, field_facts = pref.R, tref.tagged_chain, flref.combine, flref.roots_of, flref.field_facts
draw, le, dot = pref.draw, pref.le, pref.dot
FIXED = tref.FIXED                                                  # the 8 of fflonk's C0, then qK, T1, T2, T3 and the tag T0 of C0L
VALUE_NAMES = FIXED + ("a", "b", "c", "M", "Z", "Phi", "Zw", "Phiw", "T0w", "T1w")
N_VALUES, N_OPENED = 23, 30
C0L_NAMES = FIXED[8:]


class Reference(tref.Reference, flref.Reference):
    """everything the prover computes, as scalars.  tables: K >= 2 lists of rows of one to three values.  point(scalar) -> the bytes of
    [scalar] G as the transcript hashes them.  The circuit, the rows, the multiplicities and the running sum are plonk_lookup_tagged_ref's;
    zh, round1_at and the gate and permutation quotients of all_at are fflonk_lookup_ref's."""
    opening_holds = flref.Reference.opening_holds

    def __init__(self, curve, n_vars, public, gates, tables, tau, point):
        tref.Reference.__init__(self, curve, n_vars, public, gates, tables, tau, point)
        t, r = self.t, self.r
        lw8 = pref.lagrange_weights(t, pow(self.tau, 8, r))
        at8 = {k: dot(self.fixed_vals[k], lw8, r) for k in FIXED}
        self.c0 = combine([at8[k] for k in FIXED[:8]], self.tau, r)
        self.c0l = combine([at8[k] for k in C0L_NAMES] + [0, 0, 0], self.tau, r)
        self.C0, self.C0L = point(self.c0), point(self.c0l)
        self.vk_points = [self.C0, self.C0L]
        self.vkd = hashlib.sha256(curve.encode() + b"fflonklt-vk" + t.log_n.to_bytes(4, "little") + t.l.to_bytes(4, "little") + le(t.k[1]) + le(t.k[2]) + self.C0 + self.C0L).digest()

    def all_at(self, x, wires, pi_vals, z_vals, m, phi, bs, ch, rho_last=0):
        """fflonk_lookup_ref's, with t3 from the tagged L.  rho_last: L's value at the last row of H when the sum does not close; the
        quotient a forced prover commits to is then the polynomial part (L - rho) / Z_H, rho = rho_last L_(n-1)"""
        v = flref.Reference.all_at(self, x, wires, pi_vals, z_vals, m, phi, bs, ch)
        r = self.r
        rho = rho_last * pref.lagrange_weights(self.t, x)[-1] if rho_last else 0
        v["t3"] = (tref.lookup_term(r, v, ch["eta"], ch["delta"]) - rho) * pow(self.zh(x), -1, r) % r
        return v

    def prove(self, witness, blinding, multiplicities=None, force=False):
        """force: the prover checks neither the lookups nor the sum, and commits to the polynomial part of L / Z_H"""
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
        pi_vals = [(-x) % r for x in publics] + [0] * (t.n - t.l)
        # round 1: C1(tau) from a, b, c, M at tau^4
        v1 = self.round1_at(pow(tau, 4, r), wires, m, bs)
        c1s = combine([v1["a"], v1["b"], v1["c"], v1["M"]], tau, r)
        C1 = point(c1s)
        c0 = hashlib.sha256(self.curve.encode() + b"fflonklt-v1" + self.vkd + t.l.to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()
        c1 = hashlib.sha256(c0 + C1).digest()
        ch = {"beta": draw(r, c1, b"\x00"), "gamma": draw(r, c1, b"\x01"), "eta": draw(r, c1, b"\x02"), "delta": draw(r, c1, b"\x03")}
        # round 2: C2(tau) from Z, Phi, T0, T1 at tau^4, C3(tau) from T2, T3 at tau^2
        z_vals, last = self.product(wires, ch["beta"], ch["gamma"])
        assert last == 1, "the product does not close"
        phi, closes = self.running_sum(wires, m, ch["eta"], ch["delta"])
        assert force or closes == 0, "the lookup sum does not close"
        f_last, t_last = self.terms(wires, t.n - 1, ch["eta"], ch["delta"])
        rho_last = (-closes) * f_last * t_last % r                                          # L at the last row of H; 0 when the sum closes
        at = lambda x: self.all_at(x, wires, pi_vals, z_vals, m, phi, bs, ch, rho_last)
        v4, v2 = at(pow(tau, 4, r)), at(pow(tau, 2, r))
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
        # round 3: C0L on S0, the set of C0
        xi, sets4 = roots_of(self.curve, t.log_n, s)
        sets = [sets4[0], sets4[0], sets4[1], sets4[2], sets4[3]]
        vx, vxw = at(xi), at(xi * t.w % r)
        assert vxw["Z"] == vx["Zw"] and vxw["Phi"] == vx["Phiw"]
        values = [vx[k] for k in FIXED] + [vx[k] for k in ("a", "b", "c", "M", "Z", "Phi")] + [vxw[k] for k in ("Z", "Phi", "t0", "t1")]
        on = lambda v, names, hs: [combine([v[k] for k in names], h, r) for h in hs]
        ys = [on(vx, FIXED[:8], sets[0]), on(vx, C0L_NAMES, sets[1]), on(vx, ("a", "b", "c", "M"), sets[2]),
              on(vx, ("Z", "Phi", "t0", "t1"), sets[3][:4]) + on(vxw, ("Z", "Phi", "t0", "t1"), sets[3][4:]), on(vx, ("t2", "t3"), sets[4])]
        assert sum(len(y) for y in ys) == N_OPENED and len(values) == N_VALUES
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
        return {"publics": publics, "m": m, "f_tau": f_tau, "sets": sets, "ys": ys, "values": values, "w1": w1, "w2": w2, "at_xi": vx, "challenges": ch, "closes": closes,
                "proof": {"C1": C1, "C2": C2, "C3": C3, "W1": W1, "W2": point(w2), "values": values}}

    def rebuilt(self, publics, values, ch):
        """the verifier's side: the 30 opened values the 23 values imply, T0 .. T3 at xi from the identities"""
        t, r, xi = self.t, self.r, ch["xi"]
        v = dict(zip(VALUE_NAMES, values))
        lw = pref.lagrange_weights(t, xi)
        pi = -sum(x * lw[i] for i, x in enumerate(publics)) % r
        inv = pow(self.zh(xi), -1, r)
        beta, gamma = ch["beta"], ch["gamma"]
        gate = v["a"] * v["b"] * v["qM"] + v["a"] * v["qL"] + v["b"] * v["qR"] + v["c"] * v["qO"] + v["qC"] + pi
        p1 = (v["a"] + beta * xi + gamma) * (v["b"] + beta * t.k[1] * xi + gamma) * (v["c"] + beta * t.k[2] * xi + gamma) * v["Z"]
        p2 = (v["a"] + beta * v["S1"] + gamma) * (v["b"] + beta * v["S2"] + gamma) * (v["c"] + beta * v["S3"] + gamma) * v["Zw"]
        q = {"t0": gate % r * inv % r, "t1": lw[0] * (v["Z"] - 1) % r * inv % r, "t2": (p1 - p2) % r * inv % r, "t3": tref.lookup_term(r, v, ch["eta"], ch["delta"]) * inv % r}
        _, (S0, S1, S2, S3) = roots_of(self.curve, t.log_n, ch["s"])
        on = lambda parts, hs: [combine(parts, h, r) for h in hs]
        return [on(values[:8], S0), on(list(values[8:13]) + [0, 0, 0], S0), on([v["a"], v["b"], v["c"], v["M"]], S1),
                on([v["Z"], v["Phi"], q["t0"], q["t1"]], S2[:4]) + on([v["Zw"], v["Phiw"], v["T0w"], v["T1w"]], S2[4:]), on([q["t2"], q["t3"]], S3)]

    def verify(self, res, values=None):
        """the model's verifier: the opening equation over the values REBUILT from the 23 -- there is no separate identity check"""
        vals = res["values"] if values is None else values
        return self.opening_holds(res, ys=self.rebuilt(res["publics"], vals, res["challenges"]))
