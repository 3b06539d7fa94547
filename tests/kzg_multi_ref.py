"""The yardstick of the openings at several points (Boneh, Drake, Fisch, Gabizon 2020, section 4) in plain Python integers:
vanishing polynomials, Lagrange evaluation, the quotient by Z_S through SUCCESSIVE synthetic division -- a different route from the device's
partial fractions, which is kept here only to be compared against it -- the scalars of W1 and W2 under a known tau, and the verifier's
equation in the exponent.  No test, and no code shared with the library or the package's kzg.py; kzg_ref.py supplies Horner and the division
by X - z."""
import kzg_ref as ref


def poly_sub(a, b, r):
    n = max(len(a), len(b))
    return [((a[j] if j < len(a) else 0) - (b[j] if j < len(b) else 0)) % r for j in range(n)]


def poly_scale_add(acc, p, w, r):
    """acc + w p, as long as the longer of the two"""
    n = max(len(acc), len(p))
    return [((acc[j] if j < len(acc) else 0) + w * (p[j] if j < len(p) else 0)) % r for j in range(n)]


def vanishing_at(points, x, r):
    """Z_S(x) = prod_(s in S) (x - s)"""
    out = 1
    for s in points:
        out = out * (x - s) % r
    return out


def lagrange_eval(points, values, x, r):
    """r_S(x) for the interpolant of `values` on the distinct `points`: sum_s y_s prod_(s' != s) (x - s') / (s - s')"""
    out = 0
    for j, (s, y) in enumerate(zip(points, values)):
        num, den = 1, 1
        for j2, s2 in enumerate(points):
            if j2 != j:
                num = num * (x - s2) % r
                den = den * (s - s2) % r
        out = (out + y * num * pow(den, -1, r)) % r
    return out


def interpolant(points, values, r):
    """the coefficients of r_S (Newton's divided differences, expanded): len(points) of them"""
    n = len(points)
    dd = list(values)
    for lvl in range(1, n):
        for j in range(n - 1, lvl - 1, -1):
            dd[j] = (dd[j] - dd[j - 1]) * pow(points[j] - points[j - lvl], -1, r) % r
    out = [0] * n
    for j in range(n - 1, -1, -1):                      # out = out (X - points[j]) + dd[j]
        nxt = [0] * n
        for d in range(n):
            nxt[d] = (nxt[d] - points[j] * out[d]) % r
            if d + 1 < n:
                nxt[d + 1] = (nxt[d + 1] + out[d]) % r
        nxt[0] = (nxt[0] + dd[j]) % r
        out = nxt
    return out


def quotient_by_successive_division(f, points, r):
    """((f - r_S) / Z_S, values): f - r_S divided by X - s for one s after another; every remainder must be zero"""
    values = [ref.horner(f, s, r) for s in points]
    g = poly_sub(f, interpolant(points, values, r), r)
    for s in points:
        g, rem = ref.divide(g, s, r)
        assert rem == 0, "f - r_S does not vanish on S"
    return g, values


def quotient_by_partial_fractions(f, points, r):
    """the same quotient as sum_(s in S) a_s (f - f(s)) / (X - s), a_s = 1 / prod_(s' != s) (s - s'): len(f) - 1 coefficients, the top
    len(points) - 1 of them zero"""
    out = [0] * max(len(f) - 1, 0)
    for j, s in enumerate(points):
        den = 1
        for j2, s2 in enumerate(points):
            if j2 != j:
                den = den * (s - s2) % r
        q, _ = ref.divide(f, s, r)
        out = poly_scale_add(out, q, pow(den, -1, r), r)
    return out


def union(sets):
    t = []
    for s in sets:
        for p in s:
            if p not in t:
                t.append(p)
    return t


def open_scalars(polys, sets, gamma, z, tau, r):
    """(values, w1, w2): the scalars of W1 = [q(tau)] G and W2 = [(L / (X - z))(tau)] G under a known tau.
    q = sum_i gamma^i (f_i - r_i) / Z_(S_i); L = sum_i w_i (f_i - r_i(z)) - Z_T(z) q with w_i = gamma^i Z_(T \\ S_i)(z)"""
    T = union(sets)
    assert z not in T
    q, values = [], []
    for i, (f, s) in enumerate(zip(polys, sets)):
        qi, ys = quotient_by_successive_division(f, s, r)
        values.append(ys)
        q = poly_scale_add(q, qi, pow(gamma, i, r), r)
    zt = vanishing_at(T, z, r)
    L = [0]
    for i, (f, s) in enumerate(zip(polys, sets)):
        w = pow(gamma, i, r) * vanishing_at([t for t in T if t not in s], z, r) % r
        L = poly_scale_add(L, poly_sub(f, [lagrange_eval(s, values[i], z, r)], r), w, r)
    L = poly_scale_add(L, q, -zt % r, r)
    lq, rem = ref.divide(L, z, r)
    assert rem == 0, "L does not vanish at z"
    return values, ref.horner(q, tau, r), ref.horner(lq, tau, r)


def verifier_f(cs, sets, values, gamma, z, w1, r):
    """the scalar of F = sum_i w_i C_i - [sum_i w_i r_i(z)] G - Z_T(z) W1 from the scalars c_i of the commitments and w1 of W1"""
    T = union(sets)
    f = -vanishing_at(T, z, r) * w1
    for i, (c, s, ys) in enumerate(zip(cs, sets, values)):
        w = pow(gamma, i, r) * vanishing_at([t for t in T if t not in s], z, r) % r
        f += w * (c - lagrange_eval(s, ys, z, r))
    return f % r


def proof_holds(cs, sets, values, gamma, z, w1, w2, tau, r):
    """e(F + z W2, G2) e(-W2, tau G2) = 1 in the exponent: f + z w2 = tau w2"""
    return (verifier_f(cs, sets, values, gamma, z, w1, r) + z * w2 - tau * w2) % r == 0


def batch_holds(proofs, rhos, tau, r):
    """the batched equation in the exponent for proofs (cs, sets, values, gamma, z, w1, w2) under the weights rho_j"""
    total = 0
    for rho, (cs, sets, values, gamma, z, w1, w2) in zip(rhos, proofs):
        total += rho * (verifier_f(cs, sets, values, gamma, z, w1, r) + z * w2 - tau * w2)
    return total % r == 0


def interleave(polys):
    """sum_i p_i(X^k) X^i by slice assignment: out[i::k] = p_i, zero-padded"""
    k, n = len(polys), max((len(p) for p in polys), default=0)
    out = [0] * (k * n)
    for i, p in enumerate(polys):
        out[i:i + k * len(p):k] = p
    return out
