"""The KZG layer's yardstick in plain Python integers: Horner evaluation, synthetic division, the gamma fold of polynomials and values, the
scalars of the batched verification.  No test, and no code shared with the library or the package's kzg.py."""
R = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
TWO_ADICITY = {"BN128": 28, "BLS12381": 32}


def horner(coeffs, z, r):
    """p(z) mod r; coefficients lowest degree first"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % r
    return acc


def divide(coeffs, z, r):
    """(q, y): p = q (X - z) + y, q_j = sum_{i > j} c_i z^(i - j - 1)"""
    n = len(coeffs)
    if n == 0:
        return [], 0
    q = [0] * (n - 1)
    acc = 0
    for j in range(n - 1, 0, -1):
        acc = (acc * z + coeffs[j]) % r
        q[j - 1] = acc
    return q, (acc * z + coeffs[0]) % r


def fold_polys(polys, gamma, r):
    """sum_i gamma^i p_i, shorter polynomials zero-padded"""
    n = max((len(p) for p in polys), default=0)
    out = [0] * n
    g = 1
    for p in polys:
        for j, c in enumerate(p):
            out[j] = (out[j] + g * c) % r
        g = g * gamma % r
    return out


def fold_values(ys, gamma, r):
    return sum(y * pow(gamma, i, r) for i, y in enumerate(ys)) % r


def root_of_unity(curve, log_n):
    """the primitive 2^log_n-th root of the library's transforms: 7^((r - 1) / 2^log_n)"""
    r = R[curve]
    assert log_n <= TWO_ADICITY[curve]
    return pow(7, (r - 1) >> log_n, r)


def ntt(coeffs, curve):
    """values of the polynomial on the domain {omega^i}, natural order (quadratic: small sizes only)"""
    r = R[curve]
    n = len(coeffs)
    w = root_of_unity(curve, n.bit_length() - 1)
    return [horner(coeffs, pow(w, i, r), r) for i in range(n)]


def witness_scalar(coeffs, z, tau, r):
    """(p(tau) - p(z)) / (tau - z): the scalar of the opening's witness under a known tau"""
    return (horner(coeffs, tau, r) - horner(coeffs, z, r)) * pow(tau - z, -1, r) % r


def opening_holds(c, z, y, w, tau, r):
    """the pairing equation of one opening in the exponent: c - y + z w = tau w, for the scalars c, w of the points C, W"""
    return (c - y + z * w - tau * w) % r == 0


def batch_holds(openings, rhos, tau, r):
    """the batched equation in the exponent: L = sum rho_j c_j - sum rho_j y_j + sum rho_j z_j w_j, R = sum rho_j w_j, L = tau R"""
    left = sum(rho * (c - y + z * w) for rho, (c, z, y, w) in zip(rhos, openings)) % r
    right = sum(rho * w for rho, (c, z, y, w) in zip(rhos, openings)) % r
    return (left - tau * right) % r == 0
