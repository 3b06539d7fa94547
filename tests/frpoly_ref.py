"""The yardstick of the scalar-field polynomial layer in plain Python integers: running products, inversion by pow(x, -1, r), the schoolbook
product, division by X^N - 1 by long division, the coset factors from their definition.  No test, and no code shared with the library or
the package's frpoly.py."""
from kzg_ref import R, root_of_unity  # noqa: F401  (the moduli and the transforms' root, as the KZG yardstick states them)


def mont_words(vals, r):
    """integers mod r -> the n x 4 u64 Montgomery words (R = 2^256) a canonical result vector must hold, as a flat numpy array"""
    import numpy as np
    b = b"".join(((v % r << 256) % r).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype="<u8").astype(np.uint64)


def words_ints(words):
    """n x 4 u64 words -> the plain integers they spell (no reduction: a word vector that is not canonical shows)"""
    import numpy as np
    b = np.ascontiguousarray(words, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def prefix_products(v, r, inclusive=False):
    """(products, total): products[i] = prod_{j < i} v[j], or with inclusive prod_{j <= i} v[j]"""
    out, acc = [], 1
    for x in v:
        if inclusive:
            acc = acc * x % r
            out.append(acc)
        else:
            out.append(acc)
            acc = acc * x % r
    return out, acc


def inverses(v, r):
    """(inverses with zero left zero, number of zeros, index of the first zero or None)"""
    zeros = [i for i, x in enumerate(v) if x % r == 0]
    return [0 if x % r == 0 else pow(x, -1, r) for x in v], len(zeros), (zeros[0] if zeros else None)


def pointwise(op, a, b, r):
    f = {"mul": lambda x, y: x * y, "add": lambda x, y: x + y, "sub": lambda x, y: x - y}[op]
    return [f(x, y) % r for x, y in zip(a, b)]


def powers(base, scale, n, r):
    out, acc = [], scale % r
    for _ in range(n):
        out.append(acc)
        acc = acc * base % r
    return out


def terms(cols, labels, beta, gamma, r):
    n = len(cols[0])
    out = []
    for i in range(n):
        acc = 1
        for c in range(len(cols)):
            acc = acc * (cols[c][i] + (beta * labels[c][i] if labels is not None else 0) + gamma) % r
        out.append(acc)
    return out


def grand_product(num, den, r):
    """(z_0 .. z_(n-1), z_n) by the recurrence, one inversion per row"""
    z, acc = [], 1
    for a, b in zip(num, den):
        z.append(acc)
        acc = acc * a % r * pow(b, -1, r) % r
    return z, acc


def poly_mul(a, b, r):
    """schoolbook, len(a) + len(b) - 1 coefficients: every a_i b_j is formed and added to column i + j; the columns are reduced once, at the end"""
    nb = len(b)
    out = [0] * (len(a) + nb - 1)
    for i, x in enumerate(a):
        if x:
            out[i:i + nb] = [o + x * y for o, y in zip(out[i:i + nb], b)]
    return [o % r for o in out]


def poly_eval(p, x, r):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % r
    return acc


def divmod_zh(p, log_n, r):
    """long division of p by X^N - 1 from the top coefficient down: (q of max(len(p) - N, 0) coefficients, rem of N, zero-padded)"""
    N = 1 << log_n
    work = list(p)
    q = [0] * max(len(p) - N, 0)
    for i in range(len(p) - 1, N - 1, -1):
        c = work[i]
        q[i - N] = c
        work[i] = 0
        work[i - N] = (work[i - N] + c) % r       # c X^i = c X^(i-N) (X^N - 1) + c X^(i-N)
    rem = [x % r for x in work[:N]] + [0] * max(N - len(p), 0)
    return q, rem


def coset_factors(curve, log_m, log_n):
    """1 / (7^N w_m^(iN) - 1) for i < m, from the definition"""
    r = R[curve]
    m, N = 1 << log_m, 1 << log_n
    w = root_of_unity(curve, log_m)
    g = pow(7, N, r)
    return [pow((g * pow(w, i * N, r) - 1) % r, -1, r) for i in range(m)]
