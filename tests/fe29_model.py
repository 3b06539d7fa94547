"""TEST INFRASTRUCTURE ONLY.  Python-integer model of csrc/fe29_impl.hip.h (29-bit limbs, 64-bit columns, lazily reduced values) and of
the coordinate field and XYZZ point formulas of csrc/ecpt_impl.hip.h, for tests/test_gpu_fe29.py and tests/test_gpu_ecpt.py.

A batch of n field elements is an object array of shape (NR, n): limb i of every element, Python integers; the value is sum l[i] << 29 i.
Every primitive replays the device's column accumulation and carry code step by step; what the header says cannot happen is a `need`
here (ModelError, an AssertionError): a 64-bit column reaching 2^64, a 32-bit limb wrapping, an fe_sub limb the arithmetic shift of
fe_norm_s does not see as it is, a negative value, a result that is not the mathematical one.  The second half (Bounded, Curve) carries an
upper bound beside every value, checks the header's A * B condition and fe_sub's b <= M q at every call site of the point formulas from
those bounds, and the stored-point invariants on every result.  Nothing is taken from the header's comments: the limit on A * B is
floor(R' / q), computed."""
import numpy as np

LB = 29
LMASK = (1 << LB) - 1
M32 = (1 << 32) - 1
FE_WIDE_MAX = 6


class ModelError(AssertionError):
    pass


def need(cond, msg):
    if not cond:
        raise ModelError(msg)


def _all(x):
    return bool(np.all(np.asarray(x, dtype=bool)))


def _signed(x):
    """a u32 word read as int"""
    return x - ((x >> 31) << 32)


# ---- operand forms shared by the two test modules ----
def _b(x):
    return np.asarray(x, dtype=bool)


def _stack(F, cols):
    """list of per-element limb lists -> (NR, n)"""
    out = np.empty((F.NR, len(cols)), dtype=object)
    for k, c in enumerate(cols):
        assert len(c) == F.NR
        for i in range(F.NR):
            out[i, k] = int(c[i])
    return out


def _sat(F, ub):
    """every low limb 2^29 - 1, the largest top limb that keeps the value <= ub (None if even a zero top limb is too much)"""
    t = (ub + 1) // (1 << (LB * (F.NR - 1))) - 1
    return None if t < 0 else [LMASK] * (F.NR - 1) + [t]


def _flat(F, ub, limb=1 << LB):
    """every low limb exactly `limb` (2^29: not normalised), the largest top limb that keeps the value <= ub"""
    low = sum(limb << (LB * i) for i in range(F.NR - 1))
    return None if low > ub else [limb] * (F.NR - 1) + [(ub - low) >> (LB * (F.NR - 1))]


def _val(l):
    return sum(int(x) << (LB * i) for i, x in enumerate(l))


class Field:
    def __init__(self, idx, name, q, nl, nr, doc_limit):
        self.idx, self.name, self.q, self.NL, self.NR, self.doc_limit = idx, name, q, nl, nr, doc_limit
        self.R, self.Rp = 1 << (32 * nl), 1 << (LB * nr)
        self.limit = self.Rp // q                     # a < A q, b < B q with A B <= limit: a b / R' + q <= 2q
        self.qinv = (-pow(q, -1, 1 << LB)) % (1 << LB)

    def split(self, v):
        """one integer -> NR normalised limbs (the top limb keeps the excess)"""
        return [(v >> (LB * i)) & LMASK for i in range(self.NR - 1)] + [v >> (LB * (self.NR - 1))]

    def limbs(self, vals):
        """integers -> (NR, n) normalised limbs"""
        v = np.array([int(x) for x in vals] + [None], dtype=object)[:-1]
        out = np.empty((self.NR, len(v)), dtype=object)
        for i in range(self.NR - 1):
            out[i] = v & LMASK
            v = v >> LB
        out[self.NR - 1] = v
        return out

    def val(self, l):
        acc = l[0] * 1
        for i in range(1, self.NR):
            acc = acc + (l[i] << (LB * i))
        return acc

    def normalised(self, l):
        return _all(l[:-1] <= LMASK) and _all(l >= 0) and _all(l[-1] <= M32)

    def to_mont(self, x):
        """internal Montgomery form (canonical) of the integer x"""
        return x * self.Rp % self.q


FIELDS = {
    "bn254_fq": Field(0, "bn254_fq", 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47, 8, 9, 168),
    "bls12_381_fq": Field(1, "bls12_381_fq", 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab, 12, 14, 168),
    "bn254_fr": Field(2, "bn254_fr", 21888242871839275222246405745257275088548364400416034343698204186575808495617, 8, 9, 168),
    "bls12_381_fr": Field(3, "bls12_381_fr", 52435875175126190479447740508185965837690552500527637822603658699938581184513, 8, 9, 68),
}


class Model:
    """the device's arithmetic on (NR, n) limb batches"""

    def __init__(self, F):
        self.F, self.NR, self.NL, self.q = F, F.NR, F.NL, F.q
        self.Q = F.split(F.q)
        self.QM = {m: F.split(m * F.q) for m in (2, 4, 8)}
        self.ONE, self.CIN, self.COUT = F.split(F.Rp % F.q), F.split(F.Rp * F.Rp * pow(F.R, -1, F.q) % F.q), F.split(F.R % F.q)
        self.neg_limbs = None
        self.m_zero = self.m_max = None               # of the last reduction: per element, whether a step had m == 0 / m == 2^29 - 1

    # ---- helpers ----
    def const(self, limbs, n):
        out = np.empty((self.NR, n), dtype=object)
        for i in range(self.NR):
            out[i] = limbs[i]
        return out

    def zero(self, n): return self.const([0] * self.NR, n)
    def one(self, n): return self.const(self.ONE, n)

    def _u32(self, l, what):
        need(_all(l >= 0) and _all(l <= M32), f"{what}: a limb is no u32 word")

    def _acc(self, t, k, v, what):
        t[k] = t[k] + v                               # every addend is >= 0: a column only grows, and _col checks it at its final value

    def _col(self, t, k, what):
        need(_all(t[k] < (1 << 64)), f"{what}: 64-bit column {k} reaches 2^64")

    # ---- carries ----
    def norm_u(self, l, what):
        l = l.copy()
        for i in range(self.NR - 1):
            l[i + 1] = l[i + 1] + (l[i] >> LB)
            need(_all(l[i + 1] <= M32), f"{what}: limb {i + 1} wraps")
            l[i] = l[i] & LMASK
        return l

    def norm_s(self, t, what):
        """fe_norm_s on the true (possibly negative) limbs t of a difference: replays the u32 words and the arithmetic shift of the word read
        as int, and requires every word to be the true limb"""
        r = t & M32
        true = t.copy()
        self.neg_limbs = np.zeros(t.shape[1], int)     # per element: how many low limbs were negative when they were shifted
        for i in range(self.NR - 1):
            self.neg_limbs += np.asarray(true[i] < 0, dtype=bool)
            need(_all(_signed(r[i]) == true[i]), f"{what}: limb {i} does not fit the int that fe_norm_s shifts")
            true[i + 1] = true[i + 1] + (true[i] >> LB)
            r[i + 1] = (r[i + 1] + ((_signed(r[i]) >> LB) & M32)) & M32
            r[i] = r[i] & LMASK
            true[i] = true[i] & LMASK
        return r, true

    def add(self, a, b):
        self._u32(a, "fe_add"); self._u32(b, "fe_add")
        r = a + b
        need(_all(r <= M32), "fe_add: a limb sum wraps")
        r = self.norm_u(r, "fe_add")
        need(_all(self.F.val(r) == self.F.val(a) + self.F.val(b)), "fe_add: wrong value")
        return r

    def dbl(self, a): return self.add(a, a)

    def sub(self, M, a, b):
        self._u32(a, "fe_sub"); self._u32(b, "fe_sub")
        t = a + self.const(self.QM[M], a.shape[1]) - b
        r, true = self.norm_s(t, f"fe_sub<{M}>")
        want = self.F.val(a) + M * self.q - self.F.val(b)
        need(_all(want >= 0), f"fe_sub<{M}>: the value goes negative (b > {M}q + a)")
        need(_all(true[-1] >= 0) and _all(true[-1] <= M32), f"fe_sub<{M}>: the top limb is no u32 word")
        need(_all(r == true) and _all(self.F.val(r) == want), f"fe_sub<{M}>: the limbs are not those of a - b + {M}q")
        return r

    # ---- products ----
    def _columns(self, pairs, what, start=None):
        n = pairs[0][0].shape[1]
        t = [np.array([0] * n + [None], dtype=object)[:-1] for _ in range(2 * self.NR)]
        if start is not None:
            self._u32(start, what)
            for i in range(self.NR):
                t[self.NR + i] = start[i] * 1
        for a, b in pairs:
            self._u32(a, what); self._u32(b, what)
            for i in range(self.NR):
                for j in range(self.NR):
                    self._acc(t, i + j, a[i] * b[j], what)
        return t

    def _reduce(self, t, what):
        NR = self.NR
        n = len(t[0])
        self.m_zero, self.m_max = np.zeros(n, bool), np.zeros(n, bool)
        msum = 0
        for i in range(NR):
            m = (((t[i] & M32) * self.F.qinv) & M32) & LMASK
            self.m_zero |= np.asarray(m == 0, dtype=bool); self.m_max |= np.asarray(m == LMASK, dtype=bool)
            msum = msum + (m << (LB * i))
            for j in range(NR):
                self._acc(t, i + j, m * self.Q[j], what)
            self._col(t, i, what)
            need(_all((t[i] & LMASK) == 0), f"{what}: the low 29 bits of column {i} are not zero after its reduction step")
            self._acc(t, i + 1, t[i] >> LB, what)
        r = np.empty((NR, n), dtype=object)
        for k in range(NR):
            self._col(t, NR + k, what)
            if k + 1 < NR:
                r[k] = (t[NR + k] & M32) & LMASK
                self._acc(t, NR + k + 1, t[NR + k] >> LB, what)
            else:
                need(_all(t[NR + k] <= M32), f"{what}: the top limb of the result does not fit 32 bits")
                r[k] = t[NR + k]
        return r, msum

    def _product(self, pairs, what, start=None):
        t = self._columns(pairs, what, start)
        r, msum = self._reduce(t, what)
        total = sum(self.F.val(a) * self.F.val(b) for a, b in pairs) + (self.F.val(start) * self.F.Rp if start is not None else 0)
        need(_all(self.F.val(r) * self.F.Rp == total + msum * self.q), f"{what}: the result is not (sum + m q) / R'")
        need(self.F.normalised(r), f"{what}: the result's limbs are not normalised")
        return r

    def mul(self, a, b): return self._product([(a, b)], "fe_mul")
    def mul2(self, a, b, c, d): return self._product([(a, b), (c, d)], "fe_mul2")
    def mul_acc(self, a, b, c): return self._product([(a, b)], "fe_mul_acc", start=c)

    def wide(self, pairs):
        need(1 <= len(pairs) <= FE_WIDE_MAX, "fe_wide: too many pairs")
        return self._product(pairs, "fe_wide")

    def sqr(self, a):
        """the dedicated fe_sqr: cross products once against a doubled limb; the columns must be those of fe_mul(a, a)"""
        self._u32(a, "fe_sqr")
        NR, n = self.NR, a.shape[1]
        d = a << 1
        need(_all(d <= M32), "fe_sqr: a doubled limb wraps")
        t = [np.array([0] * n + [None], dtype=object)[:-1] for _ in range(2 * NR)]
        for i in range(NR):
            self._acc(t, 2 * i, a[i] * a[i], "fe_sqr")
            for j in range(i + 1, NR):
                self._acc(t, i + j, d[i] * a[j], "fe_sqr")
        ref = self._columns([(a, a)], "fe_mul")
        need(all(_all(x == y) for x, y in zip(t, ref)), "fe_sqr: the column sums differ from fe_mul(a, a)'s")
        r, msum = self._reduce(t, "fe_sqr")
        need(_all(self.F.val(r) * self.F.Rp == self.F.val(a) ** 2 + msum * self.q), "fe_sqr: wrong value")
        return r

    # ---- predicates, canonical form, inverse, layouts ----
    def is_zero_m(self, a):
        z, e = 0, 0
        for i in range(self.NR):
            z = z | a[i]; e = e | (a[i] ^ self.Q[i])
        return np.asarray(z == 0, dtype=bool) | np.asarray(e == 0, dtype=bool)

    def canon(self, a):
        self._u32(a, "fe_canon")
        t, _ = self.norm_s(a - self.const(self.Q, a.shape[1]), "fe_canon")
        neg = np.asarray(_signed(t[-1]) < 0, dtype=bool)
        need(_all(neg == np.asarray(self.F.val(a) < self.q, dtype=bool)), "fe_canon: the sign of the top limb is not the sign of a - q")
        need(_all(neg | np.asarray(self.F.val(t) == self.F.val(a) - self.q, dtype=bool)), "fe_canon: the limbs are not those of a - q")
        return np.where(neg[None, :], a, t)

    def qm2_limbs(self):
        """fe_qm2_limb, as coded"""
        out = []
        for i in range(self.NR):
            borrow, o = 2, 0
            for k in range(i + 1):
                v = self.Q[k] - borrow
                borrow = 0
                if v < 0:
                    v += 1 << LB; borrow = 1
                o = v
            out.append(o)
        return out

    def inv(self, a):
        r = self.one(a.shape[1])
        e = self.qm2_limbs()
        for i in range(self.NR - 1, -1, -1):
            for b in range(LB - 1, -1, -1):
                r = self.sqr(r)
                if (e[i] >> b) & 1:
                    r = self.mul(r, a)
        return r

    def from_std(self, w):
        """w: (NL, n) external words"""
        NL, NR = self.NL, self.NR
        x = np.empty((NR, w.shape[1]), dtype=object)
        for k in range(NR):
            bit = LB * k; wi = bit >> 5; s = bit & 31
            v = (w[wi] >> s) if wi < NL else w[0] * 0
            if s > 32 - LB and wi + 1 < NL:
                v = v | ((w[wi + 1] << (32 - s)) & M32)
            x[k] = v & LMASK
        W = sum(w[i] << (32 * i) for i in range(NL))
        need(_all(self.F.val(x) == W), "fe_from_std: the repacked limbs are not the words' integer")
        return self.mul(x, self.const(self.CIN, w.shape[1]))

    def to_std(self, a):
        NL, NR = self.NL, self.NR
        p = self.mul(a, self.const(self.COUT, a.shape[1]))
        need(_all(self.F.val(p) < 2 * self.q), "fe_to_std: fe_canon's operand reaches 2q")
        return self.words(self.canon(p), "fe_to_std")

    def words(self, x, what):
        """canonical limbs -> (NL, n) 32-bit words, as fe_to_std and fe_to_canon_words repack them"""
        NL, NR = self.NL, self.NR
        w = np.empty((NL, x.shape[1]), dtype=object)
        for j in range(NL):
            bit = 32 * j; k = bit // LB; s = bit % LB
            v = x[k] >> s
            if k + 1 < NR: v = v | ((x[k + 1] << (LB - s)) & M32)
            if k + 2 < NR and 2 * LB - s < 32: v = v | ((x[k + 2] << (2 * LB - s)) & M32)
            w[j] = v & M32
        need(_all(sum(w[i] << (32 * i) for i in range(NL)) == self.F.val(x)), f"{what}: the words are not the canonical limbs' integer")
        return w

    def to_canon_words(self, a):
        """pairing_impl.hip.h's fe_to_canon_words: the product with the plain integer 1 leaves Montgomery form"""
        p = self.mul(a, self.const([1] + [0] * (self.NR - 1), a.shape[1]))
        need(_all(self.F.val(p) < 2 * self.q), "fe_to_canon_words: fe_canon's operand reaches 2q")
        return self.words(self.canon(p), "fe_to_canon_words")


# ---- values with bounds: the call sites of ecpt_impl.hip.h -----------------------------------------------------------------------
class V:
    """limbs and an inclusive upper bound of the value, one bound for the batch"""
    __slots__ = ("l", "ub")

    def __init__(self, l, ub):
        self.l, self.ub = l, ub


class Bounded:
    def __init__(self, F):
        self.F, self.m, self.q = F, Model(F), F.q
        self.cap = F.limit * F.q * F.q                 # a.ub * b.ub <= cap  <=>  A B <= floor(R' / q)

    def new(self, l, ub, what="operand"):
        need(_all(l >= 0) and _all(l[:-1] <= 1 << LB) and _all(l[-1] <= M32), f"{what}: a low limb above 2^29 (what the products admit)")
        need(_all(self.F.val(l) <= ub), f"{what}: a value exceeds its declared bound")
        return V(l, ub)

    def zero(self, n): return V(self.m.zero(n), 0)
    def one(self, n): return V(self.m.one(n), self.q - 1)
    def add(self, a, b): return V(self.m.add(a.l, b.l), a.ub + b.ub)
    def dbl(self, a): return self.add(a, a)

    def sub(self, M, a, b, site=""):
        need(b.ub <= M * self.q, f"{site}fe_sub<{M}>: the subtrahend may reach {b.ub / self.q:.3f}q > {M}q")
        return V(self.m.sub(M, a.l, b.l), a.ub + M * self.q)

    def _prod(self, r, what):
        need(_all(self.F.val(r) < 2 * self.q), f"{what}: a result reaches 2q")
        return V(r, 2 * self.q - 1)

    def mul(self, a, b, site=""):
        need(a.ub * b.ub <= self.cap, f"{site}fe_mul: A B = {a.ub * b.ub / self.q ** 2:.2f} > {self.F.limit}")
        return self._prod(self.m.mul(a.l, b.l), site + "fe_mul")

    def mul2(self, a, b, c, d, site=""):
        need(a.ub * b.ub + c.ub * d.ub <= self.cap, f"{site}fe_mul2: A B + C D = {(a.ub * b.ub + c.ub * d.ub) / self.q ** 2:.2f} > {self.F.limit}")
        return self._prod(self.m.mul2(a.l, b.l, c.l, d.l), site + "fe_mul2")

    def renorm(self, a): return self.mul(a, self.one(a.l.shape[1]), "fe_renorm: ")

    def is_zero_m(self, a, site=""):
        """x == 0 mod q for a product x: requires x < 2q normalised, so that 0 and q are the only candidates"""
        need(a.ub < 2 * self.q and self.F.normalised(a.l), f"{site}fe_is_zero_m: the operand is no normalised value below 2q")
        z = self.m.is_zero_m(a.l)
        need(_all(z == np.asarray(self.F.val(a.l) % self.q == 0, dtype=bool)), f"{site}fe_is_zero_m: misses a representative of zero")
        return z

    def inv(self, a, replay=False):
        """fe_inv's ladder multiplies a value below 2q by a.  replay: through the model's ladder (slow: test_gpu_fe29 does it once per
        field); otherwise the canonical inverse stands in for the ladder's representative -- the call sites see the same bound"""
        need(a.ub * (2 * self.q - 1) <= self.cap, "fe_inv: the operand is too large for the products of the ladder")
        if replay:
            return self._prod(self.m.inv(a.l), "fe_inv")
        Rp = self.F.Rp
        return V(self.F.limbs([pow(int(v) * pow(Rp, -1, self.q) % self.q, self.q - 2, self.q) * Rp % self.q for v in self.F.val(a.l)]), 2 * self.q - 1)


def _uniform(mask, what):
    need(_all(mask) or not np.any(mask), f"{what}: the batch does not take one branch")
    return bool(np.any(mask))


class Curve:
    """cf and the point formulas, as ecpt_impl.hip.h has them (squaring as fe_mul(a, a): msm.hip).  A cf is a V (G1) or a pair of V (G2);
    a point is a dict X, Y, ZZ, ZZZ.  Every batch must take one branch of a formula."""

    def __init__(self, F, g2):
        self.F, self.g2, self.B, self.q = F, g2, Bounded(F), F.q

    # -- cf --
    def _map(self, f, *a):
        return tuple(f(*[x[k] for x in a]) for k in (0, 1)) if self.g2 else f(*a)

    def n_of(self, a): return (a[0] if self.g2 else a).l.shape[1]
    def cf_zero(self, n): return (self.B.zero(n), self.B.zero(n)) if self.g2 else self.B.zero(n)
    def cf_one(self, n): return (self.B.one(n), self.B.zero(n)) if self.g2 else self.B.one(n)
    def cf_add(self, a, b): return self._map(self.B.add, a, b)
    def cf_dbl(self, a): return self.cf_add(a, a)
    def cf_sub(self, M, a, b, site=""): return self._map(lambda x, y: self.B.sub(M, x, y, site), a, b)

    def cf_mul(self, a, b, site=""):
        B = self.B
        if not self.g2:
            return B.mul(a, b, site)
        n = self.n_of(a)
        nb1 = B.sub(8, B.zero(n), b[1], site + "cf_mul: ")
        return (B.mul2(a[0], b[0], a[1], nb1, site + "cf_mul c0: "), B.mul2(a[0], b[1], a[1], b[0], site + "cf_mul c1: "))

    def cf_sqr(self, a, site=""):
        B = self.B
        if not self.g2:
            return B.mul(a, a, site + "cf_sqr: ")
        n = self.n_of(a)
        na1 = B.sub(8, B.zero(n), a[1], site + "cf_sqr: ")
        return (B.mul2(a[0], a[0], a[1], na1, site + "cf_sqr c0: "), B.mul(B.dbl(a[0]), a[1], site + "cf_sqr c1: "))

    def cf_is_zero_m(self, a, site=""):
        if not self.g2:
            return self.B.is_zero_m(a, site)
        return self.B.is_zero_m(a[0], site) & self.B.is_zero_m(a[1], site)

    def cf_inv(self, a, replay=False):
        B = self.B
        if not self.g2:
            return B.inv(a, replay)
        n = B.inv(B.renorm(B.add(B.mul(a[0], a[0], "cf_inv: "), B.mul(a[1], a[1], "cf_inv: "))), replay)
        return (B.mul(a[0], n, "cf_inv: "), B.mul(B.sub(2, B.zero(self.n_of(a)), a[1], "cf_inv: "), n, "cf_inv: "))

    # -- pairing_impl.hip.h's additions to cf (the twist only) --
    def cf_red(self, a): return (self.B.renorm(a[0]), self.B.renorm(a[1]))
    def cf_neg(self, a, site=""): return self.cf_sub(2, self.cf_zero(self.n_of(a)), a, site + "cf_neg: ")
    def cf_scale(self, a, s, site=""): return (self.B.mul(a[0], s, site + "cf_scale: "), self.B.mul(a[1], s, site + "cf_scale: "))

    def to_canon_words(self, a, site=""):
        """one Fq value (a V) -> (NL, n) canonical words"""
        need(a.ub <= self.B.cap, f"{site}fe_to_canon_words: the operand is too large for the product with 1")
        return self.B.m.to_canon_words(a.l)

    def cf_val(self, a):
        """residues mod q: an (n,) array (G1) or a pair of them"""
        return tuple(self.F.val(x.l) % self.q for x in a) if self.g2 else self.F.val(a.l) % self.q

    # -- points --
    def stored(self, p, what):
        """the invariants of a stored point, from the bounds the formulas give"""
        q = self.q
        for name, ub in (("X", 8 * q - 1), ("Y", 4 * q), ("ZZ", 2 * q - 1), ("ZZZ", 2 * q - 1)):
            for c in (p[name] if self.g2 else (p[name],)):
                need(c.ub <= ub, f"{what}: {name} may reach {c.ub / q:.3f}q")
                need(self.F.normalised(c.l) and _all(self.F.val(c.l) <= c.ub), f"{what}: {name} breaks its bound")
        return p

    def pt_inf(self, n): return {k: self.cf_zero(n) for k in ("X", "Y", "ZZ", "ZZZ")}
    def pt_is_inf(self, p): return self.cf_is_zero_m(p["ZZ"], "pt_is_inf: ")

    def pt_finish(self, r, U1, S1, P, Rr, PP):
        PPP, Q = self.cf_mul(P, PP, "pt_finish PPP: "), self.cf_mul(U1, PP, "pt_finish Q: ")
        r["X"] = self.cf_sub(4, self.cf_sub(2, self.cf_sqr(Rr, "pt_finish R^2: "), PPP, "pt_finish X: "), self.cf_dbl(Q), "pt_finish X: ")
        if self.g2:
            r["Y"] = self.cf_sub(2, self.cf_mul(self.cf_sub(8, Q, r["X"], "pt_finish Q - X3: "), Rr, "pt_finish (Q - X3) R: "),
                                 self.cf_mul(S1, PPP, "pt_finish S1 PPP: "), "pt_finish Y: ")
        else:
            r["Y"] = self.B.mul2(self.cf_sub(8, Q, r["X"], "pt_finish Q - X3: "), Rr, self.cf_sub(4, self.cf_zero(self.n_of(S1)), S1, "pt_finish -S1: "), PPP, "pt_finish Y: ")

    def _dbl_core(self, X, Y, what):
        U = self.cf_dbl(Y); V_ = self.cf_sqr(U, what + " V: "); W = self.cf_mul(U, V_, what + " W: "); S = self.cf_mul(X, V_, what + " S: ")
        xx = self.cf_sqr(X, what + " xx: "); M = self.cf_add(self.cf_dbl(xx), xx)
        r = {}
        r["X"] = self.cf_sub(4, self.cf_sqr(M, what + " M^2: "), self.cf_dbl(S), what + " X: ")
        r["Y"] = self.cf_sub(2, self.cf_mul(self.cf_sub(8, S, r["X"], what + " S - X3: "), M, what + " (S - X3) M: "), self.cf_mul(W, Y, what + " W Y: "), what + " Y: ")
        return r, V_, W

    def pt_dbl_aff(self, a):
        r, V_, W = self._dbl_core(a[0], a[1], "pt_dbl_aff")
        r["ZZ"], r["ZZZ"] = V_, W
        return self.stored(r, "pt_dbl_aff")

    def pt_dbl(self, p):
        if _uniform(self.pt_is_inf(p), "pt_dbl"):
            return p
        r, V_, W = self._dbl_core(p["X"], p["Y"], "pt_dbl")
        r["ZZ"], r["ZZZ"] = self.cf_mul(V_, p["ZZ"], "pt_dbl ZZ: "), self.cf_mul(W, p["ZZZ"], "pt_dbl ZZZ: ")
        return self.stored(r, "pt_dbl")

    def pt_madd(self, p, a):
        n = self.n_of(p["X"])
        if _uniform(self.pt_is_inf(p), "pt_madd"):
            return self.stored({"X": a[0], "Y": a[1], "ZZ": self.cf_one(n), "ZZZ": self.cf_one(n)}, "pt_madd onto infinity")
        U2, S2 = self.cf_mul(a[0], p["ZZ"], "pt_madd U2: "), self.cf_mul(a[1], p["ZZZ"], "pt_madd S2: ")
        P = self.cf_sub(8, U2, p["X"], "pt_madd P: ")
        Rr = self.cf_sub(4, S2, p["Y"], "pt_madd R: ")
        if self.g2:
            P = (P[0], self.B.renorm(P[1]))
        PP = self.cf_sqr(P, "pt_madd PP: ")
        if _uniform(self.cf_is_zero_m(PP, "pt_madd PP: "), "pt_madd P == 0"):
            if _uniform(self.cf_is_zero_m(self.cf_sqr(Rr, "pt_madd R^2: "), "pt_madd R^2: "), "pt_madd R == 0"):
                return self.pt_dbl_aff(a)
            return self.pt_inf(n)
        r = {}
        self.pt_finish(r, p["X"], p["Y"], P, Rr, PP)
        r["ZZ"] = self.cf_mul(p["ZZ"], PP, "pt_madd ZZ: ")
        r["ZZZ"] = self.cf_mul(p["ZZZ"], self.cf_mul(P, PP, "pt_madd PPP: "), "pt_madd ZZZ: ")
        return self.stored(r, "pt_madd")

    def pt_add(self, p, s):
        n = self.n_of(p["X"])
        if _uniform(self.pt_is_inf(p), "pt_add p"):
            return s
        if _uniform(self.pt_is_inf(s), "pt_add q"):
            return p
        U1, U2 = self.cf_mul(p["X"], s["ZZ"], "pt_add U1: "), self.cf_mul(s["X"], p["ZZ"], "pt_add U2: ")
        S1, S2 = self.cf_mul(p["Y"], s["ZZZ"], "pt_add S1: "), self.cf_mul(s["Y"], p["ZZZ"], "pt_add S2: ")
        P, Rr = self.cf_sub(2, U2, U1, "pt_add P: "), self.cf_sub(2, S2, S1, "pt_add R: ")
        PP = self.cf_sqr(P, "pt_add PP: ")
        if _uniform(self.cf_is_zero_m(PP, "pt_add PP: "), "pt_add P == 0"):
            if _uniform(self.cf_is_zero_m(self.cf_sqr(Rr, "pt_add R^2: "), "pt_add R^2: "), "pt_add R == 0"):
                return self.pt_dbl(p)
            return self.pt_inf(n)
        r = {}
        self.pt_finish(r, U1, S1, P, Rr, PP)
        r["ZZ"] = self.cf_mul(self.cf_mul(p["ZZ"], s["ZZ"], "pt_add ZZ: "), PP, "pt_add ZZ: ")
        r["ZZZ"] = self.cf_mul(self.cf_mul(p["ZZZ"], s["ZZZ"], "pt_add ZZZ: "), self.cf_mul(P, PP, "pt_add PPP: "), "pt_add ZZZ: ")
        return self.stored(r, "pt_add")

    def pt_neg(self, p):
        r = dict(p)
        r["Y"] = self.cf_sub(4, self.cf_zero(self.n_of(p["Y"])), p["Y"], "pt_neg: ")
        return self.stored(r, "pt_neg")

    def pt_to_std_bounds(self, p):
        """pt_to_std's call sites up to the two fe_to_std: returns the internal x, y (cf) whose external words go out"""
        izzz = self.cf_inv(p["ZZZ"]); t = self.cf_mul(p["ZZ"], izzz, "pt_to_std t: "); izz = self.cf_sqr(t, "pt_to_std izz: ")
        return self.cf_mul(p["X"], izz, "pt_to_std x: "), self.cf_mul(p["Y"], izzz, "pt_to_std y: ")
