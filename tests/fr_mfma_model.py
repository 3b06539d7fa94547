"""TEST INFRASTRUCTURE ONLY.  Integer model of csrc/fr_mfma.hip.h -- the linear steps of the one-lane BN128 / BLS12-381 Poseidon kernels on
the matrix pipe -- for tests/test_fr_mfma_model.py and tests/test_gpu_fr_mfma.py.

The model reads the canonical constants itself (eigen-zkvm_amd/data/poseidon_<field>_constants.bin, layout: tools/
gen_poseidon_bn128_constants.py) and takes no table from the library.  For one output o of a layer the device's result is one definite
integer.  With bal(v) the representative of v in (-r/2, r/2] and s the Montgomery step (29 dense, 32 sparse):

    N = sum_j sum_b (byte_b(x_j) - 128) bal(c_jo 2^(s + 8b) mod r)  +  ((add_o + corr_o - bias) mod r)  +  bias
    corr_o = 128 sum_j sum_b (c_jo 2^(s + 8b) mod r) mod r,   bias = sum_q 2^(48 + 32q),   out = (N + m r) / 2^s,  m = -N / r mod 2^s

computed the device's way: per digit column (32 of them, weight 2^(8d), each asserted below 2^23 in magnitude) in integer matrices, then
eight biased words of weight 2^(32q) (each asserted inside (0, 2^49)), then the Montgomery step.  The dense layers write `out` as eight
29-bit limbs with the rest in the ninth; the sparse rounds form eight 32-bit words (asserted: out < 2^256) and repack them.  x_0^5 of a
sparse round is the exact lazy representative fe_sqr / fe_mul return: tests/fe29_model.py replays them.  The carry `lo[q] + c` of
mf_reduce_words is replayed too, so that a test can require it to have wrapped.

Beside it a plain Poseidon permutation mod r over the same file (c, M, P, S), anchored to the oracle by tests/test_fr_mfma_model.py."""
import functools
import pathlib
import struct

import numpy as np

from fe29_model import FIELDS, LB, Model

DATA = pathlib.Path(__file__).resolve().parent.parent / "eigen-zkvm_amd" / "data"
FE29 = {"bn128": "bn254_fr", "bls12381": "bls12_381_fr"}
OUT_IDX = {"bn128": 0, "bls12381": 1}                 # the state word Poseidon::hash returns
NR = 9
RP_BITS = LB * NR                                     # internal form: x R' mod r, R' = 2^261
DENSE_SHIFT, SPARSE_SHIFT = 29, 32
M32 = (1 << 32) - 1
DIGIT_OFFSET = sum(128 << (8 * d) for d in range(32))
BIAS = sum(1 << (48 + 32 * q) for q in range(8))


class MfModelError(AssertionError):
    pass


def need(cond, msg):
    if not cond:
        raise MfModelError(msg)


@functools.lru_cache(maxsize=None)
def constants(field):
    """{t: (c, M, P, S)} for t = 2..17: lists of canonical integers; M and P as [j * t + o]"""
    buf = (DATA / ("poseidon_%s_constants.bin" % field)).read_bytes()
    assert buf[:4] == b"PBN1" and struct.unpack_from("<I", buf, 4)[0] == 16
    pos, out = 8, {}
    for k in range(16):
        t, n_c, n_s = struct.unpack_from("<III", buf, pos); pos += 12
        assert t == k + 2 and n_s % (2 * t - 1) == 0 and n_c == 8 * t + n_s // (2 * t - 1)
        n = n_c + 2 * t * t + n_s
        v = [int.from_bytes(buf[pos + 32 * i:pos + 32 * i + 32], "little") for i in range(n)]
        pos += 32 * n
        out[t] = (v[:n_c], v[n_c:n_c + t * t], v[n_c + t * t:n_c + 2 * t * t], v[n_c + 2 * t * t:])
    assert pos == len(buf)
    return out


def n_rp(field, t):
    return len(constants(field)[t][3]) // (2 * t - 1)


def byte_matrix(X):
    """(n, w) integers < 2^256 -> (n, w * 32) float64 of (byte - 128), little endian"""
    n, w = X.shape
    raw = b"".join(int(v).to_bytes(32, "little") for v in X.reshape(-1))
    return np.frombuffer(raw, np.uint8).reshape(n, w * 32).astype(np.float64) - 128.0


def _obj(a):
    out = np.empty(a.shape, dtype=object)
    out[...] = a.tolist() if isinstance(a, np.ndarray) else a
    return out


class MfModel:
    def __init__(self, field, t):
        self.field, self.t = field, t
        self.F = FIELDS[FE29[field]]
        self.r = r = self.F.q
        self.c, self.M, self.P, self.S = constants(field)[t]
        self.n_rp = n_rp(field, t)
        self.fe = Model(self.F)
        self.Rp = (1 << RP_BITS) % r
        self.bias_mod = BIAS % r
        self._dense, self._sparse = {}, {}
        self._ident = self._fragment(1, SPARSE_SHIFT)

    # ---- tables, from the constants alone ----
    def bal(self, v):
        return v - self.r if self.r - v < v else v            # mf_digits: v - r where r - v < v

    def _fragment(self, coef, shift):
        """the 32 x 32 balanced digits [byte b][digit d] of coef 2^(shift + 8b) mod r, and the sum of those 32 residues"""
        r = self.r
        v = coef * (1 << shift) % r
        raw, tot = [], 0
        for _ in range(32):
            s = self.bal(v) + DIGIT_OFFSET
            need(0 <= s < 1 << 256, "a constant does not fit 32 balanced digits")
            raw.append(s.to_bytes(32, "little"))
            tot += v
            v = (v << 8) % r
        return np.frombuffer(b"".join(raw), np.uint8).reshape(32, 32).astype(np.float64) - 128.0, tot

    def _addends(self, add, corr):
        k = (add + corr - self.bias_mod) % self.r
        return np.array([(1 << 48) + ((k >> (32 * q)) & M32) for q in range(8)], np.int64)

    def c_at(self, layer):
        """index of the round constants whose image rides on the layer's addends (None: the last layer has none)"""
        t = self.t
        return None if layer == 7 else (layer + 1) * t if layer < 3 else 4 * t if layer == 3 else 5 * t + self.n_rp + (layer - 4) * t

    def mat(self, layer):
        return self.P if layer == 3 else self.M

    def dense_tables(self, layer):
        """D [t * 32 (word j, byte b)][t * 32 (output o, digit d)], K [t][8]"""
        if layer not in self._dense:
            t, r, mat = self.t, self.r, self.mat(layer)
            key = "P" if layer == 3 else "M"
            if key not in self._dense:
                D = np.zeros((t * 32, t * 32)); corr = [0] * t
                for o in range(t):
                    for j in range(t):
                        D[j * 32:(j + 1) * 32, o * 32:(o + 1) * 32], tot = self._fragment(mat[j * t + o], DENSE_SHIFT)
                        corr[o] += tot
                self._dense[key] = (D, [128 * x % r for x in corr])
            D, corr = self._dense[key]
            at = self.c_at(layer)
            K = np.zeros((t, 8), np.int64)
            for o in range(t):
                add = 0 if at is None else sum(self.c[at + j] * (1 << (RP_BITS + DENSE_SHIFT)) % r * mat[j * t + o] for j in range(t)) % r
                K[o] = self._addends(add, corr[o])
            self._dense[layer] = (D, K)
        return self._dense[layer]

    def sparse_tables(self, rnd):
        """row D [t * 32][32], column D [32 (byte of x_0^5)][(t - 1) * 32 (word k, digit d)], K [t][8]"""
        if rnd not in self._sparse:
            t, r = self.t, self.r
            Sr = self.S[(2 * t - 1) * rnd:(2 * t - 1) * (rnd + 1)]
            cr = self.c[5 * t + rnd] * (1 << (RP_BITS + SPARSE_SHIFT)) % r
            K = np.zeros((t, 8), np.int64)
            Drow = np.zeros((t * 32, 32)); corr = 0
            for j in range(t):
                Drow[j * 32:(j + 1) * 32], tot = self._fragment(Sr[j], SPARSE_SHIFT)
                corr += tot
            K[0] = self._addends(cr * Sr[0] % r, 128 * corr % r)
            Dcol = np.zeros((32, (t - 1) * 32))
            for k in range(1, t):
                Dcol[:, (k - 1) * 32:k * 32], tot = self._fragment(Sr[t + k - 1], SPARSE_SHIFT)
                K[k] = self._addends(cr * Sr[t + k - 1] % r, 128 * (tot + self._ident[1]) % r)
            self._sparse[rnd] = (Drow, Dcol, K)
        return self._sparse[rnd]

    # ---- the device's arithmetic ----
    def _finish(self, col, K, shift, what):
        """digit columns (n, o, 32) + addends (o, 8) -> out (n, o) integers, and whether `lo[q] + c` wrapped (n, o)"""
        need(bool((np.abs(col) < float(1 << 23)).all()), f"{what}: a digit column leaves (-2^23, 2^23)")
        col = col.astype(np.int64)
        n, no = col.shape[:2]
        c4 = col.reshape(n, no, 8, 4)
        W = K[None] + c4[..., 0] + (c4[..., 1] << 8) + (c4[..., 2] << 16) + (c4[..., 3] << 24)
        need(bool(((W > 0) & (W < (1 << 49))).all()), f"{what}: a biased word leaves (0, 2^49)")
        lo, hi = W & M32, W >> 32
        wrapped = np.zeros((n, no), bool)
        c = hi[..., 0]
        for q in range(1, 8):                                  # mf_reduce_words: x = lo[q] + c; c = hi[q] + (x < c)
            x = lo[..., q] + c
            w = x >> 32
            wrapped |= w.astype(bool)
            c = hi[..., q] + w
        lo_raw = np.ascontiguousarray(lo.astype("<u4")).tobytes()
        hi_raw = np.ascontiguousarray(hi.astype("<u4")).tobytes()
        V = np.empty(n * no, dtype=object)
        for i in range(n * no):
            V[i] = int.from_bytes(lo_raw[32 * i:32 * i + 32], "little") + (int.from_bytes(hi_raw[32 * i:32 * i + 32], "little") << 32)
        mask = (1 << shift) - 1
        ninv = (-pow(self.r, -1, 1 << shift)) % (1 << shift)
        m = ((V & mask) * ninv) & mask
        S = V + m * self.r
        need(bool(np.all((S & mask) == 0)), f"{what}: the Montgomery step leaves low bits")
        return (S >> shift).reshape(n, no), wrapped

    def dense(self, layer, X):
        """one dense layer on (n, t) integers < 2^256: the integers mf_dense writes (eight 29-bit limbs, the rest in the ninth)"""
        D, K = self.dense_tables(layer)
        n = X.shape[0]
        out, _ = self._finish((byte_matrix(X) @ D).reshape(n, self.t, 32), K, DENSE_SHIFT, f"dense layer {layer}")
        need(bool(np.all(out < (1 << (LB * 8 + 32)))), f"dense layer {layer}: the ninth limb overflows")
        return out

    def sparse_linear(self, rnd, Y):
        """the products of sparse round rnd on (n, t) integers < 2^256, word 0 standing for x_0^5: (out, wrapped), both (n, t)"""
        Drow, Dcol, K = self.sparse_tables(rnd)
        n, t = Y.shape[0], self.t
        B = byte_matrix(Y)
        col = np.empty((n, t, 32))
        col[:, 0] = B @ Drow
        col[:, 1:] = (B[:, :32] @ Dcol).reshape(n, t - 1, 32) + B[:, 32:].reshape(n, t - 1, 32) @ self._ident[0]
        return self._finish(col, K, SPARSE_SHIFT, f"sparse round {rnd}")

    def pow5(self, x):
        """(n,) integers < 2^256 -> the lazy representatives pow5 returns (fe_sqr, fe_sqr, fe_mul replayed by fe29_model)"""
        a = self.F.limbs(list(x))
        x2 = self.fe.sqr(a); x4 = self.fe.sqr(x2)
        return self.F.val(self.fe.mul(x4, a))

    def sparse(self, n_rounds, X):
        """the first n_rounds sparse rounds on (n, t) integers < 2^256: (out (n, t), per state whether a carry of mf_reduce_words wrapped)"""
        need(1 <= n_rounds <= self.n_rp, "no such number of sparse rounds")
        X = X.copy()
        wrapped = np.zeros(X.shape[0], bool)
        for rnd in range(n_rounds):
            X[:, 0] = self.pow5(X[:, 0])
            X, w = self.sparse_linear(rnd, X)
            need(bool(np.all(X < (1 << 256))), f"sparse round {rnd}: a result does not fit eight 32-bit words")
            wrapped |= w.any(axis=1)
        return X, wrapped

    def limbs(self, X):
        """(n, t) integers -> (n, t, NR) uint32: eight 29-bit limbs, the rest in the ninth"""
        n, t = X.shape
        out = np.zeros((n, t, NR), np.uint32)
        for i in range(n):
            for j in range(t):
                v = int(X[i, j])
                need(0 <= v < 1 << (LB * 8 + 32), "a value does not fit nine limbs")
                out[i, j] = self.F.split(v)
        return out

    @staticmethod
    def values(L):
        """(n, t, NR) uint32 -> (n, t) integers"""
        out = np.zeros(L.shape[:2], dtype=object)
        for k in range(NR):
            out = out + (_obj(L[..., k].astype(np.int64)) << (LB * k))
        return out

    # ---- plain arithmetic mod r ----
    def plain_dense(self, layer, X):
        """residues of sum_j c_jo x_j + sum_j c_jo (round constant j of the layer, internal form)"""
        t, r, mat, at = self.t, self.r, self.mat(layer), self.c_at(layer)
        cols = []
        for o in range(t):
            acc = sum(X[:, j] * mat[j * t + o] for j in range(t))
            if at is not None:
                acc = acc + sum(self.c[at + j] * self.Rp * mat[j * t + o] for j in range(t))
            cols.append(acc % r)
        return np.stack(cols, axis=1)

    def plain_sparse(self, n_rounds, X):
        """residues after the first n_rounds sparse rounds, words in the internal form"""
        t, r = self.t, self.r
        rinv4 = pow(self.Rp, -4, r)
        st = [X[:, j] % r for j in range(t)]
        for rnd in range(n_rounds):
            Sr = self.S[(2 * t - 1) * rnd:(2 * t - 1) * (rnd + 1)]
            y = (st[0] ** 5 * rinv4 + self.c[5 * t + rnd] * self.Rp) % r
            s0 = (y * Sr[0] + sum(st[j] * Sr[j] for j in range(1, t))) % r
            st = [s0] + [(st[k] + y * Sr[t + k - 1]) % r for k in range(1, t)]
        return np.stack(st, axis=1)

    def permutation(self, X):
        """the Poseidon permutation (poseidon_bn128_opt.rs hash_inner) on (n, t) canonical residues"""
        t, r, c, M, P, S = self.t, self.r, self.c, self.M, self.P, self.S
        st = [X[:, j] % r for j in range(t)]
        mul = lambda mat, st: [sum(st[j] * mat[j * t + o] for j in range(t)) % r for o in range(t)]     # noqa: E731
        st = [(st[i] + c[i]) % r for i in range(t)]
        for rd in range(4):
            st = [(st[i] ** 5 + c[(rd + 1) * t + i]) % r for i in range(t)]
            st = mul(P if rd == 3 else M, st)
        for rnd in range(self.n_rp):
            Sr = S[(2 * t - 1) * rnd:(2 * t - 1) * (rnd + 1)]
            y = (st[0] ** 5 + c[5 * t + rnd]) % r
            s0 = (y * Sr[0] + sum(st[j] * Sr[j] for j in range(1, t))) % r
            st = [s0] + [(st[k] + y * Sr[t + k - 1]) % r for k in range(1, t)]
        for rd in range(4):
            st = [(st[i] ** 5 + (c[5 * t + self.n_rp + rd * t + i] if rd < 3 else 0)) % r for i in range(t)]
            st = mul(M, st)
        return np.stack(st, axis=1)

    # ---- directed states ----
    def column_drivers(self, D, digit_cols):
        """for the digit columns `digit_cols` of a table D [word j, byte b][32] the two states that drive each as far as it goes: 0xFF
        (+127) where the digit is positive and 0x00 (-128) where it is negative, and the other way round"""
        out = []
        for d in digit_cols:
            for sign in (1, -1):
                by = np.where(D[:, d] * sign > 0, 0xFF, 0x00).astype(np.uint8).reshape(self.t, 32)
                out.append([int.from_bytes(by[j].tobytes(), "little") for j in range(self.t)])
        return out

    def wrap_state(self, rng):
        """a state whose word 1 makes `lo[q] + c` of mf_reduce_words wrap in the first sparse round (found by search: one word in 2^16)"""
        t = self.t
        x0 = self.r - 1
        y = int(self.pow5(np.array([x0], dtype=object))[0])
        _, Dcol, K = self.sparse_tables(0)
        base = (byte_matrix(np.array([[y]], dtype=object)) @ Dcol[:, :32])[0]
        for _ in range(64):
            raw = rng.bytes(32 * 8192)
            B = np.frombuffer(raw, np.uint8).reshape(8192, 32).astype(np.float64) - 128.0
            c4 = (base[None] + B @ self._ident[0]).astype(np.int64).reshape(8192, 8, 4)
            W = K[1][None] + c4[..., 0] + (c4[..., 1] << 8) + (c4[..., 2] << 16) + (c4[..., 3] << 24)
            lo, hi = W & M32, W >> 32
            c, hit = hi[:, 0], np.zeros(8192, bool)
            for q in range(1, 8):
                w = (lo[:, q] + c) >> 32
                hit |= w.astype(bool)
                c = hi[:, q] + w
            if hit.any():
                i = int(np.flatnonzero(hit)[0])
                x1 = int.from_bytes(raw[32 * i:32 * i + 32], "little")
                return [x0, x1] + [int.from_bytes(rng.bytes(32), "little") for _ in range(t - 2)]
        raise MfModelError("no word found that makes the carry of mf_reduce_words wrap")


@functools.lru_cache(maxsize=None)
def model(field, t):
    return MfModel(field, t)


@functools.lru_cache(maxsize=None)
def directed(field, t):
    """The directed states of (field, t): a list of t-word states (integers < 2^256) of odd length.  Names of the classes in the order
    of the issue: every byte 0x00 / 0x7F / 0x80 / 0xFF (the last is 2^256 - 1), alternating 0x7F / 0x80, the values around r and 2r,
    2^255 and 2^k +- 1 at the limb (29 i) and word (32 i) seams, one hot word among zeros and one zero word among 0xFF..FF at every
    index, the drivers of a few digit columns of output 0 (M, P, the row of the first sparse round), the carry of mf_reduce_words."""
    m = model(field, t)
    r = m.r
    rng = np.random.default_rng(29000 + 100 * t + (0 if field == "bn128" else 1))
    byte = lambda v: int.from_bytes(bytes([v]) * 32, "little")                     # noqa: E731
    alt = int.from_bytes(bytes([0x7F, 0x80]) * 16, "little"); tla = int.from_bytes(bytes([0x80, 0x7F]) * 16, "little")
    pats = [[byte(v)] * t for v in (0x00, 0x7F, 0x80, 0xFF)]
    pats += [[alt] * t, [tla] * t, [alt if j % 2 else tla for j in range(t)]]
    pats += [[v] * t for v in (r - 1, r, r + 1, 2 * r - 1, 2 * r)]
    seams = [1 << 255] + [(1 << k) + s for k in sorted({29 * i for i in range(1, 9)} | {32 * i for i in range(1, 8)}) for s in (-1, 1)]
    for at in range(0, len(seams), t):
        pats.append([seams[(at + j) % len(seams)] for j in range(t)])
    for j in range(t):
        pats.append([byte(0xFF) if k == j else 0 for k in range(t)])
        pats.append([0 if k == j else byte(0xFF) for k in range(t)])
    pats += m.column_drivers(m.dense_tables(0)[0][:, :32], (0, 15, 16, 31))
    pats += m.column_drivers(m.dense_tables(3)[0][:, :32], (0, 31))
    pats += m.column_drivers(m.sparse_tables(0)[0], (0, 31))
    pats.append(m.wrap_state(rng))
    if len(pats) % 2 == 0:
        pats.append([int.from_bytes(bytes(range(j, j + 32)), "little") for j in range(t)])
    assert len(pats) % 2 == 1 and all(0 <= v < 1 << 256 for p in pats for v in p)
    return pats


@functools.lru_cache(maxsize=None)
def states(field, t, n):
    """(n, t) integers < 2^256: the first half the directed states repeated with their odd period (so lanes l and l + 32, which trade
    halves through permlane32_swap, never hold the same one), the second half seeded random"""
    pats = directed(field, t)
    half = n // 2
    assert 1 < len(pats) <= half, "every directed state must appear"
    rng = np.random.default_rng(31000 + 100 * t + (0 if field == "bn128" else 1))
    X = np.empty((n, t), dtype=object)
    for i in range(n):
        for j in range(t):
            X[i, j] = pats[i % len(pats)][j] if i < half else int.from_bytes(rng.bytes(32), "little")
    for i in range(n - 32):
        assert i % 64 >= 32 or any(X[i, j] != X[i + 32, j] for j in range(t)), "lanes l and l + 32 hold the same state"
    return X


@functools.lru_cache(maxsize=None)
def permutation_inputs(field, t, n):
    """(n, t) internal-form words for the whole permutation: below 2r (the entry bound of poseidon_fr / poseidon_fr_reg), the edges
    0, 1, r - 2, r - 1, the internal forms of 0, 1 and -1, and r, r + 1, 2r - 1 rotating through the words; the second half random
    below r"""
    m = model(field, t)
    r, one = m.r, m.Rp
    edge = [0, 1, r - 1, r - 2, one, r - one, r, r + 1, 2 * r - 1, r + one, 2 * r - 2]
    rng = np.random.default_rng(33000 + 100 * t + (0 if field == "bn128" else 1))
    X = np.empty((n, t), dtype=object)
    half = n // 2
    for i in range(n):
        for j in range(t):
            if i < len(edge):
                X[i, j] = edge[i]                                                  # every word the same edge
            elif i < half:
                X[i, j] = edge[(i * 7 + j * (1 + i % 5)) % len(edge)]
            else:
                X[i, j] = int.from_bytes(rng.bytes(40), "little") % r
    return X
