"""Every primitive of the 29-bit-limb field layer (csrc/fe29_impl.hip.h) on chosen operands, for its four moduli -- Fq and Fr of BN254
and BLS12-381 -- through the probes of csrc/fe_probe.hip.  Operands and results are raw internal limbs, so the test chooses the exact
lazy representative.  The reference is tests/fe29_model.py: Python integers replaying the device's columns and carries, in which what
the header says cannot happen is an assertion; every device result must equal the model's limb for limb, and on top of that be
congruent to the mathematical value, below its documented bound and normalised.

Without a GPU (the unmarked tests): the constant tables against their definitions from q alone, the model on every generated operand,
and the operand classes of _reference() all non-empty (sizes printed: -s).  The limit on A * B is floor(R' / q), computed (169, 41291124,
169, 70); the figures in the header's comments (168 / 168 / 68) must not exceed it.  A few thousand elements per family, fe_inv on 521:
0.5 to 1 s per field on an MI355X."""
import ctypes as C
import functools
import math
import numpy as np
import pytest

from fe29_model import FE_WIDE_MAX, FIELDS, LB, LMASK, M32, Model, ModelError, _b, _flat, _sat, _stack, _val

gpu = pytest.mark.gpu
NAMES = list(FIELDS)
F_LIN, F_MUL, F_MUL2, F_ACC, F_WIDE, F_PRED, F_INV, F_STD = range(8)
N_INV_REPLAY = 24          # fe_inv elements whose ladder the model replays (the rest: pow)


def _forms(F, ub):
    """representatives at and under the value bound ub: normalised ub and ub - 1, saturated low limbs, low limbs of 2^29"""
    out = [F.split(ub), F.split(ub - 1)]
    for f in (_sat(F, ub), _flat(F, ub)):
        if f is not None:
            out.append(f)
    for l in out:
        assert _val(l) <= ub and max(l) <= 1 << LB, "a form exceeds its bound or the limb range fe_mul admits"
    return out


def _ab_pairs(F):
    """(A, B) with A B <= floor(R' / q), at the limit wherever the limit factors that way"""
    L, r = F.limit, math.isqrt(F.limit)
    out = {(1, L), (L, 1), (2, L // 2), (r, L // r), (L // r, r)}
    out |= {(a, L // a) for a in (3, 4, 6, 7, 8, 10, 11, 12, 14) if a <= L}
    return sorted(out)


@functools.lru_cache(maxsize=None)
def _operands(name):
    """the operands of every family: {family: tuple of (NR, n) batches (F_STD: the words first, (NL, n))}; deterministic"""
    F = FIELDS[name]
    q, NR, NL, Rp = F.q, F.NR, F.NL, F.Rp
    rng = np.random.default_rng(2900 + F.idx)
    rnd = lambda top: int.from_bytes(rng.bytes(64), "little") % top          # noqa: E731
    cap = F.limit * q * q
    one = Rp % q
    edge = [0, 1, 2, one, q - 2, q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1]
    for k in (3, 4, 6, 8, 10, 11):
        edge += [k * q - 1, k * q, k * q + 1]
    ops = {}

    # ---- fe_mul / fe_sqr: (a, b) with a b <= limit q^2 ----
    A, Bv = [], []
    def pair(a, b):
        assert _val(a) * _val(b) <= cap
        A.append(a); Bv.append(b)
    for x in edge:
        for y in edge:
            if x * y <= cap:
                pair(F.split(x), F.split(y))
    for a_, b_ in _ab_pairs(F):                                # at the computed limit and one step inside it, in every form
        for fa in _forms(F, a_ * q):
            for fb in _forms(F, b_ * q):
                pair(fa, fb)
    pair(F.split(1), F.split(q)); pair(F.split(1), F.split(2 * q))       # a0 b0 = q0: the first reduction step has m = 2^29 - 1
    for _ in range(16):
        pair(F.split(rnd(q) | 1), F.split(q))                            # q times anything in (0, R'): exactly q
        pair(F.split(q), F.split(rnd(11 * q) + 1))
        pair(F.split((rnd(q) >> LB) << LB), F.split(rnd(q)))                     # low limb 0: m = 0 in the first step
        pair(F.split(0), F.split(rnd(11 * q)))                           # exactly 0
    for _ in range(1200):
        ka, kb = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        if (ka + 1) * (kb + 1) <= F.limit:
            pair(F.split(rnd(q) + ka * q), F.split(rnd(q) + kb * q))
    if len(A) % 64 == 0:
        pair(F.split(3), F.split(5))
    ops[F_MUL] = (_stack(F, A), _stack(F, Bv))

    # ---- fe_mul2: a b + c d <= limit q^2 ----
    rows = []
    L = F.limit
    quads = {(10, 6, 4, 2), (10, 6, 10, 8), (8, 8, 8, 8)} if L >= 168 else {(4, 4, 4, 4), (5, 6, 5, 6)}
    h = L // 2; a_ = math.isqrt(h); b_ = h // a_
    quads.add((a_, b_, a_, (L - a_ * b_) // a_))                # the two products share the limit
    quads.add((1, L - 1, 1, 1)); quads.add((1, 1, L - 1, 1))
    for qa, qb, qc, qd in sorted(quads):
        assert qa * qb + qc * qd <= L
        fa, fb, fc, fd = (_forms(F, k * q) for k in (qa, qb, qc, qd))
        for i in range(4):
            rows.append((fa[i % len(fa)], fb[i % len(fb)], fc[i % len(fc)], fd[i % len(fd)]))      # all four in the same form
            for j in range(4):
                rows.append((fa[i % len(fa)], fb[j % len(fb)], fc[(i + j) % len(fc)], fd[(i * 3 + j) % len(fd)]))
    for x in edge[:9]:
        for y in edge[:9]:
            rows.append((F.split(x), F.split(y), F.split(edge[(x + y) % 9]), F.split(edge[(x * 7 + y) % 9])))
    rows.append((F.split(q), F.split(1), F.split(0), F.split(5)))               # exactly q
    rows.append((F.split(0), F.split(7), F.split(q - 1), F.split(0)))           # exactly 0
    for _ in range(700):
        rows.append(tuple(F.split(rnd(q) + int(rng.integers(0, 5)) * q) for _ in range(4)))
    rows = [r for r in rows if _val(r[0]) * _val(r[1]) + _val(r[2]) * _val(r[3]) <= cap]
    if len(rows) % 64 == 0:
        rows.pop()
    ops[F_MUL2] = tuple(_stack(F, [r[k] for r in rows]) for k in range(4))

    # ---- fe_mul_acc: a a coefficient (< q), b < 3q with limbs up to 2^30 - 1, c up to 8q (the hashes' running words stay below 8r) ----
    rows = []
    b_forms = [F.split(3 * q - 1), _flat(F, 3 * q - 1, (1 << 30) - 1), _flat(F, 3 * q - 1, 1 << LB), _sat(F, 3 * q - 1), F.split(0), F.split(q)]
    b_forms = [b for b in b_forms if b is not None]
    c_forms = [F.split(8 * q - 1), F.split(8 * q), _sat(F, 8 * q), F.split(0), F.split(q), F.split(2 * q - 1)]
    for a in (F.split(q - 1), _sat(F, q - 1) or F.split(q - 1), F.split(0), F.split(1), F.split(one)):
        for b in b_forms:
            for c in c_forms:
                rows.append((a, b, c))
    for _ in range(600):
        b = F.split(rnd(3 * q))
        if rng.integers(0, 2):                                    # y + constant as the hashes leave it: limb sums, not normalised
            c0 = F.split(rnd(q)); b = [x + y for x, y in zip(F.split(rnd(2 * q)), c0)]
        rows.append((F.split(rnd(q)), b, F.split(rnd(8 * q))))
    if len(rows) % 64 == 0:
        rows.pop()
    ops[F_ACC] = tuple(_stack(F, [r[k] for r in rows]) for k in range(3))

    # ---- fe_wide: FE_WIDE_MAX pairs, every prefix with sum A_i B_i <= limit ----
    if NR * (FE_WIDE_MAX + 1) <= 64:
        rows = []
        z = F.split(0)
        for a_, b_ in _ab_pairs(F):                               # n = 1 at the limit: the other pairs are zero
            for fa in _forms(F, a_ * q):
                for fb in _forms(F, b_ * q):
                    rows.append([fa, fb] + [z] * (2 * FE_WIDE_MAX - 2))
        per = L // FE_WIDE_MAX; a_ = max(1, math.isqrt(per)); b_ = per // a_
        last = L - (FE_WIDE_MAX - 1) * a_ * b_                    # n = FE_WIDE_MAX at the limit: the last pair is 1 x what is left
        assert last >= 1
        fa, fb, f1, fl = _forms(F, a_ * q), _forms(F, b_ * q), _forms(F, q), _forms(F, last * q)
        for i in range(len(fa)):
            for j in range(len(fb)):
                rows.append([fa[i], fb[j]] * (FE_WIDE_MAX - 1) + [f1[i % len(f1)], fl[j % len(fl)]])
        rows.append([F.split(q), F.split(1)] + [z] * (2 * FE_WIDE_MAX - 2))      # exactly q
        for _ in range(300):
            rows.append([F.split(rnd(q) + (int(rng.integers(0, 3)) if k % 2 else 0) * q) for k in range(2 * FE_WIDE_MAX)])
        if len(rows) % 64 == 0:
            rows.pop()
        ops[F_WIDE] = tuple(_stack(F, [r[k] for r in rows]) for k in range(2 * FE_WIDE_MAX))

    # ---- fe_add / fe_dbl / fe_sub<M>: b <= 2q so that all three M take every pair; plus pairs for one M alone (b up to M q) ----
    A, Bv = [], []
    top_w = 1 << (LB * (NR - 1))
    for M in (2, 4, 8):
        b_set = [F.split(0), F.split(M * q), F.split(M * q - 1), F.split(1), F.split(q), _sat(F, M * q), _flat(F, M * q),
                 [LMASK] * (NR - 1) + [F.split(M * q)[-1] - 1]]                   # every low limb above M q's: the borrow runs through all of them
        a_set = [F.split(0), F.split(1), F.split(q - 1), F.split(7 * q + 5), F.split(11 * q), _sat(F, 8 * q), _flat(F, 8 * q), F.split(top_w - 1), F.split(top_w)]
        for b in b_set:
            if b is None or min(b) < 0:
                continue
            assert _val(b) <= M * q
            for a in a_set:
                if a is not None:
                    A.append(a); Bv.append(b)
    for _ in range(800):
        A.append(F.split(rnd(q) + int(rng.integers(0, 10)) * q)); Bv.append(F.split(rnd(8 * q + 1)))
    if len(A) % 64 == 0:
        A.pop(); Bv.pop()
    ops[F_LIN] = (_stack(F, A), _stack(F, Bv))

    # ---- fe_is_zero_m / fe_canon: normalised values below 2q ----
    vals = [0, q - 1, q, q + 1, 2 * q - 1, 1, 2, q - 2, one]
    ql = F.split(q)
    for i in range(NR):                                           # q, and zero, with one limb altered -- for each limb
        for bit in (0, 7, 28 if i + 1 < NR else 0):
            t = list(ql); t[i] ^= 1 << bit
            if _val(t) < 2 * q:
                vals.append(_val(t))
            if 1 << (LB * i + bit) < 2 * q:
                vals.append(1 << (LB * i + bit))
    vals += [rnd(2 * q) for _ in range(500)]
    if len(vals) % 64 == 0:
        vals.pop()
    ops[F_PRED] = (F.limbs(vals),)

    # ---- fe_inv: the first N_INV_REPLAY are replayed by the model ----
    vals = [0, one, q - one, 1, q - 1, 2, 3, q, q + 1, q + one, 2 * q - 1, 2 * q - 2, one * 2 % q, (one * 2 % q) + q]
    vals += [F.to_mont(k) for k in range(2, 2 + N_INV_REPLAY - len(vals))]
    assert len(vals) == N_INV_REPLAY
    for _ in range(250):
        v = rnd(q); vals += [v, v + q]
    vals = vals[:521]
    ops[F_INV] = (F.limbs(vals),)

    # ---- fe_from_std / fe_to_std ----
    W = [0, 1, q - 1, F.R % q, F.R - 1, q, q + 1, 2 * q, F.R - q]
    for i in range(NL):
        W += [1 << (32 * i), 0xFFFFFFFF << (32 * i), 1 << (32 * i + 31), (F.R - 1) ^ (0xFFFFFFFF << (32 * i))]
    for p in sorted({LB * k for k in range(1, NR)} | {32 * j for j in range(1, NL)}):
        if p < 32 * NL:
            W += [3 << (p - 1), 1 << (p - 1), 1 << p, (F.R - 1) ^ (3 << (p - 1))]          # a set bit on each side of the straddle
    W += [rnd(q) for _ in range(300)] + [rnd(F.R) for _ in range(300)]
    a_vals = edge + [rnd(q) + int(rng.integers(0, 11)) * q for _ in range(len(W))]
    a_vals = a_vals[:len(W)]
    if len(W) % 64 == 0:
        W.pop(); a_vals.pop()
    words = np.empty((NL, len(W)), dtype=object)
    for k, v in enumerate(W):
        for i in range(NL):
            words[i, k] = (v >> (32 * i)) & M32
    ops[F_STD] = (words, F.limbs(a_vals))
    for fam, batches in ops.items():
        assert batches[0].shape[1] % 64 != 0, "one ragged final block"
    return ops


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the model on every operand: {family: list of result batches in the probe's row order}; raises ModelError where the header's
    claims fail.  Also the operand classes (per family: {class: boolean mask})."""
    F = FIELDS[name]
    m = Model(F)
    q, Rp = F.q, F.Rp
    ops = _operands(name)
    ref, cls = {}, {}
    val = F.val

    def product_checks(r, total, what, fam_cls):
        v = val(r)
        assert _b((v * Rp - total) % q == 0).all(), f"{what}: not congruent"
        assert _b(v < 2 * q).all(), f"{what}: a result reaches 2q although A B <= floor(R'/q)"
        fam_cls.update({f"{what}_in_[0,q)": _b(v < q), f"{what}_in_[q,2q)": _b(v >= q), f"{what}_exactly_0": _b(v == 0), f"{what}_exactly_q": _b(v == q),
                        f"{what}_m_is_0": m.m_zero.copy(), f"{what}_m_is_2^29-1": m.m_max.copy()})

    a, b = ops[F_MUL]
    cls[F_MUL] = c = {}
    r = m.mul(a, b); product_checks(r, val(a) * val(b), "mul", c)
    sq_ok = _b(val(a) ** 2 <= F.limit * q * q)
    s = m.sqr(a); maa = m.mul(a, a)
    assert _b(s == maa).all(), "fe_sqr and fe_mul(a, a) differ"
    assert _b(val(s)[sq_ok] < 2 * q).all()
    ref[F_MUL] = [r, s, maa]
    c["sqr_within_bound"] = sq_ok
    c["low_limbs_all_2^29-1"] = _b((a[:-1] == LMASK).all(axis=0)) & _b((b[:-1] == LMASK).all(axis=0))
    c["low_limbs_all_2^29"] = _b((a[:-1] == 1 << LB).all(axis=0)) & _b((b[:-1] == 1 << LB).all(axis=0))
    c["AB_at_the_limit"] = _b(val(a) * val(b) == F.limit * q * q)
    c["AB_one_step_inside"] = _b(val(a) * val(b) < F.limit * q * q) & _b((val(a) + 1) * (val(b) + 1) >= F.limit * q * q)
    for nm, k in (("0", 0), ("1", 1), ("R'_mod_q", Rp % q), ("q-1", q - 1), ("q", q), ("q+1", q + 1), ("2q-1", 2 * q - 1), ("11q-1", 11 * q - 1), ("11q+1", 11 * q + 1)):
        c[f"operand_{nm}"] = _b(val(a) == k) | _b(val(b) == k)

    a, b, cc, d = ops[F_MUL2]
    cls[F_MUL2] = c = {}
    r = m.mul2(a, b, cc, d); product_checks(r, val(a) * val(b) + val(cc) * val(d), "mul2", c)
    c["sum_at_the_limit"] = _b(val(a) * val(b) + val(cc) * val(d) == F.limit * q * q)
    c["low_limbs_all_2^29-1"] = _b(np.all([(x[:-1] == LMASK).all(axis=0) for x in (a, b, cc, d)], axis=0))
    c["low_limbs_all_2^29"] = _b(np.all([(x[:-1] == 1 << LB).all(axis=0) for x in (a, b, cc, d)], axis=0))
    ref[F_MUL2] = [r]

    a, b, cc = ops[F_ACC]
    cls[F_ACC] = c = {}
    r = m.mul_acc(a, b, cc)
    v = val(r)
    assert _b((v * Rp - (val(cc) * Rp + val(a) * val(b))) % q == 0).all(), "fe_mul_acc: not congruent"
    assert _b(v * Rp < val(cc) * Rp + val(a) * val(b) + q * Rp).all(), "fe_mul_acc: the result reaches c + a b / R' + q"
    c["b_limbs_at_2^30-1"] = _b((b[:-1] == (1 << 30) - 1).all(axis=0))
    c["b_limbs_above_2^29"] = _b((b[:-1] > 1 << LB).any(axis=0))
    c["c_at_8q"] = _b(val(cc) == 8 * q)
    c["c_just_under_8q"] = _b(val(cc) == 8 * q - 1)
    ref[F_ACC] = [r]

    if F_WIDE in ops:
        prs = ops[F_WIDE]
        cls[F_WIDE] = c = {}
        ref[F_WIDE] = []
        tot = 0
        for n in range(1, FE_WIDE_MAX + 1):
            pairs = [(prs[2 * k], prs[2 * k + 1]) for k in range(n)]
            tot = tot + val(pairs[-1][0]) * val(pairs[-1][1])
            r = m.wide(pairs)
            assert _b(tot <= F.limit * q * q).all() and _b((val(r) * Rp - tot) % q == 0).all() and _b(val(r) < 2 * q).all(), f"fe_wide, {n} pairs"
            ref[F_WIDE].append(r)
            if n in (1, FE_WIDE_MAX):
                c[f"n={n}_sum_at_the_limit"] = _b(tot == F.limit * q * q)
                c[f"n={n}_low_limbs_all_2^29-1"] = _b(np.all([(x[:-1] == LMASK).all(axis=0) for pr in pairs for x in pr], axis=0))
            if n == 1:
                c["n=1_exactly_q"] = _b(val(r) == q)

    a, b = ops[F_LIN]
    cls[F_LIN] = c = {}
    ref[F_LIN] = [m.add(a, b), m.dbl(a)]
    vb = val(b)
    for M in (2, 4, 8):
        ok = _b(vb <= M * q)                                     # fe_sub<M> is defined for these; the other rows of the probe are not compared
        r = np.empty_like(a)
        r[:] = -1
        r[:, ok] = m.sub(M, a[:, ok], b[:, ok])
        neg = np.zeros(a.shape[1], int); neg[ok] = m.neg_limbs
        ref[F_LIN].append(r)
        c.update({f"sub{M}_defined": ok, f"sub{M}_b=0": ok & _b(vb == 0), f"sub{M}_b=Mq": _b(vb == M * q), f"sub{M}_b=Mq-1": _b(vb == M * q - 1),
                  f"sub{M}_borrow_through_every_limb": neg == F.NR - 1, f"sub{M}_a_negative_limb": neg > 0, f"sub{M}_no_negative_limb": ok & (neg == 0),
                  f"sub{M}_a_top_limb_excess": ok & _b(a[-1] > m.Q[-1]), f"sub{M}_b_top_limb_excess": ok & _b(b[-1] > m.Q[-1]),
                  f"sub{M}_limbs_of_2^29": ok & (_b((a[:-1] == 1 << LB).all(axis=0)) | _b((b[:-1] == 1 << LB).all(axis=0)))})

    (a,) = ops[F_PRED]
    cls[F_PRED] = c = {}
    z, cn = m.is_zero_m(a), m.canon(a)
    v = val(a)
    assert _b(z == _b(v % q == 0)).all(), "fe_is_zero_m misses a representative of zero"
    assert _b(val(cn) == v % q).all() and F.normalised(cn), "fe_canon"
    ref[F_PRED] = [z, cn]
    ql = np.array(m.Q, dtype=object)[:, None]
    c.update({f"value_{n_}": _b(v == k) for n_, k in (("0", 0), ("1", 1), ("q-1", q - 1), ("q", q), ("q+1", q + 1), ("2q-1", 2 * q - 1))})
    diff = _b(a != ql)
    for i in range(F.NR):
        c[f"q_but_for_limb_{i}"] = diff[i] & (diff.sum(axis=0) == 1)
    c["canon_subtracts"] = _b(v >= q); c["canon_keeps"] = _b(v < q)

    (a,) = ops[F_INV]
    cls[F_INV] = c = {}
    head = m.inv(a[:, :N_INV_REPLAY])
    v = val(a)
    want = np.array([pow(int(x) * pow(Rp, -1, q) % q, q - 2, q) * Rp % q for x in v], dtype=object)       # (x R')^-1 R'^2 = x^-1 R'
    assert _b(val(head) % q == want[:N_INV_REPLAY]).all() and _b(val(head) < 2 * q).all(), "the model's fe_inv"
    ref[F_INV] = [head, want]
    c.update({"zero": _b(v == 0), "q_for_zero": _b(v == q), "one": _b(v == Rp % q), "minus_one": _b(v == q - Rp % q), "lazy_a+q": _b(v >= q)})

    w, a = ops[F_STD]
    cls[F_STD] = c = {}
    Wv = sum(w[i] << (32 * i) for i in range(F.NL))
    assert _b(Wv * (q - 1) <= F.limit * q * q).all(), "fe_from_std: external words the product's bound does not admit"
    x = m.from_std(w)
    assert _b(val(x) % q == Wv * Rp * pow(F.R, -1, q) % q).all() and _b(val(x) < 2 * q).all(), "fe_from_std"
    ts = m.to_std(a)
    assert _b(sum(ts[i] << (32 * i) for i in range(F.NL)) == val(a) * F.R * pow(Rp, -1, q) % q).all(), "fe_to_std"
    rt = m.to_std(x)
    assert _b(sum(rt[i] << (32 * i) for i in range(F.NL)) == Wv % q).all(), "fe_to_std(fe_from_std(w)) is not w mod q"
    ref[F_STD] = [x, ts, rt]
    c.update({"words_0": _b(Wv == 0), "words_1": _b(Wv == 1), "words_q-1": _b(Wv == q - 1), "words_R_mod_q": _b(Wv == F.R % q), "words_all_ones": _b(Wv == F.R - 1),
              "words_not_canonical": _b(Wv >= q)})
    for i in range(F.NL):
        c[f"only_word_{i}"] = _b(w[i] != 0) & _b(Wv == (w[i] << (32 * i)))
    for p in sorted({LB * k for k in range(1, F.NR)} | {32 * j for j in range(1, F.NL)}):
        if p < 32 * F.NL:
            c[f"straddle_bit_{p}"] = _b((Wv >> (p - 1)) & 3 == 3)
    return ref, cls


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------
def _consts(zk, F):
    fn = zk.lib().zk_fe29_consts_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_void_p]
    out = np.zeros(3 + 9 * 14, np.uint32)
    assert fn(F.idx, out.ctypes.data_as(C.c_void_p)) == 0
    nl, nr, qinv = (int(x) for x in out[:3])
    tabs = {k: [int(x) for x in out[3 + i * nr:3 + (i + 1) * nr]] for i, k in enumerate(("Q29", "ONE29", "CIN29", "COUT29", "RRP29", "Q2_29", "Q4_29", "Q8_29", "QM2"))}
    return nl, nr, qinv, tabs


@pytest.mark.parametrize("name", NAMES)
def test_constant_tables_match_their_definitions(zk, name):
    """No GPU: every table of the field as the library was compiled with it, against its definition from q alone"""
    F = FIELDS[name]
    nl, nr, qinv, t = _consts(zk, F)
    q, R, Rp = F.q, F.R, F.Rp
    assert (nl, nr) == (F.NL, F.NR) and 32 * nl >= q.bit_length() and LB * nr >= 32 * nl
    assert qinv == (-pow(q, -1, 1 << LB)) % (1 << LB)
    want = {"Q29": q, "ONE29": Rp % q, "CIN29": Rp * Rp * pow(R, -1, q) % q, "COUT29": R % q, "RRP29": Rp * Rp % q, "Q2_29": 2 * q, "Q4_29": 4 * q, "Q8_29": 8 * q,
            "QM2": q - 2}
    for k, v in want.items():
        assert t[k] == F.split(v), f"{name}: {k} is not the normalised limbs of its definition"
    assert Model(F).qm2_limbs() == t["QM2"]
    # the figures the comments of fe29_impl.hip.h and frhash_impl.hip.h give for A * B must not exceed what the modulus allows
    print(f"{name}: floor(R'/q) = {F.limit}, documented {F.doc_limit}")
    assert F.doc_limit <= F.limit


@pytest.mark.parametrize("name", NAMES)
def test_operands_reach_every_class_and_the_model_holds(name):
    """No GPU: the model's assertions hold on every generated operand (no 64-bit column reaches 2^64, no limb wraps, fe_norm_s sees every
    limb as it is, nothing goes negative, every result is the mathematical one, under its bound and normalised), and every class the
    code distinguishes is non-empty"""
    ref, cls = _reference(name)
    fam_names = {F_LIN: "lin", F_MUL: "mul", F_MUL2: "mul2", F_ACC: "mul_acc", F_WIDE: "wide", F_PRED: "pred", F_INV: "inv", F_STD: "std"}
    assert (F_WIDE in cls) == (FIELDS[name].NR == 9)
    for fam, c in cls.items():
        sizes = {k: int(np.sum(v)) for k, v in c.items()}
        print(f"{name} {fam_names[fam]}: " + ", ".join(f"{k}={v}" for k, v in sizes.items()))
        for k, v in sizes.items():
            assert v > 0, f"{name} {fam_names[fam]}: no operand of class {k}"


def test_fe_wide_columns_overflow_with_fourteen_limbs():
    """No GPU.  Why csrc/fe_probe.hip has no fe_wide rows for BLS12-381 Fq and fe_wide_mac refuses to compile there: six pairs of
    canonical-size operands with saturated low limbs push a column past 2^64 when NR = 14; with NR = 9 the same shape fits."""
    F = FIELDS["bls12_381_fq"]
    x = _sat(F, F.q - 1)
    assert x is not None and _val(x) < F.q
    a = _stack(F, [x])
    with pytest.raises(ModelError, match="64-bit column"):
        Model(F).wide([(a, a)] * FE_WIDE_MAX)
    assert (FE_WIDE_MAX + 1) * F.NR > 64
    Model(F).mul2(a, a, a, a)                                     # two pairs do fit
    for name in ("bn254_fq", "bn254_fr", "bls12_381_fr"):
        G = FIELDS[name]
        y = _sat(G, 4 * G.q)
        b = _stack(G, [y])
        assert (FE_WIDE_MAX + 1) * G.NR <= 64
        Model(G).wide([(b, b)] * FE_WIDE_MAX)                    # 6 x 16 = 96 <= floor(R'/q) only for BN254, but the columns hold either way


def test_the_model_rejects_what_the_header_excludes():
    """No GPU: the model is not vacuous -- it objects to a subtrahend above M q + a, to a limb fe_norm_s cannot see, and to limbs that
    overflow a column"""
    F = FIELDS["bn254_fq"]
    m = Model(F)
    with pytest.raises(ModelError, match="negative"):
        m.sub(2, F.limbs([0]), F.limbs([2 * F.q + 1]))
    with pytest.raises(ModelError, match="does not fit the int"):
        m.sub(2, _stack(F, [[1 << 31] + [0] * (F.NR - 1)]), F.limbs([0]))
    full = _stack(F, [[M32] * F.NR])
    with pytest.raises(ModelError, match="64-bit column"):
        m.mul(full, full)


# ---- on the device -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)
    return zk


def _u32(l):
    return np.ascontiguousarray(l.T.astype(np.uint32))


def _run(dev, F, fam, batches, out_words):
    fn = dev.lib().zk_fe29_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    inp = np.ascontiguousarray(np.concatenate([_u32(b) for b in batches], axis=1))
    n = inp.shape[0]
    out = np.zeros((n, out_words), np.uint32)
    assert fn(F.idx, fam, inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), n) == 0, dev.lib().zk_last_error()
    return out


def _rows(out, widths):
    res, o = [], 0
    for w in widths:
        res.append(out[:, o:o + w].T.astype(object)); o += w
    return res


def _same(got, want, what, mask=None):
    bad = _b(got != want).any(axis=0)
    if mask is not None:
        bad &= mask
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ from the model, first at index {int(np.flatnonzero(bad)[0])}: got {[hex(int(x)) for x in got[:, np.flatnonzero(bad)[0]]]}"


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_field_primitives_match_the_model(dev, name):
    """Every row of every family: limb for limb what the model computes; then, stated on their own, the properties the header documents:
    congruent to the mathematical value, below the bound, limbs normalised; fe_sqr = fe_mul(a, a) limb for limb; fe_is_zero_m and
    fe_canon exact; fe_to_std(fe_from_std(w)) = w mod q."""
    F = FIELDS[name]
    NR, NL, q, Rp = F.NR, F.NL, F.q, F.Rp
    ops = _operands(name)
    ref, cls = _reference(name)
    val = F.val

    a, b = ops[F_MUL]
    mul, sqr, maa = _rows(_run(dev, F, F_MUL, ops[F_MUL], 3 * NR), [NR] * 3)
    _same(sqr, maa, "fe_sqr against fe_mul(a, a)")
    _same(mul, ref[F_MUL][0], "fe_mul"); _same(sqr, ref[F_MUL][1], "fe_sqr")
    assert _b((val(mul) * Rp - val(a) * val(b)) % q == 0).all() and _b(val(mul) < 2 * q).all() and F.normalised(mul)
    assert _b((val(sqr) * Rp - val(a) ** 2) % q == 0).all() and _b(val(sqr)[cls[F_MUL]["sqr_within_bound"]] < 2 * q).all() and F.normalised(sqr)

    a, b, c, d = ops[F_MUL2]
    (r,) = _rows(_run(dev, F, F_MUL2, ops[F_MUL2], NR), [NR])
    _same(r, ref[F_MUL2][0], "fe_mul2")
    assert _b((val(r) * Rp - val(a) * val(b) - val(c) * val(d)) % q == 0).all() and _b(val(r) < 2 * q).all() and F.normalised(r)

    a, b, c = ops[F_ACC]
    (r,) = _rows(_run(dev, F, F_ACC, ops[F_ACC], NR), [NR])
    _same(r, ref[F_ACC][0], "fe_mul_acc")
    assert _b((val(r) * Rp - val(c) * Rp - val(a) * val(b)) % q == 0).all() and _b(val(r) * Rp < val(c) * Rp + val(a) * val(b) + q * Rp).all() and F.normalised(r)

    if F_WIDE in ops:
        rows = _rows(_run(dev, F, F_WIDE, ops[F_WIDE], FE_WIDE_MAX * NR), [NR] * FE_WIDE_MAX)
        tot = 0
        for n in range(FE_WIDE_MAX):
            tot = tot + val(ops[F_WIDE][2 * n]) * val(ops[F_WIDE][2 * n + 1])
            _same(rows[n], ref[F_WIDE][n], f"fe_wide, {n + 1} pairs")
            assert _b((val(rows[n]) * Rp - tot) % q == 0).all() and _b(val(rows[n]) < 2 * q).all() and F.normalised(rows[n])

    a, b = ops[F_LIN]
    rows = _rows(_run(dev, F, F_LIN, ops[F_LIN], 5 * NR), [NR] * 5)
    _same(rows[0], ref[F_LIN][0], "fe_add"); _same(rows[1], ref[F_LIN][1], "fe_dbl")
    assert _b(val(rows[0]) == val(a) + val(b)).all() and _b(val(rows[1]) == 2 * val(a)).all() and F.normalised(rows[0]) and F.normalised(rows[1])
    for k, M in enumerate((2, 4, 8)):
        ok = cls[F_LIN][f"sub{M}_defined"]
        _same(rows[2 + k], ref[F_LIN][2 + k], f"fe_sub<{M}>", ok)
        assert _b(val(rows[2 + k])[ok] == (val(a) + M * q - val(b))[ok]).all() and F.normalised(rows[2 + k][:, ok])

    (a,) = ops[F_PRED]
    z, cn = _rows(_run(dev, F, F_PRED, ops[F_PRED], NR + 1), [1, NR])
    assert _b(z[0] == ref[F_PRED][0].astype(int)).all(), "fe_is_zero_m"
    _same(cn, ref[F_PRED][1], "fe_canon")
    assert _b(val(cn) == val(a) % q).all()

    (a,) = ops[F_INV]
    (r,) = _rows(_run(dev, F, F_INV, ops[F_INV], NR), [NR])
    _same(r[:, :N_INV_REPLAY], ref[F_INV][0], "fe_inv (the replayed ladder)")
    assert _b(val(r) % q == ref[F_INV][1]).all() and _b(val(r) < 2 * q).all() and F.normalised(r), "fe_inv"
    assert int(val(r)[0]) == 0                                   # a = 0 -> exactly 0

    w, a = ops[F_STD]
    x, ts, rt = _rows(_run(dev, F, F_STD, ops[F_STD], NR + 2 * NL), [NR, NL, NL])
    _same(x, ref[F_STD][0], "fe_from_std"); _same(ts, ref[F_STD][1], "fe_to_std"); _same(rt, ref[F_STD][2], "fe_to_std(fe_from_std(w))")
    Wv = sum(w[i] << (32 * i) for i in range(NL))
    assert _b(sum(rt[i] << (32 * i) for i in range(NL)) == Wv % q).all()
    assert _b(val(x) < 2 * q).all() and F.normalised(x)


@gpu
def test_fe_wide_is_refused_for_fourteen_limbs(dev):
    """the probe has no fe_wide row for BLS12-381 Fq and says so instead of running one"""
    F = FIELDS["bls12_381_fq"]
    fn = dev.lib().zk_fe29_probe
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    inp = np.zeros((1, 2 * FE_WIDE_MAX * F.NR), np.uint32); out = np.zeros((1, FE_WIDE_MAX * F.NR), np.uint32)
    assert fn(F.idx, F_WIDE, inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 1) != 0
    assert b"fe_wide" in dev.lib().zk_last_error()
