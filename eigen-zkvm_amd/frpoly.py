"""Polynomial arithmetic over the scalar fields of BN254 and BLS12-381 on the device (include/zkgpu.h, "Polynomial arithmetic over the
scalar field"): running products and sums, batch inversion, pointwise work, powers, the terms of a grand product, the grand product
itself, products of polynomials and quotients by X^N - 1.  One function per entry point zk_fr_<curve>_<name>_dev.  No protocol: what a
PLONK-family prover is made of, not the prover.  Everything runs on the device; there is no CPU fallback.

A vector is a sequence of Python integers below r, or a DevArray that already holds n x 4 u64 Montgomery words (the layout of
zk_fr_<curve>_ntt_dev; kzg.to_mont / kzg.from_mont convert).  Integers in give integers out; a DevArray in gives a DevArray out -- a new
one, or `out` when it is given (`out` may be the input wherever the header allows in place).  Scalars and the totals are Python integers.
Every result is the canonical representative.  Failures raise ZkError with the library's text."""
import ctypes as C

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from .groth16 import _FR, _NAME
from .kzg import _scalar, from_mont, to_mont

MUL, ADD, SUB = 0, 1, 2         # ZK_FR_MUL, ZK_FR_ADD, ZK_FR_SUB
MAX_RATIO = 4096                # ZK_FRPOLY_MAX_RATIO
_OPS = {"mul": MUL, "add": ADD, "sub": SUB, MUL: MUL, ADD: ADD, SUB: SUB}
NO_ZERO = (1 << 64) - 1


def _fn(curve, name):
    if curve not in _FR:
        raise ZkError('frpoly: unknown curve "%s" (BN128 | BLS12381)' % curve)
    return getattr(lib(), "zk_fr_%s_%s_dev" % (_NAME[curve], name))


def tile_elems():
    return int(lib().zk_frpoly_tile_elems())


def span():
    return int(lib().zk_frpoly_span())


class _Vec:
    """one input vector on the device, and whether this call owns it"""

    def __init__(self, v, curve):
        self.on_dev = isinstance(v, DevArray)
        if self.on_dev:
            self.d, self.n = v, v.n // 4
        else:
            a = to_mont(v, curve).reshape(-1)
            self.d, self.n = (DevArray.from_host(a) if a.size else DevArray(4)), a.size // 4

    def free(self):
        if not self.on_dev:
            self.d.free()


def _result(d, n, curve, keep):
    """a DevArray of n elements -> itself (keep) or its integers, freed"""
    if keep:
        return d
    try:
        return from_mont(d.to_host()[:4 * n], curve) if n else []
    finally:
        d.free()


def _target(out, n, what="out"):
    if out is None:
        return DevArray(4 * max(n, 1))
    if not isinstance(out, DevArray) or out.n < 4 * n:
        raise ZkError("frpoly: %s must be a DevArray of at least %d elements" % (what, n))
    return out


def _int4(words):
    return int.from_bytes(np.ascontiguousarray(words, dtype="<u8").tobytes(), "little")


def prefix_product(v, curve="BN128", inclusive=False, out=None, total_only=False):
    """-> (products, total): products[i] = prod_{j < i} v[j] (inclusive: j <= i), total = prod v.  total_only: (None, total), nothing is
    written.  n = 0 gives ([], 1)."""
    return _prefix("prefix_product", v, curve, inclusive, out, total_only)


def prefix_sum(v, curve="BN128", inclusive=False, out=None, total_only=False):
    """-> (sums, total): sums[i] = sum_{j < i} v[j] (inclusive: j <= i), total = sum v: prefix_product's tiles and rules under addition.
    n = 0 gives ([], 0)."""
    return _prefix("prefix_sum", v, curve, inclusive, out, total_only)


def _prefix(name, v, curve, inclusive, out, total_only):
    fn = _fn(curve, name)
    x = _Vec(v, curve)
    tot = np.zeros(4, np.uint64)
    d_out = None
    try:
        if not total_only:
            d_out = _target(out, x.n)
        _check(fn(x.d.ptr if x.n else None, x.n, int(bool(inclusive)), d_out.ptr if d_out is not None and x.n else None, _ptr(tot), 0))
        total = _int4(tot)
        if total_only:
            return None, total
        return _result(d_out, x.n, curve, x.on_dev or out is not None), total
    except Exception:
        if d_out is not None and out is None:
            d_out.free()
        raise
    finally:
        x.free()


def batch_inverse(v, curve="BN128", out=None):
    """-> (inverses, n_zero, first_zero): a zero stays zero; first_zero is None when there is none"""
    fn = _fn(curve, "batch_inverse")
    x = _Vec(v, curve)
    nz, fz = C.c_uint64(0), C.c_uint64(0)
    d_out = _target(out, x.n)
    try:
        _check(fn(x.d.ptr, x.n, d_out.ptr, C.byref(nz), C.byref(fz), 0))
        first = None if fz.value == NO_ZERO else int(fz.value)
        return _result(d_out, x.n, curve, x.on_dev or out is not None), int(nz.value), first
    except Exception:
        if out is None:
            d_out.free()
        raise
    finally:
        x.free()


def pointwise(op, a, b, curve="BN128", out=None):
    """a[i] op b[i] for op in "mul" | "add" | "sub" (or MUL | ADD | SUB); equal lengths"""
    fn = _fn(curve, "pointwise")
    code = _OPS.get(op, op)
    x, y = _Vec(a, curve), _Vec(b, curve)
    try:
        if x.n != y.n:
            raise ZkError("frpoly: pointwise operands of %d and %d elements" % (x.n, y.n))
        d_out = _target(out, x.n)
        try:
            _check(fn(int(code), x.d.ptr, y.d.ptr, d_out.ptr, x.n, 0))
            return _result(d_out, x.n, curve, x.on_dev or y.on_dev or out is not None)
        except Exception:
            if out is None:
                d_out.free()
            raise
    finally:
        x.free(); y.free()


def powers(base, scale, n, curve="BN128", dev=False):
    """scale base^i for i < n: integers, or with dev a DevArray of Montgomery words"""
    fn = _fn(curve, "powers")
    b, s = _scalar(base, curve, "base"), _scalar(scale, curve, "scale")
    d_out = DevArray(4 * max(int(n), 1))
    try:
        _check(fn(_ptr(b), _ptr(s), int(n), d_out.ptr, 0))
        return _result(d_out, int(n), curve, dev)
    except Exception:
        d_out.free()
        raise


def terms(cols, labels, beta, gamma, curve="BN128", dev=False):
    """prod_c (cols[c][i] + beta labels[c][i] + gamma) over 1 .. 16 columns of equal length; labels None: the plain multiset form"""
    fn = _fn(curve, "terms")
    bw, gw = _scalar(beta, curve, "beta"), _scalar(gamma, curve, "gamma")
    cs = [_Vec(c, curve) for c in cols]
    ls = [_Vec(c, curve) for c in labels] if labels is not None else []
    try:
        n = cs[0].n if cs else 0
        if any(v.n != n for v in cs + ls) or (labels is not None and len(ls) != len(cs)):
            raise ZkError("frpoly: terms takes columns and labels of one length")
        cp = np.array([v.d.ptr or 0 for v in cs], dtype=np.uint64)
        lp = np.array([v.d.ptr or 0 for v in ls], dtype=np.uint64)
        d_out = DevArray(4 * max(n, 1))
        try:
            _check(fn(_ptr(cp) if cs else None, _ptr(lp) if labels is not None else None, len(cs), n, _ptr(bw), _ptr(gw), d_out.ptr, 0))
            return _result(d_out, n, curve, dev or any(v.on_dev for v in cs))
        except Exception:
            d_out.free()
            raise
    finally:
        for v in cs + ls:
            v.free()


def grand_product(num, den, curve="BN128", out=None):
    """-> (z, last): z_0 = 1, z_(i+1) = z_i num_i / den_i; z holds z_0 .. z_(n-1), last = z_n.  The products agree exactly when last == 1.
    A zero denominator is refused, its first row named."""
    fn = _fn(curve, "grand_product")
    x, y = _Vec(num, curve), _Vec(den, curve)
    last = np.zeros(4, np.uint64)
    try:
        if x.n != y.n:
            raise ZkError("frpoly: grand product over %d numerators and %d denominators" % (x.n, y.n))
        d_z = _target(out, x.n, "z")
        try:
            _check(fn(x.d.ptr, y.d.ptr, x.n, d_z.ptr, _ptr(last), 0))
            return _result(d_z, x.n, curve, x.on_dev or y.on_dev or out is not None), _int4(last)
        except Exception:
            if out is None:
                d_z.free()
            raise
    finally:
        x.free(); y.free()


def poly_mul(a, b, curve="BN128", dev=False):
    """the len(a) + len(b) - 1 coefficients of a b, leading zeros kept"""
    fn = _fn(curve, "poly_mul")
    x, y = _Vec(a, curve), _Vec(b, curve)
    try:
        n = max(x.n + y.n - 1, 0)
        d_out = DevArray(4 * max(n, 1))
        try:
            _check(fn(x.d.ptr, x.n, y.d.ptr, y.n, d_out.ptr, 0))
            return _result(d_out, n, curve, dev or x.on_dev or y.on_dev)
        except Exception:
            d_out.free()
            raise
    finally:
        x.free(); y.free()


def divmod_zh(p, log_n, curve="BN128", want_q=True, want_rem=True, dev=False):
    """p = q (X^N - 1) + rem, N = 2^log_n -> (q, rem, rem_nonzero): q has max(len(p) - N, 0) coefficients, rem has N; either is None when
    not asked for.  rem_nonzero = 0 exactly when X^N - 1 divides p."""
    fn = _fn(curve, "divmod_zh")
    x = _Vec(p, curve)
    N = 1 << int(log_n)
    nq = max(x.n - N, 0)
    keep = dev or x.on_dev
    cnt = C.c_uint64(0)
    d_q = d_r = None
    try:
        if x.n and -(-x.n // N) > MAX_RATIO:      # refused by the library too, before the remainder's N elements are asked for here
            _check(fn(x.d.ptr, x.n, int(log_n), None, None, C.byref(cnt), 0))
        d_q = DevArray(4 * max(nq, 1)) if want_q else None
        d_r = DevArray(4 * N) if want_rem else None
        _check(fn(x.d.ptr if x.n else None, x.n, int(log_n), d_q.ptr if d_q else None, d_r.ptr if d_r else None, C.byref(cnt), 0))
        q = _result(d_q, nq, curve, keep) if d_q else None
        d_q = None
        r = _result(d_r, N, curve, keep) if d_r else None
        d_r = None
        return q, r, int(cnt.value)
    finally:
        x.free()
        for d in (d_q, d_r):
            if d is not None:
                d.free()


def divide_zh_coset(evals, log_m, log_n, curve="BN128"):
    """evals[i] / (7^N w_m^(iN) - 1) for the 2^log_m values on the coset 7 H_m in the order the coset transform leaves them; a DevArray is
    divided in place and returned"""
    fn = _fn(curve, "divide_zh_coset")
    x = _Vec(evals, curve)
    try:
        if x.n != 1 << int(log_m):
            raise ZkError("frpoly: divide_zh_coset over %d values, the domain has 2^%d" % (x.n, int(log_m)))
        _check(fn(x.d.ptr, int(log_m), int(log_n), 0))
        return x.d if x.on_dev else from_mont(x.d.to_host()[:4 * x.n], curve)
    finally:
        x.free()
