"""KZG commitments over a powers-of-tau file (include/zkgpu.h, "KZG commitments"): commit to a polynomial under a
ceremony's tauG1 section, open it at a point, check many openings in one randomised pairing equation.  What snarkjs's universal-setup
provers (`ffs` / `fff` / `ffv`, test/snark_verifier.sh:67-106) are made of; no per-circuit ceremony.  Commitments are in G1 and are NOT
hiding.  Everything runs on the device; there is no CPU fallback.

A polynomial is a sequence of Python integers below r (coefficients, lowest degree first), or a DevArray that already holds them in the
layout of zk_fr_<curve>_ntt_dev (4 x u64 Montgomery per coefficient).  A point z, a value y and gamma are Python integers.  A commitment or
witness is `point_bytes` bytes in the layout of the multi-scalar sums (affine, little-endian Montgomery); all zero is the point at infinity."""
import ctypes as C
import hashlib

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from .groth16 import _FQ_WORDS, _FR, _NAME, _seed, fq_convert

M64 = (1 << 64) - 1


def _words(values):
    """integers below 2^256 -> n x 4 u64, little-endian"""
    vals = [int(v) for v in values]
    for v in vals:
        if not 0 <= v < (1 << 256):
            raise ZkError("kzg: a value does not fit 32 bytes")
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def _ints(words):
    b = np.ascontiguousarray(words, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def to_mont(values, curve):
    """canonical integers below r -> n x 4 u64 Montgomery words (R = 2^256), the layout the transforms and this module's kernels take"""
    r = _FR[curve]
    vals = [int(v) for v in values]
    for v in vals:
        if not 0 <= v < r:
            raise ZkError("kzg: a coefficient is not below the scalar field's modulus")
    return _words([(v << 256) % r for v in vals])


def from_mont(words, curve):
    r = _FR[curve]
    rinv = pow(1 << 256, -1, r)
    return [v * rinv % r for v in _ints(words)]


def _dev_poly(p, curve):
    """-> (DevArray of Montgomery words, number of coefficients, owned)"""
    if isinstance(p, DevArray):
        return p, p.n // 4, False
    a = to_mont(p, curve).reshape(-1)
    return DevArray.from_host(a), a.size // 4, True


def _scalar(v, curve, what):
    v = int(v)
    if not 0 <= v < _FR[curve]:
        raise ZkError("kzg: %s is not below the scalar field's modulus" % what)
    return _words([v]).reshape(-1)


def divide(coeffs, z, curve="BN128"):
    """(p - p(z)) / (X - z) and p(z) on the device (zk_kzg_<curve>_divide_dev): -> (q, y), q the n - 1 quotient coefficients as integers.
    Needs no file."""
    if curve not in _FR:
        raise ZkError('kzg: unknown curve "%s" (BN128 | BLS12381)' % curve)
    d, n, owned = _dev_poly(coeffs, curve)
    zw = _scalar(z, curve, "z")
    d_q = DevArray(4 * max(n - 1, 1)); d_y = DevArray(4)
    try:
        _check(getattr(lib(), "zk_kzg_%s_divide_dev" % _NAME[curve])(d.ptr, n, _ptr(zw), d_q.ptr, d_y.ptr, 0))
        q = from_mont(d_q.to_host()[:4 * max(n - 1, 0)], curve) if n > 1 else []
        return q, _ints(d_y.to_host())[0]
    finally:
        d_q.free(); d_y.free()
        if owned:
            d.free()


def evaluate(coeffs, z, curve="BN128"):
    """p(z) alone: the first two phases of `divide`, nothing but y is written"""
    d, n, owned = _dev_poly(coeffs, curve)
    zw = _scalar(z, curve, "z")
    d_y = DevArray(4)
    try:
        _check(getattr(lib(), "zk_kzg_%s_divide_dev" % _NAME[curve])(d.ptr, n, _ptr(zw), None, d_y.ptr, 0))
        return _ints(d_y.to_host())[0]
    finally:
        d_y.free()
        if owned:
            d.free()


def lincomb(polys, gamma, curve="BN128"):
    """sum_i gamma^i p_i as integers (zk_kzg_<curve>_lincomb_dev); shorter polynomials count as zero-padded"""
    devs = [_dev_poly(p, curve) for p in polys]
    n_max = max(n for _, n, _ in devs)
    ptrs = np.array([d.ptr or 0 for d, _, _ in devs], dtype=np.uint64); lens = np.array([n for _, n, _ in devs], dtype=np.uint64)
    out = DevArray(4 * max(n_max, 1))
    try:
        _check(getattr(lib(), "zk_kzg_%s_lincomb_dev" % _NAME[curve])(_ptr(ptrs), _ptr(lens), len(devs), _ptr(_scalar(gamma, curve, "gamma")), out.ptr, 0))
        return from_mont(out.to_host()[:4 * n_max], curve)
    finally:
        out.free()
        for d, _, owned in devs:
            if owned:
                d.free()


def gamma_of(curve, commitments, z):
    """The gamma of a several-polynomial opening as the command-line tools derive it: SHA-256 over the curve's name in ASCII ("BN128" |
    "BLS12381"), then every commitment in the file's encoding (point_bytes each, affine little-endian Montgomery, all zero for infinity) in
    the order of the polynomials, then z as 32 little-endian bytes; the digest read as a big-endian integer and reduced mod r."""
    h = hashlib.sha256(curve.encode("ascii"))
    for c in commitments:
        h.update(bytes(c))
    h.update(int(z).to_bytes(32, "little"))
    return int.from_bytes(h.digest(), "big") % _FR[curve]


def point_to_json(pt, curve):
    """a G1 point in the layout of the sums -> {"x", "y"} decimal strings as proof.json writes its G1 points; infinity is (0, 1)"""
    nl = _FQ_WORDS[curve]
    a = np.frombuffer(bytes(pt), dtype="<u8").astype(np.uint64)
    if not a.any():
        return {"x": "0", "y": "1"}
    d = DevArray.from_host(a)
    try:
        w = fq_convert(d, curve, to_mont=False).to_host()
    finally:
        d.free()
    xy = [int.from_bytes(w[i * nl:(i + 1) * nl].astype("<u8").tobytes(), "little") for i in range(2)]
    return {"x": str(xy[0]), "y": str(xy[1])}


def point_from_json(js, curve):
    """the inverse; a coordinate that does not fit the field's width is an error, one that is >= q is left for the verifier to refuse"""
    nl = _FQ_WORDS[curve]
    x, y = int(js["x"], 0), int(js["y"], 0)
    if (x, y) == (0, 1):
        return bytes(16 * nl)
    if not (0 <= x < (1 << (64 * nl)) and 0 <= y < (1 << (64 * nl))):
        raise ZkError("kzg: a coordinate does not fit the base field's width")
    a = np.frombuffer(x.to_bytes(8 * nl, "little") + y.to_bytes(8 * nl, "little"), dtype="<u8").astype(np.uint64)
    d = DevArray.from_host(a)
    try:
        return fq_convert(d, curve, to_mont=True).to_host().astype("<u8").tobytes()
    finally:
        d.free()


class Kzg:
    """tauG1[0, max_coeffs) of a powers-of-tau file on the device (zk_kzg_new), with G2 and tauG2[1] for verification.  max_coeffs = 0:
    everything the file has, 2^(power + 1) - 1.  The file is trusted: run Srs.check first."""

    def __init__(self, srs, max_coeffs=0):
        self.curve = srs.curve
        self._h = lib().zk_kzg_new(srs._h, int(max_coeffs))
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())
        mc, pw, pb, ob = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().zk_kzg_info(self._h, None, C.byref(mc), C.byref(pw), C.byref(pb), C.byref(ob)))
        self.max_coeffs, self.power, self.point_bytes, self.opening_bytes = mc.value, pw.value, pb.value, ob.value

    def _point(self, d_out):
        w = d_out.to_host()
        return bytes(self.point_bytes) if int(w[-1]) & 0xFFFFFFFF else w[:-1].astype("<u8").tobytes()

    def commit(self, p):
        """[p(tau)] G1; no coefficients and the zero polynomial give infinity"""
        d, n, owned = _dev_poly(p, self.curve)
        out = DevArray(self.point_bytes // 8 + 1, zero=True)
        try:
            _check(lib().zk_kzg_commit_dev(self._h, d.ptr, n, out.ptr, 0))
            return self._point(out)
        finally:
            out.free()
            if owned:
                d.free()

    def commit_evals(self, evals):
        """the commitment to the polynomial whose values on the 2^k-point domain of fr_ntt are `evals`, through the Lagrange basis in the group"""
        d, n, owned = _dev_poly(evals, self.curve)
        if n == 0 or n & (n - 1):
            raise ZkError("kzg: the number of evaluations must be a power of two")
        out = DevArray(self.point_bytes // 8 + 1, zero=True)
        try:
            _check(lib().zk_kzg_commit_evals_dev(self._h, d.ptr, n.bit_length() - 1, out.ptr, 0))
            return self._point(out)
        finally:
            out.free()
            if owned:
                d.free()

    def eval(self, p, z):
        d, n, owned = _dev_poly(p, self.curve)
        d_y = DevArray(4)
        try:
            _check(lib().zk_kzg_eval_dev(self._h, d.ptr, n, _ptr(_scalar(z, self.curve, "z")), d_y.ptr, 0))
            return _ints(d_y.to_host())[0]
        finally:
            d_y.free()
            if owned:
                d.free()

    def open(self, p, z):
        """-> (y = p(z), W = [q(tau)] G1 with q = (p - y) / (X - z))"""
        d, n, owned = _dev_poly(p, self.curve)
        d_y = DevArray(4); out = DevArray(self.point_bytes // 8 + 1, zero=True)
        try:
            _check(lib().zk_kzg_open_dev(self._h, d.ptr, n, _ptr(_scalar(z, self.curve, "z")), d_y.ptr, out.ptr, 0))
            return _ints(d_y.to_host())[0], self._point(out)
        finally:
            d_y.free(); out.free()
            if owned:
                d.free()

    def open_many(self, polys, z, gamma):
        """k polynomials at one point: -> ([p_i(z)], W of sum_i gamma^i p_i).  The verifier folds the commitments (fold_commitments) and the
        values with the same gamma and checks one opening."""
        devs = [_dev_poly(p, self.curve) for p in polys]
        ptrs = np.array([d.ptr or 0 for d, _, _ in devs], dtype=np.uint64); lens = np.array([n for _, n, _ in devs], dtype=np.uint64)
        d_ys = DevArray(4 * max(len(devs), 1)); out = DevArray(self.point_bytes // 8 + 1, zero=True)
        try:
            _check(lib().zk_kzg_open_many_dev(self._h, _ptr(ptrs), _ptr(lens), len(devs), _ptr(_scalar(z, self.curve, "z")),
                                              _ptr(_scalar(gamma, self.curve, "gamma")), d_ys.ptr, out.ptr, 0))
            return _ints(d_ys.to_host())[:len(devs)], self._point(out)
        finally:
            d_ys.free(); out.free()
            for d, _, owned in devs:
                if owned:
                    d.free()

    def fold_commitments(self, commitments, gamma):
        """sum_i gamma^i C_i"""
        buf = np.frombuffer(b"".join(bytes(c) for c in commitments), dtype=np.uint8)
        if buf.size != len(commitments) * self.point_bytes or not len(commitments):
            raise ZkError("kzg: commitments of %d bytes each expected" % self.point_bytes)
        out = np.zeros(self.point_bytes, np.uint8)
        _check(lib().zk_kzg_fold_commitments(self._h, buf.ctypes.data, len(commitments), _ptr(_scalar(gamma, self.curve, "gamma")), out.ctypes.data))
        return out.tobytes()

    def fold_values(self, ys, gamma):
        r = _FR[self.curve]
        return sum(int(y) * pow(int(gamma), i, r) for i, y in enumerate(ys)) % r

    def verify(self, openings, seed=None, locate=True):
        """openings: (C, z, y, W) tuples -> (verdict, first_bad): one randomised check of all of them (zk_kzg_verify).  verdict is ACCEPTED
        (1), REJECTED (0) or the code of a malformed opening (groth16.verdict_name); first_bad is None for an accepted batch and when
        `locate` is off.  seed: 32 bytes from which the weights are derived, FOR TESTS ONLY."""
        sd = _seed(seed, "kzg verify")
        parts = []
        for c, z, y, w in openings:
            if len(c) != self.point_bytes or len(w) != self.point_bytes:
                raise ZkError("kzg verify: points of %d bytes expected" % self.point_bytes)
            parts += [bytes(c), _words([z]).tobytes(), _words([y]).tobytes(), bytes(w)]
        buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
        m = len(openings)
        verdict, bad = C.c_int(0), C.c_uint64(0)
        _check(lib().zk_kzg_verify(self._h, buf.ctypes.data if m else None, m, sd.ctypes.data if sd is not None else None, C.byref(verdict),
                                   C.byref(bad) if locate else None))
        return verdict.value, (bad.value if locate and verdict.value != 1 else None)

    def free(self):
        if self._h:
            lib().zk_kzg_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
