"""KZG commitments over a powers-of-tau file (include/zkgpu.h, "KZG commitments"): commit to a polynomial under a
ceremony's tauG1 section, open it at a point, check many openings in one randomised pairing equation.  What snarkjs's universal-setup
provers (`ffs` / `fff` / `ffv`, test/snark_verifier.sh:67-106) are made of; no per-circuit ceremony.  Commitments are in G1 and are NOT
hiding.  Everything runs on the device; there is no CPU fallback.  Kzg.open_multi / verify_multi open several polynomials, each on its own
set of points, in one proof of two points; divide_acc and interleave are its building blocks.

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


MULTI_MAX_POINTS = 16       # ZK_KZG_MULTI_MAX_POINTS


def divide_acc(coeffs, z, w, acc, curve="BN128"):
    """acc_j + w q_j for j < n - 1 with q = (p - p(z)) / (X - z), and p(z) (zk_kzg_<curve>_divide_acc_dev): the division's last phase adding
    into a running sum, what the quotient by a vanishing polynomial is made of.  acc: at least n - 1 integers -> (the new acc, y), entries
    from n - 1 on as they were; or a DevArray of Montgomery words, updated in place -> (acc, y).  Needs no file."""
    if curve not in _FR:
        raise ZkError('kzg: unknown curve "%s" (BN128 | BLS12381)' % curve)
    d, n, owned = _dev_poly(coeffs, curve)
    on_dev = isinstance(acc, DevArray)
    n_acc = acc.n // 4 if on_dev else len(acc)
    if n_acc < max(n - 1, 0):
        raise ZkError("kzg: the running sum holds %d elements, the quotient has %d" % (n_acc, n - 1))
    d_acc = acc if on_dev else DevArray.from_host(to_mont(acc, curve).reshape(-1)) if n_acc else DevArray(4)
    d_y = DevArray(4)
    try:
        _check(getattr(lib(), "zk_kzg_%s_divide_acc_dev" % _NAME[curve])(d.ptr, n, _ptr(_scalar(z, curve, "z")), _ptr(_scalar(w, curve, "w")), d_acc.ptr, d_y.ptr, 0))
        y = _ints(d_y.to_host())[0]
        return (acc, y) if on_dev else (from_mont(d_acc.to_host()[:4 * n_acc], curve) if n_acc else [], y)
    finally:
        d_y.free()
        if not on_dev:
            d_acc.free()
        if owned:
            d.free()


def interleave(polys, curve="BN128"):
    """sum_i p_i(X^k) X^i, fflonk's combination of k polynomials into one (zk_kzg_<curve>_interleave_dev): out[j k + i] = p_i[j] for
    j < max n_i, shorter polynomials zero-padded -> k max n_i integers"""
    if curve not in _FR:
        raise ZkError('kzg: unknown curve "%s" (BN128 | BLS12381)' % curve)
    devs = [_dev_poly(p, curve) for p in polys]
    n_max = max((n for _, n, _ in devs), default=0)
    ptrs = np.array([d.ptr or 0 for d, _, _ in devs], dtype=np.uint64); lens = np.array([n for _, n, _ in devs], dtype=np.uint64)
    out = DevArray(4 * max(n_max * len(devs), 1))
    try:
        _check(getattr(lib(), "zk_kzg_%s_interleave_dev" % _NAME[curve])(_ptr(ptrs), _ptr(lens), len(devs), out.ptr, 0))
        return from_mont(out.to_host()[:4 * n_max * len(devs)], curve) if n_max else []
    finally:
        out.free()
        for d, _, owned in devs:
            if owned:
                d.free()


def challenges_of(curve, commitments, sets, values):
    """The gamma of an opening at several points as the command-line tools derive it.  SHA-256 over, in this order: the curve's name in
    ASCII ("BN128" | "BLS12381"); the 15 bytes b"kzg-multi-gamma"; the number of polynomials as 4 little-endian bytes; every commitment in the
    file's encoding (point_bytes each, all zero for infinity) in the order of the polynomials; then for every set its number of points as 4
    little-endian bytes followed by its points, 32 little-endian bytes each; then for every set its values, 32 little-endian bytes each, in
    the order of its points.  The digest read as a big-endian integer and reduced mod r."""
    h = hashlib.sha256(curve.encode("ascii") + b"kzg-multi-gamma" + len(commitments).to_bytes(4, "little"))
    for c in commitments:
        h.update(bytes(c))
    for s in sets:
        h.update(len(s).to_bytes(4, "little"))
        for p in s:
            h.update(int(p).to_bytes(32, "little"))
    for ys in values:
        for y in ys:
            h.update(int(y).to_bytes(32, "little"))
    return int.from_bytes(h.digest(), "big") % _FR[curve]


def challenge_z(curve, gamma, W1, avoid=()):
    """The z of an opening at several points: SHA-256 over the curve's name in ASCII, the 11 bytes b"kzg-multi-z", gamma as 32 little-endian
    bytes and W1 in the file's encoding; the digest read as a big-endian integer and reduced mod r.  z must lie outside the opening points
    (`avoid`): while it does not, the same bytes are hashed again with one more byte at the end, a counter that starts at 1."""
    base = curve.encode("ascii") + b"kzg-multi-z" + int(gamma).to_bytes(32, "little") + bytes(W1)
    avoid = {int(p) for p in avoid}
    z = int.from_bytes(hashlib.sha256(base).digest(), "big") % _FR[curve]
    counter = 1
    while z in avoid:
        z = int.from_bytes(hashlib.sha256(base + bytes([counter])).digest(), "big") % _FR[curve]
        counter += 1
    return z


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

    def multi_begin(self, polys, sets):
        """the first stage of open_multi, for a caller with a transcript of its own: -> a MultiOpening that holds the values"""
        return MultiOpening(self, polys, sets)

    def open_multi(self, polys, sets, transcript=challenges_of, transcript_z=challenge_z, commitments=None, gamma=None, z=None):
        """k polynomials, polynomial i on its own set sets[i] of 1 .. MULTI_MAX_POINTS distinct points, in one proof of two points
        (zk_kzg_multi_begin / _quotient / _finish) -> (values, W1, W2, gamma, z), values[i][j] = p_i(sets[i][j]).
        gamma = transcript(curve, commitments, sets, values) once the values are known and z = transcript_z(curve, gamma, W1, avoid=points)
        once W1 is; a prover with another hash passes its own two functions, or gamma and z themselves.  commitments: the C_i when the
        caller has them, else they are made here for the transcript."""
        devs = [_dev_poly(p, self.curve) for p in polys]
        m = None
        try:
            m = MultiOpening(self, [d for d, _, _ in devs], sets)
            if gamma is None:
                if commitments is None:
                    commitments = [self.commit(d) for d, _, _ in devs]
                gamma = transcript(self.curve, commitments, m.sets, m.values)
            W1 = m.quotient(gamma)
            if z is None:
                z = transcript_z(self.curve, gamma, W1, avoid=[p for s in m.sets for p in s])
            W2 = m.finish(z)
            return m.values, W1, W2, int(gamma), int(z)
        finally:
            if m is not None:
                m.free()
            for d, _, owned in devs:
                if owned:
                    d.free()

    def pack_multi(self, proof):
        """(commitments, sets, values, gamma, z, W1, W2) -> the bytes zk_kzg_multi_verify takes for one proof"""
        cs, sets, values, gamma, z, W1, W2 = proof
        if len(sets) != len(cs) or len(values) != len(cs) or any(len(s) != len(v) for s, v in zip(sets, values)):
            raise ZkError("kzg verify: as many sets and lists of values as commitments, and a value for every point")
        for pt in list(cs) + [W1, W2]:
            if len(pt) != self.point_bytes:
                raise ZkError("kzg verify: points of %d bytes expected" % self.point_bytes)
        parts = [len(cs).to_bytes(8, "little")] + [bytes(c) for c in cs] + [len(s).to_bytes(8, "little") for s in sets]
        parts += [_words([p for s in sets for p in s]).tobytes(), _words([y for v in values for y in v]).tobytes(), _words([gamma, z]).tobytes(), bytes(W1), bytes(W2)]
        return b"".join(parts)

    def verify_multi(self, proofs, seed=None, locate=True):
        """proofs: (commitments, sets, values, gamma, z, W1, W2) tuples -> (verdict, first_bad) as `verify` gives them: every proof's F
        from one small sum, then one randomised check of all of them (zk_kzg_multi_verify)."""
        sd = _seed(seed, "kzg verify")
        buf = np.frombuffer(b"".join(self.pack_multi(p) for p in proofs), dtype=np.uint8)
        m = len(proofs)
        verdict, bad = C.c_int(0), C.c_uint64(0)
        _check(lib().zk_kzg_multi_verify(self._h, buf.ctypes.data if m else None, buf.size, m, sd.ctypes.data if sd is not None else None, C.byref(verdict),
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


class MultiOpening:
    """An opening at several points between its stages (zk_kzg_multi_t): made by Kzg.multi_begin, which evaluates every polynomial on its
    set; then quotient(gamma) -> W1 and finish(z) -> W2, once each and in this order, because z is a challenge that depends on W1.  The
    polynomials it was given as DevArrays stay with the caller and must not change before finish returns."""

    def __init__(self, kzg, polys, sets):
        self._kzg, self._h = kzg, None
        self.sets = [[int(p) for p in s] for s in sets]
        if len(self.sets) != len(polys):
            raise ZkError("kzg multi: %d polynomials, %d sets" % (len(polys), len(self.sets)))
        self._devs = [_dev_poly(p, kzg.curve) for p in polys]
        flat = [p for s in self.sets for p in s]
        pts = _words(flat).reshape(-1) if flat else np.zeros(4, np.uint64)
        sizes = np.array([len(s) for s in self.sets] or [0], dtype=np.uint32)
        ptrs = np.array([d.ptr or 0 for d, _, _ in self._devs] or [0], dtype=np.uint64); lens = np.array([n for _, n, _ in self._devs] or [0], dtype=np.uint64)
        d_vals = DevArray(4 * max(len(flat), 1))
        try:
            self._h = lib().zk_kzg_multi_begin(kzg._h, _ptr(ptrs), _ptr(lens), len(self._devs), _ptr(pts), sizes.ctypes.data, d_vals.ptr, 0)
            if not self._h:
                raise ZkError(lib().zk_last_error().decode())
            ys = _ints(d_vals.to_host())[:len(flat)]
        except Exception:
            self.free()
            raise
        finally:
            d_vals.free()
        self.values, at = [], 0
        for s in self.sets:
            self.values.append(ys[at:at + len(s)]); at += len(s)

    def _stage(self, fn, scalar, what):
        out = DevArray(self._kzg.point_bytes // 8 + 1, zero=True)
        try:
            _check(fn(self._h, _ptr(_scalar(scalar, self._kzg.curve, what)), out.ptr, 0))
            return self._kzg._point(out)
        finally:
            out.free()

    def quotient(self, gamma):
        """W1 = [q(tau)] G1, q = sum_i gamma^i (p_i - r_i) / Z_(S_i); infinity when every polynomial is its own interpolant"""
        return self._stage(lib().zk_kzg_multi_quotient, gamma, "gamma")

    def finish(self, z):
        """W2 for a z outside every set"""
        return self._stage(lib().zk_kzg_multi_finish, z, "z")

    def free(self):
        if self._h:
            lib().zk_kzg_multi_free(self._h); self._h = None
        for d, _, owned in getattr(self, "_devs", []):
            if owned:
                d.free()
        self._devs = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
