"""A PLONK prover and verifier over the KZG layer (kzg.py) and the scalar-field polynomial layer (frpoly.py, DESIGN.md
3.20): setup, prove, verify.  The protocol, the transcript and the files are this module; everything over Fr runs on the
device through zk_fr_<curve>_*_dev, zk_plonk_<curve>_quotient_dev / _gate_check_dev, zk_fr_<curve>_gather_dev and Kzg.open_multi.  There is no
CPU fallback.  Cut down to what those layers do: NO linearisation polynomial (every polynomial of the identity is opened at zeta, Z at
zeta w as well, in one Shplonk proof of two points), the quotient t committed WHOLE (degree 3n + 5: the file must hold 3n + 6 G1 powers), a
circuit is a gate table, written by hand or compiled from a circom .r1cs (R1csCircuit); no custom gates, no lookups, not fflonk's
interleaved form.

Field Fr of BN128 or BLS12381.  n = 2^k >= 8 rows (smaller circuits are padded to 8, others to the next power of two; a padding row has all
selectors 0 and its wires on variable 0).  H = <w> with the w of zk_fr_<curve>_ntt_dev, w = 7^((r - 1) / n).

Circuit.  Row i must satisfy qL a + qR b + qO c + qM a b + qC + PI_i = 0.  Circuit puts one row per public input in front (qL = 1, the rest 0,
a = public[i]); PI_i = -x_i for i < l and 0 otherwise.

Wiring.  Position (column j, row i) has the label k_j w^i with k_0 = 1; k_1 < k_2 are the smallest integers >= 2 with k_1^n != 1, k_2^n != 1
and (k_2 / k_1)^n != 1.  sigma maps each position to the next position of the same variable, cyclically in (column, row) order; S_sigma_j is
the polynomial whose values on H are the labels of sigma(j, .).

Rounds.
 1. wire values gathered from the witness; a, b, c interpolated and blinded as a += (b_1 X + b_2) Z_H (b: b_3, b_4; c: b_5, b_6); [A], [B], [C]
 2. beta, gamma; z_0 = 1, z_(i+1) = z_i prod_j (w_j,i + beta k_j w^i + gamma) / prod_j (w_j,i + beta sigma_j,i + gamma), which must close with
    z_n = 1; Z += (b_7 X^2 + b_8 X + b_9) Z_H; [Z]
 3. alpha; on the coset 7 H_4n
      t = [ a b q_M + a q_L + b q_R + c q_O + q_C + PI + alpha ((a + beta X + gamma)(b + beta k_1 X + gamma)(c + beta k_2 X + gamma) Z
            - (a + beta S_sigma1 + gamma)(b + beta S_sigma2 + gamma)(c + beta S_sigma3 + gamma) Z(wX)) + alpha^2 L_1 (Z - 1) ] / Z_H
    (the bracket is zk_plonk_<curve>_quotient_dev, the division divide_zh_coset); the coefficients from 3n + 6 on must be zero; [T]
 4. zeta, drawn again while zeta = 0 or zeta^n = 1
 5. Kzg.open_multi of q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3, a, b, c, t on {zeta} and of Z on {zeta, zeta w}
The proof is [A], [B], [C], [Z], [T], the 14 values in that order, W1, W2.  The opening's own challenges are NOT in it: the verifier derives them.

Transcript.  H is SHA-256; a digest is read as a big-endian integer and reduced mod r; a scalar is 32 little-endian bytes; a point is
point_bytes bytes in the .ptau file's encoding (affine, little-endian Montgomery, all zero for infinity); "curve" is the name in ASCII
("BN128" | "BLS12381"); a counter is one byte that starts at 0 and only moves for a re-draw.
    vkd    = H(curve || "plonk-vk" || k u32le || l u32le || k_1 || k_2 || the 8 commitments)
    c0     = H(curve || "plonk-v1" || vkd || l u32le || x_0 .. x_(l-1))
    c1     = H(c0 || A || B || C)            beta = H(c1 || 00)     gamma = H(c1 || 01)
    c2     = H(c1 || Z)                      alpha = H(c2 || 00)
    c3     = H(c2 || T)                      zeta = H(c3 || ctr)
    c4     = H(c3 || the 14 values)          gamma' = H(c4 || 00)   z' = H(c4 || 01 || W1 || ctr), outside {zeta, zeta w}

Blinding.  The nine blinders come from `secrets`; blinding=[9 integers] is FOR TESTS ONLY (all zero gives the unblinded proof)."""
import ctypes as C
import hashlib
import json
import secrets

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import frpoly as fp
from .groth16 import _FR, _NAME
from .kzg import _scalar, _words, point_from_json, point_to_json, to_mont

ACCEPTED, REJECTED, INPUT_NOT_CANONICAL = 1, 0, -1
TWO_ADICITY = {"BN128": 28, "BLS12381": 32}
N_VALUES, N_FIXED = 14, 8
POINT_NAMES = ("A", "B", "C", "Z", "T", "W1", "W2")
FIXED_NAMES = ("qL", "qR", "qO", "qM", "qC", "S1", "S2", "S3")
M64 = (1 << 64) - 1


# ---- the field on the host: only what setup's integers and the verifier need --------------------------------------------------------------
def _curve(curve):
    if curve not in _FR:
        raise ZkError('plonk: unknown curve "%s" (BN128 | BLS12381)' % curve)
    return _FR[curve]


def omega(curve, log_n):
    """the generator of the 2^log_n-point domain of zk_fr_<curve>_ntt_dev: 7^((r - 1) / 2^log_n)"""
    r = _curve(curve)
    if log_n > TWO_ADICITY[curve]:
        raise ZkError("plonk: a domain of 2^%d exceeds the field's 2-adicity (%d)" % (log_n, TWO_ADICITY[curve]))
    return pow(7, (r - 1) >> log_n, r)


def coset_ks(curve, log_n):
    """(k_1, k_2): the smallest integers >= 2 with k_1 < k_2, k_1^n != 1, k_2^n != 1 and (k_2 / k_1)^n != 1, n = 2^log_n: H, k_1 H and k_2 H
    are disjoint"""
    r, n = _curve(curve), 1 << log_n
    k1 = 2
    while pow(k1, n, r) == 1:
        k1 += 1
    k2 = k1 + 1
    while pow(k2, n, r) == 1 or pow(k2 * pow(k1, -1, r) % r, n, r) == 1:
        k2 += 1
    return k1, k2


def check_size(curve, log_n):
    """n = 2^log_n rows need the coset of 4n points"""
    _curve(curve)
    if log_n + 2 > TWO_ADICITY[curve]:
        raise ZkError("plonk: n = 2^%d rows need a coset of 2^%d points, the field's 2-adicity is %d" % (log_n, log_n + 2, TWO_ADICITY[curve]))


def required_powers(n):
    """the G1 powers the file must hold: the quotient is committed whole, with 3n + 6 coefficients"""
    return 3 * n + 6


def _below(words, r):
    """words: (n, 4) u64 -> a boolean per row: the value is below r"""
    rw = [(r >> (64 * i)) & M64 for i in range(4)]
    lt = np.zeros(len(words), dtype=bool)
    eq = np.ones(len(words), dtype=bool)
    for i in (3, 2, 1, 0):
        col = words[:, i]
        lt |= eq & (col < np.uint64(rw[i]))
        eq &= col == np.uint64(rw[i])
    return lt


def _canon_words(values, r, what):
    """integers, bytes of 32 each, or an (n, 4) u64 array -> (n, 4) u64 canonical words, every value checked to be below r"""
    if isinstance(values, (bytes, bytearray, memoryview)):
        b = bytes(values)
        if len(b) % 32:
            raise ZkError("plonk: %s: %d bytes is no whole number of 32-byte values" % (what, len(b)))
        w = np.frombuffer(b, dtype="<u8").astype(np.uint64).reshape(-1, 4)
    elif isinstance(values, np.ndarray) and values.dtype == np.uint64 and values.ndim == 2 and values.shape[1] == 4:
        w = np.ascontiguousarray(values)
    else:
        vals = [int(v) for v in values]
        for i, v in enumerate(vals):
            if not 0 <= v < (1 << 256):
                raise ZkError("plonk: %s %d is not below the scalar field's modulus" % (what, i))
        w = _words(vals) if vals else np.zeros((0, 4), np.uint64)
    ok = _below(w, r)
    if not ok.all():
        raise ZkError("plonk: %s %d is not below the scalar field's modulus" % (what, int(np.argmin(ok))))
    return w


def _int_of(words_row):
    return int.from_bytes(np.ascontiguousarray(words_row, dtype="<u8").tobytes(), "little")


# ---- the transcript -----------------------------------------------------------------------------------------------------------------------
def _le(v):
    return int(v).to_bytes(32, "little")


def _draw(curve, *parts):
    return int.from_bytes(hashlib.sha256(b"".join(parts)).digest(), "big") % _FR[curve]


def vk_digest(curve, log_n, n_public, k1, k2, commitments):
    """vkd = H(curve || "plonk-vk" || k u32le || l u32le || k_1 || k_2 || the 8 commitments): curve in ASCII, k = log n and l the number of
    public inputs as 4 little-endian bytes each, k_1 and k_2 as 32 little-endian bytes, every commitment in the file's encoding, in the order
    q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3"""
    return hashlib.sha256(curve.encode("ascii") + b"plonk-vk" + int(log_n).to_bytes(4, "little") + int(n_public).to_bytes(4, "little") + _le(k1) + _le(k2) +
                          b"".join(bytes(c) for c in commitments)).digest()


def transcript_start(curve, vkd, publics):
    """c0 = H(curve || "plonk-v1" || vkd || l u32le || x_0 .. x_(l-1)): the public inputs as 32 little-endian bytes each"""
    return hashlib.sha256(curve.encode("ascii") + b"plonk-v1" + vkd + len(publics).to_bytes(4, "little") + b"".join(_le(x) for x in publics)).digest()


def transcript_wires(curve, c0, A, B, Cc):
    """c1 = H(c0 || A || B || C); beta = H(c1 || 00), gamma = H(c1 || 01) -> (c1, beta, gamma)"""
    c1 = hashlib.sha256(c0 + bytes(A) + bytes(B) + bytes(Cc)).digest()
    return c1, _draw(curve, c1, b"\x00"), _draw(curve, c1, b"\x01")


def transcript_product(curve, c1, Z):
    """c2 = H(c1 || Z); alpha = H(c2 || 00) -> (c2, alpha)"""
    c2 = hashlib.sha256(c1 + bytes(Z)).digest()
    return c2, _draw(curve, c2, b"\x00")


def transcript_quotient(curve, c2, T, n):
    """c3 = H(c2 || T); zeta = H(c3 || ctr), ctr one byte from 0, drawn again while zeta = 0 or zeta^n = 1 -> (c3, zeta)"""
    r = _FR[curve]
    c3 = hashlib.sha256(c2 + bytes(T)).digest()
    for ctr in range(256):
        zeta = _draw(curve, c3, bytes([ctr]))
        if zeta != 0 and pow(zeta, n, r) != 1:
            return c3, zeta
    raise ZkError("plonk: no evaluation point after 256 draws")


def transcript_values(curve, c3, values):
    """c4 = H(c3 || the 14 values, 32 little-endian bytes each); gamma' = H(c4 || 00) -> (c4, gamma')"""
    c4 = hashlib.sha256(c3 + b"".join(_le(v) for v in values)).digest()
    return c4, _draw(curve, c4, b"\x00")


def transcript_z(curve, c4, W1, avoid):
    """z' = H(c4 || 01 || W1 || ctr), ctr one byte from 0, drawn again while z' is one of the opening points {zeta, zeta w}"""
    avoid = {int(p) for p in avoid}
    for ctr in range(256):
        z = _draw(curve, c4, b"\x01", bytes(W1), bytes([ctr]))
        if z not in avoid:
            return z
    raise ZkError("plonk: no opening challenge after 256 draws")


# ---- circuits -------------------------------------------------------------------------------------------------------------------------------
SELECTORS = ("qL", "qR", "qO", "qM", "qC")
WIRES = ("a", "b", "c")


class Circuit:
    """A gate table.  gates: a mapping with qL, qR, qO, qM, qC (integers below r, or (m, 4) u64 canonical words) and a, b, c (variable ids) of
    one length m; public: l variable ids.  The class puts the l public rows in front and pads to n = 2^k >= 8 rows: self.sel[name] is (n, 4)
    u64, self.wire[name] n u32.  Everything here is host integers: no device work."""

    def __init__(self, n_vars, public, gates, curve="BN128"):
        r = _curve(curve)
        self.curve, self.n_vars = curve, int(n_vars)
        self.public = [int(v) for v in public]
        if self.n_vars < 1:
            raise ZkError("plonk: a circuit has at least one variable (padding rows sit on variable 0)")
        raw_sel = {s: _canon_words(gates[s], r, "selector %s of gate" % s) for s in SELECTORS}
        raw_wire = {w: np.asarray(gates[w], dtype=np.int64).reshape(-1) for w in WIRES}
        m = len(raw_wire["a"])
        if any(len(v) != m for v in list(raw_sel.values()) + list(raw_wire.values())):
            raise ZkError("plonk: the selector and wire arrays of a circuit have one length")
        for w in WIRES:
            bad = np.nonzero((raw_wire[w] < 0) | (raw_wire[w] >= self.n_vars))[0]
            if bad.size:
                raise ZkError("plonk: wire %s of gate %d is variable %d, the circuit has %d variables" % (w, int(bad[0]), int(raw_wire[w][bad[0]]), self.n_vars))
        for i, v in enumerate(self.public):
            if not 0 <= v < self.n_vars:
                raise ZkError("plonk: public input %d is variable %d, the circuit has %d variables" % (i, v, self.n_vars))
        self.gates = {**raw_sel, **{w: raw_wire[w].astype(np.uint32) for w in WIRES}}
        self.n_public, self.n_gates = len(self.public), m
        rows = self.n_public + m
        self.log_n = max(3, (rows - 1).bit_length())
        self.n = 1 << self.log_n
        check_size(curve, self.log_n)
        self.sel, self.wire = {}, {}
        for s in SELECTORS:
            a = np.zeros((self.n, 4), np.uint64)
            if s == "qL":
                a[:self.n_public, 0] = 1
            a[self.n_public:rows] = raw_sel[s]
            self.sel[s] = a
        for w in WIRES:
            a = np.zeros(self.n, np.uint32)
            if w == "a":
                a[:self.n_public] = self.public
            a[self.n_public:rows] = raw_wire[w]
            self.wire[w] = a

    def sigma(self):
        """the permutation of the 3n positions p = column n + row as integers: a stable sort by variable id, then a rotation within the
        groups -> sigma[p], the next position of p's variable (cyclically, in (column, row) order)"""
        var = np.concatenate([self.wire[w] for w in WIRES]).astype(np.int64)
        order = np.argsort(var, kind="stable")
        sv = var[order]
        first = np.ones(len(sv), dtype=bool)
        first[1:] = sv[1:] != sv[:-1]
        start = np.maximum.accumulate(np.where(first, np.arange(len(sv)), 0))         # where each element's group begins
        last = np.ones(len(sv), dtype=bool)
        last[:-1] = first[1:]
        nxt = np.where(last, order[start], np.roll(order, -1))
        out = np.empty(len(sv), dtype=np.uint32)
        out[order] = nxt
        return out

    def save(self, path):
        """the .npz of the constructor's arrays: selectors (m, 4) u64 canonical words, a, b, c u32, n_vars, public"""
        np.savez(path, n_vars=np.uint64(self.n_vars), public=np.asarray(self.public, dtype=np.uint32), **self.gates)

    @classmethod
    def load(cls, path, curve="BN128"):
        with np.load(path) as z:
            missing = [k for k in SELECTORS + WIRES + ("n_vars", "public") if k not in z]
            if missing:
                raise ZkError("plonk: %s holds no %s" % (path, ", ".join(missing)))
            gates = {k: np.asarray(z[k], dtype=np.uint64).reshape(-1, 4) for k in SELECTORS}
            gates.update({k: np.asarray(z[k]).reshape(-1) for k in WIRES})
            return cls(int(z["n_vars"]), [int(v) for v in np.asarray(z["public"]).reshape(-1)], gates, curve)


R1CS_INFO = ("n_wires", "n_public", "n_constraints", "n_gates", "n_aux", "n_segments", "max_segment_terms", "n_segment_terms")


class R1csCircuit(Circuit):
    """The gate table of a circom .r1cs (include/zkgpu.h states the compile rule): zk_plonk_<curve>_r1cs_new compiles the file
    on the host -- no device is touched -- and this is the Circuit of the tables it copies out.  Variable w < n_wires is wire w of the file,
    the n_aux auxiliaries follow; the publics are wires 1 .. l.  .origin[g] is the constraint gate g came from (g counts the file's gates:
    row l + g of the table), .segments the table that defines the auxiliaries (seg_first, seg_ptr, seg_wire, seg_coef), .info the counts of
    R1CS_INFO.  A witness for prove() is the n_wires values of the .wtns, or its bytes; the handle lives until free()."""

    def __init__(self, r1cs_bytes, curve="BN128"):
        _curve(curve)
        self.curve, self._h = curve, None
        data = np.frombuffer(bytes(r1cs_bytes), dtype=np.uint8)
        self._h = getattr(lib(), "zk_plonk_%s_r1cs_new" % _NAME[curve])(data.ctypes.data, data.size)
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())
        try:
            info = np.zeros(len(R1CS_INFO), np.uint64)
            _check(getattr(lib(), "zk_plonk_%s_r1cs_info" % _NAME[curve])(self._h, _ptr(info)))
            self.info = {k: int(v) for k, v in zip(R1CS_INFO, info)}
            m, ns, nt = self.info["n_gates"], self.info["n_segments"], self.info["n_segment_terms"]
            sel = np.zeros((5, m, 4), np.uint64)
            wires = [np.zeros(max(m, 1), np.uint32) for _ in range(4)]
            seg = {"seg_first": np.zeros(max(ns, 1), np.uint32), "seg_ptr": np.zeros(ns + 1, np.uint64), "seg_wire": np.zeros(max(nt, 1), np.uint32),
                   "seg_coef": np.zeros((max(nt, 1), 4), np.uint64)}
            _check(getattr(lib(), "zk_plonk_%s_r1cs_tables" % _NAME[curve])(self._h, _ptr(sel), *[_ptr(w) for w in wires], *[_ptr(seg[k]) for k in ("seg_first", "seg_ptr", "seg_wire", "seg_coef")]))
            gates = {s: sel[i] for i, s in enumerate(SELECTORS)}
            gates.update({w: wires[i][:m] for i, w in enumerate(WIRES)})
            self.n_wires, self.n_aux, self.origin = self.info["n_wires"], self.info["n_aux"], wires[3][:m]
            self.segments = {"seg_first": seg["seg_first"][:ns], "seg_ptr": seg["seg_ptr"], "seg_wire": seg["seg_wire"][:nt], "seg_coef": seg["seg_coef"][:nt]}
            super().__init__(self.n_wires + self.n_aux, range(1, self.info["n_public"] + 1), gates, curve)
        except Exception:
            self.free()
            raise

    def free(self):
        if getattr(self, "_h", None):
            getattr(lib(), "zk_plonk_%s_r1cs_free" % _NAME[self.curve])(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- device helpers: compositions of the layers below, by raw pointer so that a polynomial can sit inside a longer buffer -------------------
class _View(DevArray):
    """n elements of another DevArray from element `off` on; it owns nothing"""

    def __init__(self, base, off, n):
        self.ptr, self.n, self._base = base.ptr + 32 * int(off), 4 * int(n), base

    def free(self):
        pass


def _fn(curve, name):
    return getattr(lib(), "zk_fr_%s_%s_dev" % (_NAME[curve], name))


def _ntt(curve, ptr, log_n, inverse=False, coset=False):
    _check(getattr(lib(), "zk_fr_%s_ntt_dev" % _NAME[curve])(ptr, int(log_n), int(inverse), int(coset), 0))


def _add_into(curve, src_ptr, dst_ptr, n):
    """dst[i] += src[i], i < n (canonical, so a zeroed destination receives a copy)"""
    if n:
        _check(_fn(curve, "pointwise")(fp.ADD, src_ptr, dst_ptr, dst_ptr, int(n), 0))


def _powers_into(curve, base, scale, n, ptr):
    _check(_fn(curve, "powers")(_ptr(_scalar(base, curve, "base")), _ptr(_scalar(scale, curve, "scale")), int(n), ptr, 0))


def gather(src, idx, curve="BN128", out=None):
    """out[i] = src[idx[i]] on the device (zk_fr_<curve>_gather_dev): src a DevArray of elements; idx integers, checked here on the host (with
    the indices already on the device use gather_dev, where a bad index is counted by the kernel and comes back as the library's error)
    -> a DevArray of len(idx) elements"""
    _curve(curve)
    n_src = src.n // 4
    ix =np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    bad = np.nonzero((ix < 0) | (ix >= n_src))[0]
    if bad.size:
        raise ZkError("plonk: gather: index %d at position %d is not below the source's %d elements" % (int(ix[bad[0]]), int(bad[0]), n_src))
    d_idx = _upload_indices(ix)
    try:
        return gather_dev(src, d_idx, len(ix), curve, out)
    finally:
        d_idx.free()


def _upload_indices(ix):
    a = np.zeros((len(ix) + 1) // 2 * 2 or 2, np.uint32)
    a[:len(ix)] = ix
    return DevArray.from_host(a.view(np.uint64))


def gather_dev(src, d_idx, n, curve="BN128", out=None):
    """the same with the n u32 indices already on the device"""
    d_out = out if out is not None else DevArray(4 * max(int(n), 1))
    try:
        _check(_fn(curve, "gather")(src.ptr, src.n // 4, d_idx.ptr, int(n), d_out.ptr, 0))
        return d_out
    except Exception:
        if out is None:
            d_out.free()
        raise


def _mont_dev(curve, words):
    """(n, 4) u64 canonical words (checked by the caller) -> a DevArray of Montgomery words: the words times R^2 / R on the device (powers
    makes the vector of R^2, pointwise the product), so a witness of 2^20 values is never converted integer by integer"""
    n = len(words)
    d = DevArray.from_host(words.reshape(-1)) if n else DevArray(4)
    _mont_in_place(curve, d.ptr, n)
    return d


def _mont_in_place(curve, ptr, n):
    """the n canonical elements at a device address -> their Montgomery words"""
    if n:
        d_r2 = DevArray(4 * n)
        try:
            _powers_into(curve, 1, (1 << 256) % _FR[curve], n, d_r2.ptr)
            _check(_fn(curve, "pointwise")(fp.MUL, ptr, d_r2.ptr, ptr, n, 0))
        finally:
            d_r2.free()


def _r1cs_witness_words(circuit, witness):
    """what prove() and extend_witness() take for an R1csCircuit -> (n_wires, 4) u64 canonical words; every refusal on the host: the bytes of
    a .wtns over another field, a wrong count, a value that is not below r, wire 0 that is not the constant 1"""
    cv = circuit.curve
    if isinstance(witness, (bytes, bytearray, memoryview)) and bytes(witness[:4]) == b"wtns":
        from .r1cs import wtns_payload
        witness, _ = wtns_payload(bytes(witness), cv)
    ww = _canon_words(witness, _FR[cv], "witness value")
    if len(ww) != circuit.n_wires:
        raise ZkError("plonk: the witness has %d values, the .r1cs has %d wires" % (len(ww), circuit.n_wires))
    if _int_of(ww[0]) != 1:
        raise ZkError("plonk: witness value 0 is %d: wire 0 of a circom witness is the constant 1" % _int_of(ww[0]))
    return ww


def _extend_words(circuit, ww):
    cv, n = circuit.curve, circuit.n_wires
    d = DevArray(4 * circuit.n_vars)
    try:
        flat = np.ascontiguousarray(ww.reshape(-1))
        _check(lib().zk_dev_upload(d.ptr, _ptr(flat), flat.size * 8))
        _mont_in_place(cv, d.ptr, n)
        _check(getattr(lib(), "zk_plonk_%s_r1cs_extend_dev" % _NAME[cv])(circuit._h, d.ptr, 0))
        return d
    except Exception:
        d.free()
        raise


def extend_witness(circuit, witness):
    """the n_vars values of an R1csCircuit's variables on the device, as Montgomery words (what gather reads): the witness in front, then
    the auxiliaries, every one a prefix of its segment's sum (zk_plonk_<curve>_r1cs_extend_dev) -> a DevArray of n_vars x 4 words.
    witness: the n_wires canonical values of the .wtns in any form prove() takes, or the bytes of the .wtns itself."""
    if not isinstance(circuit, R1csCircuit):
        raise ZkError("plonk: extend_witness takes an R1csCircuit")
    return _extend_words(circuit, _r1cs_witness_words(circuit, witness))


def _upload_mont(curve, values, ptr):
    """a few integers -> Montgomery words at a device address"""
    a = to_mont(values, curve).reshape(-1)
    _check(lib().zk_dev_upload(ptr, _ptr(a), a.size * 8))


def _blind(curve, coef, n, bs):
    """coef += (sum_k bs[k] X^k) (X^n - 1): -bs[k] into coefficient k, bs[k] into coefficient n + k (zero until now)"""
    r = _FR[curve]
    if not any(bs):
        return
    low = DevArray.from_host(to_mont([(-b) % r for b in bs], curve).reshape(-1))
    try:
        _add_into(curve, low.ptr, coef.ptr, len(bs))
    finally:
        low.free()
    _upload_mont(curve, bs, coef.ptr + 32 * n)


def _coset_evals(curve, coef, n_coef, log_m):
    """the values on 7 H_m of the polynomial whose n_coef coefficients start at coef.ptr -> a new DevArray of m elements"""
    d = DevArray(4 << log_m, zero=True)
    try:
        _add_into(curve, coef.ptr, d.ptr, n_coef)
        _ntt(curve, d.ptr, log_m, coset=True)
        return d
    except Exception:
        d.free()
        raise


def _interpolate(curve, vals, n, extra, log_n):
    """the values on H -> a new DevArray of n + extra coefficients, the top `extra` zero"""
    d = DevArray(4 * (n + extra), zero=True)
    try:
        _add_into(curve, vals.ptr, d.ptr, n)
        _ntt(curve, d.ptr, log_n, inverse=True)
        return d
    except Exception:
        d.free()
        raise


def quotient(cols, log_n, alpha, beta, gamma, k1, k2, curve="BN128", out=None):
    """zk_plonk_<curve>_quotient_dev: cols, 15 DevArrays of 4n elements in the header's order -> the bracket of round 3 on the coset"""
    _curve(curve)
    m = 4 << int(log_n)
    if len(cols) != 15:
        raise ZkError("plonk: the quotient takes 15 columns, not %d" % len(cols))
    sc = [_scalar(v, curve, w) for v, w in ((alpha, "alpha"), (beta, "beta"), (gamma, "gamma"), (k1, "k1"), (k2, "k2"))]
    if any(c.n < 4 * m for c in cols):
        raise ZkError("plonk: every column of the quotient holds 4n = %d elements" % m)
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    d_out = out if out is not None else DevArray(4 * m)
    try:
        _check(getattr(lib(), "zk_plonk_%s_quotient_dev" % _NAME[curve])(_ptr(ptrs), int(log_n), *[_ptr(s) for s in sc], d_out.ptr, 0))
        return d_out
    except Exception:
        if out is None:
            d_out.free()
        raise


def gate_check(cols, n, curve="BN128"):
    """zk_plonk_<curve>_gate_check_dev: cols, 9 DevArrays of n elements (a, b, c, qL, qR, qO, qM, qC, PI) -> (rows that fail, the first or None)"""
    _curve(curve)
    if len(cols) != 9:
        raise ZkError("plonk: the gate check takes 9 columns, not %d" % len(cols))
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    bad, first = C.c_uint64(0), C.c_uint64(0)
    _check(getattr(lib(), "zk_plonk_%s_gate_check_dev" % _NAME[curve])(_ptr(ptrs), int(n), C.byref(bad), C.byref(first), 0))
    return int(bad.value), (None if bad.value == 0 else int(first.value))


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    """(curve, log n, l, k_1, k_2, the 8 commitments); `kzg` is the handle verify() pairs with, when the key came from a PlonkKey"""

    def __init__(self, curve, log_n, n_public, k1, k2, commitments, kzg=None):
        _curve(curve)
        self.curve, self.log_n, self.n_public, self.k1, self.k2 = curve, int(log_n), int(n_public), int(k1), int(k2)
        self.commitments = [bytes(c) for c in commitments]
        self.kzg = kzg
        if len(self.commitments) != N_FIXED:
            raise ZkError("plonk: a verification key holds %d commitments, not %d" % (N_FIXED, len(self.commitments)))
        check_size(curve, self.log_n)
        self.n = 1 << self.log_n
        self.digest = vk_digest(curve, self.log_n, self.n_public, self.k1, self.k2, self.commitments)


def vk_to_json(vk):
    return json.dumps({"protocol": "plonk-shplonk", "curve": vk.curve, "log_n": vk.log_n, "n_public": vk.n_public, "k1": str(vk.k1), "k2": str(vk.k2),
                       "commitments": {name: point_to_json(c, vk.curve) for name, c in zip(FIXED_NAMES, vk.commitments)}}, indent=1) + "\n"


def vk_from_json(text, kzg=None):
    js = json.loads(text)
    if js.get("protocol") != "plonk-shplonk":
        raise ZkError('plonk: not a verification key of this prover (protocol "%s")' % js.get("protocol"))
    return VerifyingKey(js["curve"], js["log_n"], js["n_public"], int(js["k1"], 0), int(js["k2"], 0),
                        [point_from_json(js["commitments"][name], js["curve"]) for name in FIXED_NAMES], kzg)


def proof_to_json(proof, curve):
    out = {"protocol": "plonk-shplonk", "curve": curve}
    out.update({name: point_to_json(proof[name], curve) for name in POINT_NAMES})
    out["values"] = [str(v) for v in proof["values"]]
    return json.dumps(out, indent=1) + "\n"


def proof_from_json(text, curve):
    js = json.loads(text)
    if js.get("protocol") != "plonk-shplonk" or js.get("curve") != curve:
        raise ZkError('plonk: not a proof of this prover on %s (protocol "%s", curve "%s")' % (curve, js.get("protocol"), js.get("curve")))
    proof = {name: point_from_json(js[name], curve) for name in POINT_NAMES}
    proof["values"] = [int(v, 0) for v in js["values"]]
    return proof


def proof_to_bytes(proof):
    """A || B || C || Z || T || the 14 values, 32 little-endian bytes each || W1 || W2"""
    return b"".join(bytes(proof[k]) for k in POINT_NAMES[:5]) + b"".join(_le(v) for v in proof["values"]) + bytes(proof["W1"]) + bytes(proof["W2"])


def proof_from_bytes(data, point_bytes):
    if len(data) != 7 * point_bytes + 32 * N_VALUES:
        raise ZkError("plonk: a proof is %d bytes, not %d" % (7 * point_bytes + 32 * N_VALUES, len(data)))
    pts = [data[i * point_bytes:(i + 1) * point_bytes] for i in range(5)]
    at = 5 * point_bytes
    vals = [int.from_bytes(data[at + 32 * i:at + 32 * (i + 1)], "little") for i in range(N_VALUES)]
    at += 32 * N_VALUES
    proof = dict(zip(POINT_NAMES[:5], pts))
    proof.update(values=vals, W1=data[at:at + point_bytes], W2=data[at + point_bytes:])
    return proof


class PlonkKey:
    """The proving key on the device, rebuilt from the circuit and the file (there is no proving-key file): the coefficients of the 8 fixed
    polynomials, their values on the coset 7 H_4n, the values of L_1 and of X there, the 8 commitments; beside them what rounds 1 and 2 read on
    H (the selectors' values, the labels of the positions and of sigma).  Setup is deterministic and has no secret.  self.vk is the
    verification key."""

    def __init__(self, kzg, circuit):
        cv, n, k = circuit.curve, circuit.n, circuit.log_n
        if kzg.curve != cv:
            raise ZkError("plonk: the circuit is over %s, the file over %s" % (cv, kzg.curve))
        if kzg.max_coeffs < required_powers(n):
            raise ZkError("plonk: the file holds %d G1 powers, n = %d rows need 3n + 6 = %d (a file of power %d has them)" % (kzg.max_coeffs, n, required_powers(n), k + 1))
        self.kzg, self.circuit, self.curve, self.n, self.log_n = kzg, circuit, cv, n, k
        self.k1, self.k2 = coset_ks(cv, k)
        self._bufs = []
        try:
            self._build()
        except Exception:
            self.free()
            raise

    def _keep(self, d):
        self._bufs.append(d)
        return d

    def _build(self):
        cv, n, k, c = self.curve, self.n, self.log_n, self.circuit
        w = omega(cv, k)
        self.sel_vals = [self._keep(_mont_dev(cv, c.sel[s])) for s in SELECTORS]
        # the labels of the 3n positions, then those of sigma by one gather
        self.labels = self._keep(DevArray(12 * n))
        for j, kj in enumerate((1, self.k1, self.k2)):
            _powers_into(cv, w, kj, n, self.labels.ptr + 32 * j * n)
        self.sigma_vals = self._keep(gather(self.labels, c.sigma(), cv))
        vals = self.sel_vals + [_View(self.sigma_vals, j * n, n) for j in range(3)]
        self.coef = [self._keep(_interpolate(cv, v, n, 0, k)) for v in vals]
        self.coset = [self._keep(_coset_evals(cv, d, n, k + 2)) for d in self.coef]
        l1 = DevArray(4 * n, zero=True)
        try:
            _upload_mont(cv, [1], l1.ptr)
            _ntt(cv, l1.ptr, k, inverse=True)
            self.l1_coset = self._keep(_coset_evals(cv, l1, n, k + 2))
        finally:
            l1.free()
        self.x_coset = self._keep(DevArray(16 * n))
        _powers_into(cv, omega(cv, k + 2), 7, 4 * n, self.x_coset.ptr)
        self.commitments = [self.kzg.commit(d) for d in self.coef]
        self.vk = VerifyingKey(cv, k, c.n_public, self.k1, self.k2, self.commitments, self.kzg)

    def free(self):
        for d in self._bufs:
            d.free()
        self._bufs = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def setup(kzg, circuit):
    """-> PlonkKey(kzg, circuit); its .vk is the verification key"""
    return PlonkKey(kzg, circuit)


# ---- the prover -----------------------------------------------------------------------------------------------------------------------------
def prove(key, witness, blinding=None, self_check=True, _wires=None, _opening_transcript=None, _mark=None):
    """-> (proof, publics).  witness: n_vars values below r (integers, 32-byte little-endian values, or (n_vars, 4) u64 words); on a key whose
    circuit is an R1csCircuit the n_wires values of the .wtns in one of those forms, or the bytes of the .wtns: the auxiliaries are then made
    on the device (extend_witness) and a failing gate is named as the file's gate g (row l + g) with the constraint it came from.  proof is a
    mapping with A, B, C, Z, T, W1, W2 (points, point_bytes each) and values (14 integers: q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3,
    a, b, c, t at zeta, Z at zeta and at zeta w); publics the l public inputs.  The gate equation is checked first, row by row, and a witness
    that fails names the first row; the permutation product must close.  Before returning, the proof is verified (self_check=False skips it).
    blinding: nine integers, FOR TESTS ONLY.  _wires, _opening_transcript, _mark: hooks of the tests and of tools/plonk_time.py."""
    cv, n, k, c, kzg = key.curve, key.n, key.log_n, key.circuit, key.kzg
    r = _FR[cv]
    mark = _mark or (lambda name: None)
    from_r1cs = isinstance(c, R1csCircuit) and _wires is None
    if from_r1cs:
        ww = _r1cs_witness_words(c, witness)
    else:
        ww = _canon_words(witness, r, "witness value")
        if len(ww) != c.n_vars:
            raise ZkError("plonk: the witness has %d values, the circuit has %d variables" % (len(ww), c.n_vars))
    if blinding is None:
        bs = [secrets.randbelow(r) for _ in range(9)]
    else:
        bs = [int(b) for b in blinding]
        if len(bs) != 9 or not all(0 <= b < r for b in bs):
            raise ZkError("plonk: blinding takes nine integers below the scalar field's modulus")
    publics = [_int_of(ww[v]) for v in c.public]
    w_n, w_4n = omega(cv, k), omega(cv, k + 2)
    own = []

    def keep(d):
        own.append(d)
        return d
    try:
        mark("start")
        # the wire values on H
        if _wires is not None:
            vals = [keep(DevArray.from_host(to_mont(col, cv).reshape(-1))) for col in _wires]
            if len(vals) != 3 or any(v.n != 4 * n for v in vals):
                raise ZkError("plonk: _wires takes three columns of n values")
        else:
            d_w = keep(_extend_words(c, ww) if from_r1cs else _mont_dev(cv, ww))
            vals = [keep(gather(d_w, c.wire[x], cv)) for x in WIRES]
        pi_vals = keep(DevArray(4 * n, zero=True))
        if publics:
            _upload_mont(cv, [(-x) % r for x in publics], pi_vals.ptr)
        bad, first = gate_check(vals + key.sel_vals + [pi_vals], n, cv)
        if bad and from_r1cs and first >= c.n_public:
            g = first - c.n_public
            raise ZkError("plonk: witness does not satisfy gate %d (constraint %d of the .r1cs) (%d rows)" % (g, int(c.origin[g]), bad))
        if bad:
            raise ZkError("plonk: witness does not satisfy gate %d (%d rows)" % (first, bad))
        mark("gate check")
        # round 1
        coef = [keep(_interpolate(cv, v, n, 2, k)) for v in vals]
        for j, d in enumerate(coef):
            _blind(cv, d, n, [bs[2 * j + 1], bs[2 * j]])
        A, B, Cc = [kzg.commit(d) for d in coef]
        c0 = transcript_start(cv, key.vk.digest, publics)
        c1, beta, gamma = transcript_wires(cv, c0, A, B, Cc)
        mark("round 1")
        # round 2
        labels = [_View(key.labels, j * n, n) for j in range(3)]
        sigmas = [_View(key.sigma_vals, j * n, n) for j in range(3)]
        num = keep(fp.terms(vals, labels, beta, gamma, cv, dev=True))
        den = keep(fp.terms(vals, sigmas, beta, gamma, cv, dev=True))
        z_vals, last = fp.grand_product(num, den, cv)
        keep(z_vals)
        if last != 1:
            raise ZkError("plonk: the permutation product does not close (z_n = %d): the wire values break a copy constraint" % last)
        z_coef = keep(_interpolate(cv, z_vals, n, 3, k))
        _blind(cv, z_coef, n, [bs[8], bs[7], bs[6]])
        Z = kzg.commit(z_coef)
        c2, alpha = transcript_product(cv, c1, Z)
        mark("round 2")
        # round 3
        pi_coef = keep(_interpolate(cv, pi_vals, n, 0, k))
        cols = [keep(_coset_evals(cv, d, n + 2, k + 2)) for d in coef] + [keep(_coset_evals(cv, z_coef, n + 3, k + 2))] + key.coset
        cols += [keep(_coset_evals(cv, pi_coef, n, k + 2)), key.l1_coset, key.x_coset]
        t = keep(quotient(cols, k, alpha, beta, gamma, key.k1, key.k2, cv))
        _check(_fn(cv, "divide_zh_coset")(t.ptr, k + 2, k, 0))
        _ntt(cv, t.ptr, k + 2, inverse=True, coset=True)
        n_t = required_powers(n)
        high = 4 * n - n_t                                          # the zeros batch_inverse counts: a composition, no kernel of its own
        scratch = keep(DevArray(4 * high))
        _, zeros, _ = fp.batch_inverse(_View(t, n_t, high), cv, out=scratch)
        if zeros != high:
            raise ZkError("plonk: the quotient has %d non-zero coefficients from 3n + 6 = %d on: the identity does not hold on H" % (high - zeros, n_t))
        t_view = _View(t, 0, n_t)
        T = kzg.commit(t_view)
        c3, zeta = transcript_quotient(cv, c2, T, n)
        mark("round 3")
        # rounds 4 and 5
        state = {}

        def opening_gamma(curve, commitments, sets, values):
            state["c4"], g = transcript_values(curve, c3, [y for ys in values for y in ys])
            return g

        def opening_z(curve, g, W1, avoid=()):
            return transcript_z(curve, state["c4"], W1, avoid)
        polys = key.coef + [_View(d, 0, n + 2) for d in coef] + [t_view, _View(z_coef, 0, n + 3)]
        sets = [[zeta]] * 12 + [[zeta, zeta * w_n % r]]
        values, W1, W2, _, _ = kzg.open_multi(polys, sets, transcript=_opening_transcript or opening_gamma, transcript_z=opening_z if _opening_transcript is None else _plain_z,
                                              commitments=key.commitments + [A, B, Cc, T, Z])
        mark("round 5")
        proof = {"A": A, "B": B, "C": Cc, "Z": Z, "T": T, "values": [y for ys in values for y in ys], "W1": W1, "W2": W2}
    finally:
        for d in own:
            d.free()
    if self_check:
        verdict, _ = verify(key.vk, [publics], [proof])
        if verdict != ACCEPTED:
            raise ZkError("plonk: the proof just made is not accepted (verdict %d)" % verdict)
    return proof, publics


def _plain_z(curve, gamma, W1, avoid=()):
    from .kzg import challenge_z
    return challenge_z(curve, gamma, W1, avoid=avoid)


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------------
def challenges(vk, publics, proof):
    """every challenge of a proof from the verification key, the public inputs and the proof's own points and values -> a mapping with beta,
    gamma, alpha, zeta, gamma_open (gamma') and z_open (z')"""
    cv, r = vk.curve, _FR[vk.curve]
    c0 = transcript_start(cv, vk.digest, publics)
    c1, beta, gamma = transcript_wires(cv, c0, proof["A"], proof["B"], proof["C"])
    c2, alpha = transcript_product(cv, c1, proof["Z"])
    c3, zeta = transcript_quotient(cv, c2, proof["T"], vk.n)
    c4, g = transcript_values(cv, c3, proof["values"])
    zw = zeta * omega(cv, vk.log_n) % r
    return {"beta": beta, "gamma": gamma, "alpha": alpha, "zeta": zeta, "gamma_open": g, "z_open": transcript_z(cv, c4, proof["W1"], (zeta, zw))}


def public_input_at(curve, log_n, publics, zeta):
    """PI(zeta) = -sum_i x_i L_i(zeta), L_i(zeta) = w^i (zeta^n - 1) / (n (zeta - w^i)); zeta is outside H"""
    r, n, w = _FR[curve], 1 << log_n, omega(curve, log_n)
    zh = (pow(zeta, n, r) - 1) % r
    acc, wi = 0, 1
    for x in publics:
        acc = (acc + x * wi % r * pow(n * (zeta - wi) % r, -1, r)) % r
        wi = wi * w % r
    return -acc * zh % r


def identity_holds(curve, log_n, k1, k2, publics, values, ch):
    """the identity of round 3 at zeta in the field, from the 14 values: the bracket equals t(zeta) Z_H(zeta)"""
    r, n = _FR[curve], 1 << log_n
    ql, qr, qo, qm, qc, s1, s2, s3, a, b, c, t, z, zw = values
    beta, gamma, alpha, zeta = ch["beta"], ch["gamma"], ch["alpha"], ch["zeta"]
    zh = (pow(zeta, n, r) - 1) % r
    l1 = zh * pow(n * (zeta - 1) % r, -1, r) % r
    gate = (a * b % r * qm + a * ql + b * qr + c * qo + qc + public_input_at(curve, log_n, publics, zeta)) % r
    p1 = (a + beta * zeta + gamma) * (b + beta * k1 % r * zeta + gamma) % r * (c + beta * k2 % r * zeta + gamma) % r * z % r
    p2 = (a + beta * s1 + gamma) * (b + beta * s2 + gamma) % r * (c + beta * s3 + gamma) % r * zw % r
    return (gate + alpha * (p1 - p2) + alpha * alpha % r * l1 % r * (z - 1) - t * zh) % r == 0


def host_check(vk, publics, proof, point_bytes=None):
    """what the verifier decides on the host, before any device work: lengths (an error), every scalar below r (else INPUT_NOT_CANONICAL),
    the challenges, the identity (else REJECTED) -> (verdict, the tuple Kzg.verify_multi takes, built with the verifier's OWN gamma' and z')"""
    cv, r = vk.curve, _FR[vk.curve]
    missing = [k for k in POINT_NAMES + ("values",) if k not in proof]
    if missing:
        raise ZkError("plonk: the proof holds no %s" % ", ".join(missing))
    if len(proof["values"]) != N_VALUES:
        raise ZkError("plonk: a proof holds %d values, not %d" % (N_VALUES, len(proof["values"])))
    pb = point_bytes if point_bytes is not None else len(vk.commitments[0])
    for name in POINT_NAMES:
        if len(proof[name]) != pb:
            raise ZkError("plonk: point %s of the proof is %d bytes, not %d" % (name, len(proof[name]), pb))
    if len(publics) != vk.n_public:
        raise ZkError("plonk: %d public inputs, the verification key has %d" % (len(publics), vk.n_public))
    values, publics = [int(v) for v in proof["values"]], [int(x) for x in publics]
    if not all(0 <= v < r for v in values + publics):
        return INPUT_NOT_CANONICAL, None
    ch = challenges(vk, publics, proof)
    if not identity_holds(cv, vk.log_n, vk.k1, vk.k2, publics, values, ch):
        return REJECTED, None
    zeta = ch["zeta"]
    sets = [[zeta]] * 12 + [[zeta, zeta * omega(cv, vk.log_n) % r]]
    vals = [[v] for v in values[:12]] + [values[12:]]
    cs = vk.commitments + [proof["A"], proof["B"], proof["C"], proof["T"], proof["Z"]]
    return ACCEPTED, (cs, sets, vals, ch["gamma_open"], ch["z_open"], proof["W1"], proof["W2"])


def verify(vk, publics, proofs, kzg=None, seed=None, locate=True):
    """m proofs under one verification key: publics[i] are proof i's public inputs -> (verdict, first_bad) as Kzg.verify_multi gives them.
    The host part of every proof first (host_check), then ONE randomised pairing check of all of them: two pairings.  kzg: the handle to pair
    with, when the key does not carry one.  seed: 32 bytes for the weights, FOR TESTS ONLY."""
    kzg = kzg if kzg is not None else vk.kzg
    if kzg is None:
        raise ZkError("plonk: verify needs the Kzg handle of the file (kzg=), this verification key carries none")
    if kzg.curve != vk.curve:
        raise ZkError("plonk: the verification key is over %s, the file over %s" % (vk.curve, kzg.curve))
    if len(publics) != len(proofs):
        raise ZkError("plonk: %d lists of public inputs for %d proofs" % (len(publics), len(proofs)))
    tuples, bad = [], None
    for i, (x, p) in enumerate(zip(publics, proofs)):
        verdict, tup = host_check(vk, x, p, kzg.point_bytes)
        if verdict != ACCEPTED:
            bad = (verdict, i)
            break
        tuples.append(tup)
    if bad is None:
        return kzg.verify_multi(tuples, seed=seed, locate=locate)
    if not locate:
        return REJECTED, None
    if tuples:                                                      # a proof before the one the host refused may fail the pairing check
        verdict, first = kzg.verify_multi(tuples, seed=seed, locate=True)
        if verdict != ACCEPTED:
            return verdict, first
    return bad
