"""PLONK's arithmetisation, once, under the provers that share it: plonk.py and fflonk.py.  This is the
LAYER: the field and the domain on the host, canonical words, the transcript's primitives, the gate table (Circuit, R1csCircuit) and the
witness path, the device helpers composed from frpoly.py and zk_fr_<curve>_*_dev, the part of a proving key that is the circuit's alone
(ArithKey), the prover's steps up to Z and the division by Z_H, the identity's terms at a point, and what the two verifiers and proof codecs
have in common.  A PROTOCOL is what a prover's docstring states beyond that: its transcript's domain strings and rounds, what it commits to
and opens, its key and proof files.  Nothing here knows which protocol calls it; `who` is the caller's name in front of its messages.

Field Fr of BN128 or BLS12381.  n = 2^k >= 8 rows, H = <w> with the w of zk_fr_<curve>_ntt_dev, w = 7^((r - 1) / n).  Row i must satisfy
qL a + qR b + qO c + qM a b + qC + PI_i = 0; one row per public input in front (qL = 1, a = public[i]), PI_i = -x_i for i < l and 0 otherwise.
Position (column j, row i) has the label k_j w^i with k_0 = 1 and (k_1, k_2) = coset_ks; sigma maps each position to the next one of the same
variable, cyclically in (column, row) order.  A transcript's H is SHA-256; a digest is read as a big-endian integer and reduced mod r; a scalar
is 32 little-endian bytes; a counter is one byte that starts at 0 and only moves for a re-draw."""
import ctypes as C
import hashlib
import json
import secrets

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import frpoly as fp
from .groth16 import _FR as FR, _NAME
from .kzg import _scalar, _words, challenge_z, point_from_json, point_to_json, to_mont

ACCEPTED, REJECTED, INPUT_NOT_CANONICAL = 1, 0, -1
TWO_ADICITY = {"BN128": 28, "BLS12381": 32}
SELECTORS = ("qL", "qR", "qO", "qM", "qC")
WIRES = ("a", "b", "c")
FIXED_NAMES = SELECTORS + ("S1", "S2", "S3")
M64 = (1 << 64) - 1


# ---- the field on the host: only what setup's integers and the verifiers need ---------------------------------------------------------------
def modulus(curve):
    if curve not in FR:
        raise ZkError('plonk: unknown curve "%s" (BN128 | BLS12381)' % curve)
    return FR[curve]


def omega(curve, log_n):
    """the generator of the 2^log_n-point domain of zk_fr_<curve>_ntt_dev: 7^((r - 1) / 2^log_n)"""
    r = modulus(curve)
    if log_n > TWO_ADICITY[curve]:
        raise ZkError("plonk: a domain of 2^%d exceeds the field's 2-adicity (%d)" % (log_n, TWO_ADICITY[curve]))
    return pow(7, (r - 1) >> log_n, r)


def coset_ks(curve, log_n):
    """(k_1, k_2): the smallest integers >= 2 with k_1 < k_2, k_1^n != 1, k_2^n != 1 and (k_2 / k_1)^n != 1, n = 2^log_n: H, k_1 H and k_2 H
    are disjoint"""
    r, n = modulus(curve), 1 << log_n
    k1 = 2
    while pow(k1, n, r) == 1:
        k1 += 1
    k2 = k1 + 1
    while pow(k2, n, r) == 1 or pow(k2 * pow(k1, -1, r) % r, n, r) == 1:
        k2 += 1
    return k1, k2


def check_size(curve, log_n):
    """n = 2^log_n rows need the coset of 4n points"""
    modulus(curve)
    if log_n + 2 > TWO_ADICITY[curve]:
        raise ZkError("plonk: n = 2^%d rows need a coset of 2^%d points, the field's 2-adicity is %d" % (log_n, log_n + 2, TWO_ADICITY[curve]))


def smallest_power(n_powers):
    """the smallest power of a .ptau file that holds n_powers G1 powers: a file of power p has 2^(p + 1) - 1"""
    p = 0
    while (2 << p) - 1 < n_powers:
        p += 1
    return p


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


def canon_words(values, r, what):
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


def int_of(words_row):
    return int.from_bytes(np.ascontiguousarray(words_row, dtype="<u8").tobytes(), "little")


# ---- the transcript's primitives ------------------------------------------------------------------------------------------------------------
def le(v):
    return int(v).to_bytes(32, "little")


def draw(curve, *parts):
    return int.from_bytes(hashlib.sha256(b"".join(parts)).digest(), "big") % FR[curve]


def draw_until(curve, prefix, ok, what):
    """H(prefix || ctr), ctr one byte from 0, drawn again while ok(value) is false; `what`: the caller's words for running out"""
    for ctr in range(256):
        v = draw(curve, prefix, bytes([ctr]))
        if ok(v):
            return v
    raise ZkError("%s after 256 draws" % what)


def plain_z(curve, gamma, W1, avoid=()):
    """the KZG layer's own z', for a prover run under a caller's opening transcript"""
    return challenge_z(curve, gamma, W1, avoid=avoid)


# ---- circuits -------------------------------------------------------------------------------------------------------------------------------
class Circuit:
    """A gate table.  gates: a mapping with qL, qR, qO, qM, qC (integers below r, or (m, 4) u64 canonical words) and a, b, c (variable ids) of
    one length m; public: l variable ids.  The class puts the l public rows in front and pads to n = 2^k >= 8 rows: self.sel[name] is (n, 4)
    u64, self.wire[name] n u32.  min_rows: n holds at least this many rows as well (a protocol whose circuit carries a table of that many).
    Everything here is host integers: no device work."""

    def __init__(self, n_vars, public, gates, curve="BN128", min_rows=0):
        r = modulus(curve)
        self.curve, self.n_vars = curve, int(n_vars)
        self.public = [int(v) for v in public]
        if self.n_vars < 1:
            raise ZkError("plonk: a circuit has at least one variable (padding rows sit on variable 0)")
        raw_sel = {s: canon_words(gates[s], r, "selector %s of gate" % s) for s in SELECTORS}
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
        self.log_n = max(3, (max(rows, int(min_rows)) - 1).bit_length())
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
            if "qN" in z and not getattr(cls, "has_next", False):
                raise ZkError("plonk: %s holds a next-row selector qN: it is a circuit of plonk_next.py" % path)
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

    _NEW = "r1cs_new"                                                 # the call that compiles: a subclass under another rule names its own

    def _more_gates(self, gates, m):
        """further columns of the m gates, for a subclass whose rule emits them"""

    def __init__(self, r1cs_bytes, curve="BN128"):
        modulus(curve)
        self.curve, self._h = curve, None
        data = np.frombuffer(bytes(r1cs_bytes), dtype=np.uint8)
        self._h = getattr(lib(), "zk_plonk_%s_%s" % (_NAME[curve], self._NEW))(data.ctypes.data, data.size)
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
            self._more_gates(gates, m)
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
class View(DevArray):
    """n elements of another DevArray from element `off` on; it owns nothing"""

    def __init__(self, base, off, n):
        self.ptr, self.n, self._base = base.ptr + 32 * int(off), 4 * int(n), base

    def free(self):
        pass


def fr_fn(curve, name):
    return getattr(lib(), "zk_fr_%s_%s_dev" % (_NAME[curve], name))


def ntt(curve, ptr, log_n, inverse=False, coset=False):
    _check(fr_fn(curve, "ntt")(ptr, int(log_n), int(inverse), int(coset), 0))


def add_into(curve, src_ptr, dst_ptr, n):
    """dst[i] += src[i], i < n (canonical, so a zeroed destination receives a copy)"""
    if n:
        _check(fr_fn(curve, "pointwise")(fp.ADD, src_ptr, dst_ptr, dst_ptr, int(n), 0))


def powers_into(curve, base, scale, n, ptr):
    _check(fr_fn(curve, "powers")(_ptr(_scalar(base, curve, "base")), _ptr(_scalar(scale, curve, "scale")), int(n), ptr, 0))


def gather(src, idx, curve="BN128", out=None):
    """out[i] = src[idx[i]] on the device (zk_fr_<curve>_gather_dev): src a DevArray of elements; idx integers, checked here on the host (with
    the indices already on the device use gather_dev, where a bad index is counted by the kernel and comes back as the library's error)
    -> a DevArray of len(idx) elements"""
    modulus(curve)
    n_src = src.n // 4
    ix = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    bad = np.nonzero((ix < 0) | (ix >= n_src))[0]
    if bad.size:
        raise ZkError("plonk: gather: index %d at position %d is not below the source's %d elements" % (int(ix[bad[0]]), int(bad[0]), n_src))
    d_idx = upload_indices(ix)
    try:
        return gather_dev(src, d_idx, len(ix), curve, out)
    finally:
        d_idx.free()


def upload_indices(ix):
    a = np.zeros((len(ix) + 1) // 2 * 2 or 2, np.uint32)
    a[:len(ix)] = ix
    return DevArray.from_host(a.view(np.uint64))


def gather_dev(src, d_idx, n, curve="BN128", out=None):
    """the same with the n u32 indices already on the device"""
    d_out = out if out is not None else DevArray(4 * max(int(n), 1))
    try:
        _check(fr_fn(curve, "gather")(src.ptr, src.n // 4, d_idx.ptr, int(n), d_out.ptr, 0))
        return d_out
    except Exception:
        if out is None:
            d_out.free()
        raise


def mont_dev(curve, words):
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
            powers_into(curve, 1, (1 << 256) % FR[curve], n, d_r2.ptr)
            _check(fr_fn(curve, "pointwise")(fp.MUL, ptr, d_r2.ptr, ptr, n, 0))
        finally:
            d_r2.free()


def r1cs_witness_words(circuit, witness):
    """what prove() and extend_witness() take for an R1csCircuit -> (n_wires, 4) u64 canonical words; every refusal on the host: the bytes of
    a .wtns over another field, a wrong count, a value that is not below r, wire 0 that is not the constant 1"""
    cv = circuit.curve
    if isinstance(witness, (bytes, bytearray, memoryview)) and bytes(witness[:4]) == b"wtns":
        from .r1cs import wtns_payload
        witness, _ = wtns_payload(bytes(witness), cv)
    ww = canon_words(witness, FR[cv], "witness value")
    if len(ww) != circuit.n_wires:
        raise ZkError("plonk: the witness has %d values, the .r1cs has %d wires" % (len(ww), circuit.n_wires))
    if int_of(ww[0]) != 1:
        raise ZkError("plonk: witness value 0 is %d: wire 0 of a circom witness is the constant 1" % int_of(ww[0]))
    return ww


def extend_words(circuit, ww):
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
    return extend_words(circuit, r1cs_witness_words(circuit, witness))


def upload_mont(curve, values, ptr):
    """a few integers -> Montgomery words at a device address"""
    a = to_mont(values, curve).reshape(-1)
    _check(lib().zk_dev_upload(ptr, _ptr(a), a.size * 8))


def blind(curve, coef, n, bs):
    """coef += (sum_k bs[k] X^k) (X^n - 1): -bs[k] into coefficient k, bs[k] into coefficient n + k (zero until now)"""
    r = FR[curve]
    if not any(bs):
        return
    low = DevArray.from_host(to_mont([(-b) % r for b in bs], curve).reshape(-1))
    try:
        add_into(curve, low.ptr, coef.ptr, len(bs))
    finally:
        low.free()
    upload_mont(curve, bs, coef.ptr + 32 * n)


def coset_evals(curve, coef, n_coef, log_m):
    """the values on 7 H_m of the polynomial whose n_coef coefficients start at coef.ptr -> a new DevArray of m elements"""
    d = DevArray(4 << log_m, zero=True)
    try:
        add_into(curve, coef.ptr, d.ptr, n_coef)
        ntt(curve, d.ptr, log_m, coset=True)
        return d
    except Exception:
        d.free()
        raise


def interpolate(curve, vals, n, extra, log_n):
    """the values on H -> a new DevArray of n + extra coefficients, the top `extra` zero"""
    d = DevArray(4 * (n + extra), zero=True)
    try:
        add_into(curve, vals.ptr, d.ptr, n)
        ntt(curve, d.ptr, log_n, inverse=True)
        return d
    except Exception:
        d.free()
        raise


def gate_check(cols, n, curve="BN128"):
    """zk_plonk_<curve>_gate_check_dev: cols, 9 DevArrays of n elements (a, b, c, qL, qR, qO, qM, qC, PI) -> (rows that fail, the first or None)"""
    modulus(curve)
    if len(cols) != 9:
        raise ZkError("plonk: the gate check takes 9 columns, not %d" % len(cols))
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    bad, first = C.c_uint64(0), C.c_uint64(0)
    _check(getattr(lib(), "zk_plonk_%s_gate_check_dev" % _NAME[curve])(_ptr(ptrs), int(n), C.byref(bad), C.byref(first), 0))
    return int(bad.value), (None if bad.value == 0 else int(first.value))


# ---- the part of a proving key that is the circuit's alone ----------------------------------------------------------------------------------
class ArithKey:
    """What both provers keep on the device, rebuilt from the circuit and the file (there is no proving-key file): what rounds 1 and 2 read on
    H (the selectors' values, the labels of the positions and of sigma), the values of the 8 fixed polynomials, of L_1 and of X on the coset
    7 H_4n.  The coefficients of the 8 fixed polynomials go to _fixed(), which a protocol writes: with KEEPS_COEF they stay the key's, without
    it they are freed as soon as _fixed() returns.  required: (the formula in words, the G1 powers the file must hold)."""
    KEEPS_COEF = True
    TAKES_NEXT = False                                                # plonk_next.py's key: the one that reads a circuit's next-row selector

    def __init__(self, kzg, circuit, who, required):
        cv, n, k = circuit.curve, circuit.n, circuit.log_n
        if getattr(circuit, "has_next", False) and not self.TAKES_NEXT:
            raise ZkError("%s: the circuit has a next-row selector qN, which this prover does not read: prove it with plonk_next.py" % who)
        if kzg.curve != cv:
            raise ZkError("%s: the circuit is over %s, the file over %s" % (who, cv, kzg.curve))
        if kzg.max_coeffs < required[1]:
            raise ZkError("%s: the file holds %d G1 powers, n = %d rows need %s = %d (a file of power %d has them)" % (who, kzg.max_coeffs, n, *required, smallest_power(required[1])))
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
        self.sel_vals = [self._keep(mont_dev(cv, c.sel[s])) for s in SELECTORS]
        # the labels of the 3n positions, then those of sigma by one gather
        self.labels = self._keep(DevArray(12 * n))
        for j, kj in enumerate((1, self.k1, self.k2)):
            powers_into(cv, w, kj, n, self.labels.ptr + 32 * j * n)
        self.sigma_vals = self._keep(gather(self.labels, c.sigma(), cv))
        coef, loose = [], []
        try:
            for v in self.sel_vals + [View(self.sigma_vals, j * n, n) for j in range(3)]:
                coef.append(interpolate(cv, v, n, 0, k))
                (self._bufs if self.KEEPS_COEF else loose).append(coef[-1])
            self.coset = [self._keep(coset_evals(cv, d, n, k + 2)) for d in coef]
            self._fixed(coef)
        finally:
            for d in loose:
                d.free()
        l1 = DevArray(4 * n, zero=True)
        try:
            upload_mont(cv, [1], l1.ptr)
            ntt(cv, l1.ptr, k, inverse=True)
            self.l1_coset = self._keep(coset_evals(cv, l1, n, k + 2))
        finally:
            l1.free()
        self.x_coset = self._keep(DevArray(16 * n))
        powers_into(cv, omega(cv, k + 2), 7, 4 * n, self.x_coset.ptr)

    def free(self):
        for d in self._bufs:
            d.free()
        self._bufs = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- the prover's steps that are no protocol's ----------------------------------------------------------------------------------------------
COUNT_WORDS = {9: "nine", 10: "ten", 14: "fourteen"}


def witness_columns(key, witness, blinding, _wires, who, keep, mark=lambda name: None, n_blinders=9, check=None):
    """what prove() takes -> (the three value columns on H, PI's values, the public inputs, the nine blinders; n_blinders of them for a
    protocol that blinds more polynomials).  Every refusal of the witness and of the blinders on the host first; then, between the marks
    "start" and "gate check", the columns gathered from the witness (on an R1csCircuit from the extended one) and the gate equation row by
    row: a witness that fails names the first row.  check(vals, pi_vals) -> (rows that fail, the first): a protocol's own gate equation in
    place of gate_check."""
    cv, n, c = key.curve, key.n, key.circuit
    r = FR[cv]
    from_r1cs = isinstance(c, R1csCircuit) and _wires is None
    if from_r1cs:
        ww = r1cs_witness_words(c, witness)
    else:
        ww = canon_words(witness, r, "witness value")
        if len(ww) != c.n_vars:
            raise ZkError("%s: the witness has %d values, the circuit has %d variables" % (who, len(ww), c.n_vars))
    if blinding is None:
        bs = [secrets.randbelow(r) for _ in range(n_blinders)]
    else:
        bs = [int(b) for b in blinding]
        if len(bs) != n_blinders or not all(0 <= b < r for b in bs):
            raise ZkError("%s: blinding takes %s integers below the scalar field's modulus" % (who, COUNT_WORDS.get(n_blinders, str(n_blinders))))
    publics = [int_of(ww[v]) for v in c.public]
    mark("start")
    if _wires is not None:
        vals = [keep(DevArray.from_host(to_mont(col, cv).reshape(-1))) for col in _wires]
        if len(vals) != 3 or any(v.n != 4 * n for v in vals):
            raise ZkError("%s: _wires takes three columns of n values" % who)
    else:
        d_w = keep(extend_words(c, ww) if from_r1cs else mont_dev(cv, ww))
        vals = [keep(gather(d_w, c.wire[x], cv)) for x in WIRES]
    pi_vals = keep(DevArray(4 * n, zero=True))
    if publics:
        upload_mont(cv, [(-x) % r for x in publics], pi_vals.ptr)
    bad, first = check(vals, pi_vals) if check is not None else gate_check(vals + key.sel_vals + [pi_vals], n, cv)
    if bad and from_r1cs and first >= c.n_public:
        g = first - c.n_public
        raise ZkError("%s: witness does not satisfy gate %d (constraint %d of the .r1cs) (%d rows)" % (who, g, int(c.origin[g]), bad))
    if bad:
        raise ZkError("%s: witness does not satisfy gate %d (%d rows)" % (who, first, bad))
    mark("gate check")
    return vals, pi_vals, publics, bs


def blinded_wires(key, vals, bs, keep):
    """a, b, c interpolated and blinded as a += (b_1 X + b_2) Z_H (b: b_3, b_4; c: b_5, b_6) -> three vectors of n + 2 coefficients"""
    coef = [keep(interpolate(key.curve, v, key.n, 2, key.log_n)) for v in vals]
    for j, d in enumerate(coef):
        blind(key.curve, d, key.n, [bs[2 * j + 1], bs[2 * j]])
    return coef


def permutation_product(key, vals, beta, gamma, bs, who, keep):
    """z_0 = 1, z_(i+1) = z_i prod_j (w_j,i + beta k_j w^i + gamma) / prod_j (w_j,i + beta sigma_j,i + gamma), which must close with z_n = 1;
    Z += (b_7 X^2 + b_8 X + b_9) Z_H -> Z's n + 3 coefficients"""
    cv, n = key.curve, key.n
    num = keep(fp.terms(vals, [View(key.labels, j * n, n) for j in range(3)], beta, gamma, cv, dev=True))
    den = keep(fp.terms(vals, [View(key.sigma_vals, j * n, n) for j in range(3)], beta, gamma, cv, dev=True))
    z_vals, last = fp.grand_product(num, den, cv)
    keep(z_vals)
    if last != 1:
        raise ZkError("%s: the permutation product does not close (z_n = %d): the wire values break a copy constraint" % (who, last))
    z_coef = keep(interpolate(cv, z_vals, n, 3, key.log_n))
    blind(cv, z_coef, n, [bs[8], bs[7], bs[6]])
    return z_coef


def quotient_coeffs(cv, k, d, n_coef, message, keep):
    """a numerator's values on the coset 7 H_4n, in place -> the view of the quotient by Z_H's n_coef coefficients; those from n_coef on must
    be zero (batch_inverse's zero count: a composition, no kernel of its own), else ZkError(message % (how many are not, n_coef))"""
    _check(fr_fn(cv, "divide_zh_coset")(d.ptr, k + 2, k, 0))
    ntt(cv, d.ptr, k + 2, inverse=True, coset=True)
    high = (4 << k) - n_coef
    scratch = keep(DevArray(4 * high))
    _, zeros, _ = fp.batch_inverse(View(d, n_coef, high), cv, out=scratch)
    if zeros != high:
        raise ZkError(message % (high - zeros, n_coef))
    return View(d, 0, n_coef)


# ---- the verifiers' common part -------------------------------------------------------------------------------------------------------------
def public_input_at(curve, log_n, publics, zeta):
    """PI(zeta) = -sum_i x_i L_i(zeta), L_i(zeta) = w^i (zeta^n - 1) / (n (zeta - w^i)); zeta is outside H"""
    r, n, w = FR[curve], 1 << log_n, omega(curve, log_n)
    zh = (pow(zeta, n, r) - 1) % r
    acc, wi = 0, 1
    for x in publics:
        acc = (acc + x * wi % r * pow(n * (zeta - wi) % r, -1, r)) % r
        wi = wi * w % r
    return -acc * zh % r


def identity_terms(curve, log_n, k1, k2, publics, x, v, beta, gamma):
    """the identity's terms at a point x outside H, in the field, from the values v[name] there (the FIXED_NAMES, a, b, c, Z, and Zw = Z(x w))
    -> (gate + PI, the permutation difference P1 - P2, L_1 (Z - 1), Z_H), each below r"""
    r, n = FR[curve], 1 << log_n
    a, b, c, z = v["a"], v["b"], v["c"], v["Z"]
    zh = (pow(x, n, r) - 1) % r
    l1 = zh * pow(n * (x - 1) % r, -1, r) % r
    gate = (a * b % r * v["qM"] + a * v["qL"] + b * v["qR"] + c * v["qO"] + v["qC"] + public_input_at(curve, log_n, publics, x)) % r
    p1 = (a + beta * x + gamma) * (b + beta * k1 % r * x + gamma) % r * (c + beta * k2 % r * x + gamma) % r * z % r
    p2 = (a + beta * v["S1"] + gamma) * (b + beta * v["S2"] + gamma) % r * (c + beta * v["S3"] + gamma) % r * v["Zw"] % r
    return gate, (p1 - p2) % r, l1 * (z - 1) % r, zh


def check_proof_shape(proof, point_names, n_values, point_bytes, n_public, publics, r, who):
    """the head of a host_check: what is missing or of the wrong length is an error -> (values, publics) as integers, or None when one of
    them is not below r (INPUT_NOT_CANONICAL)"""
    missing = [k for k in point_names + ("values",) if k not in proof]
    if missing:
        raise ZkError("%s: the proof holds no %s" % (who, ", ".join(missing)))
    if len(proof["values"]) != n_values:
        raise ZkError("%s: a proof holds %d values, not %d" % (who, n_values, len(proof["values"])))
    for name in point_names:
        if len(proof[name]) != point_bytes:
            raise ZkError("%s: point %s of the proof is %d bytes, not %d" % (who, name, len(proof[name]), point_bytes))
    if len(publics) != n_public:
        raise ZkError("%s: %d public inputs, the verification key has %d" % (who, len(publics), n_public))
    values, publics = [int(v) for v in proof["values"]], [int(x) for x in publics]
    return (values, publics) if all(0 <= v < r for v in values + publics) else None


def verify_batch(vk, publics, proofs, host_check, kzg, seed, locate, who):
    """m proofs under one verification key: the host part of every proof first (host_check), then ONE randomised pairing check of all of them
    -> (verdict, first_bad) as Kzg.verify_multi gives them"""
    kzg = kzg if kzg is not None else vk.kzg
    if kzg is None:
        raise ZkError("%s: verify needs the Kzg handle of the file (kzg=), this verification key carries none" % who)
    if kzg.curve != vk.curve:
        raise ZkError("%s: the verification key is over %s, the file over %s" % (who, vk.curve, kzg.curve))
    if len(publics) != len(proofs):
        raise ZkError("%s: %d lists of public inputs for %d proofs" % (who, len(publics), len(proofs)))
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


# ---- the proof codecs: (protocol, point_names) are the caller's -----------------------------------------------------------------------------
def proof_to_json(proof, curve, protocol, point_names):
    out = {"protocol": protocol, "curve": curve}
    out.update({name: point_to_json(proof[name], curve) for name in point_names})
    out["values"] = [str(v) for v in proof["values"]]
    return json.dumps(out, indent=1) + "\n"


def proof_from_json(text, curve, protocol, point_names, who):
    js = json.loads(text)
    if js.get("protocol") != protocol or js.get("curve") != curve:
        raise ZkError('%s: not a proof of this prover on %s (protocol "%s", curve "%s")' % (who, curve, js.get("protocol"), js.get("curve")))
    proof = {name: point_from_json(js[name], curve) for name in point_names}
    proof["values"] = [int(v, 0) for v in js["values"]]
    return proof


def proof_to_bytes(proof, before, after=()):
    """the points named in `before` || the values, 32 little-endian bytes each || the points named in `after`"""
    return b"".join(bytes(proof[k]) for k in before) + b"".join(le(v) for v in proof["values"]) + b"".join(bytes(proof[k]) for k in after)


def proof_from_bytes(data, point_bytes, before, n_values, after, who):
    size = (len(before) + len(after)) * point_bytes + 32 * n_values
    if len(data) != size:
        raise ZkError("%s: a proof is %d bytes, not %d" % (who, size, len(data)))
    at = len(before) * point_bytes
    proof = {name: data[i * point_bytes:(i + 1) * point_bytes] for i, name in enumerate(before)}
    proof["values"] = [int.from_bytes(data[at + 32 * i:at + 32 * (i + 1)], "little") for i in range(n_values)]
    at += 32 * n_values
    proof.update({name: data[at + i * point_bytes:at + (i + 1) * point_bytes] for i, name in enumerate(after)})
    return proof
