"""Host-side mirror of compressor12 exec (recursion/src/compressor12/compressor12_exec.rs:17-103) over libzkgpu's
C ABI: the PlonkAdd sums and the s_map gather run on the device and leave the committed trace in HBM."""
import numpy as np

from . import DevArray, ZkError, _check, lib


class Compressor12Exec:
    def __init__(self, exec_text, n_witness):
        b = exec_text.encode() if isinstance(exec_text, str) else bytes(exec_text)
        self.n_witness = n_witness
        self._h = lib().zk_c12_exec_new(b, len(b), n_witness)
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())
        self.depth = lib().zk_c12_exec_depth(self._h)

    def run(self, witness, n_rows, stream=0):
        """witness: u64 host array or DevArray of n_witness words -> DevArray [n_rows][12] (row-major), the .cm content"""
        d_w = witness if isinstance(witness, DevArray) else DevArray.from_host(np.ascontiguousarray(witness, dtype=np.uint64))
        cm = DevArray(max(n_rows * 12, 1))
        _check(lib().zk_c12_exec_dev(self._h, d_w.ptr, d_w.n, n_rows, cm.ptr, stream))
        return cm

    def free(self):
        if self._h:
            lib().zk_c12_exec_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _text(p):
    import ctypes
    if not p:
        raise ZkError(lib().zk_last_error().decode())
    try:
        return ctypes.string_at(p).decode()
    finally:
        lib().zk_string_free(p)


class Compressor12Setup:
    """`zkit compressor12_setup` (recursion/src/compressor12/{compressor12_setup,plonk_setup}.rs) over libzkgpu: the R1CS
    reader, R1CS -> PLONK and the row packing run on the host when the object is made (no GPU needed for .pil and
    .exec_text); consts() runs the S columns, their wiring and the fill of the [N][n_const] matrix on the device."""

    def __init__(self, handle):
        self._h = handle
        L = lib()
        self.n_bits, self.n_publics, self.n_used = L.zk_c12_setup_n_bits(handle), L.zk_c12_setup_n_publics(handle), L.zk_c12_setup_n_used(handle)
        self.n_const, self.n_gates, self.n_adds = L.zk_c12_setup_n_const(handle), L.zk_c12_setup_n_gates(handle), L.zk_c12_setup_n_adds(handle)

    @classmethod
    def from_r1cs(cls, r1cs, force_n_bits=0):
        b = bytes(r1cs)
        h = lib().zk_c12_setup_new(b, len(b), force_n_bits)
        if not h:
            raise ZkError(lib().zk_last_error().decode())
        return cls(h)

    @property
    def pil(self):
        return _text(lib().zk_c12_setup_pil(self._h))

    @property
    def exec_text(self):
        return _text(lib().zk_c12_setup_exec(self._h))

    def gates(self):
        """[n_gates][8] u64: sl, sr, so, qm, ql, qr, qo, qc (r1cs2plonk.rs:10)"""
        o = np.zeros((self.n_gates, 8), np.uint64)
        if self.n_gates:
            _check(lib().zk_c12_setup_gates(self._h, o.ctypes.data))
        return o

    def consts(self, stream=0):
        """-> DevArray [2^n_bits][n_const] (row-major): the content of the .const file, born in HBM"""
        out = DevArray((1 << self.n_bits) * self.n_const)
        _check(lib().zk_c12_setup_consts_dev(self._h, out.ptr, stream))
        return out

    def consts_host(self):
        o = np.empty((1 << self.n_bits) * self.n_const, np.uint64)
        _check(lib().zk_c12_setup_consts(self._h, o.ctypes.data))
        return o

    def free(self):
        if self._h:
            lib().zk_c12_setup_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sigma(s_map, n_bits, n_const=12, col0=0, out=None, stream=0):
    """The copy-constraint wiring on its own (zk_c12_sigma_dev).  s_map: [n_used][12] wire ids < 2^32 (0 = no wire), the
    .exec order -> DevArray [2^n_bits][n_const] whose columns [col0, col0 + 12) are S; the other columns are left as they
    were (zero when the array is made here)."""
    m = np.ascontiguousarray(s_map, dtype=np.uint32).reshape(-1, 12)
    packed = np.zeros((m.size + 1) // 2, np.uint64)                     # the u32 map in a buffer of whole u64 words
    packed.view(np.uint32)[:m.size] = m.reshape(-1)
    d_map = DevArray.from_host(packed) if m.size else None
    if out is None:
        out = DevArray((1 << n_bits) * n_const, zero=True)
    _check(lib().zk_c12_sigma_dev(d_map.ptr if d_map else None, m.shape[0], n_bits, n_const, col0, out.ptr, stream))
    return out
