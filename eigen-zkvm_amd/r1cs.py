"""wtns_check: a witness against its R1CS on the device (csrc/r1cs_check.hip behind zk_r1cs_check_*) -- what `snarkjs wtns check`
answers, for the scalar fields of BN254 and BLS12-381 ("BN128", "BLS12381": the Groth16 circuits) and for Goldilocks ("GL": the
compressor's circuits, custom gates included).  The report's shape is documented in include/zkgpu.h.  There is no CPU fallback."""
import ctypes as C
import json
import struct

import numpy as np

from . import DevArray, ZkError, _check, lib

FIELDS = {"BN128": (32, 21888242871839275222246405745257275088548364400416034343698204186575808495617),
          "BLS12381": (32, 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001),
          "GL": (8, 0xFFFFFFFF00000001)}


def wtns_payload(wtns_bytes, field):
    """the values of a .wtns file (iden3 binary format: header section 1, values section 2) as bytes, after checking that the file
    is over `field` -> (bytes, n_values)"""
    b = bytes(wtns_bytes)
    size, prime = FIELDS[field]
    if b[:4] != b"wtns" or len(b) < 12:
        raise ZkError("wtns: Invalid file header")
    secs, o = {}, 12
    for _ in range(struct.unpack_from("<I", b, 8)[0]):
        if o + 12 > len(b):
            raise ZkError("wtns: truncated file")
        t, sz = struct.unpack_from("<IQ", b, o); o += 12
        secs[t] = b[o:o + sz]; o += sz
    if 1 not in secs or 2 not in secs or len(secs[1]) < 4:
        raise ZkError("wtns: header or value section missing")
    fs = struct.unpack_from("<I", secs[1])[0]
    if fs != size or len(secs[1]) != 8 + fs or int.from_bytes(secs[1][4:4 + fs], "little") != prime:
        raise ZkError("wtns: the file is not a witness over %s (%d-byte field elements)" % (field, size))
    n = struct.unpack_from("<I", secs[1], 4 + fs)[0]
    if len(secs[2]) != n * size:
        raise ZkError("wtns: Invalid witness section size")
    return secs[2], n


class R1csCheck:
    """One handle per (field, .r1cs): the three matrices resident on the device in CSR form, over "GL" the custom-gate uses too.
    `.info` = {"n_wires", "n_constraints", "n_custom_uses", "n_public"}."""

    def __init__(self, field, r1cs_bytes):
        self.field = field
        r = np.frombuffer(bytes(r1cs_bytes), dtype=np.uint8)
        self._h = lib().zk_r1cs_check_new(field.encode(), r.ctypes.data, r.size)
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())
        w, p, n, u = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().zk_r1cs_check_info(self._h, C.byref(w), C.byref(n), C.byref(u), C.byref(p)))
        self.info = {"n_wires": w.value, "n_constraints": n.value, "n_custom_uses": u.value, "n_public": p.value}
        self.value_bytes = FIELDS[field][0]

    def run(self, witness, max_findings=16, n_values=None):
        """-> the report (dict).  witness: bytes or a numpy buffer of little-endian canonical values (32 B or 8 B each), a list of
        integers, or device memory (a DevArray, or a torch device tensor: its pointer is passed, the values are taken as canonical)"""
        vb = self.value_bytes
        if isinstance(witness, DevArray):
            n = witness.n * 8 // vb if n_values is None else n_values
            p = lib().zk_r1cs_check_run_dev(self._h, witness.ptr, n, max_findings)
        elif hasattr(witness, "data_ptr") and getattr(witness, "is_cuda", False):
            n = witness.numel() * witness.element_size() // vb if n_values is None else n_values
            p = lib().zk_r1cs_check_run_dev(self._h, witness.data_ptr(), n, max_findings)
        else:
            if isinstance(witness, (list, tuple)):
                witness = b"".join(int(v).to_bytes(vb, "little") for v in witness)
            a = np.ascontiguousarray(np.frombuffer(witness, dtype=np.uint8) if isinstance(witness, (bytes, bytearray, memoryview)) else np.asarray(witness)).view(np.uint8).reshape(-1)
            if a.size % vb:
                raise ZkError("R1csCheck.run: the buffer does not hold whole %d-byte values" % vb)
            p = lib().zk_r1cs_check_run(self._h, a.ctypes.data, a.size // vb if n_values is None else n_values, max_findings)
        if not p:
            raise ZkError(lib().zk_last_error().decode())
        try:
            return json.loads(C.string_at(p).decode())
        finally:
            lib().zk_string_free(p)

    def free(self):
        if self._h:
            lib().zk_r1cs_check_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
