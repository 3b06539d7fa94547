"""Host-side mirror of the reference's Groth16 entry points over libzkgpu's C ABI (include/zkgpu.h, "Groth16 around
the multi-scalar sums"): groth16/src/api.rs:144-205 groth16_prove = read the key, read the circuit, read the
witness, create_random_proof, serialize_proof; and api.rs:42-66 groth16_setup = the key itself (keygen).  Everything
after the witness is on the device; there is no CPU fallback."""
import ctypes as C
import json
import secrets

import numpy as np

from . import DevArray, ZkError, _check, _np, _ptr, lib
from .key_check_lines import POINT_CLASSES, contribution_check_line, key_check_line, key_check_skipped_line, key_check_srs_line, srs_check_line  # noqa: F401

_FR = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
       "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
_NAME = {"BN128": "bn254", "BLS12381": "bls12_381"}
_FQ_WORDS = {"BN128": 4, "BLS12381": 6}


def fr_ntt(data, curve="BN128", inverse=False, coset=False):
    """EvaluationDomain::{fft, ifft, coset_fft, icoset_fft} on an n x 4 u64 array of Montgomery Fr limbs (n = 2^k);
    a DevArray is transformed in place, a host array is copied and returned"""
    fn = "zk_fr_%s_ntt" % _NAME[curve]
    if isinstance(data, DevArray):
        n = data.n // 4
        _check(getattr(lib(), fn + "_dev")(data.ptr, n.bit_length() - 1, int(inverse), int(coset), 0)); return data
    a = _np(data).reshape(-1).copy()
    n = a.size // 4
    if n == 0 or n & (n - 1):
        raise ZkError("fr ntt: length must be a power of two")
    _check(getattr(lib(), fn)(_ptr(a), n.bit_length() - 1, int(inverse), int(coset))); return a.reshape(-1, 4)


def fr_quotient(d_a, d_b, d_c, curve="BN128"):
    """create_proof's h block on three DevArrays of 2^k Montgomery Fr elements; d_a is overwritten with the coefficients"""
    n = d_a.n // 4
    _check(getattr(lib(), "zk_fr_%s_quotient_dev" % _NAME[curve])(d_a.ptr, d_b.ptr, d_c.ptr, n.bit_length() - 1, 0)); return d_a


def wtns_values(wtns_bytes, curve="BN128"):
    """load_witness_from_bin_reader (algebraic/src/reader.rs:86-137): the n x 4 u64 canonical values of a .wtns file"""
    off, n = C.c_uint64(0), C.c_uint64(0)
    buf = np.frombuffer(wtns_bytes, dtype=np.uint8)
    _check(lib().zk_groth16_wtns_payload(buf.ctypes.data, buf.size, curve.encode(), C.byref(off), C.byref(n)))
    return np.frombuffer(wtns_bytes, dtype="<u8", count=4 * n.value, offset=off.value).reshape(-1, 4).copy()


class Groth16Setup:
    """The state groth16_prove rebuilds per call (api.rs:161-171), kept resident: proving key as device bases, the
    circuit's three CSR matrices, the density index lists and the transform tables of its domain."""

    def __init__(self, curve, r1cs_bytes, params_bytes):
        if curve not in _FR:
            raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
        self.curve = curve
        r = np.frombuffer(r1cs_bytes, dtype=np.uint8); p = np.frombuffer(params_bytes, dtype=np.uint8)
        self._h = lib().zk_groth16_setup_new(curve.encode(), r.ctypes.data, r.size, p.ctypes.data, p.size)
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().zk_groth16_setup_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.n_wires, self.n_inputs, self.domain_log = a.value, b.value, c.value

    def prove(self, witness, r=None, s=None, d_h=None):
        """witness: n_wires x 4 u64 canonical (host array or DevArray); r, s: blinding scalars (drawn here when None,
        as create_random_proof does).  -> (proof.json dict, points: A || B || C u64 Montgomery words)"""
        mod = _FR[self.curve]
        r = secrets.randbelow(mod) if r is None else r
        s = secrets.randbelow(mod) if s is None else s
        if not (0 <= r < mod and 0 <= s < mod):
            raise ZkError("groth16: r and s must be canonical field elements")
        rw = np.array([(r >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
        sw = np.array([(s >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
        pts = np.zeros(8 * _FQ_WORDS[self.curve], np.uint64)
        if isinstance(witness, DevArray):
            p = lib().zk_groth16_prove_dev(self._h, witness.ptr, witness.n // 4, _ptr(rw), _ptr(sw), _ptr(pts), d_h.ptr if d_h is not None else None)
        else:
            w = _np(witness).reshape(-1)
            p = lib().zk_groth16_prove(self._h, _ptr(w), w.size // 4, _ptr(rw), _ptr(sw), _ptr(pts))
        if not p:
            raise ZkError(lib().zk_last_error().decode())
        try:
            return json.loads(C.string_at(p).decode()), pts
        finally:
            lib().zk_string_free(p)

    def free(self):
        if self._h:
            lib().zk_groth16_setup_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def keygen(curve, r1cs_bytes, trapdoor=None, to_hex=False, timing=None, srs=None, check_srs=True):
    """`zkit groth16_setup` (groth16/src/api.rs:42-66): the circuit-specific key of an .r1cs, made on the device.
    trapdoor: (tau, alpha, beta, gamma, delta) as integers, or None to let the library draw them from the operating system
    (nothing of them survives the call).  -> (bellman Parameters bytes, verification_key.json text); `timing`, a list,
    receives the milliseconds of the transform, the column sums, the G1 points, the G2 points and serialisation.
    srs: an Srs -- the key for (tau, alpha, beta, 1, 1) of that powers-of-tau file instead, made in the group (`timing` then: G1
    transforms, G1 column sums, uploads and h, G2 transform and sums, serialisation).  check_srs: run Srs.check first and make no key from
    a file with findings."""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    if srs is not None and trapdoor is not None:
        raise ZkError("groth16 keygen: a powers-of-tau file and a trapdoor exclude each other")
    td = None
    if trapdoor is not None:
        if len(trapdoor) != 5:
            raise ZkError("groth16 keygen: the trapdoor is (tau, alpha, beta, gamma, delta)")
        td = np.array([[(int(v) % _FR[curve] >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in trapdoor], dtype=np.uint64).reshape(-1)
    r = np.frombuffer(r1cs_bytes, dtype=np.uint8)
    if srs is not None:
        if check_srs:
            found = srs.check()["findings"]
            if found:
                raise ZkError("groth16 setup: the powers-of-tau file fails its check: " + "; ".join(srs_check_line(f) for f in found))
        h = lib().zk_groth16_keygen_from_srs(curve.encode(), r.ctypes.data, r.size, srs._h)
    else:
        h = lib().zk_groth16_keygen_new(curve.encode(), r.ctypes.data, r.size, _ptr(td) if td is not None else None)
    if not h:
        raise ZkError(lib().zk_last_error().decode())
    try:
        n = lib().zk_groth16_keygen_params_size(h)
        buf = np.empty(n, np.uint8)
        _check(lib().zk_groth16_keygen_params(h, buf.ctypes.data, n))
        p = lib().zk_groth16_keygen_vk_json(h, int(bool(to_hex)))
        if not p:
            raise ZkError(lib().zk_last_error().decode())
        try:
            vk = C.string_at(p).decode()
        finally:
            lib().zk_string_free(p)
        if timing is not None:
            ms = (C.c_double * 5)()
            _check(lib().zk_groth16_keygen_timing(h, ms)); timing[:] = list(ms)
        return buf.tobytes(), vk
    finally:
        lib().zk_groth16_keygen_free(h)


def _report(p):
    if not p:
        raise ZkError(lib().zk_last_error().decode())
    try:
        return json.loads(C.string_at(p).decode())
    finally:
        lib().zk_string_free(p)


def _seed(seed, who):
    if seed is not None and len(seed) != 32:
        raise ZkError("%s: the seed is 32 bytes" % who)
    return None if seed is None else np.frombuffer(bytes(seed), dtype=np.uint8)


class Srs:
    """A snarkjs powers-of-tau file (.ptau), opened on the host: sections tauG1, tauG2, alphaTauG1, betaTauG1, betaG2 of the curve's
    points.  `power`: the file serves circuits of up to 2^power rows."""

    def __init__(self, curve, path):
        if curve not in _FR:
            raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
        self.curve = curve
        self._h = lib().zk_srs_open(curve.encode(), str(path).encode())
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())
        a, b = C.c_uint32(0), C.c_uint32(0)
        _check(lib().zk_srs_info(self._h, C.byref(a), C.byref(b)))
        self.power, self.ceremony_power = a.value, b.value

    def check(self, seed=None, max_findings=16):
        """every point's class and the sections' structure (zk_srs_check) -> the report as a dict; seed: 32 bytes, tests only"""
        sd = _seed(seed, "srs check")
        return _report(lib().zk_srs_check(self._h, sd.ctypes.data if sd is not None else None, int(max_findings)))

    def transcript_count(self):
        """the records of the file's transcript of contributions (host only); -1: the file has none"""
        n = C.c_int64(0)
        _check(lib().zk_srs_transcript_count(self._h, C.byref(n)))
        return n.value

    def contribute(self, out_path, secrets=None, beacon=None):
        """zk_srs_contribute: write to out_path this file with tau, alpha, beta multiplied by three factors, and one more record in its
        transcript.  secrets: (t, a, b) integers in [1, r) -- tests only; None lets the library draw them from the operating system and
        nothing of them survives the call.  beacon: (seed of 32 bytes, iter_log) for a contribution whose factors anyone can recompute."""
        if secrets is not None and beacon is not None:
            raise ZkError("ptau contribute: a beacon takes no secrets")
        sw = sd = None
        it = 0
        if secrets is not None:
            if len(secrets) != 3 or not all(0 < int(v) < _FR[self.curve] for v in secrets):
                raise ZkError("ptau contribute: three factors in [1, r)")
            sw = np.array([(int(v) >> (64 * i)) & (2**64 - 1) for v in secrets for i in range(4)], dtype=np.uint64)
        if beacon is not None:
            sd, it = _seed(beacon[0], "ptau beacon"), int(beacon[1])
            if not 0 <= it <= 40:
                raise ZkError("ptau beacon: iter_log in [0, 40]")
        _check(lib().zk_srs_contribute(self._h, str(out_path).encode(), _ptr(sw) if sw is not None else None,
                                       sd.ctypes.data if sd is not None else None, it))

    def verify(self, seed=None, max_findings=16):
        """zk_srs_verify: Srs.check's report under "file", the transcript's hash chain, every proof of knowledge and beacon, and the last
        record's images against the file -> the report as a dict; seed: 32 bytes, tests only"""
        sd = _seed(seed, "srs verify")
        return _report(lib().zk_srs_verify(self._h, sd.ctypes.data if sd is not None else None, int(max_findings)))

    def free(self):
        if self._h:
            lib().zk_srs_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def srs_new(curve, power, path):
    """zk_srs_new (host only): the powers-of-tau file of tau = alpha = beta = 1 with an empty transcript, where a ceremony starts"""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    _check(lib().zk_srs_new(curve.encode(), int(power), str(path).encode()))


def srs_verify_lines(report):
    """one line per finding of Srs.verify's report, the file's own findings (Srs.check) first"""
    out = []
    for f in report["file"]["findings"]:
        out.append("ptau file: %s %s" % (f["kind"], " ".join("%s=%s" % (k, v) for k, v in f.items() if k != "kind")))
    text = {"no_transcript": "the file has no transcript of contributions (section %(section)s)",
            "chain_hash": "contribution %(contribution)s: the chain hash is not the hash of the records before it",
            "pok_invalid": "contribution %(contribution)s: no valid proof of knowledge of the %(which)s factor",
            "beacon_mismatch": "contribution %(contribution)s: the %(which)s image is not the beacon's recomputed factor times the image before",
            "image_mismatch": "the file's %(which)s point is not the image of the last contribution (%(contribution)s)"}
    for f in report["findings"]:
        out.append("ptau transcript: " + text[f["kind"]] % f)
    return out


def group_ntt(d_points, curve="BN128", group="g1", inverse=False, stream=0):
    """EvaluationDomain::{fft, ifft} whose elements are points: a DevArray of 2^k affine points (u64 Montgomery words, all zero =
    infinity), in place; natural order, the omega of fr_ntt, 1 / n in the inverse"""
    pw = _FQ_WORDS[curve] * (2 if group == "g1" else 4)
    n = d_points.n // pw
    if n == 0 or n & (n - 1) or n * pw != d_points.n:
        raise ZkError("group ntt: the array must hold a power of two of whole points")
    _check(getattr(lib(), "zk_%s_%s_ntt_dev" % (group, _NAME[curve]))(d_points.ptr, n.bit_length() - 1, int(inverse), stream)); return d_points


def mul_scalar(d_points, k, curve="BN128", group="g1", stream=0):
    """[k] P_i for every point of a DevArray and one integer k -> a new DevArray"""
    pw = _FQ_WORDS[curve] * (2 if group == "g1" else 4)
    n = d_points.n // pw
    kw = np.array([(int(k) % _FR[curve] >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    out = DevArray(max(1, n) * pw)
    _check(getattr(lib(), "zk_%s_%s_mul_scalar_dev" % (group, _NAME[curve]))(d_points.ptr, n, DevArray.from_host(kw).ptr, out.ptr, stream)); return out


def mul_scalars(d_points, scalars, curve="BN128", group="g1", stream=0, glv=False):
    """[k_i] P_i for the points of a DevArray and one integer per point -> a new DevArray.  The walk starts at each scalar's top set
    bit: short scalars are cheap.  A zero scalar or the all-zero point gives the all-zero encoding.  glv=True (G1 only, points of the
    subgroup of order r): the same bytes through the endomorphism split, about half the point operations for full-width scalars."""
    if glv and group != "g1":
        raise ZkError("mul_scalars: the endomorphism split exists for g1 only")
    pw = _FQ_WORDS[curve] * (2 if group == "g1" else 4)
    n = d_points.n // pw
    if n * pw != d_points.n or len(scalars) != n:
        raise ZkError("mul_scalars: the array must hold whole points and one scalar for each")
    kw = np.array([((int(k) % _FR[curve]) >> (64 * i)) & (2**64 - 1) for k in scalars for i in range(4)], dtype=np.uint64)
    out = DevArray(max(1, n) * pw)
    if n:
        fn = "zk_%s_%s_mul_scalars%s_dev" % (group, _NAME[curve], "_glv" if glv else "")
        _check(getattr(lib(), fn)(d_points.ptr, n, DevArray.from_host(kw).ptr, out.ptr, stream))
    return out


def contribute(curve, params_bytes, delta=None):
    """One contribution to a key's delta: delta_g1, delta_g2 times delta, l and h divided by it, everything else copied -> the new key's
    bytes.  delta: an integer in [1, r), or None to let the library draw it from the operating system (nothing of it survives the call)."""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    dw = None
    if delta is not None:
        if not 0 < int(delta) < _FR[curve]:
            raise ZkError("groth16 contribute: delta must be a non-zero canonical field element")
        dw = np.array([(int(delta) >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    p = np.frombuffer(params_bytes, dtype=np.uint8)
    out = np.empty(p.size, np.uint8)
    _check(lib().zk_groth16_params_contribute(curve.encode(), p.ctypes.data, p.size, _ptr(dw) if dw is not None else None, out.ctypes.data))
    return out.tobytes()


def contribute_pok(curve, params_bytes, transcript=b"", delta=None):
    """zk_groth16_params_contribute_pok: contribute() plus a proof of knowledge of the ratio of the two deltas, appended to the key's
    transcript -> (the new key's bytes, the new transcript's bytes).  transcript: the bytes so far, or empty to start one at this key."""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    dw = None
    if delta is not None:
        if not 0 < int(delta) < _FR[curve]:
            raise ZkError("groth16 contribute: delta must be a non-zero canonical field element")
        dw = np.array([(int(delta) >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    p = np.frombuffer(params_bytes, dtype=np.uint8)
    t = np.frombuffer(bytes(transcript), dtype=np.uint8)
    head, rec = 48, 96 + 4 * 8 * _FQ_WORDS[curve]
    count = max(0, t.size - head) // rec + 1
    out = np.empty(p.size, np.uint8)
    out_t = np.empty(lib().zk_groth16_key_transcript_size(curve.encode(), count), np.uint8)
    _check(lib().zk_groth16_params_contribute_pok(curve.encode(), p.ctypes.data, p.size, _ptr(dw) if dw is not None else None,
                                                  t.ctypes.data if t.size else None, t.size, out.ctypes.data, out_t.ctypes.data))
    return out.tobytes(), out_t.tobytes()


def key_transcript_check(curve, initial_bytes, final_bytes, transcript, seed=None, max_findings=16):
    """zk_groth16_key_transcript_check: the transcript's chain and proofs from the initial key's delta_g1 to the final key's, and
    contribution_check(initial, final) under "keys" -> the report as a dict.  Whether the initial key is a delta = 1 key of its circuit is
    key_check_srs's question.  seed: 32 bytes, tests only."""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    a, b, t = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (initial_bytes, final_bytes, transcript))
    sd = _seed(seed, "groth16 key transcript")
    return _report(lib().zk_groth16_key_transcript_check(curve.encode(), a.ctypes.data, a.size, b.ctypes.data, b.size, t.ctypes.data, t.size,
                                                         sd.ctypes.data if sd is not None else None, int(max_findings)))


def key_transcript_lines(report):
    """one line per finding of key_transcript_check's report, the two keys' own findings (contribution_check) first"""
    out = ["keys: %s %s" % (f["kind"], " ".join("%s=%s" % (k, v) for k, v in f.items() if k != "kind")) for f in report["keys"]["findings"]]
    text = {"initial_key_mismatch": "the transcript starts at another key than the initial one",
            "chain_hash": "contribution %(contribution)s: the chain hash is not the hash of the records before it",
            "pok_invalid": "contribution %(contribution)s: no valid proof of knowledge of the ratio of the two deltas",
            "final_key_mismatch": "the transcript does not end at the final key (%(what)s)"}
    return out + ["key transcript: " + text[f["kind"]] % f for f in report["findings"]]


def contribution_check(curve, old_params, new_params, seed=None, max_findings=16):
    """zk_groth16_contribution_check: what a contribution may and may not have changed between two keys -> the report as a dict"""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    sd = _seed(seed, "groth16 contribution check")
    a = np.frombuffer(old_params, dtype=np.uint8); b = np.frombuffer(new_params, dtype=np.uint8)
    return _report(lib().zk_groth16_contribution_check(curve.encode(), a.ctypes.data, a.size, b.ctypes.data, b.size,
                                                       sd.ctypes.data if sd is not None else None, int(max_findings)))


def key_check_srs(curve, r1cs_bytes, params_bytes, srs, seed=None, max_findings=16):
    """zk_groth16_key_check_srs (include/zkgpu.h): is this key a key for this circuit over this powers-of-tau file?  Every query against the
    circuit's polynomials at the file's tau by random linear combinations, and alpha_g1, beta_g1, beta_g2 word for word -> the report as a
    dict.  What key_check cannot see; it does not repeat key_check's findings (a section with an invalid point or a wrong length is listed
    under "skipped") nor Srs.check's.  srs: an Srs of the same curve.  seed: 32 bytes, tests only."""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    if not isinstance(srs, Srs) or not srs._h:
        raise ZkError("groth16 key check: srs is an open Srs")
    sd = _seed(seed, "groth16 key check")
    r = np.frombuffer(r1cs_bytes, dtype=np.uint8); p = np.frombuffer(params_bytes, dtype=np.uint8)
    return _report(lib().zk_groth16_key_check_srs(curve.encode(), r.ctypes.data, r.size, p.ctypes.data, p.size, srs._h,
                                                  sd.ctypes.data if sd is not None else None, int(max_findings)))


def fq_convert(d_elems, curve="BN128", to_mont=True, stream=0):
    """Fq::from_repr / into_repr on a DevArray of base-field elements, in place"""
    nl = _FQ_WORDS[curve]
    _check(getattr(lib(), "zk_fq_%s_convert_dev" % _NAME[curve])(d_elems.ptr, d_elems.n // nl, int(to_mont), stream)); return d_elems


# ---- verification (`zkit groth16_verify`, api.rs:302-341) ----
ACCEPTED, REJECTED, INPUT_NOT_CANONICAL, INPUT_COUNT, NOT_ON_CURVE, NOT_IN_SUBGROUP, VERDICT_ERROR = 1, 0, -1, -2, -3, -4, -100


def verdict_name(v):
    return lib().zk_groth16_verdict_name(int(v)).decode()


def pairing(g1, g2, curve="BN128", final_exp=True):
    """n pairs in the layout of the multi-scalar sums (g1: n x 2 Fq, g2: n x 4 Fq as u64 Montgomery words; all zero = infinity)
    -> n x 12 x (4 | 6) u64: the GT values as canonical Fq, c0 and c1 of the coefficients of w^0 .. w^5"""
    if curve not in _FR:
        raise ZkError('pairing: unknown curve "%s" (BN128 | BLS12381)' % curve)
    nl = _FQ_WORDS[curve]
    a, b = np.ascontiguousarray(_np(g1)).reshape(-1), np.ascontiguousarray(_np(g2)).reshape(-1)
    n = a.size // (2 * nl)
    if a.size != n * 2 * nl or b.size != n * 4 * nl:
        raise ZkError("pairing: g1 must hold n x 2 and g2 n x 4 base-field elements")
    out = np.zeros((n, 12, nl), np.uint64)
    _check(getattr(lib(), "zk_pairing_%s" % _NAME[curve])(_ptr(a), _ptr(b), n, _ptr(out), int(bool(final_exp))))
    return out


def pairing_product(g1, g2, curve="BN128", final_exp=True):
    """prod_i e(g1_i, g2_i) for n pairs in the layout `pairing` takes -> ONE GT value, 12 x (4 | 6) u64; n = 0 gives one"""
    if curve not in _FR:
        raise ZkError('pairing: unknown curve "%s" (BN128 | BLS12381)' % curve)
    nl = _FQ_WORDS[curve]
    a, b = np.ascontiguousarray(_np(g1)).reshape(-1), np.ascontiguousarray(_np(g2)).reshape(-1)
    n = a.size // (2 * nl)
    if a.size != n * 2 * nl or b.size != n * 4 * nl:
        raise ZkError("pairing: g1 must hold n x 2 and g2 n x 4 base-field elements")
    out = np.zeros((12, nl), np.uint64)
    _check(getattr(lib(), "zk_pairing_product_%s" % _NAME[curve])(_ptr(a) if n else None, _ptr(b) if n else None, n, _ptr(out), int(bool(final_exp))))
    return out


class Groth16VerifyingKey:
    """bellman's PreparedVerifyingKey on the device: e(alpha, beta), the line tables of -gamma and -delta, the IC points.
    Stricter than the reference (which reads points unchecked): every point must be on its curve and of order r, every public
    input below r; the verdict says which check failed (ACCEPTED = 1, REJECTED = 0, negative = malformed input)."""

    def __init__(self, curve, vk_json):
        if curve not in _FR:
            raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
        self.curve = curve
        text = vk_json if isinstance(vk_json, str) else json.dumps(vk_json)
        self._h = lib().zk_groth16_vk_new(curve.encode(), text.encode())
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().zk_groth16_vk_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.n_public, self.proof_bytes = a.value, b.value

    def verify(self, proof_json, public):
        """proof.json (text or dict) and the public inputs (public_input.json text, or a list of integers / strings) -> verdict"""
        p = proof_json if isinstance(proof_json, str) else json.dumps(proof_json)
        u = public if isinstance(public, str) else json.dumps([str(x) for x in public])
        v = lib().zk_groth16_verify_json(self._h, p.encode(), u.encode())
        if v == VERDICT_ERROR:
            raise ZkError(lib().zk_last_error().decode())
        return v

    def verify_batch(self, points, publics):
        """points: n x (A || B || C) u64 Montgomery words as Groth16Setup.prove returns them; publics: n lists of n_public
        integers -> n verdicts (numpy int32)"""
        pts = np.ascontiguousarray(_np(points)).reshape(-1)
        n = pts.size * 8 // self.proof_bytes
        if pts.size * 8 != n * self.proof_bytes or len(publics) != n:
            raise ZkError("groth16 verify: points must hold n proofs and publics n input lists")
        out = np.zeros(n, np.int32)
        ok = [i for i in range(n) if len(publics[i]) == self.n_public and all(0 <= int(x) < 2**256 for x in publics[i])]
        bad = set(range(n)) - set(ok)
        for i in bad:
            out[i] = INPUT_COUNT if len(publics[i]) != self.n_public else INPUT_NOT_CANONICAL
        if ok:
            sel = np.ascontiguousarray(pts.reshape(n, -1)[ok]).reshape(-1)
            pub = np.array([[(int(x) >> (64 * k)) & (2**64 - 1) for x in publics[i] for k in range(4)] for i in ok], dtype=np.uint64).reshape(-1)
            v = np.zeros(len(ok), np.int32)
            _check(lib().zk_groth16_verify_batch(self._h, _ptr(sel), _ptr(pub) if pub.size else None, len(ok), _ptr(v)))
            out[ok] = v
        return out

    def verify_aggregate(self, points, publics, seed=None, locate=True):
        """All n proofs in one randomised pairing check (zk_groth16_verify_aggregate): -> (verdict, first_bad).  (ACCEPTED, None) when every
        proof is good; a batch with a wrong proof is accepted with probability about 2^-128 over the secret weights.  Otherwise, with
        locate, the per-proof path names the first proof it does not accept and its verdict; without it (REJECTED, None).
        seed: 32 bytes, FOR TESTS ONLY -- None draws the weights from the operating system."""
        pts = np.ascontiguousarray(_np(points)).reshape(-1)
        n = pts.size * 8 // self.proof_bytes
        if pts.size * 8 != n * self.proof_bytes or len(publics) != n:
            raise ZkError("groth16 verify: points must hold n proofs and publics n input lists")
        for i in range(n):                                   # what verify_batch settles on the host: the first such proof is the answer
            if len(publics[i]) != self.n_public or not all(0 <= int(x) < 2**256 for x in publics[i]):
                code = INPUT_COUNT if len(publics[i]) != self.n_public else INPUT_NOT_CANONICAL
                if not locate:
                    return REJECTED, None
                if i:
                    v, fb = self.verify_aggregate(pts.reshape(n, -1)[:i], publics[:i], seed, True)
                    if v != ACCEPTED:
                        return v, fb
                return code, i
        sd = _seed(seed, "groth16 verify")
        pub = np.array([(int(x) >> (64 * k)) & (2**64 - 1) for row in publics for x in row for k in range(4)], dtype=np.uint64)
        verdict, first = C.c_int(VERDICT_ERROR), C.c_uint64(0)
        _check(lib().zk_groth16_verify_aggregate(self._h, _ptr(pts) if n else None, _ptr(pub) if pub.size else None, n,
                                                 sd.ctypes.data if sd is not None else None, C.byref(verdict), C.byref(first) if locate else None))
        return verdict.value, (int(first.value) if locate and verdict.value != ACCEPTED else None)

    def proof_words(self, proof_json, public):
        """proof.json and public_input.json (text) through the library's readers -> (points, inputs) as verify_batch takes them, or the
        verdict (INPUT_COUNT, INPUT_NOT_CANONICAL) the file-level form gives without looking at a point"""
        pts, pub = np.zeros(self.proof_bytes // 8, np.uint64), np.zeros(max(1, 4 * self.n_public), np.uint64)
        v = lib().zk_groth16_proof_words(self._h, proof_json.encode(), public.encode(), _ptr(pts), _ptr(pub))
        if v == VERDICT_ERROR:
            raise ZkError(lib().zk_last_error().decode())
        if v != ACCEPTED:
            return v
        return pts, [sum(int(pub[4 * j + k]) << (64 * k) for k in range(4)) for j in range(self.n_public)]

    def free(self):
        if self._h:
            lib().zk_groth16_vk_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- groth16_key_check: a proving key against its circuit, before it is taken on faith ----


def points_check(points, curve, group, plain=False):
    """n affine points in the layout of the multi-scalar sums (u64 Montgomery words, all zero = infinity; a host array or a DevArray),
    group "g1" | "g2" -> {class: (exact number of points, smallest index or None)} for POINT_CLASSES.  plain: [r]P = O bit by
    bit instead of the endomorphism tests -- the same answer, the comparator."""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    if group not in ("g1", "g2"):
        raise ZkError('points check: group must be "g1" or "g2"')
    pw = _FQ_WORDS[curve] * (2 if group == "g1" else 4)
    fn = "zk_points_check_%s" % _NAME[curve]
    out = np.zeros(8, np.uint64)
    if isinstance(points, DevArray):
        d_out = DevArray.from_host(out)
        _check(getattr(lib(), fn + "_dev")(1 if group == "g1" else 2, points.ptr, points.n // pw, int(bool(plain)), d_out.ptr, 0))
        out = d_out.to_host()
    else:
        a = np.ascontiguousarray(_np(points)).reshape(-1)
        if a.size % pw:
            raise ZkError("points check: the array does not hold whole points")
        _check(getattr(lib(), fn)(1 if group == "g1" else 2, _ptr(a) if a.size else None, a.size // pw, int(bool(plain)), _ptr(out)))
    return {k: (int(out[2 * i]), int(out[2 * i + 1]) if out[2 * i] else None) for i, k in enumerate(POINT_CLASSES)}


def key_check(curve, r1cs_bytes, params_bytes, vk_json=None, seed=None, max_findings=16):
    """zk_groth16_key_check (include/zkgpu.h): section lengths against the circuit, every point's class, the G1 / G2 copies tied by
    pairings, verification_key.json against the embedded copy -> the report as a dict.  seed: 32 bytes, for tests only (None: the
    operating system's randomness).  Not checked: h, l, ic and a against the circuit's polynomials -- `groth16_prove --verify` is
    the functional test.  With ZK_KEY_CHECK_TIMING set in the environment the report also carries "timing_ms" (tools/key_check_time.py)."""
    if curve not in _FR:
        raise ZkError('groth16: unknown curve "%s" (BN128 | BLS12381)' % curve)
    if seed is not None and len(seed) != 32:
        raise ZkError("groth16 key check: the seed is 32 bytes")
    r = np.frombuffer(r1cs_bytes, dtype=np.uint8); p = np.frombuffer(params_bytes, dtype=np.uint8)
    text = None if vk_json is None else (vk_json if isinstance(vk_json, str) else json.dumps(vk_json)).encode()
    sd = None if seed is None else np.frombuffer(bytes(seed), dtype=np.uint8)
    s = lib().zk_groth16_key_check(curve.encode(), r.ctypes.data, r.size, p.ctypes.data, p.size, text, sd.ctypes.data if sd is not None else None, int(max_findings))
    if not s:
        raise ZkError(lib().zk_last_error().decode())
    try:
        return json.loads(C.string_at(s).decode())
    finally:
        lib().zk_string_free(s)
