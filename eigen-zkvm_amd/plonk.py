"""A PLONK prover and verifier over the KZG layer (kzg.py) and the scalar-field polynomial layer (frpoly.py, DESIGN.md
3.20): setup, prove, verify.  The protocol, the transcript and the files are this module; the arithmetisation under it --
circuits, the witness path, the key's fixed columns, the steps up to Z, the identity's terms -- is plonk_arith.py, whose names are offered
here as well.  Everything over Fr runs on the device through zk_fr_<curve>_*_dev, zk_plonk_<curve>_quotient_dev / _gate_check_dev,
zk_fr_<curve>_gather_dev and Kzg.open_multi.  There is no CPU fallback.  Cut down to what those layers do: NO linearisation polynomial (every
polynomial of the identity is opened at zeta, Z at zeta w as well, in one Shplonk proof of two points), the quotient t committed WHOLE
(degree 3n + 5: the file must hold 3n + 6 G1 powers), a circuit is a gate table, written by hand or compiled from a circom .r1cs (R1csCircuit,
DESIGN.md 3.22); no custom gates, not fflonk's interleaved form.  Lookups are a protocol of their own on the same layer: plonk_lookup.py
(DESIGN.md 3.24).

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
import hashlib
import json

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import plonk_arith as pa
from .groth16 import _NAME
from .kzg import _scalar, point_from_json, point_to_json
# the layer's names, for this module and for its callers: what plonk.py offered before the layer was lifted out of it stays here
from .plonk_arith import (ACCEPTED, FIXED_NAMES, FR, INPUT_NOT_CANONICAL, M64, R1CS_INFO, REJECTED, SELECTORS, TWO_ADICITY, WIRES, ArithKey, Circuit, R1csCircuit, View, add_into,
                          canon_words, check_size, coset_ks, draw, draw_until, extend_witness, extend_words, gate_check, gather, gather_dev, int_of, le, modulus, omega,
                          public_input_at, upload_indices)

N_VALUES, N_FIXED = 14, 8
POINT_NAMES = ("A", "B", "C", "Z", "T", "W1", "W2")
VALUE_NAMES = FIXED_NAMES + ("a", "b", "c", "t", "Z", "Zw")
PROTOCOL = "plonk-shplonk"


def required_powers(n):
    """the G1 powers the file must hold: the quotient is committed whole, with 3n + 6 coefficients"""
    return 3 * n + 6


# ---- the transcript -----------------------------------------------------------------------------------------------------------------------
def vk_digest(curve, log_n, n_public, k1, k2, commitments):
    """vkd = H(curve || "plonk-vk" || k u32le || l u32le || k_1 || k_2 || the 8 commitments): curve in ASCII, k = log n and l the number of
    public inputs as 4 little-endian bytes each, k_1 and k_2 as 32 little-endian bytes, every commitment in the file's encoding, in the order
    q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3"""
    return hashlib.sha256(curve.encode("ascii") + b"plonk-vk" + int(log_n).to_bytes(4, "little") + int(n_public).to_bytes(4, "little") + le(k1) + le(k2) +
                          b"".join(bytes(c) for c in commitments)).digest()


def transcript_start(curve, vkd, publics):
    """c0 = H(curve || "plonk-v1" || vkd || l u32le || x_0 .. x_(l-1)): the public inputs as 32 little-endian bytes each"""
    return hashlib.sha256(curve.encode("ascii") + b"plonk-v1" + vkd + len(publics).to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()


def transcript_wires(curve, c0, A, B, Cc):
    """c1 = H(c0 || A || B || C); beta = H(c1 || 00), gamma = H(c1 || 01) -> (c1, beta, gamma)"""
    c1 = hashlib.sha256(c0 + bytes(A) + bytes(B) + bytes(Cc)).digest()
    return c1, draw(curve, c1, b"\x00"), draw(curve, c1, b"\x01")


def transcript_product(curve, c1, Z):
    """c2 = H(c1 || Z); alpha = H(c2 || 00) -> (c2, alpha)"""
    c2 = hashlib.sha256(c1 + bytes(Z)).digest()
    return c2, draw(curve, c2, b"\x00")


def transcript_quotient(curve, c2, T, n):
    """c3 = H(c2 || T); zeta = H(c3 || ctr), ctr one byte from 0, drawn again while zeta = 0 or zeta^n = 1 -> (c3, zeta)"""
    r = FR[curve]
    c3 = hashlib.sha256(c2 + bytes(T)).digest()
    return c3, draw_until(curve, c3, lambda zeta: zeta != 0 and pow(zeta, n, r) != 1, "plonk: no evaluation point")


def transcript_values(curve, c3, values):
    """c4 = H(c3 || the 14 values, 32 little-endian bytes each); gamma' = H(c4 || 00) -> (c4, gamma')"""
    c4 = hashlib.sha256(c3 + b"".join(le(v) for v in values)).digest()
    return c4, draw(curve, c4, b"\x00")


def transcript_z(curve, c4, W1, avoid):
    """z' = H(c4 || 01 || W1 || ctr), ctr one byte from 0, drawn again while z' is one of the opening points {zeta, zeta w}"""
    avoid = {int(p) for p in avoid}
    return draw_until(curve, c4 + b"\x01" + bytes(W1), lambda z: z not in avoid, "plonk: no opening challenge")


# ---- the device call that is this protocol's ------------------------------------------------------------------------------------------------
def quotient(cols, log_n, alpha, beta, gamma, k1, k2, curve="BN128", out=None):
    """zk_plonk_<curve>_quotient_dev: cols, 15 DevArrays of 4n elements in the header's order -> the bracket of round 3 on the coset"""
    modulus(curve)
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


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    """(curve, log n, l, k_1, k_2, the 8 commitments); `kzg` is the handle verify() pairs with, when the key came from a PlonkKey"""

    def __init__(self, curve, log_n, n_public, k1, k2, commitments, kzg=None):
        modulus(curve)
        self.curve, self.log_n, self.n_public, self.k1, self.k2 = curve, int(log_n), int(n_public), int(k1), int(k2)
        self.commitments = [bytes(c) for c in commitments]
        self.kzg = kzg
        if len(self.commitments) != N_FIXED:
            raise ZkError("plonk: a verification key holds %d commitments, not %d" % (N_FIXED, len(self.commitments)))
        check_size(curve, self.log_n)
        self.n = 1 << self.log_n
        self.digest = vk_digest(curve, self.log_n, self.n_public, self.k1, self.k2, self.commitments)


def vk_to_json(vk):
    return json.dumps({"protocol": PROTOCOL, "curve": vk.curve, "log_n": vk.log_n, "n_public": vk.n_public, "k1": str(vk.k1), "k2": str(vk.k2),
                       "commitments": {name: point_to_json(c, vk.curve) for name, c in zip(FIXED_NAMES, vk.commitments)}}, indent=1) + "\n"


def vk_from_json(text, kzg=None):
    js = json.loads(text)
    if js.get("protocol") != PROTOCOL:
        raise ZkError('plonk: not a verification key of this prover (protocol "%s")' % js.get("protocol"))
    return VerifyingKey(js["curve"], js["log_n"], js["n_public"], int(js["k1"], 0), int(js["k2"], 0),
                        [point_from_json(js["commitments"][name], js["curve"]) for name in FIXED_NAMES], kzg)


def proof_to_json(proof, curve):
    return pa.proof_to_json(proof, curve, PROTOCOL, POINT_NAMES)


def proof_from_json(text, curve):
    return pa.proof_from_json(text, curve, PROTOCOL, POINT_NAMES, "plonk")


def proof_to_bytes(proof):
    """A || B || C || Z || T || the 14 values, 32 little-endian bytes each || W1 || W2"""
    return pa.proof_to_bytes(proof, POINT_NAMES[:5], POINT_NAMES[5:])


def proof_from_bytes(data, point_bytes):
    return pa.proof_from_bytes(data, point_bytes, POINT_NAMES[:5], N_VALUES, POINT_NAMES[5:], "plonk")


class PlonkKey(ArithKey):
    """The proving key on the device: ArithKey's columns, and beside them the coefficients of the 8 fixed polynomials, which round 5 opens,
    and their 8 commitments.  Setup is deterministic and has no secret.  self.vk is the verification key."""

    def __init__(self, kzg, circuit):
        super().__init__(kzg, circuit, "plonk", ("3n + 6", required_powers(circuit.n)))

    def _fixed(self, coef):
        self.coef = coef

    def _build(self):
        super()._build()
        self.commitments = [self.kzg.commit(d) for d in self.coef]
        self.vk = VerifyingKey(self.curve, self.log_n, self.circuit.n_public, self.k1, self.k2, self.commitments, self.kzg)


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
    cv, n, k, kzg = key.curve, key.n, key.log_n, key.kzg
    mark = _mark or (lambda name: None)
    own = []

    def keep(d):
        own.append(d)
        return d
    try:
        vals, pi_vals, publics, bs = pa.witness_columns(key, witness, blinding, _wires, "plonk", keep, mark)
        # round 1
        coef = pa.blinded_wires(key, vals, bs, keep)
        A, B, Cc = [kzg.commit(d) for d in coef]
        c0 = transcript_start(cv, key.vk.digest, publics)
        c1, beta, gamma = transcript_wires(cv, c0, A, B, Cc)
        mark("round 1")
        # round 2
        z_coef = pa.permutation_product(key, vals, beta, gamma, bs, "plonk", keep)
        Z = kzg.commit(z_coef)
        c2, alpha = transcript_product(cv, c1, Z)
        mark("round 2")
        # round 3
        pi_coef = keep(pa.interpolate(cv, pi_vals, n, 0, k))
        cols = [keep(pa.coset_evals(cv, d, n + 2, k + 2)) for d in coef] + [keep(pa.coset_evals(cv, z_coef, n + 3, k + 2))] + key.coset
        cols += [keep(pa.coset_evals(cv, pi_coef, n, k + 2)), key.l1_coset, key.x_coset]
        t = keep(quotient(cols, k, alpha, beta, gamma, key.k1, key.k2, cv))
        t_view = pa.quotient_coeffs(cv, k, t, required_powers(n), "plonk: the quotient has %d non-zero coefficients from 3n + 6 = %d on: the identity does not hold on H", keep)
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
        polys = key.coef + [View(d, 0, n + 2) for d in coef] + [t_view, View(z_coef, 0, n + 3)]
        sets = [[zeta]] * 12 + [[zeta, zeta * omega(cv, k) % FR[cv]]]
        values, W1, W2, _, _ = kzg.open_multi(polys, sets, transcript=_opening_transcript or opening_gamma, transcript_z=opening_z if _opening_transcript is None else pa.plain_z,
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


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------------
def challenges(vk, publics, proof):
    """every challenge of a proof from the verification key, the public inputs and the proof's own points and values -> a mapping with beta,
    gamma, alpha, zeta, gamma_open (gamma') and z_open (z')"""
    cv, r = vk.curve, FR[vk.curve]
    c0 = transcript_start(cv, vk.digest, publics)
    c1, beta, gamma = transcript_wires(cv, c0, proof["A"], proof["B"], proof["C"])
    c2, alpha = transcript_product(cv, c1, proof["Z"])
    c3, zeta = transcript_quotient(cv, c2, proof["T"], vk.n)
    c4, g = transcript_values(cv, c3, proof["values"])
    zw = zeta * omega(cv, vk.log_n) % r
    return {"beta": beta, "gamma": gamma, "alpha": alpha, "zeta": zeta, "gamma_open": g, "z_open": transcript_z(cv, c4, proof["W1"], (zeta, zw))}


def identity_holds(curve, log_n, k1, k2, publics, values, ch):
    """the identity of round 3 at zeta in the field, from the 14 values: the bracket equals t(zeta) Z_H(zeta)"""
    v, alpha = dict(zip(VALUE_NAMES, values)), ch["alpha"]
    gate, perm, l1z, zh = pa.identity_terms(curve, log_n, k1, k2, publics, ch["zeta"], v, ch["beta"], ch["gamma"])
    return (gate + alpha * perm + alpha * alpha * l1z - v["t"] * zh) % FR[curve] == 0


def host_check(vk, publics, proof, point_bytes=None):
    """what the verifier decides on the host, before any device work: lengths (an error), every scalar below r (else INPUT_NOT_CANONICAL),
    the challenges, the identity (else REJECTED) -> (verdict, the tuple Kzg.verify_multi takes, built with the verifier's OWN gamma' and z')"""
    cv, r = vk.curve, FR[vk.curve]
    shape = pa.check_proof_shape(proof, POINT_NAMES, N_VALUES, point_bytes if point_bytes is not None else len(vk.commitments[0]), vk.n_public, publics, r, "plonk")
    if shape is None:
        return INPUT_NOT_CANONICAL, None
    values, publics = shape
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
    return pa.verify_batch(vk, publics, proofs, host_check, kzg, seed, locate, "plonk")
