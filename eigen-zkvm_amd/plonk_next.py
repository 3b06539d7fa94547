"""PLONK with a next-row term: plonk.py's prover and verifier over a gate that also reads the c-wire of the row after it.  A
protocol of its own beside plonk.py on the same layers: kzg.py, frpoly.py and the arithmetisation of plonk_arith.py.  Everything over Fr runs
on the device through zk_fr_<curve>_*_dev, zk_plonk_<curve>_next_quotient_dev / _next_gate_check_dev, zk_fr_<curve>_gather_dev and
Kzg.open_multi.  There is no CPU fallback.  As in plonk.py: NO linearisation polynomial, the quotient t committed WHOLE, a circuit is a gate
table, written by hand (NextCircuit) or compiled from a circom .r1cs under the chain rule (NextR1csCircuit; include/zkgpu.h states the rule).
Not here: the term in the fflonk and lookup provers, other custom gates.

Field Fr of BN128 or BLS12381.  n = 2^k >= 8 rows (smaller circuits are padded to 8, others to the next power of two; a padding row has all
selectors 0 and its wires on variable 0).  H = <w> with the w of zk_fr_<curve>_ntt_dev, w = 7^((r - 1) / n).

Circuit.  Row i must satisfy qL a + qR b + qO c + qM a b + qC + qN c' + PI_i = 0 with c' the c of row i + 1 mod n: the next row is cyclic
on H.  NextCircuit puts one row per public input in front (qL = 1, the rest 0, a = public[i]); PI_i = -x_i for i < l and 0 otherwise.  Public
rows and padding rows have qN = 0.  A gate table of plonk.Circuit, qN = 0 everywhere, is a circuit of this protocol.

Wiring.  As plonk.py's: position (column j, row i) has the label k_j w^i with k_0 = 1; k_1 < k_2 are the smallest integers >= 2 with
k_1^n != 1, k_2^n != 1 and (k_2 / k_1)^n != 1.  sigma maps each position to the next position of the same variable, cyclically in (column,
row) order; S_sigma_j is the polynomial whose values on H are the labels of sigma(j, .).

Rounds.
 1. wire values gathered from the witness; a, b interpolated and blinded as a += (b_1 X + b_2) Z_H (b: b_3, b_4); c is opened at two points
    and takes three blinders, c += (b_5 X^2 + b_6 X + b_7) Z_H; [A], [B], [C]
 2. beta, gamma; z_0 = 1, z_(i+1) = z_i prod_j (w_j,i + beta k_j w^i + gamma) / prod_j (w_j,i + beta sigma_j,i + gamma), which must close with
    z_n = 1; Z += (b_8 X^2 + b_9 X + b_10) Z_H; [Z]
 3. alpha; on the coset 7 H_4n
      t = [ a b q_M + a q_L + b q_R + c q_O + q_C + q_N c(wX) + PI
            + alpha ((a + beta X + gamma)(b + beta k_1 X + gamma)(c + beta k_2 X + gamma) Z
            - (a + beta S_sigma1 + gamma)(b + beta S_sigma2 + gamma)(c + beta S_sigma3 + gamma) Z(wX)) + alpha^2 L_1 (Z - 1) ] / Z_H
    (the bracket is zk_plonk_<curve>_next_quotient_dev, the division divide_zh_coset); t has degree 3n + 6: the file must hold 3n + 7 G1
    powers, and the coefficients from 3n + 7 on must be zero; [T]
 4. zeta, drawn again while zeta = 0 or zeta^n = 1
 5. Kzg.open_multi of q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3, q_N, a, b, t on {zeta} and of c and Z on {zeta, zeta w}; in the
    opening the polynomials stand in the order q_L .. q_N, a, b, c, t, Z (the power of gamma' each one takes)
The proof is [A], [B], [C], [Z], [T], the 16 values, W1, W2.  The 16 values: q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3, q_N, a,
b, c, t, Z at zeta, then Z and c at zeta w.  The opening's own challenges are NOT in it: the verifier derives them.

Verifier.  Lengths, then every scalar below r, then the challenges, then the identity of round 3 at zeta in the field from the 16 values,
with q_N(zeta) c(zeta w) in the gate part -- all on the host, before any device work; then ONE randomised pairing check of the batch.

Transcript.  H is SHA-256; a digest is read as a big-endian integer and reduced mod r; a scalar is 32 little-endian bytes; a point is
point_bytes bytes in the .ptau file's encoding (affine, little-endian Montgomery, all zero for infinity); "curve" is the name in ASCII
("BN128" | "BLS12381"); a counter is one byte that starts at 0 and only moves for a re-draw.
    vkd    = H(curve || "plonk-next-vk" || k u32le || l u32le || k_1 || k_2 || the 9 commitments)
    c0     = H(curve || "plonk-next-v1" || vkd || l u32le || x_0 .. x_(l-1))
    c1     = H(c0 || A || B || C)            beta = H(c1 || 00)     gamma = H(c1 || 01)
    c2     = H(c1 || Z)                      alpha = H(c2 || 00)
    c3     = H(c2 || T)                      zeta = H(c3 || ctr)
    c4     = H(c3 || the 16 values)          gamma' = H(c4 || 00)   z' = H(c4 || 01 || W1 || ctr), outside {zeta, zeta w}

Blinding.  The ten blinders come from `secrets`; blinding=[10 integers] is FOR TESTS ONLY (all zero gives the unblinded proof)."""
import ctypes as C
import hashlib
import json

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import plonk_arith as pa
from .groth16 import _NAME
from .kzg import _scalar, point_from_json, point_to_json
from .plonk_arith import (ACCEPTED, FIXED_NAMES, FR, INPUT_NOT_CANONICAL, REJECTED, SELECTORS, WIRES, ArithKey, Circuit, R1csCircuit, View, canon_words, check_size, draw, draw_until,
                          extend_witness, le, modulus, omega)

WHO = "plonk next"
N_VALUES, N_FIXED, N_BLINDERS = 16, 9, 10
NEXT_FIXED_NAMES = FIXED_NAMES + ("qN",)
POINT_NAMES = ("A", "B", "C", "Z", "T", "W1", "W2")
VALUE_NAMES = NEXT_FIXED_NAMES + ("a", "b", "c", "t", "Z", "Zw", "cw")
PROTOCOL = "plonk-shplonk-next"
CIRCUIT, R1CS_CIRCUIT = "NextCircuit", "NextR1csCircuit"       # what tools/plonk_cli.py loads a gate table and compiles an .r1cs as


def required_powers(n):
    """the G1 powers the file must hold: the quotient is committed whole, with 3n + 7 coefficients"""
    return 3 * n + 7


# ---- circuits -------------------------------------------------------------------------------------------------------------------------------
class NextCircuit(Circuit):
    """A gate table whose gates may read the next row.  gates: Circuit's mapping and, optionally, qN (integers below r, or (m, 4) u64
    canonical words): the coefficient of the NEXT row's c in the gate's equation; without it qN is zero and the table is plonk.Circuit's.
    self.sel["qN"] is (n, 4) u64, zero on public and padding rows.  The row after the last is row 0."""
    has_next = True

    def __init__(self, n_vars, public, gates, curve="BN128", min_rows=0):
        r = modulus(curve)
        qn = canon_words(gates["qN"], r, "selector qN of gate") if "qN" in gates else None
        super().__init__(n_vars, public, gates, curve, min_rows)
        if qn is None:
            qn = np.zeros((self.n_gates, 4), np.uint64)
        if len(qn) != self.n_gates:
            raise ZkError("plonk: the selector and wire arrays of a circuit have one length")
        self.gates["qN"] = qn
        a = np.zeros((self.n, 4), np.uint64)
        a[self.n_public:self.n_public + self.n_gates] = qn
        self.sel["qN"] = a

    @classmethod
    def load(cls, path, curve="BN128"):
        """Circuit.save's .npz, with qN ((m, 4) u64 canonical words) when the circuit has it: a file without qN loads with zeros"""
        with np.load(path) as z:
            missing = [k for k in SELECTORS + WIRES + ("n_vars", "public") if k not in z]
            if missing:
                raise ZkError("%s: %s holds no %s" % (WHO, path, ", ".join(missing)))
            gates = {k: np.asarray(z[k], dtype=np.uint64).reshape(-1, 4) for k in SELECTORS + (("qN",) if "qN" in z else ())}
            gates.update({k: np.asarray(z[k]).reshape(-1) for k in WIRES})
            return cls(int(z["n_vars"]), [int(v) for v in np.asarray(z["public"]).reshape(-1)], gates, curve)


class NextR1csCircuit(R1csCircuit, NextCircuit):
    """The gate table of a circom .r1cs under the CHAIN rule (include/zkgpu.h states it): a sum of m >= 3 signals is a running sum down column
    c, two terms a row, in ceil(m / 2) gates and as many auxiliaries.  zk_plonk_<curve>_next_r1cs_new compiles on the host; everything else is
    R1csCircuit's: .origin, .segments, .info, the witness of prove() and extend_witness() (the auxiliaries are every second prefix of a
    segment and its last), free()."""
    _NEW = "next_r1cs_new"

    def _more_gates(self, gates, m):
        qn = np.zeros((max(m, 1), 4), np.uint64)
        _check(getattr(lib(), "zk_plonk_%s_next_r1cs_qn" % _NAME[self.curve])(self._h, _ptr(qn)))
        gates["qN"] = qn[:m]


# ---- the transcript -----------------------------------------------------------------------------------------------------------------------
def vk_digest(curve, log_n, n_public, k1, k2, commitments):
    """vkd = H(curve || "plonk-next-vk" || k u32le || l u32le || k_1 || k_2 || the 9 commitments), in the order q_L, q_R, q_O, q_M, q_C,
    S_sigma1, S_sigma2, S_sigma3, q_N"""
    return hashlib.sha256(curve.encode("ascii") + b"plonk-next-vk" + int(log_n).to_bytes(4, "little") + int(n_public).to_bytes(4, "little") + le(k1) + le(k2) +
                          b"".join(bytes(c) for c in commitments)).digest()


def transcript_start(curve, vkd, publics):
    """c0 = H(curve || "plonk-next-v1" || vkd || l u32le || x_0 .. x_(l-1))"""
    return hashlib.sha256(curve.encode("ascii") + b"plonk-next-v1" + vkd + len(publics).to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()


def transcript_wires(curve, c0, A, B, Cc):
    """c1 = H(c0 || A || B || C); beta = H(c1 || 00), gamma = H(c1 || 01) -> (c1, beta, gamma)"""
    c1 = hashlib.sha256(c0 + bytes(A) + bytes(B) + bytes(Cc)).digest()
    return c1, draw(curve, c1, b"\x00"), draw(curve, c1, b"\x01")


def transcript_product(curve, c1, Z):
    """c2 = H(c1 || Z); alpha = H(c2 || 00) -> (c2, alpha)"""
    c2 = hashlib.sha256(c1 + bytes(Z)).digest()
    return c2, draw(curve, c2, b"\x00")


def transcript_quotient(curve, c2, T, n):
    """c3 = H(c2 || T); zeta = H(c3 || ctr), drawn again while zeta = 0 or zeta^n = 1 -> (c3, zeta)"""
    r = FR[curve]
    c3 = hashlib.sha256(c2 + bytes(T)).digest()
    return c3, draw_until(curve, c3, lambda zeta: zeta != 0 and pow(zeta, n, r) != 1, WHO + ": no evaluation point")


def transcript_values(curve, c3, values):
    """c4 = H(c3 || the 16 values, 32 little-endian bytes each); gamma' = H(c4 || 00) -> (c4, gamma')"""
    c4 = hashlib.sha256(c3 + b"".join(le(v) for v in values)).digest()
    return c4, draw(curve, c4, b"\x00")


def transcript_z(curve, c4, W1, avoid):
    """z' = H(c4 || 01 || W1 || ctr), drawn again while z' is one of the opening points {zeta, zeta w}"""
    avoid = {int(p) for p in avoid}
    return draw_until(curve, c4 + b"\x01" + bytes(W1), lambda z: z not in avoid, WHO + ": no opening challenge")


def _proof_order(per_poly):
    """the opening's values, polynomial by polynomial (.., a, b, [c, cw], t, [Z, Zw]) -> the proof's 16"""
    flat = [ys[0] for ys in per_poly]
    return flat + [per_poly[13][1], per_poly[11][1]]


def _opening_order(values):
    """the proof's 16 values -> the opening's, polynomial by polynomial"""
    return [[v] for v in values[:11]] + [[values[11], values[15]], [values[12]], [values[13], values[14]]]


def _sets(curve, log_n, zeta):
    zw = zeta * omega(curve, log_n) % FR[curve]
    return [[zeta]] * 11 + [[zeta, zw], [zeta], [zeta, zw]]


# ---- the device calls that are this protocol's ----------------------------------------------------------------------------------------------
def quotient(cols, log_n, alpha, beta, gamma, k1, k2, curve="BN128", out=None):
    """zk_plonk_<curve>_next_quotient_dev: cols, 16 DevArrays of 4n elements in the header's order (plonk.quotient's 15, then q_N) -> the
    bracket of round 3 on the coset"""
    modulus(curve)
    m = 4 << int(log_n)
    if len(cols) != 16:
        raise ZkError("%s: the quotient takes 16 columns, not %d" % (WHO, len(cols)))
    sc = [_scalar(v, curve, w) for v, w in ((alpha, "alpha"), (beta, "beta"), (gamma, "gamma"), (k1, "k1"), (k2, "k2"))]
    if any(c.n < 4 * m for c in cols):
        raise ZkError("%s: every column of the quotient holds 4n = %d elements" % (WHO, m))
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    d_out = out if out is not None else DevArray(4 * m)
    try:
        _check(getattr(lib(), "zk_plonk_%s_next_quotient_dev" % _NAME[curve])(_ptr(ptrs), int(log_n), *[_ptr(s) for s in sc], d_out.ptr, 0))
        return d_out
    except Exception:
        if out is None:
            d_out.free()
        raise


def gate_check(cols, n, curve="BN128"):
    """zk_plonk_<curve>_next_gate_check_dev: cols, 10 DevArrays of n elements (a, b, c, qL, qR, qO, qM, qC, PI, qN) -> (rows that fail, the
    first or None); row n - 1 reads the c of row 0"""
    modulus(curve)
    if len(cols) != 10:
        raise ZkError("%s: the gate check takes 10 columns, not %d" % (WHO, len(cols)))
    if any(c.n < 4 * int(n) for c in cols):
        raise ZkError("%s: every column of the gate check holds n = %d elements" % (WHO, int(n)))
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    bad, first = C.c_uint64(0), C.c_uint64(0)
    _check(getattr(lib(), "zk_plonk_%s_next_gate_check_dev" % _NAME[curve])(_ptr(ptrs), int(n), C.byref(bad), C.byref(first), 0))
    return int(bad.value), (None if bad.value == 0 else int(first.value))


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    """(curve, log n, l, k_1, k_2, the 9 commitments); `kzg` is the handle verify() pairs with, when the key came from a NextKey"""

    def __init__(self, curve, log_n, n_public, k1, k2, commitments, kzg=None):
        modulus(curve)
        self.curve, self.log_n, self.n_public, self.k1, self.k2 = curve, int(log_n), int(n_public), int(k1), int(k2)
        self.commitments = [bytes(c) for c in commitments]
        self.kzg = kzg
        if len(self.commitments) != N_FIXED:
            raise ZkError("%s: a verification key holds %d commitments, not %d" % (WHO, N_FIXED, len(self.commitments)))
        check_size(curve, self.log_n)
        self.n = 1 << self.log_n
        self.digest = vk_digest(curve, self.log_n, self.n_public, self.k1, self.k2, self.commitments)


def vk_to_json(vk):
    return json.dumps({"protocol": PROTOCOL, "curve": vk.curve, "log_n": vk.log_n, "n_public": vk.n_public, "k1": str(vk.k1), "k2": str(vk.k2),
                       "commitments": {name: point_to_json(c, vk.curve) for name, c in zip(NEXT_FIXED_NAMES, vk.commitments)}}, indent=1) + "\n"


def vk_from_json(text, kzg=None):
    js = json.loads(text)
    if js.get("protocol") != PROTOCOL:
        raise ZkError('%s: not a verification key of this prover (protocol "%s")' % (WHO, js.get("protocol")))
    return VerifyingKey(js["curve"], js["log_n"], js["n_public"], int(js["k1"], 0), int(js["k2"], 0),
                        [point_from_json(js["commitments"][name], js["curve"]) for name in NEXT_FIXED_NAMES], kzg)


def proof_to_json(proof, curve):
    return pa.proof_to_json(proof, curve, PROTOCOL, POINT_NAMES)


def proof_from_json(text, curve):
    return pa.proof_from_json(text, curve, PROTOCOL, POINT_NAMES, WHO)


def proof_to_bytes(proof):
    """A || B || C || Z || T || the 16 values, 32 little-endian bytes each || W1 || W2"""
    return pa.proof_to_bytes(proof, POINT_NAMES[:5], POINT_NAMES[5:])


def proof_from_bytes(data, point_bytes):
    return pa.proof_from_bytes(data, point_bytes, POINT_NAMES[:5], N_VALUES, POINT_NAMES[5:], WHO)


class NextKey(ArithKey):
    """The proving key on the device: ArithKey's columns; beside them q_N on H and on the coset, the coefficients of the 9 fixed polynomials,
    which round 5 opens, and their 9 commitments.  Setup is deterministic and has no secret.  self.vk is the verification key.  circuit: a
    NextCircuit, a NextR1csCircuit, or a plonk.Circuit (its q_N is zero); an R1csCircuit of the other rule is proved here as it is."""
    TAKES_NEXT = True

    def __init__(self, kzg, circuit):
        if not isinstance(circuit, Circuit):
            raise ZkError("%s: the key takes a Circuit" % WHO)
        if hasattr(circuit, "table"):
            raise ZkError("%s: a LookupCircuit is proved with plonk_lookup.py: this prover has no lookups" % WHO)
        super().__init__(kzg, circuit, WHO, ("3n + 7", required_powers(circuit.n)))

    def _fixed(self, coef):
        self.coef = list(coef)

    def _build(self):
        super()._build()
        cv, n, k, c = self.curve, self.n, self.log_n, self.circuit
        qn = c.sel["qN"] if "qN" in c.sel else np.zeros((n, 4), np.uint64)
        self.qn_vals = self._keep(pa.mont_dev(cv, np.ascontiguousarray(qn)))
        qn_coef = self._keep(pa.interpolate(cv, self.qn_vals, n, 0, k))
        self.qn_coset = self._keep(pa.coset_evals(cv, qn_coef, n, k + 2))
        self.coef.append(qn_coef)
        self.commitments = [self.kzg.commit(d) for d in self.coef]
        self.vk = VerifyingKey(cv, k, c.n_public, self.k1, self.k2, self.commitments, self.kzg)


def setup(kzg, circuit):
    """-> NextKey(kzg, circuit); its .vk is the verification key"""
    return NextKey(kzg, circuit)


# ---- the prover -----------------------------------------------------------------------------------------------------------------------------
def prove(key, witness, blinding=None, self_check=True, _wires=None, _opening_transcript=None, _mark=None):
    """-> (proof, publics).  witness: as plonk.prove takes it: n_vars values below r, or on a key over an R1csCircuit the n_wires values of
    the .wtns or its bytes.  proof is a mapping with A, B, C, Z, T, W1, W2 (points) and values (the 16 integers of VALUE_NAMES); publics the l
    public inputs.  The gate equation -- with the next row's c -- is checked first, row by row, and a witness that fails names the first
    row (a row that fails only through its next-row term is named like any other; over an R1csCircuit with the gate and its constraint);
    the permutation product must close.  Before returning, the proof is verified (self_check=False skips it).  blinding: ten integers, FOR
    TESTS ONLY.  _wires, _opening_transcript, _mark: hooks of the tests and of tools/plonk_next_time.py."""
    cv, n, k, kzg = key.curve, key.n, key.log_n, key.kzg
    mark = _mark or (lambda name: None)
    own = []

    def keep(d):
        own.append(d)
        return d

    def check(vals, pi_vals):
        return gate_check(vals + key.sel_vals + [pi_vals, key.qn_vals], n, cv)
    try:
        vals, pi_vals, publics, bs = pa.witness_columns(key, witness, blinding, _wires, WHO, keep, mark, n_blinders=N_BLINDERS, check=check)
        # round 1: a and b with two blinders, c with three
        coef = [keep(pa.interpolate(cv, v, n, e, k)) for v, e in zip(vals, (2, 2, 3))]
        pa.blind(cv, coef[0], n, [bs[1], bs[0]])
        pa.blind(cv, coef[1], n, [bs[3], bs[2]])
        pa.blind(cv, coef[2], n, [bs[6], bs[5], bs[4]])
        n_coef = (n + 2, n + 2, n + 3)
        A, B, Cc = [kzg.commit(d) for d in coef]
        c0 = transcript_start(cv, key.vk.digest, publics)
        c1, beta, gamma = transcript_wires(cv, c0, A, B, Cc)
        mark("round 1")
        # round 2 (permutation_product reads its three blinders at 6, 7, 8)
        z_coef = pa.permutation_product(key, vals, beta, gamma, [0] * 6 + bs[7:10], WHO, keep)
        Z = kzg.commit(z_coef)
        c2, alpha = transcript_product(cv, c1, Z)
        mark("round 2")
        # round 3
        pi_coef = keep(pa.interpolate(cv, pi_vals, n, 0, k))
        cols = [keep(pa.coset_evals(cv, d, m, k + 2)) for d, m in zip(coef, n_coef)] + [keep(pa.coset_evals(cv, z_coef, n + 3, k + 2))] + key.coset
        cols += [keep(pa.coset_evals(cv, pi_coef, n, k + 2)), key.l1_coset, key.x_coset, key.qn_coset]
        t = keep(quotient(cols, k, alpha, beta, gamma, key.k1, key.k2, cv))
        t_view = pa.quotient_coeffs(cv, k, t, required_powers(n), WHO + ": the quotient has %d non-zero coefficients from 3n + 7 = %d on: the identity does not hold on H", keep)
        T = kzg.commit(t_view)
        c3, zeta = transcript_quotient(cv, c2, T, n)
        mark("round 3")
        # rounds 4 and 5
        state = {}

        def opening_gamma(curve, commitments, sets, values):
            state["c4"], g = transcript_values(curve, c3, _proof_order(values))
            return g

        def opening_z(curve, g, W1, avoid=()):
            return transcript_z(curve, state["c4"], W1, avoid)
        polys = key.coef + [View(d, 0, m) for d, m in zip(coef, n_coef)] + [t_view, View(z_coef, 0, n + 3)]
        values, W1, W2, _, _ = kzg.open_multi(polys, _sets(cv, k, zeta), transcript=_opening_transcript or opening_gamma,
                                              transcript_z=opening_z if _opening_transcript is None else pa.plain_z, commitments=key.commitments + [A, B, Cc, T, Z])
        mark("round 5")
        proof = {"A": A, "B": B, "C": Cc, "Z": Z, "T": T, "values": _proof_order(values), "W1": W1, "W2": W2}
    finally:
        for d in own:
            d.free()
    if self_check:
        verdict, _ = verify(key.vk, [publics], [proof])
        if verdict != ACCEPTED:
            raise ZkError("%s: the proof just made is not accepted (verdict %d)" % (WHO, verdict))
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
    """the identity of round 3 at zeta in the field, from the 16 values: the bracket, with q_N(zeta) c(zeta w) in it, equals t(zeta) Z_H(zeta)"""
    v, alpha = dict(zip(VALUE_NAMES, values)), ch["alpha"]
    gate, perm, l1z, zh = pa.identity_terms(curve, log_n, k1, k2, publics, ch["zeta"], v, ch["beta"], ch["gamma"])
    return (gate + v["qN"] * v["cw"] + alpha * perm + alpha * alpha * l1z - v["t"] * zh) % FR[curve] == 0


def host_check(vk, publics, proof, point_bytes=None):
    """what the verifier decides on the host, before any device work: lengths (an error), every scalar below r (else INPUT_NOT_CANONICAL),
    the challenges, the identity (else REJECTED) -> (verdict, the tuple Kzg.verify_multi takes, built with the verifier's OWN gamma' and z')"""
    cv, r = vk.curve, FR[vk.curve]
    shape = pa.check_proof_shape(proof, POINT_NAMES, N_VALUES, point_bytes if point_bytes is not None else len(vk.commitments[0]), vk.n_public, publics, r, WHO)
    if shape is None:
        return INPUT_NOT_CANONICAL, None
    values, publics = shape
    ch = challenges(vk, publics, proof)
    if not identity_holds(cv, vk.log_n, vk.k1, vk.k2, publics, values, ch):
        return REJECTED, None
    cs = vk.commitments + [proof["A"], proof["B"], proof["C"], proof["T"], proof["Z"]]
    return ACCEPTED, (cs, _sets(cv, vk.log_n, ch["zeta"]), _opening_order(values), ch["gamma_open"], ch["z_open"], proof["W1"], proof["W2"])


def verify(vk, publics, proofs, kzg=None, seed=None, locate=True):
    """m proofs under one verification key: publics[i] are proof i's public inputs -> (verdict, first_bad) as Kzg.verify_multi gives them.
    The host part of every proof first (host_check), then ONE randomised pairing check of all of them: two pairings.  kzg: the handle to pair
    with, when the key does not carry one.  seed: 32 bytes for the weights, FOR TESTS ONLY."""
    return pa.verify_batch(vk, publics, proofs, host_check, kzg, seed, locate, WHO)
