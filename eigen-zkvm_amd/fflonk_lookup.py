"""fflonk with lookups: the log-derivative lookup argument of plonk_lookup.py on the interleaved commitments of fflonk.py
(DESIGN.md 3.23): setup, prove, verify.  A fourth protocol on the arithmetisation of plonk_arith.py.  A verification key of
TWO G1 points, a proof of five G1 points and 22 scalars, two pairings for m proofs.  The protocol, the transcript and the files are this
module; everything over Fr of size n or more runs on the device: the layer's calls, the argument's zk_plonk_<curve>_lookup_table_new /
_lookup_count_dev / _lookup_terms_dev / _lookup_summands_dev with zk_fr_<curve>_batch_inverse_dev and _prefix_sum_dev, the four numerators
from ONE launch of zk_fflonk_<curve>_lookup_quotients_dev, zk_kzg_<curve>_interleave_dev and Kzg.open_multi.  There is no CPU fallback.
This is the project's own transcript (SHA-256), not snarkjs's keccak or its file formats.  It imports nothing from plonk.py; keys and proofs
of plonk.py, fflonk.py and plonk_lookup.py are refused here, as this module's are there.

Field, circuit (plonk_lookup.LookupCircuit, the same .npz), wiring, k_1, k_2, sigma, H, w = 7^((r - 1) / n), n = 2^k >= 8 (holds the public
rows, the gates and the table), the public rows and PI, the padding of the table by repeating its last row, the multiplicity rule (the
smallest index of a repeated row takes the whole count), f = a + eta b + eta^2 c and t = t1 + eta t2 + eta^2 t3 are plonk_lookup.py's.
interleave_t(f_0 .. f_(t-1)) = sum_m f_m(X^t) X^m is fflonk.py's.

Setup.  C0 = interleave_8 of the eight fixed polynomials in FIXED_NAMES order (8n coefficients), exactly fflonk.py's;
C0L = interleave_4(q_K, t1, t2, t3) (4n coefficients).  The key is curve, k, l, k_1, k_2, [C0], [C0L].  The twelve fixed polynomials are
never committed one by one.  No secret, no key file.

Rounds.
 1. a, b, c from the witness, the gate equation checked row by row first, then the lookups; blinded as a += (b_1 X + b_2) Z_H (b: b_3,
    b_4; c: b_5, b_6).  m counted on the device, interpolated over H and blinded as M += (b_10 X + b_11) Z_H.
    C1 = interleave_4(a, b, c, M), 4n + 8 coefficients; [C1].  M is committed before eta and delta exist; T0 depends on a, b, c alone, so it
    can move to round 2, and leaves C1 for M.
 2. beta, gamma, eta, delta.  Z by frpoly.terms and grand_product, which must close; Z += (b_7 X^2 + b_8 X + b_9) Z_H, n + 3 coefficients.
    phi_0 = 0, phi_(i+1) = phi_i + qK_i / (delta + f_i) - m_i / (delta + t_i) by lookup_terms, ONE batch_inverse over 2n, lookup_summands
    and prefix_sum, which must close with phi_n = 0 (a zero denominator is named by its row); Phi += (b_12 X^2 + b_13 X + b_14) Z_H, n + 3
    coefficients.  Four quotients, each a numerator on the coset 7 H_4n -> divide_zh_coset -> the inverse coset transform:
      T0 = (a b q_M + a q_L + b q_R + c q_O + q_C + PI) / Z_H, 2n + 2 coefficients
      T1 = L_1 (Z - 1) / Z_H, n + 2 coefficients
      T2 = [(a + beta X + gamma)(b + beta k_1 X + gamma)(c + beta k_2 X + gamma) Z
            - (a + beta S_sigma1 + gamma)(b + beta S_sigma2 + gamma)(c + beta S_sigma3 + gamma) Z(wX)] / Z_H, 3n + 6 coefficients
      T3 = L / Z_H, L = (Phi(wX) - Phi(X)) (delta + f)(delta + t) - q_K (delta + t) + M (delta + f); deg L <= 3n + 2: 2n + 3 coefficients
    The four numerators leave ONE launch of zk_fflonk_<curve>_lookup_quotients_dev; the coefficients from 2n + 2, n + 2, 3n + 6 and 2n + 3
    on must be zero (batch_inverse's zero count), else prove raises with the polynomial's name and the count.
    C2 = interleave_4(Z, Phi, T0, T1), 8n + 8 coefficients; C3 = interleave_2(T2, T3), 6n + 12 coefficients; [C2], [C3].
    The file must hold 8n + 8 G1 powers (one of power k + 3 does, the power fflonk.py needs).
 3. one seed s, no root extracted: h0 = s, h1 = s^2, h3 = s^4, xi = s^8, so h0^8 = h1^4 = h3^2 = xi.  w_8 = w^(n/8), w_4 = w_8^2,
    w_4n = 7^((r - 1) / (4n)), so w_4n^4 = w and (h1 w_4n)^4 = xi w.  s is drawn again while s = 0 or xi^n = 1.  The opening sets:
      S0 = {h0 w_8^j : j < 8} for C0
      S1 = {h1 w_4^j : j < 4} for C0L and for C1 (the same set twice)
      S2 = {h1 w_4^j : j < 4} then {h1 w_4n w_4^j : j < 4} for C2 (8 points, distinct because n >= 8)
      S3 = {h3, -h3} for C3
    26 opened values.  k + 2 must not exceed the field's 2-adicity, which the coset already requires.
 4. ONE Kzg.open_multi([C0, C0L, C1, C2, C3], [S0, S1, S1, S2, S3]) under this module's gamma' and z'.  The 22 values -- the 12 fixed in
    plonk_lookup.FIXED order, a, b, c, M, Z, Phi at xi, then Z, Phi, T0, T1 at xi w -- come from the 26 opened values on the host by
    fflonk.parts_of.  T0 .. T3 at xi recovered the same way must be what the identities give (the prover's free self check).
The proof is [C1], [C2], [C3], W1, W2 and the 22 values.  The opening's own challenges are NOT in it: the verifier derives them.

Verifier.  Lengths; every scalar below r (else INPUT_NOT_CANONICAL); every challenge recomputed; PI(xi); T0, T1, T2 at xi from the 22 values
by plonk_arith.identity_terms and T3 by plonk_lookup.lookup_term, each over Z_H(xi); the 26 opened values rebuilt with fflonk.host_values:
the 8 fixed on S0, (q_K, t1, t2, t3) on S1, (a, b, c, M) on S1, (Z, Phi, T0, T1)(xi) on the first half of S2 and (Z, Phi, T0, T1)(xi w) on the
second, (T2, T3)(xi) on S3; then ONE Kzg.verify_multi for all m proofs.  There is no alpha and no separate identity check.

Transcript.  Conventions as in fflonk.py: H is SHA-256; a digest is read as a big-endian integer and reduced mod r; a scalar is 32
little-endian bytes; a point is point_bytes bytes in the .ptau file's encoding; "curve" is the name in ASCII; a counter is one byte that
starts at 0 and only moves for a re-draw.
    vkd    = H(curve || "fflonkl-vk" || k u32le || l u32le || k_1 || k_2 || C0 || C0L)
    c0     = H(curve || "fflonkl-v1" || vkd || l u32le || x_0 .. x_(l-1))
    c1     = H(c0 || C1)                     beta, gamma, eta, delta = H(c1 || 00 / 01 / 02 / 03)
    c2     = H(c1 || C2 || C3)               s = H(c2 || ctr)
    c3     = H(c2 || the 22 values)          gamma' = H(c3 || 00)   z' = H(c3 || 01 || W1 || ctr), outside every opening point

Blinding.  The fourteen blinders come from `secrets`, in plonk_lookup.py's numbering; blinding=[14 integers] is FOR TESTS ONLY (all zero
gives the unblinded proof).

Not built: tables of another width than three, several tables in one circuit (the tagged lookups of plonk_lookup.py, DESIGN.md 3.26: the
interleaved C0L has four slots, and a fifth polynomial T0 changes its opening sets; setup refuses a tagged circuit and says so), lookups in
a circuit compiled from an .r1cs, snarkjs's files or its keccak transcript, a Solidity verifier."""
import hashlib
import json

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import frpoly as fp
from . import plonk_arith as pa
from .fflonk import host_values, interleave_dev, parts_of
from .groth16 import _NAME
from .kzg import _scalar, point_from_json, point_to_json, to_mont
from .plonk_arith import ACCEPTED, FIXED_NAMES, FR, INPUT_NOT_CANONICAL, REJECTED, ArithKey, R1csCircuit, View, check_size, draw, draw_until, le, modulus, omega, smallest_power
from .plonk_lookup import LookupCircuit, LookupTable, count, lookup_term, range_table, summands, terms, xor_table

WHO = "fflonk lookup"
N_VALUES, N_OPENED, N_FIXED, N_BLINDERS = 22, 26, 12, 14
LOOKUP_FIXED = ("qK", "T1", "T2", "T3")
FIXED = FIXED_NAMES + LOOKUP_FIXED        # plonk_lookup.FIXED
POINT_NAMES = ("C1", "C2", "C3", "W1", "W2")
VALUE_NAMES = FIXED + ("a", "b", "c", "M", "Z", "Phi", "Zw", "Phiw", "T0w", "T1w")
PROTOCOL = "fflonk-shplonk-lookup"
CIRCUIT = "LookupCircuit"                 # the class tools/plonk_cli.py loads a circuit file with
QUOTIENT_NAMES = ("T0", "T1", "T2", "T3")
QUOTIENT_COLS = 21                        # ZK_FFLONK_LOOKUP_QUOTIENT_COLS


def required_powers(n):
    """the G1 powers the file must hold: C2 = interleave_4(Z, Phi, T0, T1) has 4 (2n + 2) = 8n + 8 coefficients (C3 has 6n + 12)"""
    return 8 * n + 8


def file_power(log_n):
    """the smallest power of a .ptau file that holds them for n = 2^log_n rows: k + 3"""
    return smallest_power(required_powers(1 << log_n))


def quotient_coeffs(n):
    """the coefficients of T0, T1, T2, T3"""
    return 2 * n + 2, n + 2, 3 * n + 6, 2 * n + 3


# ---- the field on the host ----------------------------------------------------------------------------------------------------------------
def roots(curve, log_n, s):
    """the seed s -> a mapping with h0, h1, h3, xi, xiw and the four opening sets S0, S1, S2, S3 in the order of round 3"""
    r, n = modulus(curve), 1 << log_n
    check_size(curve, log_n)
    if log_n < 3:
        raise ZkError("%s: n = 2^%d rows: a circuit has at least 8" % (WHO, log_n))
    w = omega(curve, log_n)
    w8, w4n = pow(w, n // 8, r), omega(curve, log_n + 2)
    w4 = w8 * w8 % r
    h0, h1, h3 = s % r, pow(s, 2, r), pow(s, 4, r)
    xi = pow(s, 8, r)
    S1 = [h1 * pow(w4, j, r) % r for j in range(4)]
    return {"h0": h0, "h1": h1, "h3": h3, "xi": xi, "xiw": xi * w % r, "S0": [h0 * pow(w8, j, r) % r for j in range(8)], "S1": S1,
            "S2": S1 + [h1 * w4n % r * pow(w4, j, r) % r for j in range(4)], "S3": [h3, (r - h3) % r]}


def all_points(rt):
    """every opening point of a proof, for z' to avoid"""
    return rt["S0"] + rt["S2"] + rt["S3"]


def quotients_at(curve, log_n, k1, k2, publics, ch, xi, v):
    """(T0, T1, T2, T3)(xi) in the field from the values v[name] of VALUE_NAMES (Zw, Phiw at xi w; T0w, T1w are not read): what the
    identities give.  ch: a mapping with beta, gamma, eta, delta"""
    r = FR[curve]
    gate, perm, l1z, zh = pa.identity_terms(curve, log_n, k1, k2, publics, xi, v, ch["beta"], ch["gamma"])
    zh_inv = pow(zh, -1, r)
    return tuple(t * zh_inv % r for t in (gate, l1z, perm, lookup_term(curve, v, ch["eta"], ch["delta"])))


def opened_values(curve, log_n, k1, k2, publics, values, ch, rt):
    """the 26 values the opening must have, from the proof's 22 and the roots rt = roots(..) -> [on S0, on S1 (C0L), on S1 (C1), on S2, on S3]"""
    v = dict(zip(VALUE_NAMES, values))
    t0, t1, t2, t3 = quotients_at(curve, log_n, k1, k2, publics, ch, rt["xi"], v)
    return [host_values(curve, list(values[:8]), rt["S0"]), host_values(curve, list(values[8:12]), rt["S1"]), host_values(curve, [v["a"], v["b"], v["c"], v["M"]], rt["S1"]),
            host_values(curve, [v["Z"], v["Phi"], t0, t1], rt["S2"][:4]) + host_values(curve, [v["Zw"], v["Phiw"], v["T0w"], v["T1w"]], rt["S2"][4:]),
            host_values(curve, [t2, t3], rt["S3"])]


def values_of(curve, opened, rt):
    """the proof's 22 values and (T0, T1, T2, T3)(xi) from the 26 opened ones -> (values, (t0, t1, t2, t3))"""
    fixed = parts_of(curve, opened[0], rt["S0"]) + parts_of(curve, opened[1], rt["S1"])
    wires_m = parts_of(curve, opened[2], rt["S1"])
    z, phi, t0, t1 = parts_of(curve, opened[3][:4], rt["S2"][:4])
    t2, t3 = parts_of(curve, opened[4], rt["S3"])
    return fixed + wires_m + [z, phi] + parts_of(curve, opened[3][4:], rt["S2"][4:]), (t0, t1, t2, t3)


# ---- the transcript -----------------------------------------------------------------------------------------------------------------------
def vk_digest(curve, log_n, n_public, k1, k2, c0_point, c0l_point):
    """vkd = H(curve || "fflonkl-vk" || k u32le || l u32le || k_1 || k_2 || C0 || C0L)"""
    return hashlib.sha256(curve.encode("ascii") + b"fflonkl-vk" + int(log_n).to_bytes(4, "little") + int(n_public).to_bytes(4, "little") + le(k1) + le(k2) + bytes(c0_point) +
                          bytes(c0l_point)).digest()


def transcript_start(curve, vkd, publics):
    """c0 = H(curve || "fflonkl-v1" || vkd || l u32le || x_0 .. x_(l-1))"""
    return hashlib.sha256(curve.encode("ascii") + b"fflonkl-v1" + vkd + len(publics).to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()


def transcript_round1(curve, c0, C1):
    """c1 = H(c0 || C1); beta, gamma, eta, delta = H(c1 || 00 .. 03) -> (c1, beta, gamma, eta, delta)"""
    c1 = hashlib.sha256(c0 + bytes(C1)).digest()
    return (c1,) + tuple(draw(curve, c1, bytes([i])) for i in range(4))


def transcript_round2(curve, c1, C2, C3, log_n):
    """c2 = H(c1 || C2 || C3); s = H(c2 || ctr), ctr one byte from 0, drawn again while s = 0 or xi^n = 1 with xi = s^8 -> (c2, s)"""
    r = FR[curve]
    c2 = hashlib.sha256(c1 + bytes(C2) + bytes(C3)).digest()
    return c2, draw_until(curve, c2, lambda s: s != 0 and pow(s, 8 << log_n, r) != 1, "%s: no seed" % WHO)


def transcript_values(curve, c2, values):
    """c3 = H(c2 || the 22 values, 32 little-endian bytes each); gamma' = H(c3 || 00) -> (c3, gamma')"""
    c3 = hashlib.sha256(c2 + b"".join(le(v) for v in values)).digest()
    return c3, draw(curve, c3, b"\x00")


def transcript_z(curve, c3, W1, avoid):
    """z' = H(c3 || 01 || W1 || ctr), ctr one byte from 0, drawn again while z' is one of the opening points"""
    avoid = {int(p) for p in avoid}
    return draw_until(curve, c3 + b"\x01" + bytes(W1), lambda z: z not in avoid, "%s: no opening challenge" % WHO)


# ---- the device call that is this protocol's ----------------------------------------------------------------------------------------------
def quotients(cols, log_n, beta, gamma, k1, k2, eta, delta, curve="BN128", outs=None, want=(True, True, True, True)):
    """zk_fflonk_<curve>_lookup_quotients_dev: cols, 21 DevArrays of 4n elements -- the 15 of zk_plonk_<curve>_quotient_dev in their order,
    then q_K, t1, t2, t3, M, Phi -> [out0, out1, out2, out3] on the coset: the gate numerator with PI, L_1 (Z - 1), the permutation
    difference, the lookup argument's L.  want[j] false: output j is not computed (None in its place) and the columns it alone reads are not
    read.  outs: four DevArrays (or None) to write into."""
    modulus(curve)
    m = 4 << int(log_n)
    if len(cols) != QUOTIENT_COLS:
        raise ZkError("%s: the quotients take %d columns, not %d" % (WHO, QUOTIENT_COLS, len(cols)))
    sc = [_scalar(v, curve, w) for v, w in ((beta, "beta"), (gamma, "gamma"), (k1, "k1"), (k2, "k2"), (eta, "eta"), (delta, "delta"))]
    if any(c.n < 4 * m for c in cols):
        raise ZkError("%s: every column of the quotients holds 4n = %d elements" % (WHO, m))
    outs = list(outs) if outs is not None else [None] * 4
    if len(outs) != 4 or len(want) != 4:
        raise ZkError("%s: the quotients have four outputs" % WHO)
    if any(o is not None and o.n < 4 * m for o in outs):
        raise ZkError("%s: every output of the quotients holds 4n = %d elements" % (WHO, m))
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    made = []
    try:
        for j in range(4):
            if want[j] and outs[j] is None:
                outs[j] = DevArray(4 * m)
                made.append(outs[j])
            elif not want[j]:
                outs[j] = None
        _check(getattr(lib(), "zk_fflonk_%s_lookup_quotients_dev" % _NAME[curve])(_ptr(ptrs), int(log_n), *[_ptr(s) for s in sc], *[o.ptr if o is not None else None for o in outs], 0))
        return outs
    except Exception:
        for d in made:
            d.free()
        raise


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    """(curve, log n, l, k_1, k_2, [C0], [C0L]); `kzg` is the handle verify() pairs with, when the key came from an FflonkLookupKey"""

    def __init__(self, curve, log_n, n_public, k1, k2, c0, c0l, kzg=None):
        modulus(curve)
        self.curve, self.log_n, self.n_public, self.k1, self.k2 = curve, int(log_n), int(n_public), int(k1), int(k2)
        self.c0, self.c0l, self.kzg = bytes(c0), bytes(c0l), kzg
        check_size(curve, self.log_n)
        if self.log_n < 3:
            raise ZkError("%s: n = 2^%d rows: a circuit has at least 8" % (WHO, self.log_n))
        if len(self.c0) != len(self.c0l):
            raise ZkError("%s: the two points of a verification key have one length" % WHO)
        self.n = 1 << self.log_n
        self.digest = vk_digest(curve, self.log_n, self.n_public, self.k1, self.k2, self.c0, self.c0l)


def vk_to_json(vk):
    return json.dumps({"protocol": PROTOCOL, "curve": vk.curve, "log_n": vk.log_n, "n_public": vk.n_public, "k1": str(vk.k1), "k2": str(vk.k2),
                       "C0": point_to_json(vk.c0, vk.curve), "C0L": point_to_json(vk.c0l, vk.curve)}, indent=1) + "\n"


def vk_from_json(text, kzg=None):
    js = json.loads(text)
    if js.get("protocol") != PROTOCOL:
        raise ZkError('%s: not a verification key of this prover (protocol "%s")' % (WHO, js.get("protocol")))
    return VerifyingKey(js["curve"], js["log_n"], js["n_public"], int(js["k1"], 0), int(js["k2"], 0), point_from_json(js["C0"], js["curve"]), point_from_json(js["C0L"], js["curve"]), kzg)


def proof_to_json(proof, curve):
    return pa.proof_to_json(proof, curve, PROTOCOL, POINT_NAMES)


def proof_from_json(text, curve):
    return pa.proof_from_json(text, curve, PROTOCOL, POINT_NAMES, WHO)


def proof_to_bytes(proof):
    """C1 || C2 || C3 || W1 || W2 || the 22 values, 32 little-endian bytes each"""
    return pa.proof_to_bytes(proof, POINT_NAMES)


def proof_from_bytes(data, point_bytes):
    return pa.proof_from_bytes(data, point_bytes, POINT_NAMES, N_VALUES, (), WHO)


class FflonkLookupKey(ArithKey):
    """The proving key on the device: ArithKey's columns; beside them q_K and the table's three columns on H and on the coset, the hash table
    over the padded table's rows, the 8n coefficients of C0 and the 4n of C0L, and the points [C0], [C0L].  The twelve fixed polynomials are
    NOT committed one by one, and their own coefficient vectors do not outlive the interleaving.  Setup is deterministic and has no secret.
    self.vk is the verification key."""
    KEEPS_COEF = False

    def __init__(self, kzg, circuit):
        if isinstance(circuit, R1csCircuit):
            raise ZkError("%s: an R1csCircuit has no lookups: prove it with fflonk.py" % WHO)
        if not isinstance(circuit, LookupCircuit):
            raise ZkError("%s: the key takes a LookupCircuit" % WHO)
        if getattr(circuit, "tagged", False):
            raise ZkError("%s: the circuit has %d tagged tables: fflonk with lookups proves one table (C0L interleaves four polynomials and has no slot for T0); "
                          "plonk_lookup.py proves a tagged circuit" % (WHO, len(circuit.table_sizes)))
        self.table = None
        super().__init__(kzg, circuit, WHO, ("8n + 8", required_powers(circuit.n)))

    def _fixed(self, coef):
        self.c0_coef = self._keep(interleave_dev(coef, [self.n] * 8, self.curve))

    def _build(self):
        super()._build()
        cv, n, k, c = self.curve, self.n, self.log_n, self.circuit
        self.qk_vals = self._keep(pa.mont_dev(cv, c.sel["qK"]))
        self.t_vals = [self._keep(pa.mont_dev(cv, np.ascontiguousarray(c.table[j]))) for j in range(3)]
        self.table = LookupTable(*self.t_vals, n, cv)
        more = []
        try:
            for v in [self.qk_vals] + self.t_vals:
                more.append(pa.interpolate(cv, v, n, 0, k))
            self.lookup_coset = [self._keep(pa.coset_evals(cv, d, n, k + 2)) for d in more]
            self.c0l_coef = self._keep(interleave_dev(more, [n] * 4, cv))
        finally:
            for d in more:
                d.free()
        self.c0, self.c0l = self.kzg.commit(self.c0_coef), self.kzg.commit(self.c0l_coef)
        self.vk = VerifyingKey(cv, k, c.n_public, self.k1, self.k2, self.c0, self.c0l, self.kzg)

    def free(self):
        if getattr(self, "table", None) is not None:
            self.table.free()
            self.table = None
        super().free()


def setup(kzg, circuit):
    """-> FflonkLookupKey(kzg, circuit); its .vk is the verification key"""
    return FflonkLookupKey(kzg, circuit)


# ---- the prover -----------------------------------------------------------------------------------------------------------------------------
NOT_ZERO = WHO + ": %s has %%d non-zero coefficients from %%d on: the identity does not hold on H"


def lookup_sum(key, vals, m_vals, eta, delta, bs, keep):
    """phi_0 = 0, phi_(i+1) = phi_i + qK_i / (delta + f_i) - m_i / (delta + t_i), which must close with phi_n = 0;
    Phi += (b_12 X^2 + b_13 X + b_14) Z_H -> Phi's n + 3 coefficients"""
    cv, n = key.curve, key.n
    d = keep(terms(vals + key.t_vals, n, eta, delta, cv))
    _, zeros, first = fp.batch_inverse(d, cv, out=d)
    if zeros:
        raise ZkError("%s: the denominator delta + %s of row %d is zero (%d zero denominators in all)" % (WHO, "f" if first < n else "t", first % n, zeros))
    s = keep(summands(d, key.qk_vals, m_vals, n, cv))
    phi, last = fp.prefix_sum(s, cv, out=s)
    if last != 0:
        raise ZkError("%s: the lookup sum does not close (phi_n = %d): the multiplicities are not those of the selected rows" % (WHO, last))
    phi_coef = keep(pa.interpolate(cv, phi, n, 3, key.log_n))
    pa.blind(cv, phi_coef, n, [bs[13], bs[12], bs[11]])
    return phi_coef


def prove(key, witness, blinding=None, self_check=True, _wires=None, _multiplicities=None, _opening_transcript=None, _mark=None):
    """-> (proof, publics).  witness: n_vars values below r (integers, 32-byte little-endian values, or (n_vars, 4) u64 words).  proof is a
    mapping with C1, C2, C3, W1, W2 (points, point_bytes each) and values (22 integers in VALUE_NAMES order); publics the l public inputs.
    The gate equation is checked first, row by row, then the lookups: a selected row whose (a, b, c) is no row of the table is named with the
    count of such rows; the permutation product and the lookup sum must close.  Before returning, the proof is verified (self_check=False
    skips it).  blinding: fourteen integers, FOR TESTS ONLY.  _wires, _opening_transcript, _mark: hooks of the tests and of
    tools/fflonk_lookup_time.py, and _wires skips no check; _multiplicities (n integers, FOR TESTS ONLY) replaces the counted m."""
    cv, n, k, kzg = key.curve, key.n, key.log_n, key.kzg
    mark = _mark or (lambda name: None)
    ncs = quotient_coeffs(n)
    own = []

    def keep(d):
        own.append(d)
        return d
    try:
        vals, pi_vals, publics, bs = pa.witness_columns(key, witness, blinding, _wires, WHO, keep, mark, n_blinders=N_BLINDERS)
        m_vals, bad, first = count(key.table, vals[0], vals[1], vals[2], key.qk_vals, n)
        keep(m_vals)
        if bad:
            raise ZkError("%s: witness does not satisfy lookup at row %d (%d rows): (a, b, c) is not a row of the table" % (WHO, first, bad))
        if _multiplicities is not None:
            if len(_multiplicities) != n:
                raise ZkError("%s: _multiplicities takes n values" % WHO)
            m_vals = keep(DevArray.from_host(to_mont(_multiplicities, cv).reshape(-1)))
        mark("lookup check")
        # round 1: M is committed before eta and delta exist
        coef = pa.blinded_wires(key, vals, bs, keep)
        m_coef = keep(pa.interpolate(cv, m_vals, n, 2, k))
        pa.blind(cv, m_coef, n, [bs[10], bs[9]])
        c1_coef = keep(interleave_dev(coef + [m_coef], [n + 2] * 4, cv))
        C1 = kzg.commit(c1_coef)
        c0h = transcript_start(cv, key.vk.digest, publics)
        c1h, beta, gamma, eta, delta = transcript_round1(cv, c0h, C1)
        ch = {"beta": beta, "gamma": gamma, "eta": eta, "delta": delta}
        mark("round 1")
        # round 2: both sums, then every column on the coset and the four numerators from one launch
        z_coef = pa.permutation_product(key, vals, beta, gamma, bs, WHO, keep)
        phi_coef = lookup_sum(key, vals, m_vals, eta, delta, bs, keep)
        pi_coef = keep(pa.interpolate(cv, pi_vals, n, 0, k))
        cols = [keep(pa.coset_evals(cv, d, n + 2, k + 2)) for d in coef] + [keep(pa.coset_evals(cv, z_coef, n + 3, k + 2))] + key.coset
        cols += [keep(pa.coset_evals(cv, pi_coef, n, k + 2)), key.l1_coset, key.x_coset] + key.lookup_coset
        cols += [keep(pa.coset_evals(cv, m_coef, n + 2, k + 2)), keep(pa.coset_evals(cv, phi_coef, n + 3, k + 2))]
        ts = [keep(d) for d in quotients(cols, k, beta, gamma, key.k1, key.k2, eta, delta, cv)]
        views = [pa.quotient_coeffs(cv, k, d, nc, NOT_ZERO % name, keep) for d, nc, name in zip(ts, ncs, QUOTIENT_NAMES)]
        c2_coef = keep(interleave_dev([View(z_coef, 0, n + 3), View(phi_coef, 0, n + 3), views[0], views[1]], [n + 3, n + 3, ncs[0], ncs[1]], cv))
        c3_coef = keep(interleave_dev(views[2:], list(ncs[2:]), cv))
        C2, C3 = kzg.commit(c2_coef), kzg.commit(c3_coef)
        c2h, s = transcript_round2(cv, c1h, C2, C3, k)
        mark("round 2")
        # rounds 3 and 4
        rt = roots(cv, k, s)
        sets = [rt["S0"], rt["S1"], rt["S1"], rt["S2"], rt["S3"]]
        state = {}

        def opening_gamma(curve, commitments, sets_, opened):
            state["values"], state["t"] = values_of(curve, opened, rt)
            state["c3"], g = transcript_values(curve, c2h, state["values"])
            return g

        def opening_z(curve, g, W1, avoid=()):
            return transcript_z(curve, state["c3"], W1, avoid)

        def loose_gamma(curve, commitments, sets_, opened):
            state["values"], state["t"] = values_of(curve, opened, rt)
            return _opening_transcript(curve, commitments, sets_, opened)
        _, W1, W2, _, _ = kzg.open_multi([key.c0_coef, key.c0l_coef, c1_coef, c2_coef, c3_coef], sets, transcript=opening_gamma if _opening_transcript is None else loose_gamma,
                                         transcript_z=opening_z if _opening_transcript is None else pa.plain_z, commitments=[key.c0, key.c0l, C1, C2, C3])
        mark("round 4")
        values = state["values"]
        want_t = quotients_at(cv, k, key.k1, key.k2, publics, ch, rt["xi"], dict(zip(VALUE_NAMES, values)))
        if tuple(state["t"]) != tuple(want_t):
            at = [q for q, got, want in zip(QUOTIENT_NAMES, state["t"], want_t) if got != want]
            raise ZkError("%s: internal error: %s at xi is not what the identity gives from the opened values" % (WHO, ", ".join(at)))
        proof = {"C1": C1, "C2": C2, "C3": C3, "W1": W1, "W2": W2, "values": values}
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
    gamma, eta, delta, s, xi, gamma_open (gamma') and z_open (z')"""
    cv = vk.curve
    c0 = transcript_start(cv, vk.digest, publics)
    c1, beta, gamma, eta, delta = transcript_round1(cv, c0, proof["C1"])
    c2, s = transcript_round2(cv, c1, proof["C2"], proof["C3"], vk.log_n)
    c3, g = transcript_values(cv, c2, proof["values"])
    rt = roots(cv, vk.log_n, s)
    return {"beta": beta, "gamma": gamma, "eta": eta, "delta": delta, "s": s, "xi": rt["xi"], "gamma_open": g, "z_open": transcript_z(cv, c3, proof["W1"], all_points(rt))}


def host_check(vk, publics, proof, point_bytes=None):
    """what the verifier decides on the host, before any device work: lengths (an error), every scalar below r (else INPUT_NOT_CANONICAL), the
    challenges, the 26 values the opening must have -> (verdict, the tuple Kzg.verify_multi takes, built with the verifier's OWN gamma' and
    z').  The identities are not checked here: they are what the rebuilt values of T0 .. T3 make the opening enforce."""
    cv = vk.curve
    shape = pa.check_proof_shape(proof, POINT_NAMES, N_VALUES, point_bytes if point_bytes is not None else len(vk.c0), vk.n_public, publics, FR[cv], WHO)
    if shape is None:
        return INPUT_NOT_CANONICAL, None
    values, publics = shape
    ch = challenges(vk, publics, proof)
    rt = roots(cv, vk.log_n, ch["s"])
    ys = opened_values(cv, vk.log_n, vk.k1, vk.k2, publics, values, ch, rt)
    return ACCEPTED, ([vk.c0, vk.c0l, proof["C1"], proof["C2"], proof["C3"]], [rt["S0"], rt["S1"], rt["S1"], rt["S2"], rt["S3"]], ys, ch["gamma_open"], ch["z_open"], proof["W1"],
                      proof["W2"])


def verify(vk, publics, proofs, kzg=None, seed=None, locate=True):
    """m proofs under one verification key: publics[i] are proof i's public inputs -> (verdict, first_bad) as Kzg.verify_multi gives them.
    The host part of every proof first (host_check), then ONE randomised pairing check of all of them: two pairings.  kzg: the handle to pair
    with, when the key does not carry one.  seed: 32 bytes for the weights, FOR TESTS ONLY."""
    return pa.verify_batch(vk, publics, proofs, host_check, kzg, seed, locate, WHO)
