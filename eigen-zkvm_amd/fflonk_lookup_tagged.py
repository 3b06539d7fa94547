"""fflonk with TAGGED lookups: several tables in one circuit, bound by a tag column (plonk_lookup.py's tagged variant), on the
interleaved commitments of fflonk_lookup.py: setup, prove, verify.  A sixth protocol on the arithmetisation
of plonk_arith.py.  A verification key of TWO G1 points, a proof of five G1 points and 23 scalars, two pairings for m proofs.  The protocol,
the transcript and the files are this module; what it shares with fflonk_lookup.py, fflonk.py, plonk_lookup.py and plonk_arith.py is imported
from them, never copied.  Everything over Fr of size n or more runs on the device: the layer's calls, the tagged argument's
zk_plonk_<curve>_lookup_tagged_table_new / _tagged_count_dev / _tagged_terms_dev, _lookup_summands_dev with zk_fr_<curve>_batch_inverse_dev
and _prefix_sum_dev, the four numerators from ONE launch of zk_fflonk_<curve>_lookup_tagged_quotients_dev
(csrc/fflonk_lookup_tagged_impl.hip.h), zk_kzg_<curve>_interleave_dev and Kzg.open_multi.  There is no CPU fallback.  This is the project's own
transcript (SHA-256), not snarkjs's keccak or its file formats.  Keys and proofs of plonk.py, fflonk.py, plonk_lookup.py (both of its
protocols) and fflonk_lookup.py are refused here by name, as this module's are there.

Names.  DESIGN.md 3.26 calls the tag column T0, and plonk_lookup.TAGGED_FIXED ends in "T0"; fflonk calls its first quotient T0.  Among the
VALUES a bare T0 .. T3 is a fixed column -- the tag, then the table's three -- and T0w, T1w are quotients at xi w, as in fflonk_lookup.py.  In
prose the tag column is Tg, and T0 .. T3 are the four quotients.

Field, circuit (plonk_lookup.LookupCircuit(tables=[..]) with K = 2 .. 65535 tables, the same tagged .npz), wiring, k_1, k_2, sigma, H,
w = 7^((r - 1) / n), n = 2^k >= 8 (holds the public rows, the gates and the concatenated tables), the public rows and PI, the padding of the
table by repeating its last row, its tag included, q_K in {0 .. K} as a row's tag and its weight, the multiplicity rule
m_j = Tg_j x count (the smallest index of a repeated tagged row takes the whole count), f = a + eta b + eta^2 c + eta^3 q_K,
t = t1 + eta t2 + eta^2 t3 + eta^3 Tg and the soundness argument are plonk_lookup.py's tagged variant, unchanged.
interleave_t(f_0 .. f_(t-1)) = sum_m f_m(X^t) X^m is fflonk.py's.  An untagged LookupCircuit is refused by name: fflonk_lookup.py proves it.

Setup.  C0 = interleave_8 of the eight fixed polynomials in FIXED_NAMES order (8n coefficients), exactly fflonk.py's;
C0L = interleave_8(q_K, t1, t2, t3, Tg, 0, 0, 0) (8n coefficients: five polynomials need eight slots, three stay zero).  The key is curve, k,
l, k_1, k_2, [C0], [C0L]: still two points.  The thirteen fixed polynomials are never committed one by one.  No secret, no key file.

Rounds.
 1. a, b, c from the witness, the gate equation checked row by row first, then the lookups (a selected row that is no row of the table its
    q_K names is refused with row, count and table); blinded as in fflonk_lookup.py.  m counted on the device with its weight Tg,
    interpolated over H and blinded as M += (b_10 X + b_11) Z_H.  C1 = interleave_4(a, b, c, M), 4n + 8 coefficients; [C1].
 2. beta, gamma, eta, delta.  Z as in fflonk_lookup.py.  phi_0 = 0, phi_(i+1) = phi_i + qK_i / (delta + f_i) - m_i / (delta + t_i) by
    lookup_tagged_terms, ONE batch_inverse over 2n, lookup_summands and prefix_sum, which must close with phi_n = 0 (a zero denominator is
    named by its row); Phi += (b_12 X^2 + b_13 X + b_14) Z_H.  Four quotients, each a numerator on the coset 7 H_4n -> divide_zh_coset ->
    the inverse coset transform: T0, T1, T2 are fflonk_lookup.py's, and
      T3 = L / Z_H, L = (Phi(wX) - Phi(X)) (delta + f)(delta + t) - q_K (delta + t) + M (delta + f)
    with the tagged f and t.  The new terms eta^3 q_K and eta^3 Tg are fixed polynomials of degree below n, so deg L <= 3n + 2 still and the
    sizes 2n + 2, n + 2, 3n + 6, 2n + 3 do not move.  The four numerators leave ONE launch of
    zk_fflonk_<curve>_lookup_tagged_quotients_dev; the coefficients above those sizes must be zero, else prove raises with the polynomial's
    name and the count.  C2 = interleave_4(Z, Phi, T0, T1), 8n + 8 coefficients; C3 = interleave_2(T2, T3), 6n + 12 coefficients; [C2], [C3].
    The file must hold 8n + 8 G1 powers (one of power k + 3 does): C0L's 8n fit.
 3. the seed s, h0, h1, h3, xi, the redraw rule and the sets S0 .. S3 are fflonk_lookup.py's (roots).  C0L is opened on S0, the set C0 is
    opened on (the same set twice, as S1 is used twice there): [S0, S0, S1, S2, S3] for [C0, C0L, C1, C2, C3].  30 opened values.  all_points
    is unchanged.
 4. ONE Kzg.open_multi([C0, C0L, C1, C2, C3], [S0, S0, S1, S2, S3]) under this module's gamma' and z'.  The 23 values -- the 13 fixed in
    plonk_lookup.TAGGED_FIXED order, a, b, c, M, Z, Phi at xi, then Z, Phi, T0, T1 at xi w -- come from the 30 opened values on the host by
    fflonk.parts_of.  T0 .. T3 at xi recovered the same way must be what the identities give, and the three parts of C0L that parts_of
    recovers for slots 5 .. 7 must be zero (the prover's free self check).
The proof is [C1], [C2], [C3], W1, W2 and the 23 values.  The opening's own challenges are NOT in it: the verifier derives them.

Verifier.  As fflonk_lookup.py's: lengths; every scalar below r (else INPUT_NOT_CANONICAL); every challenge recomputed; PI(xi); T0, T1, T2
at xi by plonk_arith.identity_terms and T3 by plonk_lookup.lookup_term(.., tagged=True), each over Z_H(xi); the 30 opened values rebuilt with
fflonk.host_values: the 8 fixed on S0, (q_K, t1, t2, t3, Tg, 0, 0, 0) on S0, (a, b, c, M) on S1, (Z, Phi, T0, T1)(xi) and (.)(xi w) on the two
halves of S2, (T2, T3)(xi) on S3; then ONE Kzg.verify_multi for all m proofs.  There is no alpha and no separate identity check.

Transcript.  Conventions as in fflonk.py: H is SHA-256; a digest is read as a big-endian integer and reduced mod r; a scalar is 32
little-endian bytes; a point is point_bytes bytes in the .ptau file's encoding; "curve" is the name in ASCII; a counter is one byte that
starts at 0 and only moves for a re-draw.
    vkd    = H(curve || "fflonklt-vk" || k u32le || l u32le || k_1 || k_2 || C0 || C0L)
    c0     = H(curve || "fflonklt-v1" || vkd || l u32le || x_0 .. x_(l-1))
    c1     = H(c0 || C1)                     beta, gamma, eta, delta = H(c1 || 00 / 01 / 02 / 03)
    c2     = H(c1 || C2 || C3)               s = H(c2 || ctr)
    c3     = H(c2 || the 23 values)          gamma' = H(c3 || 00)   z' = H(c3 || 01 || W1 || ctr), outside every opening point
The protocol name in the JSON codecs is "fflonk-shplonk-lookup-tagged".

Blinding.  The fourteen blinders come from `secrets`, in plonk_lookup.py's numbering; blinding=[14 integers] is FOR TESTS ONLY (all zero
gives the unblinded proof).

Not built: tables wider than three, lookups in a circuit compiled from an .r1cs, a linearisation polynomial, snarkjs's files or its keccak
transcript, a C one-call prover."""
import hashlib
import json

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import fflonk_lookup as fl
from . import frpoly as fp
from . import plonk_arith as pa
from .fflonk import host_values, interleave_dev, parts_of
from .fflonk_lookup import all_points, file_power, quotient_coeffs, required_powers, roots, transcript_round1, transcript_round2, transcript_z
from .groth16 import _NAME
from .kzg import _scalar, point_from_json, point_to_json, to_mont
from .plonk_arith import ACCEPTED, FR, INPUT_NOT_CANONICAL, REJECTED, ArithKey, R1csCircuit, View, check_size, draw, le, modulus
from .plonk_lookup import MAX_TABLES, TAGGED_FIXED, LookupCircuit, LookupTable, count, lookup_term, range_table, summands, terms, xor_table

WHO = "fflonk lookup tagged"
N_VALUES, N_OPENED, N_FIXED, N_BLINDERS = 23, 30, 13, 14
FIXED = TAGGED_FIXED                      # the 8 of C0, then qK, T1, T2, T3 and the tag column T0 (Tg) of C0L
C0L_SLOTS = 8                             # interleave_8(q_K, t1, t2, t3, Tg, 0, 0, 0)
POINT_NAMES = fl.POINT_NAMES
VALUE_NAMES = FIXED + ("a", "b", "c", "M", "Z", "Phi", "Zw", "Phiw", "T0w", "T1w")
PROTOCOL = "fflonk-shplonk-lookup-tagged"
CIRCUIT = "LookupCircuit"                 # the class tools/plonk_cli.py loads a circuit file with
QUOTIENT_NAMES = fl.QUOTIENT_NAMES
QUOTIENT_COLS = 22                        # ZK_FFLONK_LOOKUP_TAGGED_QUOTIENT_COLS
OTHER_PROTOCOLS = {"plonk-shplonk": "plonk.py", "fflonk-shplonk": "fflonk.py", "plonk-shplonk-lookup": "plonk_lookup.py", "plonk-shplonk-lookup-tagged": "plonk_lookup.py",
                   "fflonk-shplonk-lookup": "fflonk_lookup.py"}


# ---- the field on the host ----------------------------------------------------------------------------------------------------------------
def quotients_at(curve, log_n, k1, k2, publics, ch, xi, v):
    """(T0, T1, T2, T3)(xi) in the field from the values v[name] of VALUE_NAMES (v["T0"] is the tag column; Zw, Phiw at xi w; T0w, T1w are not
    read): what the identities give.  ch: a mapping with beta, gamma, eta, delta"""
    r = FR[curve]
    gate, perm, l1z, zh = pa.identity_terms(curve, log_n, k1, k2, publics, xi, v, ch["beta"], ch["gamma"])
    zh_inv = pow(zh, -1, r)
    return tuple(t * zh_inv % r for t in (gate, l1z, perm, lookup_term(curve, v, ch["eta"], ch["delta"], tagged=True)))


def opened_values(curve, log_n, k1, k2, publics, values, ch, rt):
    """the 30 values the opening must have, from the proof's 23 and the roots rt = roots(..) -> [on S0 (C0), on S0 (C0L), on S1, on S2, on S3]"""
    v = dict(zip(VALUE_NAMES, values))
    t0, t1, t2, t3 = quotients_at(curve, log_n, k1, k2, publics, ch, rt["xi"], v)
    return [host_values(curve, list(values[:8]), rt["S0"]), host_values(curve, list(values[8:N_FIXED]) + [0] * (C0L_SLOTS - 5), rt["S0"]),
            host_values(curve, [v["a"], v["b"], v["c"], v["M"]], rt["S1"]),
            host_values(curve, [v["Z"], v["Phi"], t0, t1], rt["S2"][:4]) + host_values(curve, [v["Zw"], v["Phiw"], v["T0w"], v["T1w"]], rt["S2"][4:]),
            host_values(curve, [t2, t3], rt["S3"])]


def values_of(curve, opened, rt):
    """the proof's 23 values, (T0, T1, T2, T3)(xi) and the three parts of C0L's slots 5 .. 7 (zero in an honest opening) from the 30 opened
    values -> (values, (t0, t1, t2, t3), [z5, z6, z7])"""
    lookup = parts_of(curve, opened[1], rt["S0"])
    fixed = parts_of(curve, opened[0], rt["S0"]) + lookup[:5]
    wires_m = parts_of(curve, opened[2], rt["S1"])
    z, phi, t0, t1 = parts_of(curve, opened[3][:4], rt["S2"][:4])
    t2, t3 = parts_of(curve, opened[4], rt["S3"])
    return fixed + wires_m + [z, phi] + parts_of(curve, opened[3][4:], rt["S2"][4:]), (t0, t1, t2, t3), lookup[5:]


# ---- the transcript -----------------------------------------------------------------------------------------------------------------------
def vk_digest(curve, log_n, n_public, k1, k2, c0_point, c0l_point):
    """vkd = H(curve || "fflonklt-vk" || k u32le || l u32le || k_1 || k_2 || C0 || C0L)"""
    return hashlib.sha256(curve.encode("ascii") + b"fflonklt-vk" + int(log_n).to_bytes(4, "little") + int(n_public).to_bytes(4, "little") + le(k1) + le(k2) + bytes(c0_point) +
                          bytes(c0l_point)).digest()


def transcript_start(curve, vkd, publics):
    """c0 = H(curve || "fflonklt-v1" || vkd || l u32le || x_0 .. x_(l-1))"""
    return hashlib.sha256(curve.encode("ascii") + b"fflonklt-v1" + vkd + len(publics).to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()


def transcript_values(curve, c2, values):
    """c3 = H(c2 || the 23 values, 32 little-endian bytes each); gamma' = H(c3 || 00) -> (c3, gamma')"""
    c3 = hashlib.sha256(c2 + b"".join(le(v) for v in values)).digest()
    return c3, draw(curve, c3, b"\x00")


# ---- the device call that is this protocol's ----------------------------------------------------------------------------------------------
def quotients(cols, log_n, beta, gamma, k1, k2, eta, delta, curve="BN128", outs=None, want=(True, True, True, True)):
    """zk_fflonk_<curve>_lookup_tagged_quotients_dev: cols, 22 DevArrays of 4n elements -- the 21 of zk_fflonk_<curve>_lookup_quotients_dev in
    their order, then the tag column Tg -> [out0, out1, out2, out3] on the coset: the gate numerator with PI, L_1 (Z - 1), the permutation
    difference, the tagged lookup argument's L.  want[j] false: output j is not computed (None in its place) and the columns it alone reads
    are not read.  outs: four DevArrays (or None) to write into."""
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
        _check(getattr(lib(), "zk_fflonk_%s_lookup_tagged_quotients_dev" % _NAME[curve])(_ptr(ptrs), int(log_n), *[_ptr(s) for s in sc], *[o.ptr if o is not None else None for o in outs], 0))
        return outs
    except Exception:
        for d in made:
            d.free()
        raise


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    """(curve, log n, l, k_1, k_2, [C0], [C0L]); `kzg` is the handle verify() pairs with, when the key came from an FflonkLookupTaggedKey.  The
    shape is fflonk_lookup.VerifyingKey's; the digest is under this protocol's domain string"""

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
        raise ZkError('%s: not a verification key of this prover (protocol "%s")%s' % (WHO, js.get("protocol"), _belongs(js.get("protocol"))))
    return VerifyingKey(js["curve"], js["log_n"], js["n_public"], int(js["k1"], 0), int(js["k2"], 0), point_from_json(js["C0"], js["curve"]), point_from_json(js["C0L"], js["curve"]), kzg)


def _belongs(protocol):
    """the module a key or a proof of another protocol of the family belongs to, for the refusal"""
    return ": %s proves and verifies it" % OTHER_PROTOCOLS[protocol] if protocol in OTHER_PROTOCOLS else ""


def proof_to_json(proof, curve):
    return pa.proof_to_json(proof, curve, PROTOCOL, POINT_NAMES)


def proof_from_json(text, curve):
    return pa.proof_from_json(text, curve, PROTOCOL, POINT_NAMES, WHO)


def proof_to_bytes(proof):
    """C1 || C2 || C3 || W1 || W2 || the 23 values, 32 little-endian bytes each"""
    return pa.proof_to_bytes(proof, POINT_NAMES)


def proof_from_bytes(data, point_bytes):
    return pa.proof_from_bytes(data, point_bytes, POINT_NAMES, N_VALUES, (), WHO)


class FflonkLookupTaggedKey(ArithKey):
    """The proving key on the device: ArithKey's columns; beside them q_K, the table's three columns and the tag column Tg on H and on the
    coset, the tagged hash table over the padded table's rows, the 8n coefficients of C0 and the 8n of C0L, and the points [C0], [C0L].  The
    thirteen fixed polynomials are NOT committed one by one, and their own coefficient vectors do not outlive the interleaving.  Setup is
    deterministic and has no secret.  self.vk is the verification key."""
    KEEPS_COEF = False

    def __init__(self, kzg, circuit):
        if isinstance(circuit, R1csCircuit):
            raise ZkError("%s: an R1csCircuit has no lookups: prove it with fflonk.py" % WHO)
        if not isinstance(circuit, LookupCircuit):
            raise ZkError("%s: the key takes a LookupCircuit" % WHO)
        if not getattr(circuit, "tagged", False):
            raise ZkError("%s: the circuit has one untagged table: this prover takes LookupCircuit(tables=[..]) with 2 .. %d tagged tables; fflonk_lookup.py proves a circuit of one table" %
                          (WHO, MAX_TABLES))
        self.table = None
        super().__init__(kzg, circuit, WHO, ("8n + 8", required_powers(circuit.n)))

    def _fixed(self, coef):
        self.c0_coef = self._keep(interleave_dev(coef, [self.n] * 8, self.curve))

    def _build(self):
        super()._build()
        cv, n, k, c = self.curve, self.n, self.log_n, self.circuit
        self.qk_vals = self._keep(pa.mont_dev(cv, c.sel["qK"]))
        self.t_vals = [self._keep(pa.mont_dev(cv, np.ascontiguousarray(c.table[j]))) for j in range(3)]
        self.tag_vals = self._keep(pa.mont_dev(cv, c.tag_col))                             # Tg on H: the thirteenth fixed polynomial
        self.table = LookupTable(*self.t_vals, n, cv, tag=self.tag_vals)
        more = []
        try:
            for v in [self.qk_vals] + self.t_vals + [self.tag_vals]:
                more.append(pa.interpolate(cv, v, n, 0, k))
            self.lookup_coset = [self._keep(pa.coset_evals(cv, d, n, k + 2)) for d in more]      # q_K, t1, t2, t3, Tg
            more.append(DevArray(4 * n, zero=True))                                        # slots 5 .. 7 of C0L
            self.c0l_coef = self._keep(interleave_dev(more + [more[5]] * 2, [n] * C0L_SLOTS, cv))
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
    """-> FflonkLookupTaggedKey(kzg, circuit); its .vk is the verification key"""
    return FflonkLookupTaggedKey(kzg, circuit)


# ---- the prover -----------------------------------------------------------------------------------------------------------------------------
NOT_ZERO = WHO + ": %s has %%d non-zero coefficients from %%d on: the identity does not hold on H"


def lookup_sum(key, vals, m_vals, eta, delta, bs, keep):
    """phi_0 = 0, phi_(i+1) = phi_i + qK_i / (delta + f_i) - m_i / (delta + t_i) with the tagged f and t, which must close with phi_n = 0;
    Phi += (b_12 X^2 + b_13 X + b_14) Z_H -> Phi's n + 3 coefficients"""
    cv, n = key.curve, key.n
    d = keep(terms(vals + [key.qk_vals] + key.t_vals + [key.tag_vals], n, eta, delta, cv, tagged=True))
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
    mapping with C1, C2, C3, W1, W2 (points, point_bytes each) and values (23 integers in VALUE_NAMES order); publics the l public inputs.
    The gate equation is checked first, row by row, then the lookups: a selected row whose (a, b, c) is no row of the table its q_K names is
    named with the count of such rows and that table (a tuple of another table is no row of that one); the permutation product and the
    lookup sum must close.  Before returning, the proof is verified (self_check=False skips it).  blinding: fourteen integers, FOR TESTS
    ONLY.  _wires, _opening_transcript, _mark: hooks of the tests and of tools/fflonk_lookup_time.py, and _wires skips no check;
    _multiplicities (n integers, FOR TESTS ONLY) replaces the counted m."""
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
            raise ZkError("%s: witness does not satisfy lookup at row %d (%d rows): (a, b, c) is not a row of table %d, the table the row's qK names" %
                          (WHO, first, bad, int(key.circuit.sel["qK"][first, 0])))
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
        cols += [keep(pa.coset_evals(cv, pi_coef, n, k + 2)), key.l1_coset, key.x_coset] + key.lookup_coset[:4]
        cols += [keep(pa.coset_evals(cv, m_coef, n + 2, k + 2)), keep(pa.coset_evals(cv, phi_coef, n + 3, k + 2)), key.lookup_coset[4]]
        ts = [keep(d) for d in quotients(cols, k, beta, gamma, key.k1, key.k2, eta, delta, cv)]
        views = [pa.quotient_coeffs(cv, k, d, nc, NOT_ZERO % name, keep) for d, nc, name in zip(ts, ncs, QUOTIENT_NAMES)]
        c2_coef = keep(interleave_dev([View(z_coef, 0, n + 3), View(phi_coef, 0, n + 3), views[0], views[1]], [n + 3, n + 3, ncs[0], ncs[1]], cv))
        c3_coef = keep(interleave_dev(views[2:], list(ncs[2:]), cv))
        C2, C3 = kzg.commit(c2_coef), kzg.commit(c3_coef)
        c2h, s = transcript_round2(cv, c1h, C2, C3, k)
        mark("round 2")
        # rounds 3 and 4
        rt = roots(cv, k, s)
        sets = [rt["S0"], rt["S0"], rt["S1"], rt["S2"], rt["S3"]]
        state = {}

        def opening_gamma(curve, commitments, sets_, opened):
            state["values"], state["t"], state["zero"] = values_of(curve, opened, rt)
            state["c3"], g = transcript_values(curve, c2h, state["values"])
            return g

        def opening_z(curve, g, W1, avoid=()):
            return transcript_z(curve, state["c3"], W1, avoid)

        def loose_gamma(curve, commitments, sets_, opened):
            state["values"], state["t"], state["zero"] = values_of(curve, opened, rt)
            return _opening_transcript(curve, commitments, sets_, opened)
        _, W1, W2, _, _ = kzg.open_multi([key.c0_coef, key.c0l_coef, c1_coef, c2_coef, c3_coef], sets, transcript=opening_gamma if _opening_transcript is None else loose_gamma,
                                         transcript_z=opening_z if _opening_transcript is None else pa.plain_z, commitments=[key.c0, key.c0l, C1, C2, C3])
        mark("round 4")
        values = state["values"]
        want_t = quotients_at(cv, k, key.k1, key.k2, publics, ch, rt["xi"], dict(zip(VALUE_NAMES, values)))
        if tuple(state["t"]) != tuple(want_t):
            at = [q for q, got, want in zip(QUOTIENT_NAMES, state["t"], want_t) if got != want]
            raise ZkError("%s: internal error: %s at xi is not what the identity gives from the opened values" % (WHO, ", ".join(at)))
        if any(state["zero"]):
            raise ZkError("%s: internal error: slots 5 .. 7 of C0L are not zero at xi" % WHO)
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
    challenges, the 30 values the opening must have -> (verdict, the tuple Kzg.verify_multi takes, built with the verifier's OWN gamma' and
    z').  The identities are not checked here: they are what the rebuilt values of T0 .. T3 make the opening enforce."""
    cv = vk.curve
    shape = pa.check_proof_shape(proof, POINT_NAMES, N_VALUES, point_bytes if point_bytes is not None else len(vk.c0), vk.n_public, publics, FR[cv], WHO)
    if shape is None:
        return INPUT_NOT_CANONICAL, None
    values, publics = shape
    ch = challenges(vk, publics, proof)
    rt = roots(cv, vk.log_n, ch["s"])
    ys = opened_values(cv, vk.log_n, vk.k1, vk.k2, publics, values, ch, rt)
    return ACCEPTED, ([vk.c0, vk.c0l, proof["C1"], proof["C2"], proof["C3"]], [rt["S0"], rt["S0"], rt["S1"], rt["S2"], rt["S3"]], ys, ch["gamma_open"], ch["z_open"], proof["W1"],
                      proof["W2"])


def verify(vk, publics, proofs, kzg=None, seed=None, locate=True):
    """m proofs under one verification key: publics[i] are proof i's public inputs -> (verdict, first_bad) as Kzg.verify_multi gives them.
    The host part of every proof first (host_check), then ONE randomised pairing check of all of them: two pairings.  kzg: the handle to pair
    with, when the key does not carry one.  seed: 32 bytes for the weights, FOR TESTS ONLY."""
    return pa.verify_batch(vk, publics, proofs, host_check, kzg, seed, locate, WHO)
