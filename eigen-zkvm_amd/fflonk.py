"""An fflonk prover and verifier on the interleaved commitments of the KZG layer (kzg.py) over PLONK's arithmetisation
(plonk_arith.py): setup, prove, verify.  A verification key of ONE G1 point, a proof of four G1 points and
15 scalars, two pairings for m proofs.  The protocol, the transcript and the files are this module; everything over Fr of size n or more runs
on the device through the layer's calls, zk_fflonk_<curve>_quotients_dev, zk_kzg_<curve>_interleave_dev (device to device) and
Kzg.open_multi.  There is no CPU fallback.  This is the project's own transcript (SHA-256), not snarkjs's keccak or its file formats.

Field, circuit, wiring, k_1, k_2, sigma, H, w = 7^((r - 1) / n), n = 2^k >= 8, the public rows and PI are the layer's: Circuit and R1csCircuit
are plonk_arith's, the same objects plonk.py offers.

Interleaving.  interleave_t(f_0 .. f_(t-1)) = sum_m f_m(X^t) X^m: coefficient j t + m is coefficient j of f_m, shorter polynomials zero-padded.

Setup.  The eight fixed polynomials of n coefficients each, in FIXED_NAMES order q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3, give
C0 = interleave_8 of 8n coefficients.  The verification key is curve, k, l, k_1, k_2 and [C0].  No secret, no key file.

Rounds.
 1. a, b, c from the witness, the gate equation checked row by row first; blinded as a += (b_1 X + b_2) Z_H (b: b_3, b_4; c: b_5, b_6), n + 2
    coefficients each.  T0 = (a b q_M + a q_L + b q_R + c q_O + q_C + PI) / Z_H, 2n + 2 coefficients.
    C1 = interleave_4(a, b, c, T0), 8n + 8 coefficients; [C1]
 2. beta, gamma; Z by frpoly.terms and grand_product, which must close; Z += (b_7 X^2 + b_8 X + b_9) Z_H, n + 3 coefficients.
    T1 = L_1 (Z - 1) / Z_H, n + 2 coefficients.
    T2 = [(a + beta X + gamma)(b + beta k_1 X + gamma)(c + beta k_2 X + gamma) Z
          - (a + beta S_sigma1 + gamma)(b + beta S_sigma2 + gamma)(c + beta S_sigma3 + gamma) Z(wX)] / Z_H, 3n + 6 coefficients.
    C2 = interleave_3(Z, T1, T2), 9n + 18 coefficients; [C2].  The file must hold 9n + 18 G1 powers (one of power k + 3 does).
    The three numerators are zk_fflonk_<curve>_quotients_dev on the coset 7 H_4n (T0's in round 1, before beta and gamma exist; T1's and
    T2's together in round 2), each divided by divide_zh_coset and brought back by the inverse coset transform; the coefficients from 2n + 2,
    n + 2 and 3n + 6 on must be zero.
 3. one seed s, every root a power of it: h0 = s^3, h1 = s^6, h2 = s^8, xi = s^24, so h0^8 = h1^4 = h2^3 = xi; h3 = h2 w^e with
    e = 3^(-1) mod n, so h3^3 = xi w and no cube root is extracted.  w_8 = w^(n/8), w_4 = w_8^2, w_3 = 7^((r - 1) / 3).  s is drawn again while
    s = 0 or xi^n = 1.  The opening sets:
      S0 = {h0 w_8^j : j < 8} for C0;  S1 = {h1 w_4^j : j < 4} for C1;  S2 = {h2, h2 w_3, h2 w_3^2, h3, h3 w_3, h3 w_3^2} for C2
 4. Kzg.open_multi([C0, C1, C2], [S0, S1, S2]) under this module's gamma' and z'.  The 15 values q_L, q_R, q_O, q_M, q_C, S_sigma1,
    S_sigma2, S_sigma3, a, b, c, Z at xi, then Z, T1, T2 at xi w, come from the 18 opened values on the host by the inverse transforms of
    size t: f_m(x^t) = (1 / t) sum_j y_j (x w_t^j)^(-m).  T0, T1, T2 at xi recovered the same way must be what the identities give.
The proof is [C1], [C2], W1, W2 and the 15 values.  The opening's own challenges are NOT in it: the verifier derives them.

Verifier.  Lengths; every scalar below r (else INPUT_NOT_CANONICAL); every challenge recomputed; PI(xi); from the 15 values
    T0(xi) = (gate + PI)(xi) / Z_H(xi),  T1(xi) = L_1(xi) (Z(xi) - 1) / Z_H(xi),  T2(xi) from both products and Z(xi w)
then the 18 opened values y(x) = sum_m v_m x^m rebuilt (host_values): the eight fixed values on S0, (a, b, c, T0) on S1, (Z, T1, T2)(xi) on
the h2 half of S2 and (Z, T1, T2)(xi w) on the h3 half; one Kzg.verify_multi for all m proofs.  The identities are enforced through the opening
itself: there is no alpha and no separate identity check.

Transcript.  Conventions as in plonk.py: H is SHA-256; a digest is read as a big-endian integer and reduced mod r; a scalar is 32
little-endian bytes; a point is point_bytes bytes in the .ptau file's encoding; "curve" is the name in ASCII; a counter is one byte that starts
at 0 and only moves for a re-draw.
    vkd    = H(curve || "fflonk-vk" || k u32le || l u32le || k_1 || k_2 || C0)
    c0     = H(curve || "fflonk-v1" || vkd || l u32le || x_0 .. x_(l-1))
    c1     = H(c0 || C1)                     beta = H(c1 || 00)     gamma = H(c1 || 01)
    c2     = H(c1 || C2)                     s = H(c2 || ctr)
    c3     = H(c2 || the 15 values)          gamma' = H(c3 || 00)   z' = H(c3 || 01 || W1 || ctr), outside the 18 points

Blinding.  The nine blinders come from `secrets`; blinding=[9 integers] is FOR TESTS ONLY (all zero gives the unblinded proof)."""
import hashlib
import json

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import plonk_arith as pa
from .groth16 import _NAME
from .kzg import _scalar, point_from_json, point_to_json
# the layer's names, for this module and for its callers
from .plonk_arith import (ACCEPTED, FIXED_NAMES, FR, INPUT_NOT_CANONICAL, REJECTED, SELECTORS, TWO_ADICITY, WIRES, ArithKey, Circuit, R1csCircuit, View, check_size, coset_ks, draw,
                          draw_until, gate_check, gather, le, modulus, omega, public_input_at, smallest_power)

N_VALUES, N_OPENED = 15, 18
POINT_NAMES = ("C1", "C2", "W1", "W2")
VALUE_NAMES = FIXED_NAMES + ("a", "b", "c", "Z", "Zw", "T1w", "T2w")
PROTOCOL = "fflonk-shplonk"
QUOTIENT_NAMES = ("T0", "T1", "T2")


def required_powers(n):
    """the G1 powers the file must hold: C2 = interleave_3(Z, T1, T2) has 3 (3n + 6) = 9n + 18 coefficients"""
    return 9 * n + 18


def file_power(log_n):
    """the smallest power of a .ptau file that holds them for n = 2^log_n rows"""
    return smallest_power(required_powers(1 << log_n))


def quotient_coeffs(n):
    """the coefficients of T0, T1, T2"""
    return 2 * n + 2, n + 2, 3 * n + 6


# ---- the field on the host: the roots of a proof and the two directions between opened values and parts --------------------------------------
def omega3(curve):
    """the element of order 3 the h2 and h3 halves of S2 are spread by: 7^((r - 1) / 3)"""
    r = modulus(curve)
    return pow(7, (r - 1) // 3, r)


def roots(curve, log_n, s):
    """the seed s -> a mapping with h0, h1, h2, h3, xi, xiw and the three opening sets S0, S1, S2 in the order of round 3"""
    r, n = modulus(curve), 1 << log_n
    check_size(curve, log_n)
    w = omega(curve, log_n)
    w8, w3 = pow(w, n // 8, r), omega3(curve)
    w4 = w8 * w8 % r
    h0, h1, h2 = pow(s, 3, r), pow(s, 6, r), pow(s, 8, r)
    h3 = h2 * pow(w, pow(3, -1, n), r) % r
    xi = pow(s, 24, r)
    return {"h0": h0, "h1": h1, "h2": h2, "h3": h3, "xi": xi, "xiw": xi * w % r,
            "S0": [h0 * pow(w8, j, r) % r for j in range(8)], "S1": [h1 * pow(w4, j, r) % r for j in range(4)],
            "S2": [h2 * pow(w3, j, r) % r for j in range(3)] + [h3 * pow(w3, j, r) % r for j in range(3)]}


def host_values(curve, parts, points):
    """y(x) = sum_m parts[m] x^m for every x of `points`: the values of interleave_t(f_0 .. f_(t-1)) at x from the parts f_m(x^t), which are
    the same for every x of a set {h w_t^j} -> as many integers as points"""
    r = modulus(curve)
    out = []
    for x in points:
        acc = 0
        for v in reversed(parts):
            acc = (acc * x + v) % r
        out.append(acc)
    return out


def parts_of(curve, ys, points):
    """the inverse, a transform of size t = len(points) on the host: points = {h w_t^j}, ys the opened values there ->
    f_m(h^t) = (1 / t) sum_j y_j (h w_t^j)^(-m), m < t"""
    r = modulus(curve)
    t = len(points)
    inv = [pow(x, -1, r) for x in points]
    tinv = pow(t, -1, r)
    return [sum(y * pow(ix, m, r) for y, ix in zip(ys, inv)) % r * tinv % r for m in range(t)]


def quotients_at(curve, log_n, k1, k2, publics, beta, gamma, xi, v):
    """(T0, T1, T2)(xi) in the field from the values v[name] of VALUE_NAMES (Zw = Z(xi w); T1w, T2w are not read): what the identities give"""
    gate, perm, l1z, zh = pa.identity_terms(curve, log_n, k1, k2, publics, xi, v, beta, gamma)
    zh_inv = pow(zh, -1, FR[curve])
    return tuple(t * zh_inv % FR[curve] for t in (gate, l1z, perm))


def opened_values(curve, log_n, k1, k2, publics, values, beta, gamma, rt):
    """the 18 values the opening must have, from the proof's 15 and the roots rt = roots(..) -> [on S0, on S1, on S2]"""
    v = dict(zip(VALUE_NAMES, values))
    t0, t1, t2 = quotients_at(curve, log_n, k1, k2, publics, beta, gamma, rt["xi"], v)
    return [host_values(curve, list(values[:8]), rt["S0"]), host_values(curve, [v["a"], v["b"], v["c"], t0], rt["S1"]),
            host_values(curve, [v["Z"], t1, t2], rt["S2"][:3]) + host_values(curve, [v["Zw"], v["T1w"], v["T2w"]], rt["S2"][3:])]


def values_of(curve, opened, rt):
    """the proof's 15 values and (T0, T1, T2)(xi) from the 18 opened ones -> (values, (t0, t1, t2))"""
    fixed = parts_of(curve, opened[0], rt["S0"])
    a, b, c, t0 = parts_of(curve, opened[1], rt["S1"])
    z, t1, t2 = parts_of(curve, opened[2][:3], rt["S2"][:3])
    return fixed + [a, b, c, z] + parts_of(curve, opened[2][3:], rt["S2"][3:]), (t0, t1, t2)


# ---- the transcript -----------------------------------------------------------------------------------------------------------------------
def vk_digest(curve, log_n, n_public, k1, k2, c0_point):
    """vkd = H(curve || "fflonk-vk" || k u32le || l u32le || k_1 || k_2 || C0)"""
    return hashlib.sha256(curve.encode("ascii") + b"fflonk-vk" + int(log_n).to_bytes(4, "little") + int(n_public).to_bytes(4, "little") + le(k1) + le(k2) + bytes(c0_point)).digest()


def transcript_start(curve, vkd, publics):
    """c0 = H(curve || "fflonk-v1" || vkd || l u32le || x_0 .. x_(l-1))"""
    return hashlib.sha256(curve.encode("ascii") + b"fflonk-v1" + vkd + len(publics).to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()


def transcript_round1(curve, c0, C1):
    """c1 = H(c0 || C1); beta = H(c1 || 00), gamma = H(c1 || 01) -> (c1, beta, gamma)"""
    c1 = hashlib.sha256(c0 + bytes(C1)).digest()
    return c1, draw(curve, c1, b"\x00"), draw(curve, c1, b"\x01")


def transcript_round2(curve, c1, C2, log_n):
    """c2 = H(c1 || C2); s = H(c2 || ctr), ctr one byte from 0, drawn again while s = 0 or xi^n = 1 with xi = s^24 -> (c2, s)"""
    r = FR[curve]
    c2 = hashlib.sha256(c1 + bytes(C2)).digest()
    return c2, draw_until(curve, c2, lambda s: s != 0 and pow(s, 24 << log_n, r) != 1, "fflonk: no seed")


def transcript_values(curve, c2, values):
    """c3 = H(c2 || the 15 values, 32 little-endian bytes each); gamma' = H(c3 || 00) -> (c3, gamma')"""
    c3 = hashlib.sha256(c2 + b"".join(le(v) for v in values)).digest()
    return c3, draw(curve, c3, b"\x00")


def transcript_z(curve, c3, W1, avoid):
    """z' = H(c3 || 01 || W1 || ctr), ctr one byte from 0, drawn again while z' is one of the 18 opening points"""
    avoid = {int(p) for p in avoid}
    return draw_until(curve, c3 + b"\x01" + bytes(W1), lambda z: z not in avoid, "fflonk: no opening challenge")


# ---- device helpers ---------------------------------------------------------------------------------------------------------------------------
def interleave_dev(polys, lens, curve):
    """zk_kzg_<curve>_interleave_dev device to device: polys, DevArrays (or views) of lens[i] coefficients -> a new DevArray of
    len(polys) max(lens) coefficients, out[j t + i] = polys[i][j]"""
    t, n_max = len(polys), max(lens)
    ptrs = np.array([d.ptr for d in polys], dtype=np.uint64)
    ls = np.array([int(v) for v in lens], dtype=np.uint64)
    out = DevArray(4 * t * n_max)
    try:
        _check(getattr(lib(), "zk_kzg_%s_interleave_dev" % _NAME[curve])(_ptr(ptrs), _ptr(ls), t, out.ptr, 0))
        return out
    except Exception:
        out.free()
        raise


def quotients(cols, log_n, beta, gamma, k1, k2, curve="BN128", outs=None, want=(True, True, True)):
    """zk_fflonk_<curve>_quotients_dev: cols, 15 DevArrays of 4n elements in the order of zk_plonk_<curve>_quotient_dev -> [out0, out1, out2]
    on the coset: the gate numerator with PI, L_1 (Z - 1), the permutation difference.  want[j] false: output j is not computed (None in its
    place) and the columns it alone reads are not read.  outs: three DevArrays (or None) to write into."""
    modulus(curve)
    m = 4 << int(log_n)
    if len(cols) != 15:
        raise ZkError("fflonk: the quotients take 15 columns, not %d" % len(cols))
    sc = [_scalar(v, curve, w) for v, w in ((beta, "beta"), (gamma, "gamma"), (k1, "k1"), (k2, "k2"))]
    if any(c.n < 4 * m for c in cols):
        raise ZkError("fflonk: every column of the quotients holds 4n = %d elements" % m)
    outs = list(outs) if outs is not None else [None] * 3
    if len(outs) != 3 or len(want) != 3:
        raise ZkError("fflonk: the quotients have three outputs")
    if any(o is not None and o.n < 4 * m for o in outs):
        raise ZkError("fflonk: every output of the quotients holds 4n = %d elements" % m)
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    made = []
    try:
        for j in range(3):
            if want[j] and outs[j] is None:
                outs[j] = DevArray(4 * m)
                made.append(outs[j])
            elif not want[j]:
                outs[j] = None
        _check(getattr(lib(), "zk_fflonk_%s_quotients_dev" % _NAME[curve])(_ptr(ptrs), int(log_n), *[_ptr(s) for s in sc], *[o.ptr if o is not None else None for o in outs], 0))
        return outs
    except Exception:
        for d in made:
            d.free()
        raise


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    """(curve, log n, l, k_1, k_2, [C0]); `kzg` is the handle verify() pairs with, when the key came from an FflonkKey"""

    def __init__(self, curve, log_n, n_public, k1, k2, c0, kzg=None):
        modulus(curve)
        self.curve, self.log_n, self.n_public, self.k1, self.k2 = curve, int(log_n), int(n_public), int(k1), int(k2)
        self.c0, self.kzg = bytes(c0), kzg
        check_size(curve, self.log_n)
        if self.log_n < 3:
            raise ZkError("fflonk: n = 2^%d rows: a circuit has at least 8" % self.log_n)
        self.n = 1 << self.log_n
        self.digest = vk_digest(curve, self.log_n, self.n_public, self.k1, self.k2, self.c0)


def vk_to_json(vk):
    return json.dumps({"protocol": PROTOCOL, "curve": vk.curve, "log_n": vk.log_n, "n_public": vk.n_public, "k1": str(vk.k1), "k2": str(vk.k2),
                       "C0": point_to_json(vk.c0, vk.curve)}, indent=1) + "\n"


def vk_from_json(text, kzg=None):
    js = json.loads(text)
    if js.get("protocol") != PROTOCOL:
        raise ZkError('fflonk: not a verification key of this prover (protocol "%s")' % js.get("protocol"))
    return VerifyingKey(js["curve"], js["log_n"], js["n_public"], int(js["k1"], 0), int(js["k2"], 0), point_from_json(js["C0"], js["curve"]), kzg)


def vk_to_bytes(vk):
    """curve's name, a zero byte, k u32le, l u32le, k_1, k_2 as 32 little-endian bytes each, C0"""
    return vk.curve.encode("ascii") + b"\x00" + vk.log_n.to_bytes(4, "little") + vk.n_public.to_bytes(4, "little") + le(vk.k1) + le(vk.k2) + vk.c0


def vk_from_bytes(data, kzg=None):
    data = bytes(data)
    at = data.find(b"\x00")
    if at < 0 or len(data) < at + 73:
        raise ZkError("fflonk: %d bytes are no verification key" % len(data))
    body = data[at + 1:]
    try:
        curve = data[:at].decode("ascii")
    except UnicodeDecodeError:
        raise ZkError("fflonk: %d bytes are no verification key" % len(data))
    return VerifyingKey(curve, int.from_bytes(body[:4], "little"), int.from_bytes(body[4:8], "little"), int.from_bytes(body[8:40], "little"),
                        int.from_bytes(body[40:72], "little"), body[72:], kzg)


def proof_to_json(proof, curve):
    return pa.proof_to_json(proof, curve, PROTOCOL, POINT_NAMES)


def proof_from_json(text, curve):
    return pa.proof_from_json(text, curve, PROTOCOL, POINT_NAMES, "fflonk")


def proof_to_bytes(proof):
    """C1 || C2 || W1 || W2 || the 15 values, 32 little-endian bytes each"""
    return pa.proof_to_bytes(proof, POINT_NAMES)


def proof_from_bytes(data, point_bytes):
    return pa.proof_from_bytes(data, point_bytes, POINT_NAMES, N_VALUES, (), "fflonk")


class FflonkKey(ArithKey):
    """The proving key on the device: ArithKey's columns, and beside them the 8n coefficients of C0 = interleave_8 of the eight fixed
    polynomials and the point [C0].  The eight are NOT committed one by one, and their own coefficient vectors do not outlive the interleaving.
    Setup is deterministic and has no secret.  self.vk is the verification key."""
    KEEPS_COEF = False

    def __init__(self, kzg, circuit):
        super().__init__(kzg, circuit, "fflonk", ("9n + 18", required_powers(circuit.n)))

    def _fixed(self, coef):
        self.c0_coef = self._keep(interleave_dev(coef, [self.n] * 8, self.curve))

    def _build(self):
        super()._build()
        self.c0 = self.kzg.commit(self.c0_coef)
        self.vk = VerifyingKey(self.curve, self.log_n, self.circuit.n_public, self.k1, self.k2, self.c0, self.kzg)


def setup(kzg, circuit):
    """-> FflonkKey(kzg, circuit); its .vk is the verification key"""
    return FflonkKey(kzg, circuit)


# ---- the prover -----------------------------------------------------------------------------------------------------------------------------
NOT_ZERO = "fflonk: %s has %%d non-zero coefficients from %%d on: the identity does not hold on H"


def prove(key, witness, blinding=None, self_check=True, _wires=None, _opening_transcript=None, _mark=None):
    """-> (proof, publics).  witness: as plonk.prove takes it (n_vars values below r; on a key whose circuit is an R1csCircuit the n_wires
    values of the .wtns or its bytes: the auxiliaries are then made on the device and a failing gate is named with its constraint).  proof is
    a mapping with C1, C2, W1, W2 (points, point_bytes each) and values (15 integers in VALUE_NAMES order).  The gate equation is checked
    first, row by row; the permutation product must close.  Before returning, the proof is verified (self_check=False skips it).
    blinding: nine integers, FOR TESTS ONLY.  _wires, _opening_transcript, _mark: hooks of the tests and of tools/fflonk_time.py."""
    cv, n, k, kzg = key.curve, key.n, key.log_n, key.kzg
    mark = _mark or (lambda name: None)
    n0, n1, n2 = quotient_coeffs(n)
    own = []

    def keep(d):
        own.append(d)
        return d
    try:
        vals, pi_vals, publics, bs = pa.witness_columns(key, witness, blinding, _wires, "fflonk", keep, mark)
        # round 1: T0 needs neither Z nor beta, gamma, which do not exist yet; a's column stands where Z's pointer must be valid
        coef = pa.blinded_wires(key, vals, bs, keep)
        pi_coef = keep(pa.interpolate(cv, pi_vals, n, 0, k))
        wire_cos = [keep(pa.coset_evals(cv, d, n + 2, k + 2)) for d in coef]
        pi_cos = keep(pa.coset_evals(cv, pi_coef, n, k + 2))
        cols = wire_cos + [wire_cos[0]] + key.coset + [pi_cos, key.l1_coset, key.x_coset]
        t0 = keep(quotients(cols, k, 0, 0, key.k1, key.k2, cv, want=(True, False, False))[0])
        t0_view = pa.quotient_coeffs(cv, k, t0, n0, NOT_ZERO % "T0", keep)
        c1_coef = keep(interleave_dev(coef + [t0_view], [n + 2] * 3 + [n0], cv))
        C1 = kzg.commit(c1_coef)
        c0h = transcript_start(cv, key.vk.digest, publics)
        c1h, beta, gamma = transcript_round1(cv, c0h, C1)
        mark("round 1")
        # round 2
        z_coef = pa.permutation_product(key, vals, beta, gamma, bs, "fflonk", keep)
        cols[3] = keep(pa.coset_evals(cv, z_coef, n + 3, k + 2))
        _, t1, t2 = quotients(cols, k, beta, gamma, key.k1, key.k2, cv, want=(False, True, True))
        keep(t1); keep(t2)
        t1_view = pa.quotient_coeffs(cv, k, t1, n1, NOT_ZERO % "T1", keep)
        t2_view = pa.quotient_coeffs(cv, k, t2, n2, NOT_ZERO % "T2", keep)
        c2_coef = keep(interleave_dev([View(z_coef, 0, n + 3), t1_view, t2_view], [n + 3, n1, n2], cv))
        C2 = kzg.commit(c2_coef)
        c2h, s = transcript_round2(cv, c1h, C2, k)
        mark("round 2")
        # rounds 3 and 4
        rt = roots(cv, k, s)
        sets = [rt["S0"], rt["S1"], rt["S2"]]
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
        _, W1, W2, _, _ = kzg.open_multi([key.c0_coef, c1_coef, c2_coef], sets, transcript=opening_gamma if _opening_transcript is None else loose_gamma,
                                         transcript_z=opening_z if _opening_transcript is None else pa.plain_z, commitments=[key.c0, C1, C2])
        mark("round 4")
        values = state["values"]
        want_t = quotients_at(cv, k, key.k1, key.k2, publics, beta, gamma, rt["xi"], dict(zip(VALUE_NAMES, values)))
        if tuple(state["t"]) != tuple(want_t):
            at = [q for q, got, want in zip(QUOTIENT_NAMES, state["t"], want_t) if got != want]
            raise ZkError("fflonk: internal error: %s at xi is not what the identity gives from the opened values" % ", ".join(at))
        proof = {"C1": C1, "C2": C2, "W1": W1, "W2": W2, "values": values}
    finally:
        for d in own:
            d.free()
    if self_check:
        verdict, _ = verify(key.vk, [publics], [proof])
        if verdict != ACCEPTED:
            raise ZkError("fflonk: the proof just made is not accepted (verdict %d)" % verdict)
    return proof, publics


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------------
def challenges(vk, publics, proof):
    """every challenge of a proof from the verification key, the public inputs and the proof's own points and values -> a mapping with beta,
    gamma, s, xi, gamma_open (gamma') and z_open (z')"""
    cv = vk.curve
    c0 = transcript_start(cv, vk.digest, publics)
    c1, beta, gamma = transcript_round1(cv, c0, proof["C1"])
    c2, s = transcript_round2(cv, c1, proof["C2"], vk.log_n)
    c3, g = transcript_values(cv, c2, proof["values"])
    rt = roots(cv, vk.log_n, s)
    return {"beta": beta, "gamma": gamma, "s": s, "xi": rt["xi"], "gamma_open": g, "z_open": transcript_z(cv, c3, proof["W1"], rt["S0"] + rt["S1"] + rt["S2"])}


def host_check(vk, publics, proof, point_bytes=None):
    """what the verifier decides on the host, before any device work: lengths (an error), every scalar below r (else INPUT_NOT_CANONICAL), the
    challenges, the 18 values the opening must have -> (verdict, the tuple Kzg.verify_multi takes, built with the verifier's OWN gamma' and
    z').  The identities are not checked here: they are what the rebuilt values of T0, T1, T2 make the opening enforce."""
    cv = vk.curve
    shape = pa.check_proof_shape(proof, POINT_NAMES, N_VALUES, point_bytes if point_bytes is not None else len(vk.c0), vk.n_public, publics, FR[cv], "fflonk")
    if shape is None:
        return INPUT_NOT_CANONICAL, None
    values, publics = shape
    ch = challenges(vk, publics, proof)
    rt = roots(cv, vk.log_n, ch["s"])
    ys = opened_values(cv, vk.log_n, vk.k1, vk.k2, publics, values, ch["beta"], ch["gamma"], rt)
    return ACCEPTED, ([vk.c0, proof["C1"], proof["C2"]], [rt["S0"], rt["S1"], rt["S2"]], ys, ch["gamma_open"], ch["z_open"], proof["W1"], proof["W2"])


def verify(vk, publics, proofs, kzg=None, seed=None, locate=True):
    """m proofs under one verification key: publics[i] are proof i's public inputs -> (verdict, first_bad) as Kzg.verify_multi gives them.
    The host part of every proof first (host_check), then ONE randomised pairing check of all of them: two pairings.  kzg: the handle to pair
    with, when the key does not carry one.  seed: 32 bytes for the weights, FOR TESTS ONLY."""
    return pa.verify_batch(vk, publics, proofs, host_check, kzg, seed, locate, "fflonk")
