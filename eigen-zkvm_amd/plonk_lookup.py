"""PLONK with lookups: the prover and verifier of plonk.py with the log-derivative lookup argument (logUp) beside the
permutation argument: setup, prove, verify.  A third protocol on the arithmetisation of plonk_arith.py; it shares no code
with plonk.py or fflonk.py and its keys and proofs are refused by them, as theirs are here.  Everything over Fr runs on the device: the calls
of plonk.py, and for the argument zk_plonk_<curve>_lookup_table_new / _lookup_count_dev (a hash table over the table's rows and the count
of how often each is used), _lookup_terms_dev, zk_fr_<curve>_batch_inverse_dev, _lookup_summands_dev, zk_fr_<curve>_prefix_sum_dev and
_lookup_quotient_dev.  There is no CPU fallback.  Several tables in one circuit are the TAGGED variant below.  Not built:
tables wider than three, lookups under fflonk (fflonk.py knows no q_K; fflonk_lookup.py has one table and refuses a tagged circuit;
fflonk_lookup_tagged.py, DESIGN.md 3.27, is the tagged argument under fflonk, a protocol of its own), lookups in a circuit compiled from an
.r1cs, a linearisation polynomial.

A LOOKUP CIRCUIT is a gate table (plonk_arith.Circuit) plus a selector qK per gate, which must be 0 or 1, and a table of T >= 1 rows of
three field values (t1, t2, t3).  n = 2^k >= 8 must hold the l public rows plus the gates, and must also hold T.  The table is padded to n
rows by REPEATING ITS LAST ROW (zeros are never used: a zero row would silently put (0, 0, 0) into the table).  Public rows and padding rows
of the gate table have qK = 0.  A row with qK = 1 claims that (a_i, b_i, c_i) is a row of the table; it must still satisfy its gate
equation (all-zero selectors make that trivial).

Multiplicities.  m_j is the number of selected rows whose tuple equals table row j.  When the table holds the same row more than once, the
SMALLEST index takes the whole count and the others get 0.  This rule is part of the protocol: proofs are compared byte for byte.

Rounds, as far as they differ from plonk.py's.
 1. as there, and m interpolated over H and blinded as m += (b_10 X + b_11) Z_H; [A], [B], [C], [M]
 2. beta, gamma, eta, delta; Z as there.  With f_i = a_i + eta b_i + eta^2 c_i and t_i = t1_i + eta t2_i + eta^2 t3_i:
    phi_0 = 0, phi_(i+1) = phi_i + qK_i / (delta + f_i) - m_i / (delta + t_i), which must close with phi_n = 0; a zero denominator is
    refused (batch_inverse's zero count names the row); Phi += (b_12 X^2 + b_13 X + b_14) Z_H; [Z], [Phi]
 3. alpha; the bracket of plonk.py gains alpha^3 L,
      L = (Phi(wX) - Phi(X)) (delta + f)(delta + t) - q_K (delta + t) + M (delta + f)
    (zk_plonk_<curve>_lookup_quotient_dev, after zk_plonk_<curve>_quotient_dev).  There is no boundary term for Phi: the telescoping sum
    over H is what forces sum qK / (delta + f) = sum m / (delta + t).  deg L <= 3n + 2, so t keeps its 3n + 6 coefficients; [T]
 4. zeta as there
 5. Kzg.open_multi of the 12 fixed polynomials q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3, q_K, t1, t2, t3 and of a, b, c, t, M
    on {zeta}, and of Z and Phi on {zeta, zeta w}
The proof is [A], [B], [C], [M], [Z], [Phi], [T], the 21 values in that order (Z: zeta, zeta w; then Phi: zeta, zeta w), W1, W2.

Transcript.  H, scalars, points, "curve" and counters as in plonk.py.
    vkd    = H(curve || "plonkl-vk" || k u32le || l u32le || k_1 || k_2 || the 12 commitments)
    c0     = H(curve || "plonkl-v1" || vkd || l u32le || x_0 .. x_(l-1))
    c1     = H(c0 || A || B || C || M)       beta = H(c1 || 00)   gamma = H(c1 || 01)   eta = H(c1 || 02)   delta = H(c1 || 03)
    c2     = H(c1 || Z || Phi)               alpha = H(c2 || 00)
    c3     = H(c2 || T)                      zeta = H(c3 || ctr)
    c4     = H(c3 || the 21 values)          gamma' = H(c4 || 00)   z' = H(c4 || 01 || W1 || ctr), outside {zeta, zeta w}

Blinding.  The fourteen blinders come from `secrets`; blinding=[14 integers] is FOR TESTS ONLY (all zero gives the unblinded proof).

The verifier is plonk.py's: shape, canonical scalars, every challenge recomputed, the identity in the field on the host from the 21 values
(gate + alpha perm + alpha^2 L_1 (Z - 1) + alpha^3 L - t Z_H = 0), then ONE Kzg.verify_multi for the whole batch.

TAGGED LOOKUPS: a circuit built with tables=[rows, rows, ...] holds K tables, 2 <= K <= 65535, numbered from 1; a circuit
with one table (table=) is the protocol above, byte for byte.  The variant is the circuit's and the key's, never the caller's.  A table's
rows hold one, two or three values and are padded with zeros on the right.  The tables are concatenated in order into T = sum T_k rows
(T0_j, t1_j, t2_j, t3_j) with T0_j = k, the number of row j's table, and padded to n by repeating the last row, its tag included.  On the
gate side qK_i is in {0, 1, .., K}: 0 is no lookup, k claims that (a_i, b_i, c_i) is a row of table k.  q_K is both the row's tag and its
weight; no second selector is committed.
    f_i = a_i + eta b_i + eta^2 c_i + eta^3 qK_i        t_j = t1_j + eta t2_j + eta^2 t3_j + eta^3 T0_j
    m_j = T0_j x (the selected rows i with (qK_i, a_i, b_i, c_i) = (T0_j, t1_j, t2_j, t3_j)), an integer below 2^46
The smallest index of a repeated tagged row takes the whole count; the same (t1, t2, t3) under two tags are two rows.  The sum phi and the
identity L keep their form with these f, t and m; deg L <= 3n + 2 still (the new terms are fixed polynomials of degree below n), so the
3n + 6 powers stay.  Soundness: as rational functions of delta, sum_i qK_i / (delta + f_i) = sum_j m_j / (delta + t_j) forces, for every
value v, sum_{i: f_i = v} qK_i = sum_{j: t_j = v} m_j in the field.  For a v that is no t_j the right side is 0 and the left a sum of at
most n <= 2^30 integers in [1, K], K < 2^16: positive and below 2^46, far below r, so not zero in the field -- a selected row cannot hide
outside the table.  eta binds tag and tuple together by Schwartz-Zippel, as it binds the three columns above: f_i = t_j for random eta
means (qK_i, a_i, b_i, c_i) = (T0_j, t1_j, t2_j, t3_j) but for probability 3 / r, so a tuple of table 2 does not serve a row tagged 1.
There are thirteen fixed polynomials, the twelve above and then T0; the proof is the same seven points, 22 values (T0(zeta) after
t3(zeta)), W1 and W2; the fourteen blinders keep their numbering.  The transcript has its own domain strings,
    vkd    = H(curve || "plonklt-vk" || k u32le || l u32le || k_1 || k_2 || the 13 commitments)
    c0     = H(curve || "plonklt-v1" || vkd || l u32le || x_0 .. x_(l-1))
and c1 .. c4 as above (c4 over the 22 values); the protocol name in the JSON codecs is "plonk-shplonk-lookup-tagged".  A key or a proof of
the single-table protocol is refused by the tagged one and the reverse.  Device: zk_plonk_<curve>_lookup_tagged_table_new / _count_dev /
_terms_dev / _quotient_dev (csrc/plonk_lookup_tagged_impl.hip.h); the summands, the running sum and the inverses are the calls above."""
import ctypes as C
import hashlib
import json

import numpy as np

from . import DevArray, ZkError, _check, _ptr, lib
from . import frpoly as fp
from . import plonk_arith as pa
from .groth16 import _NAME
from .kzg import _scalar, point_from_json, point_to_json, to_mont
from .plonk_arith import ACCEPTED, FIXED_NAMES, FR, INPUT_NOT_CANONICAL, REJECTED, SELECTORS, TWO_ADICITY, WIRES, ArithKey, Circuit, R1csCircuit, View, canon_words, draw, draw_until, le, modulus, omega

WHO = "plonk lookup"
N_VALUES, N_FIXED, N_BLINDERS = 21, 12, 14
LOOKUP_FIXED = ("qK", "T1", "T2", "T3")
FIXED = FIXED_NAMES + LOOKUP_FIXED
POINT_NAMES = ("A", "B", "C", "M", "Z", "Phi", "T", "W1", "W2")
VALUE_NAMES = FIXED + ("a", "b", "c", "t", "M", "Z", "Zw", "Phi", "Phiw")
PROTOCOL = "plonk-shplonk-lookup"
CIRCUIT = "LookupCircuit"                 # the class tools/plonk_cli.py loads a circuit file with
MAX_TABLE_ROWS = 1 << 30                  # ZK_PLONK_LOOKUP_MAX_ROWS
# the tagged variant: one more fixed polynomial, T0, and its value after T3's
MAX_TABLES = 65535                        # ZK_PLONK_LOOKUP_MAX_TABLES
TAGGED_N_VALUES, TAGGED_N_FIXED = 22, 13
TAGGED_FIXED = FIXED + ("T0",)
TAGGED_VALUE_NAMES = TAGGED_FIXED + VALUE_NAMES[N_FIXED:]
TAGGED_PROTOCOL = "plonk-shplonk-lookup-tagged"


def _protocol(tagged):
    return TAGGED_PROTOCOL if tagged else PROTOCOL


def _fixed_names(tagged):
    return TAGGED_FIXED if tagged else FIXED


def _n_values(tagged):
    return TAGGED_N_VALUES if tagged else N_VALUES


def required_powers(n):
    """the G1 powers the file must hold: the quotient is committed whole, with 3n + 6 coefficients (deg L <= 3n + 2 changes nothing)"""
    return 3 * n + 6


# ---- circuits -------------------------------------------------------------------------------------------------------------------------------
def check_table_size(curve, n_rows):
    """T >= 1 rows must fit n = 2^k rows whose coset of 4n points the field has"""
    modulus(curve)
    if n_rows < 1:
        raise ZkError("%s: a table has at least one row" % WHO)
    limit = min(1 << (TWO_ADICITY[curve] - 2), MAX_TABLE_ROWS)
    if n_rows > limit:
        raise ZkError("%s: a table of %d rows does not fit n <= 2^%d rows on %s" % (WHO, n_rows, limit.bit_length() - 1, curve))


def range_table(bits):
    """the rows (v, 0, 0) for v < 2^bits: a row with qK = 1 proves a < 2^bits when b and c sit on a zero"""
    return [(v, 0, 0) for v in range(1 << int(bits))]


def xor_table(bits):
    """the rows (x, y, x ^ y) for x, y < 2^bits"""
    return [(x, y, x ^ y) for x in range(1 << int(bits)) for y in range(1 << int(bits))]


def _table_words(table, r):
    """rows of three integers, or a (T, 3, 4) u64 array of canonical words -> (T, 3, 4) u64"""
    if isinstance(table, np.ndarray) and table.dtype == np.uint64 and table.ndim == 3 and table.shape[1:] == (3, 4):
        flat = canon_words(np.ascontiguousarray(table).reshape(-1, 4), r, "table value")
    else:
        rows = [tuple(row) for row in table]
        if any(len(row) != 3 for row in rows):
            raise ZkError("%s: a table row holds three values" % WHO)
        flat = canon_words([v for row in rows for v in row], r, "table value")
    return flat.reshape(-1, 3, 4)


def _tagged_words(tables, r, curve):
    """K tables of rows of one, two or three values (or (T_k, 3, 4) u64 canonical words) -> (the (T, 3, 4) u64 words of the concatenated
    rows, short rows padded with zeros on the right; the (T,) u32 tags 1 .. K; the sizes T_k)"""
    try:
        tables = list(tables)
        sizes = [len(t) for t in tables]
    except TypeError:
        raise ZkError("%s: tables= is a sequence of tables, a table a sequence of rows" % WHO)
    if not 2 <= len(tables) <= MAX_TABLES:
        raise ZkError("%s: tables= takes 2 .. %d tables, not %d (one table is table=)" % (WHO, MAX_TABLES, len(tables)))
    for k, size in enumerate(sizes):
        if size < 1:
            raise ZkError("%s: table %d is empty: a table has at least one row" % (WHO, k + 1))
    check_table_size(curve, sum(sizes))
    words = []
    for k, t in enumerate(tables):
        if not isinstance(t, np.ndarray):
            rows = [tuple(row) for row in t]
            wide = next((j for j, row in enumerate(rows) if not 1 <= len(row) <= 3), None)
            if wide is not None:
                raise ZkError("%s: row %d of table %d holds %d values: a table row holds one, two or three" % (WHO, wide, k + 1, len(rows[wide])))
            t = [row + (0,) * (3 - len(row)) for row in rows]
        words.append(_table_words(t, r))
    return np.concatenate(words), np.repeat(np.arange(1, len(tables) + 1, dtype=np.uint32), sizes), sizes


class LookupCircuit(Circuit):
    """A gate table with lookups.  gates: Circuit's mapping plus qK (0 or 1 per gate; integers or (m, 4) u64 words); table: T >= 1 rows of
    three values below r (or (T, 3, 4) u64 canonical words).  n holds the public rows, the gates and the table.  self.sel["qK"] is (n, 4)
    u64 (0 on public and padding rows), self.table (3, n, 4) u64: the table by column, padded to n rows by repeating its last row;
    self.n_table = T.  Host integers only.
    tables=[rows, rows, ...] in place of table= (exactly one of the two) builds the TAGGED circuit of K = len(tables) tables, 2 <= K <= 65535,
    whose rows hold one to three values: qK is 0 .. K per gate, self.tagged is True, self.table holds the concatenated rows, self.table_tag
    ((T,) u32) their tags 1 .. K, self.tag_col ((n, 4) u64) the tag column padded with the last row's tag, self.table_sizes the T_k."""

    def __init__(self, n_vars, public, gates, table=None, curve="BN128", tables=None):
        r = modulus(curve)
        if (table is None) == (tables is None):
            raise ZkError("%s: a lookup circuit takes table= (one table) or tables= (several tables, tagged): exactly one of the two" % WHO)
        self.tagged = tables is not None
        if "qK" not in gates:
            raise ZkError("%s: the gates of a lookup circuit carry a selector qK" % WHO)
        qk = canon_words(gates["qK"], r, "selector qK of gate")
        if self.tagged:
            tw, self.table_tag, self.table_sizes = _tagged_words(tables, r, curve)
            n_rows, top = len(tw), len(self.table_sizes)
            bad = np.nonzero((qk[:, 0] > top) | qk[:, 1:].any(axis=1))[0]
            if bad.size:
                raise ZkError("%s: selector qK of gate %d names no table: the circuit has tables 1 .. %d (0 is no lookup)" % (WHO, int(bad[0]), top))
        else:
            bad = np.nonzero((qk[:, 0] > 1) | qk[:, 1:].any(axis=1))[0]
            if bad.size:
                raise ZkError("%s: selector qK of gate %d is not 0 or 1" % (WHO, int(bad[0])))
            try:
                n_rows = len(table)
            except TypeError:
                raise ZkError("%s: a table is a sequence of rows" % WHO)
            check_table_size(curve, n_rows)
            tw = _table_words(table, r)
            self.table_sizes = [n_rows]
        super().__init__(n_vars, public, gates, curve, min_rows=n_rows)
        if len(qk) != self.n_gates:
            raise ZkError("plonk: the selector and wire arrays of a circuit have one length")
        self.gates["qK"] = qk
        self.n_table, self.table_rows = n_rows, tw
        a = np.zeros((self.n, 4), np.uint64)
        a[self.n_public:self.n_public + self.n_gates] = qk
        self.sel["qK"] = a
        self.table = np.empty((3, self.n, 4), np.uint64)
        self.table[:, :n_rows] = tw.transpose(1, 0, 2)
        self.table[:, n_rows:] = tw[-1][:, None, :]
        if self.tagged:
            self.tag_col = np.zeros((self.n, 4), np.uint64)
            self.tag_col[:n_rows, 0] = self.table_tag
            self.tag_col[n_rows:, 0] = self.table_tag[-1]

    def save(self, path):
        """Circuit.save's .npz with qK ((m, 4) u64) and table ((T, 3, 4) u64 canonical words) added; a tagged circuit adds table_tag ((T,) u32)"""
        more = {"table_tag": self.table_tag} if self.tagged else {}
        np.savez(path, n_vars=np.uint64(self.n_vars), public=np.asarray(self.public, dtype=np.uint32), table=self.table_rows, **more, **self.gates)

    @classmethod
    def load(cls, path, curve="BN128"):
        """a file without table_tag is a circuit of one table; with it, the tagged circuit whose tables are the runs of equal tags"""
        with np.load(path) as z:
            missing = [k for k in SELECTORS + ("qK",) + WIRES + ("n_vars", "public", "table") if k not in z]
            if missing:
                raise ZkError("%s: %s holds no %s" % (WHO, path, ", ".join(missing)))
            gates = {k: np.asarray(z[k], dtype=np.uint64).reshape(-1, 4) for k in SELECTORS + ("qK",)}
            gates.update({k: np.asarray(z[k]).reshape(-1) for k in WIRES})
            head = (int(z["n_vars"]), [int(v) for v in np.asarray(z["public"]).reshape(-1)], gates)
            table = np.asarray(z["table"], dtype=np.uint64).reshape(-1, 3, 4)
            if "table_tag" not in z:
                return cls(*head, table, curve)
            tag = np.asarray(z["table_tag"]).reshape(-1).astype(np.int64)
            if len(tag) != len(table) or len(tag) == 0 or tag[0] != 1 or not np.isin(np.diff(tag), (0, 1)).all():
                raise ZkError("%s: table_tag of %s is not the tags 1 .. K of the table's %d rows in order" % (WHO, path, len(table)))
            return cls(*head, curve=curve, tables=np.split(table, np.nonzero(np.diff(tag))[0] + 1))


# ---- the transcript -----------------------------------------------------------------------------------------------------------------------
def vk_digest(curve, log_n, n_public, k1, k2, commitments, tagged=False):
    """vkd = H(curve || "plonkl-vk" || k u32le || l u32le || k_1 || k_2 || the 12 commitments), in the order q_L, q_R, q_O, q_M, q_C, S_sigma1,
    S_sigma2, S_sigma3, q_K, t1, t2, t3; tagged: "plonklt-vk" and the 13 commitments, T0 last"""
    return hashlib.sha256(curve.encode("ascii") + (b"plonklt-vk" if tagged else b"plonkl-vk") + int(log_n).to_bytes(4, "little") + int(n_public).to_bytes(4, "little") + le(k1) + le(k2) +
                          b"".join(bytes(c) for c in commitments)).digest()


def transcript_start(curve, vkd, publics, tagged=False):
    """c0 = H(curve || "plonkl-v1" || vkd || l u32le || x_0 .. x_(l-1)); tagged: "plonklt-v1" in its place"""
    return hashlib.sha256(curve.encode("ascii") + (b"plonklt-v1" if tagged else b"plonkl-v1") + vkd + len(publics).to_bytes(4, "little") + b"".join(le(x) for x in publics)).digest()


def transcript_wires(curve, c0, A, B, Cc, M):
    """c1 = H(c0 || A || B || C || M); beta, gamma, eta, delta = H(c1 || 00 .. 03) -> (c1, beta, gamma, eta, delta)"""
    c1 = hashlib.sha256(c0 + bytes(A) + bytes(B) + bytes(Cc) + bytes(M)).digest()
    return (c1,) + tuple(draw(curve, c1, bytes([i])) for i in range(4))


def transcript_sums(curve, c1, Z, Phi):
    """c2 = H(c1 || Z || Phi); alpha = H(c2 || 00) -> (c2, alpha)"""
    c2 = hashlib.sha256(c1 + bytes(Z) + bytes(Phi)).digest()
    return c2, draw(curve, c2, b"\x00")


def transcript_quotient(curve, c2, T, n):
    """c3 = H(c2 || T); zeta = H(c3 || ctr), drawn again while zeta = 0 or zeta^n = 1 -> (c3, zeta)"""
    r = FR[curve]
    c3 = hashlib.sha256(c2 + bytes(T)).digest()
    return c3, draw_until(curve, c3, lambda zeta: zeta != 0 and pow(zeta, n, r) != 1, "%s: no evaluation point" % WHO)


def transcript_values(curve, c3, values):
    """c4 = H(c3 || the 21 values, 32 little-endian bytes each); gamma' = H(c4 || 00) -> (c4, gamma')"""
    c4 = hashlib.sha256(c3 + b"".join(le(v) for v in values)).digest()
    return c4, draw(curve, c4, b"\x00")


def transcript_z(curve, c4, W1, avoid):
    """z' = H(c4 || 01 || W1 || ctr), drawn again while z' is one of the opening points {zeta, zeta w}"""
    avoid = {int(p) for p in avoid}
    return draw_until(curve, c4 + b"\x01" + bytes(W1), lambda z: z not in avoid, "%s: no opening challenge" % WHO)


# ---- the device calls that are this protocol's ----------------------------------------------------------------------------------------------
def _fn(curve, name):
    modulus(curve)
    return getattr(lib(), "zk_plonk_%s_lookup_%s" % (_NAME[curve], name))


class LookupTable:
    """zk_plonk_<curve>_lookup_table_new: the rows (t1[j], t2[j], t3[j]), j < n_rows, of three DevArrays as a hash table on the device; the
    columns may be freed once this returns.  free() releases it.  tag: a fourth DevArray, the rows' tags 1 .. 65535 as field elements:
    zk_plonk_<curve>_lookup_tagged_table_new, the table of the tagged argument (self.tagged), whose rows are (tag[j], t1[j], t2[j], t3[j])."""

    def __init__(self, t1, t2, t3, n_rows, curve="BN128", tag=None):
        self.curve, self.n_rows, self._h, self.tagged = curve, int(n_rows), None, tag is not None
        fn = _fn(curve, "tagged_table_new" if self.tagged else "table_new")
        cols = ([tag] if self.tagged else []) + [t1, t2, t3]
        if any(d.n < 4 * self.n_rows for d in cols):
            raise ZkError("%s: every column of the table holds %d elements" % (WHO, self.n_rows))
        self._h = fn(*[d.ptr for d in cols], self.n_rows, 0)
        if not self._h:
            raise ZkError(lib().zk_last_error().decode())

    def free(self):
        if getattr(self, "_h", None):
            _fn(self.curve, "table_free")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def count(table, a, b, c, qk, n, out=None):
    """zk_plonk_<curve>_lookup_count_dev over n rows -> (the n multiplicities as a DevArray, the selected rows that miss, the first or None);
    over a tagged table zk_plonk_<curve>_lookup_tagged_count_dev: a row's key is (qK, a, b, c) and m_j = tag_j x count_j"""
    d_out = out if out is not None else DevArray(4 * max(int(n), 1))
    bad, first = C.c_uint64(0), C.c_uint64(0)
    try:
        _check(_fn(table.curve, "tagged_count_dev" if table.tagged else "count_dev")(table._h, a.ptr, b.ptr, c.ptr, qk.ptr, int(n), d_out.ptr, C.byref(bad), C.byref(first), 0))
        return d_out, int(bad.value), (None if bad.value == 0 else int(first.value))
    except Exception:
        if out is None:
            d_out.free()
        raise


def terms(cols, n, eta, delta, curve="BN128", tagged=False):
    """zk_plonk_<curve>_lookup_terms_dev: cols, 6 DevArrays (a, b, c, t1, t2, t3) -> a DevArray of 2n elements: delta + f, then delta + t;
    tagged: zk_plonk_<curve>_lookup_tagged_terms_dev over 8 DevArrays (a, b, c, qK, t1, t2, t3, T0)"""
    fn = _fn(curve, "tagged_terms_dev" if tagged else "terms_dev")
    if len(cols) != (8 if tagged else 6):
        raise ZkError("%s: the terms take %d columns, not %d" % (WHO, 8 if tagged else 6, len(cols)))
    sc = [_scalar(eta, curve, "eta"), _scalar(delta, curve, "delta")]
    ptrs = np.array([d.ptr for d in cols], dtype=np.uint64)
    d_out = DevArray(8 * max(int(n), 1))
    try:
        _check(fn(_ptr(ptrs), int(n), _ptr(sc[0]), _ptr(sc[1]), d_out.ptr, 0))
        return d_out
    except Exception:
        d_out.free()
        raise


def summands(inv, qk, m, n, curve="BN128"):
    """zk_plonk_<curve>_lookup_summands_dev -> a DevArray: out[i] = qK[i] inv[i] - m[i] inv[n + i]"""
    d_out = DevArray(4 * max(int(n), 1))
    try:
        _check(_fn(curve, "summands_dev")(inv.ptr, qk.ptr, m.ptr, int(n), d_out.ptr, 0))
        return d_out
    except Exception:
        d_out.free()
        raise


def lookup_quotient(cols, log_n, alpha, eta, delta, acc, curve="BN128", tagged=False):
    """zk_plonk_<curve>_lookup_quotient_dev: cols, 9 DevArrays of 4n elements (a, b, c, q_K, t1, t2, t3, M, Phi on the coset); acc += alpha^3 L;
    tagged: zk_plonk_<curve>_lookup_tagged_quotient_dev over 10 DevArrays (a, b, c, q_K, t1, t2, t3, T0, M, Phi)"""
    fn = _fn(curve, "tagged_quotient_dev" if tagged else "quotient_dev")
    if len(cols) != (10 if tagged else 9):
        raise ZkError("%s: the quotient takes %d columns, not %d" % (WHO, 10 if tagged else 9, len(cols)))
    m = 4 << int(log_n)
    sc = [_scalar(v, curve, w) for v, w in ((alpha, "alpha"), (eta, "eta"), (delta, "delta"))]
    if any(d.n < 4 * m for d in list(cols) + [acc]):
        raise ZkError("%s: every column of the quotient holds 4n = %d elements" % (WHO, m))
    ptrs = np.array([d.ptr for d in cols], dtype=np.uint64)
    _check(fn(_ptr(ptrs), int(log_n), *[_ptr(s) for s in sc], acc.ptr, 0))
    return acc


def _gate_quotient(cols, log_n, alpha, beta, gamma, k1, k2, curve):
    """zk_plonk_<curve>_quotient_dev, unchanged: the bracket of plonk.py on the coset -> a new DevArray"""
    sc = [_scalar(v, curve, w) for v, w in ((alpha, "alpha"), (beta, "beta"), (gamma, "gamma"), (k1, "k1"), (k2, "k2"))]
    ptrs = np.array([c.ptr for c in cols], dtype=np.uint64)
    d_out = DevArray(16 << int(log_n))
    try:
        _check(getattr(lib(), "zk_plonk_%s_quotient_dev" % _NAME[curve])(_ptr(ptrs), int(log_n), *[_ptr(s) for s in sc], d_out.ptr, 0))
        return d_out
    except Exception:
        d_out.free()
        raise


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    """(curve, log n, l, k_1, k_2, the 12 commitments); `kzg` is the handle verify() pairs with, when the key came from a LookupKey.  With 13
    commitments (T0 last) it is a key of the tagged protocol: self.tagged, and the digest under that protocol's domain string"""

    def __init__(self, curve, log_n, n_public, k1, k2, commitments, kzg=None):
        modulus(curve)
        self.curve, self.log_n, self.n_public, self.k1, self.k2 = curve, int(log_n), int(n_public), int(k1), int(k2)
        self.commitments = [bytes(c) for c in commitments]
        self.kzg = kzg
        if len(self.commitments) not in (N_FIXED, TAGGED_N_FIXED):
            raise ZkError("%s: a verification key holds %d commitments (%d when its tables are tagged), not %d" % (WHO, N_FIXED, TAGGED_N_FIXED, len(self.commitments)))
        self.tagged = len(self.commitments) == TAGGED_N_FIXED
        pa.check_size(curve, self.log_n)
        self.n = 1 << self.log_n
        self.digest = vk_digest(curve, self.log_n, self.n_public, self.k1, self.k2, self.commitments, self.tagged)


def _refuse_other(what, got, tagged):
    """a key or a proof of the single-table protocol under the tagged one, or the reverse, by name"""
    if tagged is not None and got == _protocol(not tagged):
        kind = ("single-table", "tagged")
        raise ZkError('%s: %s of the %s protocol ("%s"), not of the %s protocol ("%s")' % (WHO, what, kind[not tagged], got, kind[tagged], _protocol(tagged)))


def vk_to_json(vk):
    return json.dumps({"protocol": _protocol(vk.tagged), "curve": vk.curve, "log_n": vk.log_n, "n_public": vk.n_public, "k1": str(vk.k1), "k2": str(vk.k2),
                       "commitments": {name: point_to_json(c, vk.curve) for name, c in zip(_fixed_names(vk.tagged), vk.commitments)}}, indent=1) + "\n"


def vk_from_json(text, kzg=None, tagged=None):
    """tagged: None takes a key of either protocol of this module (the file says which), True or False that one alone"""
    js = json.loads(text)
    _refuse_other("a verification key", js.get("protocol"), tagged)
    if js.get("protocol") not in (PROTOCOL, TAGGED_PROTOCOL):
        raise ZkError('%s: not a verification key of this prover (protocol "%s")' % (WHO, js.get("protocol")))
    names = _fixed_names(js["protocol"] == TAGGED_PROTOCOL)
    return VerifyingKey(js["curve"], js["log_n"], js["n_public"], int(js["k1"], 0), int(js["k2"], 0), [point_from_json(js["commitments"][name], js["curve"]) for name in names], kzg)


def proof_to_json(proof, curve):
    """the protocol's name is the tagged one's when the proof holds its 22 values"""
    return pa.proof_to_json(proof, curve, _protocol(len(proof["values"]) == TAGGED_N_VALUES), POINT_NAMES)


def proof_from_json(text, curve, tagged=None):
    """tagged: None takes a proof of either protocol of this module (the file says which), True or False that one alone"""
    got = json.loads(text).get("protocol")
    _refuse_other("a proof", got, tagged)
    proof = pa.proof_from_json(text, curve, TAGGED_PROTOCOL if got == TAGGED_PROTOCOL else PROTOCOL, POINT_NAMES, WHO)
    if len(proof["values"]) != _n_values(got == TAGGED_PROTOCOL):
        raise ZkError("%s: a proof holds %d values, not %d" % (WHO, _n_values(got == TAGGED_PROTOCOL), len(proof["values"])))
    return proof


def proof_to_bytes(proof):
    """A || B || C || M || Z || Phi || T || the 21 values (tagged: 22), 32 little-endian bytes each || W1 || W2"""
    return pa.proof_to_bytes(proof, POINT_NAMES[:7], POINT_NAMES[7:])


def proof_from_bytes(data, point_bytes, tagged=False):
    return pa.proof_from_bytes(data, point_bytes, POINT_NAMES[:7], _n_values(tagged), POINT_NAMES[7:], WHO)


class LookupKey(ArithKey):
    """The proving key on the device: ArithKey's columns; beside them q_K and the table's three columns on H and on the coset, the hash
    table over the padded table's rows, the coefficients of the 12 fixed polynomials and their commitments.  Setup is deterministic and has
    no secret.  self.vk is the verification key.  Over a tagged circuit (self.tagged) the tag column T0 is a fourth column of the table and
    the thirteenth fixed polynomial, and the key, its vk and its proofs are the tagged protocol's."""

    def __init__(self, kzg, circuit):
        if isinstance(circuit, R1csCircuit):
            raise ZkError("%s: an R1csCircuit has no lookups: prove it with plonk.py" % WHO)
        if not isinstance(circuit, LookupCircuit):
            raise ZkError("%s: the key takes a LookupCircuit" % WHO)
        self.table = None
        super().__init__(kzg, circuit, WHO, ("3n + 6", required_powers(circuit.n)))

    def _fixed(self, coef):
        self.coef = list(coef)

    def _build(self):
        super()._build()
        cv, n, k, c = self.curve, self.n, self.log_n, self.circuit
        self.qk_vals = self._keep(pa.mont_dev(cv, c.sel["qK"]))
        self.t_vals = [self._keep(pa.mont_dev(cv, np.ascontiguousarray(c.table[j]))) for j in range(3)]
        self.tagged = c.tagged
        self.tag_vals = [self._keep(pa.mont_dev(cv, c.tag_col))] if c.tagged else []       # T0 on H: the thirteenth fixed polynomial
        self.table = LookupTable(*self.t_vals, n, cv, tag=self.tag_vals[0] if c.tagged else None)
        more = [self._keep(pa.interpolate(cv, v, n, 0, k)) for v in [self.qk_vals] + self.t_vals + self.tag_vals]
        self.lookup_coset = [self._keep(pa.coset_evals(cv, d, n, k + 2)) for d in more]
        self.coef += more
        self.commitments = [self.kzg.commit(d) for d in self.coef]
        self.vk = VerifyingKey(cv, k, c.n_public, self.k1, self.k2, self.commitments, self.kzg)

    def free(self):
        if getattr(self, "table", None) is not None:
            self.table.free()
            self.table = None
        super().free()


def setup(kzg, circuit):
    """-> LookupKey(kzg, circuit); its .vk is the verification key"""
    return LookupKey(kzg, circuit)


# ---- the prover -----------------------------------------------------------------------------------------------------------------------------
def lookup_sum(key, vals, m_vals, eta, delta, bs, keep):
    """phi_0 = 0, phi_(i+1) = phi_i + qK_i / (delta + f_i) - m_i / (delta + t_i), which must close with phi_n = 0;
    Phi += (b_12 X^2 + b_13 X + b_14) Z_H -> Phi's n + 3 coefficients"""
    cv, n = key.curve, key.n
    d = keep(terms(vals + [key.qk_vals] + key.t_vals + key.tag_vals if key.tagged else vals + key.t_vals, n, eta, delta, cv, tagged=key.tagged))
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
    mapping with A, B, C, M, Z, Phi, T, W1, W2 (points) and values (the 21 integers of VALUE_NAMES); publics the l public inputs.  The gate
    equation is checked first, row by row, then the lookups: a selected row whose (a, b, c) is no row of the table is named with the count
    of such rows (under a tagged key also with the table its qK names: a tuple of another table is no row of that one); the permutation
    product and the lookup sum must close.  Under a tagged key the proof holds the 22 values of TAGGED_VALUE_NAMES.  Before returning, the proof is verified (self_check=False skips
    it).  blinding: fourteen integers, FOR TESTS ONLY.  _wires, _opening_transcript, _mark: as in plonk.py, and _wires skips no check;
    _multiplicities (n integers, FOR TESTS ONLY) replaces the counted m."""
    cv, n, k, kzg = key.curve, key.n, key.log_n, key.kzg
    mark = _mark or (lambda name: None)
    own = []

    def keep(d):
        own.append(d)
        return d
    try:
        vals, pi_vals, publics, bs = pa.witness_columns(key, witness, blinding, _wires, WHO, keep, mark, n_blinders=N_BLINDERS)
        m_vals, bad, first = count(key.table, vals[0], vals[1], vals[2], key.qk_vals, n)
        keep(m_vals)
        if bad and key.tagged:
            raise ZkError("%s: witness does not satisfy lookup at row %d (%d rows): (a, b, c) is not a row of table %d, the table the row's qK names" %
                          (WHO, first, bad, int(key.circuit.sel["qK"][first, 0])))
        if bad:
            raise ZkError("%s: witness does not satisfy lookup at row %d (%d rows): (a, b, c) is not a row of the table" % (WHO, first, bad))
        if _multiplicities is not None:
            if len(_multiplicities) != n:
                raise ZkError("%s: _multiplicities takes n values" % WHO)
            m_vals = keep(DevArray.from_host(to_mont(_multiplicities, cv).reshape(-1)))
        mark("lookup check")
        # round 1
        coef = pa.blinded_wires(key, vals, bs, keep)
        m_coef = keep(pa.interpolate(cv, m_vals, n, 2, k))
        pa.blind(cv, m_coef, n, [bs[10], bs[9]])
        A, B, Cc, M = [kzg.commit(d) for d in coef + [m_coef]]
        c0 = transcript_start(cv, key.vk.digest, publics, key.tagged)
        c1, beta, gamma, eta, delta = transcript_wires(cv, c0, A, B, Cc, M)
        mark("round 1")
        # round 2
        z_coef = pa.permutation_product(key, vals, beta, gamma, bs, WHO, keep)
        phi_coef = lookup_sum(key, vals, m_vals, eta, delta, bs, keep)
        Z, Phi = kzg.commit(z_coef), kzg.commit(phi_coef)
        c2, alpha = transcript_sums(cv, c1, Z, Phi)
        mark("round 2")
        # round 3
        pi_coef = keep(pa.interpolate(cv, pi_vals, n, 0, k))
        wires_coset = [keep(pa.coset_evals(cv, d, n + 2, k + 2)) for d in coef]
        cols = wires_coset + [keep(pa.coset_evals(cv, z_coef, n + 3, k + 2))] + key.coset
        cols += [keep(pa.coset_evals(cv, pi_coef, n, k + 2)), key.l1_coset, key.x_coset]
        t = keep(_gate_quotient(cols, k, alpha, beta, gamma, key.k1, key.k2, cv))
        lookup_quotient(wires_coset + key.lookup_coset + [keep(pa.coset_evals(cv, m_coef, n + 2, k + 2)), keep(pa.coset_evals(cv, phi_coef, n + 3, k + 2))], k, alpha, eta, delta, t, cv, tagged=key.tagged)
        t_view = pa.quotient_coeffs(cv, k, t, required_powers(n), WHO + ": the quotient has %d non-zero coefficients from 3n + 6 = %d on: the identity does not hold on H", keep)
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
        polys = key.coef + [View(d, 0, n + 2) for d in coef] + [t_view, View(m_coef, 0, n + 2), View(z_coef, 0, n + 3), View(phi_coef, 0, n + 3)]
        zw = zeta * omega(cv, k) % FR[cv]
        sets = [[zeta]] * (len(key.coef) + 5) + [[zeta, zw]] * 2
        values, W1, W2, _, _ = kzg.open_multi(polys, sets, transcript=_opening_transcript or opening_gamma, transcript_z=opening_z if _opening_transcript is None else pa.plain_z,
                                              commitments=key.commitments + [A, B, Cc, T, M, Z, Phi])
        mark("round 5")
        proof = {"A": A, "B": B, "C": Cc, "M": M, "Z": Z, "Phi": Phi, "T": T, "values": [y for ys in values for y in ys], "W1": W1, "W2": W2}
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
    gamma, eta, delta, alpha, zeta, gamma_open (gamma') and z_open (z')"""
    cv, r = vk.curve, FR[vk.curve]
    c0 = transcript_start(cv, vk.digest, publics, vk.tagged)
    c1, beta, gamma, eta, delta = transcript_wires(cv, c0, proof["A"], proof["B"], proof["C"], proof["M"])
    c2, alpha = transcript_sums(cv, c1, proof["Z"], proof["Phi"])
    c3, zeta = transcript_quotient(cv, c2, proof["T"], vk.n)
    c4, g = transcript_values(cv, c3, proof["values"])
    zw = zeta * omega(cv, vk.log_n) % r
    return {"beta": beta, "gamma": gamma, "eta": eta, "delta": delta, "alpha": alpha, "zeta": zeta, "gamma_open": g, "z_open": transcript_z(cv, c4, proof["W1"], (zeta, zw))}


def lookup_term(curve, v, eta, delta, tagged=False):
    """L at a point from the values there: (Phi(w x) - Phi(x)) (delta + f)(delta + t) - q_K (delta + t) + M (delta + f); tagged: f and t
    carry their fourth column, eta^3 q_K and eta^3 T0 (v["T0"])"""
    r = FR[curve]
    f = (delta + v["a"] + eta * v["b"] + eta * eta % r * v["c"]) % r
    t = (delta + v["T1"] + eta * v["T2"] + eta * eta % r * v["T3"]) % r
    if tagged:
        f, t = (f + pow(eta, 3, r) * v["qK"]) % r, (t + pow(eta, 3, r) * v["T0"]) % r
    return ((v["Phiw"] - v["Phi"]) * f % r * t - v["qK"] * t + v["M"] * f) % r


def identity_holds(curve, log_n, k1, k2, publics, values, ch):
    """the identity of round 3 at zeta in the field, from the 21 values (the 22 of the tagged protocol): the bracket equals t(zeta) Z_H(zeta)"""
    v, alpha, r = dict(zip(TAGGED_VALUE_NAMES if len(values) == TAGGED_N_VALUES else VALUE_NAMES, values)), ch["alpha"], FR[curve]
    gate, perm, l1z, zh = pa.identity_terms(curve, log_n, k1, k2, publics, ch["zeta"], v, ch["beta"], ch["gamma"])
    return (gate + alpha * perm + alpha * alpha % r * l1z + pow(alpha, 3, r) * lookup_term(curve, v, ch["eta"], ch["delta"], len(values) == TAGGED_N_VALUES) - v["t"] * zh) % r == 0


def host_check(vk, publics, proof, point_bytes=None):
    """what the verifier decides on the host, before any device work: lengths (an error), every scalar below r (else INPUT_NOT_CANONICAL),
    the challenges, the identity (else REJECTED) -> (verdict, the tuple Kzg.verify_multi takes, built with the verifier's OWN gamma' and z')"""
    cv, r = vk.curve, FR[vk.curve]
    nf = len(vk.commitments)
    shape = pa.check_proof_shape(proof, POINT_NAMES, _n_values(vk.tagged), point_bytes if point_bytes is not None else len(vk.commitments[0]), vk.n_public, publics, r, WHO)
    if shape is None:
        return INPUT_NOT_CANONICAL, None
    values, publics = shape
    ch = challenges(vk, publics, proof)
    if not identity_holds(cv, vk.log_n, vk.k1, vk.k2, publics, values, ch):
        return REJECTED, None
    zeta = ch["zeta"]
    zw = zeta * omega(cv, vk.log_n) % r
    sets = [[zeta]] * (nf + 5) + [[zeta, zw]] * 2
    vals = [[v] for v in values[:nf + 5]] + [values[nf + 5:nf + 7], values[nf + 7:nf + 9]]
    cs = vk.commitments + [proof["A"], proof["B"], proof["C"], proof["T"], proof["M"], proof["Z"], proof["Phi"]]
    return ACCEPTED, (cs, sets, vals, ch["gamma_open"], ch["z_open"], proof["W1"], proof["W2"])


def verify(vk, publics, proofs, kzg=None, seed=None, locate=True):
    """m proofs under one verification key: publics[i] are proof i's public inputs -> (verdict, first_bad) as Kzg.verify_multi gives them.
    The host part of every proof first (host_check), then ONE randomised pairing check of all of them: two pairings."""
    return pa.verify_batch(vk, publics, proofs, host_check, kzg, seed, locate, WHO)
