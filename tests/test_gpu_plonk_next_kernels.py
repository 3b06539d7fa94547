"""The kernels of the PLONK prover with a next-row term (csrc/plonk_next_impl.hip.h) word for word against Python integers on
both fields: the numerator of the quotient with q_N c[(i + 4) mod m] at log_n = 3 and 5, the row-by-row gate check that reads c[(i + 1) mod n],
and the extension of a witness under the chain rule (a store step of 2).  An input element is the 256-bit integer its words are (any value
below 2^256) and stands for words / 2^256 mod r; every output word vector must be the canonical Montgomery representative.  Exact: no
tolerance anywhere."""
import importlib, random

import numpy as np
import pytest

import plonk_next_ref as nref
import plonk_r1cs_ref as model
import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")
ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
NAMES = ("a", "b", "c", "Z", "qL", "qR", "qO", "qM", "qC", "S1", "S2", "S3", "PI", "L1", "X", "qN")   # the order of zk_plonk_<curve>_next_quotient_dev
TOP = (1 << 256) - 1


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def pn(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_next")


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


def _dev(zk, words):
    a = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in words), dtype="<u8").astype(np.uint64)
    return zk.DevArray.from_host(a)


def _host(d, n):
    b = d.to_host()[:4 * n].astype("<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _want_quotient(r, cols, m, alpha, beta, gamma, k1, k2):
    rinv = pow(1 << 256, -1, r)
    val = {k: [w * rinv % r for w in cols[k]] for k in NAMES}
    out = []
    for i in range(m):
        v = {k: val[k][i] for k in NAMES}
        v["Zw"], v["cw"] = val["Z"][(i + 4) % m], val["c"][(i + 4) % m]
        out.append((nref.bracket(r, v, v["X"], v["PI"], v["L1"], beta, gamma, alpha, k1, k2) << 256) % r)
    return out


def _run(zk, fn, names, cv, log_n, cols, *scalars):
    ds = [_dev(zk, cols[k]) for k in names]
    try:
        out = fn(ds, log_n, *scalars, cv)
        try:
            return _host(out, 4 << log_n)
        finally:
            out.free()
    finally:
        for d in ds:
            d.free()


@pytest.mark.parametrize("log_n", (3, 5))
@pytest.mark.parametrize("cv", CURVES)
def test_quotient_word_for_word(zk, pn, plonk, cv, log_n):
    r, m, rng = nref.R[cv], 4 << log_n, random.Random(0x2810 + log_n + len(cv))
    mont = lambda v: (v << 256) % r
    rand = lambda: {k: [mont(rng.randrange(r)) for _ in range(m)] for k in NAMES}
    const = lambda w: {k: [w] * m for k in NAMES}
    wide = {k: [rng.randrange(r, 1 << 256) for _ in range(m)] for k in NAMES}             # words >= r but < 2^256
    for k in NAMES:
        wide[k][0], wide[k][1], wide[k][m - 1] = TOP, r, TOP
    # c alone distinct at the wrap, q_N = 1: elements 4n - 4 .. 4n - 1 read c at 0 .. 3, and Z is constant so that only c tells
    wrap = const(mont(1))
    wrap["c"] = [mont(i + 2) for i in range(m)]
    # q_N and the c it reads both at 2^256 - 1 in the same element, everything else random: elements 0 (reads c[4]) and m - 4 (reads c[0])
    pair = rand()
    for i in (0, m - 4):
        pair["qN"][i], pair["c"][(i + 4) % m] = TOP, TOP
    sc = lambda: [rng.randrange(r) for _ in range(3)]
    big = (rng.randrange(4, r), rng.randrange(4, r))
    cases_ = [("random, k = 2, 3", rand(), sc(), (2, 3)),
              ("random, large k", rand(), sc(), big),
              ("all zero", const(0), sc(), (2, 3)),
              ("all r - 1, every scalar r - 1", const(mont(r - 1)), [r - 1] * 3, (r - 1, r - 1)),
              ("every operand 2^256 - 1, every scalar r - 1", const(TOP), [r - 1] * 3, (r - 1, r - 1)),
              ("every operand 2^256 - 1, small k by additions, every scalar r - 1", const(TOP), [r - 1] * 3, (2, 3)),
              ("words >= r", wide, sc(), (2, 3)),
              ("words >= r, large k, scalars r - 1", wide, [r - 1] * 3, big),
              ("q_N and its c at 2^256 - 1 in one element", pair, sc(), (2, 3)),
              ("the wrap of c(wX)", wrap, sc(), (2, 3)),
              ("alpha = beta = gamma = 0", rand(), [0, 0, 0], (2, 3))]
    for name, cols, (alpha, beta, gamma), (k1, k2) in cases_:
        got = _run(zk, pn.quotient, NAMES, cv, log_n, cols, alpha, beta, gamma, k1, k2)
        want = _want_quotient(r, cols, m, alpha, beta, gamma, k1, k2)
        assert all(w < r for w in got), name                                               # canonical
        assert got[m - 4:] == want[m - 4:], name                                           # the four elements that wrap
        assert got == want, name
    # the wrap is read: the last four outputs move with c[0 .. 3], which only q_N reaches from there
    moved = {k: list(v) for k, v in wrap.items()}
    for i in range(4):
        moved["c"][i] = mont(1000 + i)
    s = sc()
    a, b = (_run(zk, pn.quotient, NAMES, cv, log_n, cols, *s, 2, 3) for cols in (wrap, moved))
    assert all(a[i] != b[i] for i in range(m - 4, m))
    # q_N = 0 everywhere: the parent's kernel's output on the same columns, word for word
    for cols in (rand(), wide, const(TOP)):
        cols = dict(cols, qN=[0] * m)
        s = sc()
        assert _run(zk, pn.quotient, NAMES, cv, log_n, cols, *s, 2, 3) == _run(zk, plonk.quotient, NAMES[:15], cv, log_n, cols, *s, 2, 3)


@pytest.mark.parametrize("cv", CURVES)
def test_quotient_refusals(zk, pn, cv):
    r = nref.R[cv]
    cols = [_dev(zk, [0] * 32) for _ in range(16)]
    try:
        with pytest.raises(pn.ZkError, match="plonk next: quotient: the output overlaps column 15"):
            pn.quotient(cols, 3, 1, 2, 3, 2, 3, cv, out=cols[15])
        with pytest.raises(pn.ZkError, match="beta is not below"):
            pn.quotient(cols, 3, 1, r, 3, 2, 3, cv)
        with pytest.raises(pn.ZkError, match="every column of the quotient holds 4n = 64"):
            pn.quotient(cols, 4, 1, 2, 3, 2, 3, cv)
        with pytest.raises(pn.ZkError, match="takes 16 columns"):
            pn.quotient(cols[:15], 3, 1, 2, 3, 2, 3, cv)
        with pytest.raises(pn.ZkError, match="takes 10 columns"):
            pn.gate_check(cols[:9], 8, cv)
        with pytest.raises(pn.ZkError, match="holds n = 64 elements"):
            pn.gate_check(cols[:10], 64, cv)
    finally:
        for d in cols:
            d.free()


def _gate_rows(r, n, rng):
    """n rows that satisfy the gate equation with the next row's c (cyclic), as values per column in the order a, b, c, qL, qR, qO, qM, qC,
    PI, qN: c is drawn first for every row, then q_C closes each row"""
    cs = [rng.randrange(1, r) for _ in range(n)]
    rows = []
    for i in range(n):
        a, b, ql, qr, qo, qm, pi, qn = (rng.randrange(r) for _ in range(8))
        qc = -(ql * a + qr * b + qo * cs[i] + qm * a * b + qn * cs[(i + 1) % n] + pi) % r
        rows.append((a, b, cs[i], ql, qr, qo, qm, qc, pi, qn))
    return rows


@pytest.mark.parametrize("n", (8, 2048, 2049))
@pytest.mark.parametrize("cv", CURVES)
def test_gate_check_counts_exactly(zk, pn, cv, n):
    r, rng = nref.R[cv], random.Random(0x2820 + len(cv) + n)
    rows = _gate_rows(r, n, rng)
    mont = lambda v: (v << 256) % r
    fixed = [_dev(zk, [mont(row[j]) for row in rows]) for j in range(10)]

    def run(cols=()):
        """the columns in `cols` (index -> values) replace the satisfied ones"""
        ds = {j: _dev(zk, [mont(v) for v in vals]) for j, vals in dict(cols).items()}
        try:
            return pn.gate_check([ds.get(j, fixed[j]) for j in range(10)], n, cv)
        finally:
            for d in ds.values():
                d.free()

    def col(j, at, delta=1):
        vals = [row[j] for row in rows]
        for i in at:
            vals[i] = (vals[i] + delta) % r
        return vals
    try:
        assert run() == (0, None)
        # c of row 0 moved: row 0 fails through q_O and row n - 1 ONLY through the wrap; with q_O of row 0 zero the wrap row alone
        assert run(cols={2: col(2, [0])}) == (2, 0)
        qo0, qc0 = col(5, [0], -rows[0][5]), col(7, [0], rows[0][5] * rows[0][2])          # q_O[0] = 0, q_C[0] takes its share: row 0 still holds
        assert run(cols={5: qo0, 7: qc0}) == (0, None)
        assert run(cols={5: qo0, 7: qc0, 2: col(2, [0])}) == (1, n - 1)
        # a failure only through q_N: the selector itself moved, at the first row, across a workgroup's edge and at the wrap row
        for at in [[0], [n - 1], [n - 1, 0], [n // 2, 3]] + ([[255], [256], [255, 256], [2047], [n - 1, 1024, 7]] if n > 8 else []):
            assert run(cols={9: col(9, at)}) == (len(at), min(at)), at
        # c[i] moved with q_O[i] = 0: row i - 1 alone fails, through its q_N
        i = n // 2
        qo, qc = col(5, [i], -rows[i][5]), col(7, [i], rows[i][5] * rows[i][2])
        assert run(cols={5: qo, 7: qc, 2: col(2, [i])}) == (1, i - 1)
        assert run(cols={7: col(7, range(n))}) == (n, 0)
        # the largest representative below 2^256 of every word of satisfied rows: still satisfied
        lift = lambda w: w + r * ((TOP - w) // r)
        ds = [_dev(zk, [lift(mont(row[j])) for row in rows]) for j in range(10)]
        try:
            assert pn.gate_check(ds, n, cv) == (0, None)
        finally:
            for d in ds:
                d.free()
    finally:
        for d in fixed:
            d.free()


# ---- the extension under the chain rule ---------------------------------------------------------------------------------------------------
def edge_lengths(T):
    return sorted({3, 4, 5, T - 2, T - 1, T, T + 1, T + 2, 127, 128, 129, 255, 64 * 5 + 1})


def edges(field, T):
    """one product constraint per length t: (sum of t wires, each times p - 1) * b = out, every wire p - 1 -> (r1cs bytes, witness)"""
    p = model.R[field]
    lengths = edge_lengths(T)
    w = [1] + [p - 1] * max(lengths)
    b = len(w); w.append(p - 1)
    cons = []
    for t in lengths:
        w.append(t * (p - 1) * (p - 1) * (p - 1) % p)
        cons.append(([(j, p - 1) for j in range(1, t + 1)], [(b, 1)], [(len(w) - 1, 1)]))
    return cases.write(field, len(w), cons), w


@pytest.mark.parametrize("field", CURVES)
@pytest.mark.parametrize("name", ("shapes", "edges"))
def test_the_extension_with_step_two_is_the_models_word_for_word(zk, pn, name, field):
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    T = int(zk.lib().zk_plonk_r1cs_wave_min_terms())
    data, w = cases.shapes(field)[:2] if name == "shapes" else edges(field, T)
    m = nref.Compiled(data, field)
    ext = m.extend(w)
    assert not m.failing_gates(ext)
    lens = [len(t) for _, t in m.segments]
    if name == "shapes":
        assert max(lens) == 1000 and min(lens) <= 4 and any(n % 2 for n in lens) and len(lens) == 10     # short chains, odd and even, beside the long row
    else:
        assert lens == edge_lengths(T) and 255 in lens and {T - 1, T + 1} <= set(lens) and (T - 1) % 2 and sum(n >= T for n in lens) > 4    # odd m through the wave kernel
    want = kzg.to_mont(ext, field)
    c = pn.NextR1csCircuit(data, field)
    try:
        assert (c.n_vars, c.n_wires, c.n_aux) == (m.n_vars, m.n_wires, m.n_aux)
        buf = want.copy()
        buf[m.n_wires:] = np.uint64(0xFFFFFFFFFFFFFFFF)                               # what the call must overwrite; the front it must leave
        for _ in range(2):                                                            # the second call finds the table on the device
            d = zk.DevArray.from_host(buf.reshape(-1))
            try:
                zk._check(getattr(zk.lib(), "zk_plonk_%s_r1cs_extend_dev" % ABI[field])(c._h, d.ptr, None))
                got = d.to_host().reshape(-1, 4)
            finally:
                d.free()
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, "variable %d of %d differs (n_wires = %d)" % (int(bad[0]), m.n_vars, m.n_wires)
    finally:
        c.free()
