"""pil_verify on the GPU (csrc/pil_check.hip, check1 in csrc/expr_bytecode.hip): the device's report against the plain-Python checker
(tests/pil_check_ref.py), the whole report, field by field and exactly -- these are integers and minima, there is no tolerance.
Each corruption is checked on the CPU first to be the case its name says."""
import functools
import importlib
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import pil_check_ref as REF
from test_pil_check_host import D, INPUTS, load_input

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
P = REF.P
N = 1024
GL_STRUCT = {"nBits": 10, "nBitsExt": 11, "nQueries": 8, "verificationHashType": "GL", "steps": [{"nBits": 11}, {"nBits": 7}, {"nBits": 3}]}


@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)
    return zk


@functools.lru_cache(maxsize=None)
def _input(name):
    return load_input(name)


@functools.lru_cache(maxsize=None)
def _checker(name):
    import eigen_zkvm_amd
    return eigen_zkvm_amd.PilCheck(_input(name)[0])


def _compare(dev, name, const=None, cm=None):
    """device report == reference report on (a corrupted copy of) input `name`; -> the report"""
    pil, c0, m0 = _input(name)
    const, cm = c0 if const is None else const, m0 if cm is None else cm
    want = REF.check(pil, const, cm)
    got = _checker(name).run(const, cm)
    assert got == want
    return got


def _cell(name, cm, row, col, value=None):
    """a copy of the trace with one cell changed (flipped in its lowest bit when no value is given)"""
    w = _input(name)[0]["nCommitments"]
    out = cm.copy()
    out[row * w + col] = (int(out[row * w + col]) ^ 1) if value is None else value
    return out


# ---- clean inputs, publics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
def test_clean_inputs_have_no_findings(dev, name):
    rep = _compare(dev, name)
    assert rep["findings"] == [] and rep["n"] == N
    assert rep["checked"]["polIdentities"] == len(_input(name)[0]["polIdentities"])


def test_publics_are_the_provers(dev):
    stark = importlib.import_module("eigen_zkvm_amd.stark")
    pil, const, cm = _input("fib")
    ss = GL_STRUCT
    setup = stark.NativeStarkSetup(const, stark.generate_program(json.dumps(pil), json.dumps(ss)), json.dumps(ss), eval_mode="bytecode")
    zkin = setup.gen(cm)
    setup.free()
    assert len(zkin["publics"]) == 3
    assert _compare(dev, "fib")["publics"] == [str(p) for p in zkin["publics"]]


# ---- polynomial identities: fib ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [77, 0, N - 1])
def test_one_flipped_cell(dev, row):
    _, _, cm = _input("fib")
    rep = _compare(dev, "fib", cm=_cell("fib", cm, row, 0))
    f = rep["findings"]
    assert f and all(x["kind"] == "identity" for x in f)
    rows = {int(x["first_row"]) for x in f}
    assert (row - 1) % N in rows or row in rows                               # the row itself, or the one that reads it through `next`
    # (fib's identities are gated by 1 - LLAST, so row N - 1 itself never fails: test_chunk_loop and test_one_wave hold the wrap of `next`)


def test_three_flipped_cells_count_rows_and_keep_the_minimum(dev):
    _, _, cm = _input("fib")
    bad = cm
    for row in (700, 301, 302):
        bad = _cell("fib", bad, row, 1)
    f = _compare(dev, "fib", cm=bad)["findings"]
    assert f and max(int(x["n_rows"]) for x in f) >= 3
    assert min(int(x["first_row"]) for x in f) in (300, 301)


def test_every_row_of_a_column_replaced(dev):
    pil, _, cm = _input("fib")
    bad = cm.copy()
    bad[0::pil["nCommitments"]] = np.random.default_rng(5).integers(0, P, size=N, dtype=np.uint64)
    f = _compare(dev, "fib", cm=bad)["findings"]
    assert any(int(x["n_rows"]) >= N - 2 and x["first_row"] == "0" for x in f)   # the all-lanes-fail path


# ---- the chunk loop: a' = a + b -----------------------------------------------------------------------------------------------------------
def _sum_pil(n):
    cm = lambda i, nxt=False: {"op": "cm", "deg": 1, "id": i, "next": nxt}
    return {"nCommitments": 2, "nQ": 0, "nIm": 0, "nConstants": 1, "publics": [],
            "references": {"Global.L1": {"type": "constP", "id": 0, "polDeg": n, "isArray": False},
                           "Sum.a": {"type": "cmP", "id": 0, "polDeg": n, "isArray": False}, "Sum.b": {"type": "cmP", "id": 1, "polDeg": n, "isArray": False}},
            "expressions": [{"op": "sub", "deg": 1, "values": [cm(0, True), {"op": "add", "deg": 1, "values": [cm(0), cm(1)]}]}],
            "polIdentities": [{"e": 0, "fileName": "sum.pil", "line": 5}],
            "plookupIdentities": [], "permutationIdentities": [], "connectionIdentities": []}


@functools.lru_cache(maxsize=None)
def _sum_input(nbits):
    n = 1 << nbits
    b = np.random.default_rng(nbits).integers(0, 1 << 20, size=n, dtype=np.uint64)
    a = np.ones(n, dtype=np.uint64)
    a[1:] += np.cumsum(b[:-1], dtype=np.uint64)                               # a[i + 1] = a[i] + b[i], no reduction needed below 2^40
    b[n - 1] = (1 - int(a[n - 1])) % P                                        # the wrap: a[0] = a[N - 1] + b[N - 1]
    cm = np.empty(2 * n, dtype=np.uint64); cm[0::2] = a; cm[1::2] = b
    const = np.zeros(n, dtype=np.uint64); const[0] = 1
    import eigen_zkvm_amd
    pil = _sum_pil(n)
    return pil, const, cm, eigen_zkvm_amd.PilCheck(pil)


def _sum_case(dev, nbits, bad_row):
    pil, const, cm, chk = _sum_input(nbits)
    if bad_row is not None:
        cm = cm.copy(); cm[2 * bad_row + 1] = (int(cm[2 * bad_row + 1]) + 1) % P
    want = REF.check(pil, const, cm)
    assert chk.run(const, cm) == want
    if bad_row is None:
        assert want["findings"] == []
    else:                                                                     # the only bad cell: one failing row, value a' - a - b = -1
        (f,) = want["findings"]
        assert (f["n_rows"], f["first_row"], f["value"], f["fileName"], f["line"]) == ("1", str(bad_row), str(P - 1), "sum.pil", 5)


@pytest.mark.parametrize("bad_row", [None, (1 << 18) + 64 + 5, (1 << 19) - 1])
def test_chunk_loop(dev, bad_row):
    """2^19 rows: a wave of the capped grid (4096 waves) walks two chunks, 2^18 rows apart; the finding comes from the second"""
    _sum_case(dev, 19, bad_row)


@pytest.mark.parametrize("bad_row", [None, 0, 63])
def test_one_wave(dev, bad_row):
    _sum_case(dev, 6, bad_row)


# ---- plookup: f = (a, b', a b') under sel, t = (A, B, cc) under SEL --------------------------------------------------------------------------
def _plookup_sides():
    pil, const, cm = _input("plookup")
    R = REF.Rows(pil, const, cm)
    (pl,) = pil["plookupIdentities"]
    f = list(zip(*[R.exp(k).tolist() for k in pl["f"]])); t = list(zip(*[R.exp(k).tolist() for k in pl["t"]]))
    return f, t, R.exp(pl["selF"]).tolist(), R.exp(pl["selT"]).tolist()


def test_plookup_selected_row_with_a_missing_tuple(dev):
    f, t, sf, st = _plookup_sides()
    assert sf[3] == 1
    (x,) = _compare(dev, "plookup", cm=_cell("plookup", _input("plookup")[2], 3, 1, 999983))["findings"]
    assert (x["kind"], x["n_rows"], x["first_row"], x["values"][0], x["fileName"], x["line"]) == ("plookup", "1", "3", "999983", "plookup.pil", 9)


def test_plookup_unselected_row_is_not_looked_up(dev):
    f, t, sf, st = _plookup_sides()
    row = sf.index(0)
    assert _compare(dev, "plookup", cm=_cell("plookup", _input("plookup")[2], row, 1, 999983))["findings"] == []


def test_plookup_tuple_with_two_columns_swapped(dev):
    """(q, p, p q) against a table that holds (p, q, p q) and not (q, p, p q): equal as a set of words, not as a tuple.  The fixture's table
    is a whole multiplication table, symmetric in its first two columns, so the case is built: the t row (q, p, p q) is deselected."""
    pil, const, cm = _input("plookup")
    f, t, sf, st = _plookup_sides()
    p, q = 2, 3
    lost = [i for i in range(N) if st[i] and t[i] == (q, p, p * q)]
    bad_const = const.copy()
    for i in lost:
        bad_const[i * pil["nConstants"] + 1] = 0                             # SEL
    table = {t[i] for i in range(N) if st[i] and i not in lost}
    assert lost and (p, q, p * q) in table and (q, p, p * q) not in table and (q, p, p * q) not in [f[i] for i in range(N) if sf[i]]
    row = next(i for i in range(N - 1) if sf[i] and not sf[i + 1])            # b is read at the next row: that row must not look anything up
    assert _compare(dev, "plookup", const=bad_const)["findings"] == []
    (x,) = _compare(dev, "plookup", const=bad_const, cm=_cell("plookup", _cell("plookup", cm, row, 1, q), row + 1, 2, p))["findings"]
    assert (x["kind"], x["n_rows"], x["first_row"], x["values"]) == ("plookup", "1", str(row), [str(q), str(p), str(p * q)])
    assert _compare(dev, "plookup", const=bad_const, cm=_cell("plookup", _cell("plookup", cm, row, 1, p), row + 1, 2, q))["findings"] == []   # unswapped: held


def test_plookup_selector_outside_0_1(dev):
    f, t, sf, st = _plookup_sides()
    assert sf[5] == 1
    (x,) = _compare(dev, "plookup", cm=_cell("plookup", _input("plookup")[2], 5, 0, 2))["findings"]
    assert (x["kind"], x["identity"], x["side"], x["n_rows"], x["first_row"], x["value"]) == ("selector", "plookup", "f", "1", "5", "2")


# ---- permutation: f = (c, c) under selC, t = (d, d) under selD --------------------------------------------------------------------------------
def test_permutation_one_tuple_changed(dev):
    (x,) = _compare(dev, "pe", cm=_cell("pe", _input("pe")[2], 0, 2, 999983))["findings"]
    assert (x["kind"], x["n_f_unmatched"], x["n_t_unmatched"], x["first_f_row"], x["first_t_row"]) == ("permutation", "1", "1", "0", "0")
    assert (x["f_values"], x["t_values"]) == (["999983", "999983"], ["1", "1"])


def test_permutation_multiplicity(dev):
    pil, const, cm = _input("pe")
    c = cm[2::6]
    assert cm[4] == 1 and cm[2 * 6 + 4] == 1 and c[0] != c[2]                 # rows 0 and 2 are selected f rows with different tuples
    (x,) = _compare(dev, "pe", cm=_cell("pe", cm, 0, 2, int(c[2])))["findings"]
    assert (x["n_f_unmatched"], x["n_t_unmatched"], x["first_f_row"]) == ("1", "1", "0")      # (c2, c2) twice against once; (c0, c0) lost on the t side
    assert x["f_values"] == [str(c[2])] * 2 and x["t_values"] == [str(c[0])] * 2


def test_permutation_t_row_deselected(dev):
    pil, const, cm = _input("pe")
    assert cm[4 * 6 + 5] == 1
    (x,) = _compare(dev, "pe", cm=_cell("pe", cm, 4, 5, 0))["findings"]
    assert (x["n_f_unmatched"], x["n_t_unmatched"], x["first_t_row"], x["t_values"]) == ("1", "0", None, None)
    assert x["f_values"] == [str(cm[4 * 6 + 3])] * 2


# ---- connection: { a, b, c } wired by { S1, S2, S3 } -------------------------------------------------------------------------------------------
def test_connection_one_wired_cell_changed(dev):
    pil, const, cm = _input("connection")
    where = REF.identity_cells(N, 3)
    j, i = next((j, i) for i in range(N) for j in range(3) if where[int(const[i * 4 + 1 + j])] != (j, i))
    jj, ii = where[int(const[i * 4 + 1 + j])]
    old = int(cm[i * 3 + j])
    f = _compare(dev, "connection", cm=_cell("connection", cm, i, j, 999983))["findings"]
    (x,) = f
    assert x["kind"] == "connection" and int(x["n_cells"]) >= 1
    cells = {(x["col"], int(x["row"])): x["value"], (x["partner_col"], int(x["partner_row"])): x["partner_value"]}
    assert (j, i) in cells and cells[(j, i)] == "999983" and str(old) in cells.values()
    assert (jj, ii) in cells or int(x["n_cells"]) >= 2                       # (the cell wired to (j, i) differs as well, and may come first)


def test_connection_value_that_names_no_cell(dev):
    pil, const, cm = _input("connection")
    assert 5 not in REF.identity_cells(N, 3)
    bad = const.copy(); bad[200 * 4 + 2] = 5                                  # S2 at row 200
    f = _compare(dev, "connection", const=bad)["findings"]
    x = f[0]
    assert (x["kind"], x["n_cells"], x["col"], x["row"], x["value"]) == ("connection_value", "1", 1, "200", "5")
    assert all(y["kind"] == "connection" for y in f[1:])


# ---- device-resident inputs -----------------------------------------------------------------------------------------------------------------------
def test_device_resident_inputs(dev):
    pil, const, cm = _input("fib")
    bad = _cell("fib", cm, 77, 0)
    d_const, d_cm = dev.DevArray.from_host(const), dev.DevArray.from_host(bad)
    chk = _checker("fib")
    got = chk.run(d_const, d_cm)
    assert got == chk.run(const, bad) == REF.check(pil, const, bad)
    assert np.array_equal(d_cm.to_host(), bad) and np.array_equal(d_const.to_host(), const)   # borrowed, not written
    d_const.free(); d_cm.free()


# ---- the command line, one fresh process each ---------------------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run([sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")] + args, capture_output=True, text=True, timeout=300)


def test_cli_pil_verify_clean(dev, tmp_path):
    r = _cli(["pil_verify", "-p", str(D / "fib.pil.json"), "--o", str(D / "fib.const"), "--m", str(D / "fib.cm"), "--report", str(tmp_path / "r.json")])
    assert r.returncode == 0, r.stderr
    assert json.load(open(tmp_path / "r.json"))["findings"] == []


def test_cli_pil_verify_findings(dev, tmp_path):
    pil, const, cm = _input("fib")
    bad = _cell("fib", cm, 77, 0)
    bad.astype("<u8").tofile(tmp_path / "bad.cm")
    r = _cli(["pil_verify", "-p", str(D / "fib.pil.json"), "--o", str(D / "fib.const"), "--m", str(tmp_path / "bad.cm"), "--report", str(tmp_path / "r.json")])
    assert r.returncode == 1, r.stderr
    want = REF.check(pil, const, bad)
    assert json.load(open(tmp_path / "r.json")) == want
    lines = r.stdout.splitlines()
    assert len(lines) == len(want["findings"]) > 0
    for line, f in zip(lines, want["findings"]):
        assert line.startswith("fibonacci.pil:%d: identity %d: " % (f["line"], f["index"]))


def test_cli_stark_prove_check_trace_stops(dev, tmp_path):
    _, _, cm = _input("fib")
    _cell("fib", cm, 77, 0).astype("<u8").tofile(tmp_path / "bad.cm")
    (tmp_path / "ss.json").write_text(json.dumps(GL_STRUCT))
    r = _cli(["stark_prove", "-s", str(tmp_path / "ss.json"), "-p", str(D / "fib.pil.json"), "--o", str(D / "fib.const"), "--m", str(tmp_path / "bad.cm"),
              "--i", str(tmp_path / "zkin.json"), "--check-trace", "--eval", "bytecode"])
    assert r.returncode == 1
    assert "fibonacci.pil:" in r.stderr and not (tmp_path / "zkin.json").exists()
