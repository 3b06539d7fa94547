"""wtns_check without a GPU: the plain-Python checker the device tests compare against (tests/r1cs_check_ref.py) accepts the
witnesses of the project's satisfiable circuits and reports exactly what is planted; the .sym parser; the command line's new
flags; the six prototypes of include/zkgpu.h."""
import pathlib
import re
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import c12_setup_circuits as CIRC  # noqa: E402
import c12_setup_ref as REF  # noqa: E402
import groth16 as G  # noqa: E402
import r1cs_check_cases as CASES  # noqa: E402
import r1cs_check_ref as RC  # noqa: E402
import zkgpu_prove  # noqa: E402

GOLD = ROOT / "tests" / "golden" / "groth16"
KIND = {"cmuladd": "cmuladd", "poseidon": "poseidon12", "fft4": "fft4", "evpol4": "evpol4"}


def clean(rep):
    return rep["findings"] == [] and not any(rep["n_failing"].values())


def test_ref_accepts_plain_circuit():
    b, w = CIRC.plain_circuit()
    rep = RC.check(RC.circuit("GL", b), w)
    assert clean(rep) and rep["checked"]["constraint"] == 29 and rep["n_wires"] == len(w)


@pytest.mark.parametrize("kind", ["cmuladd", "poseidon", "fft4", "evpol4"])
def test_ref_accepts_custom_gate_witnesses(kind):
    b, w = CIRC.with_custom(kind)
    rep = RC.check(RC.circuit("GL", b), w)
    assert clean(rep) and rep["checked"][KIND[kind]] == (2 if kind == "fft4" else 1)


@pytest.mark.parametrize("field", ["BN128", "BLS12381"])
def test_ref_accepts_synthetic_r1cs(field):
    p = RC.PRIMES[field]
    r, w = G.synthetic_r1cs(p, 40, seed=5)
    b = REF.write_r1cs(r["n_wires"], r["n_pub_out"], r["n_pub_in"], r["n_prv_in"], r["constraints"], field_size=32, prime=p)
    rep = RC.check(RC.circuit(field, b), w)
    assert clean(rep) and rep["n_constraints"] == len(r["constraints"])


@pytest.mark.parametrize("field", CASES.FIELDS)
def test_ref_names_the_one_broken_constraint(field):
    p = RC.PRIMES[field]
    b, w, outs = CASES.products(field, 257)
    circ = RC.circuit(field, b)
    assert clean(RC.check(circ, w))
    for i in (0, 63, 64, 256):
        rep = RC.check(circ, CASES.corrupt(w, outs[i], p=p))
        (f,) = rep["findings"]
        assert f["kind"] == "constraint" and f["index"] == i and rep["n_failing"]["constraint"] == 1
        assert int(f["a"]) * int(f["b"]) % p == w[outs[i]] and int(f["c"]) == (w[outs[i]] + 1) % p
        assert f["wires"]["c"] == [[outs[i], "1"]]


@pytest.mark.parametrize("field", CASES.FIELDS)
def test_ref_row_shapes_and_one_wire(field):
    p = RC.PRIMES[field]
    b, w, long_row, cw = CASES.shapes(field)
    circ = RC.circuit(field, b)
    assert clean(RC.check(circ, w))
    (f,) = RC.check(circ, CASES.corrupt(w, cw, p=p))["findings"]
    assert (f["index"], f["a"], f["b"], f["c"]) == (long_row, "1000", "1", "1001") and len(f["wires"]["a"]) == 1000
    b2, w2, _ = CASES.products(field, 5)
    rep = RC.check(RC.circuit(field, b2), [2] + w2[1:])
    assert rep["findings"] == [{"kind": "one_wire", "value": "2"}] and rep["n_failing"]["one_wire"] == 1


def test_ref_max_findings_keeps_the_lowest_and_counts_all():
    b, w, outs = CASES.products("GL", 1000)
    import random
    bad = sorted(random.Random(9).sample(range(1000), 200))
    for i in bad: w[outs[i]] = (w[outs[i]] + 1) % REF.P
    rep = RC.check(RC.circuit("GL", b), w, max_findings=16)
    assert [f["index"] for f in rep["findings"]] == bad[:16] and rep["n_failing"]["constraint"] == 200


def test_ref_reference_fixtures():
    b = (GOLD / "mycircuit_bls12381.r1cs").read_bytes()
    circ = RC.circuit("BLS12381", b)
    assert clean(RC.check(circ, [1, 33, 3, 11]))
    assert RC.check(circ, [1, 34, 3, 11])["findings"][0]["index"] == 0
    import numpy as np
    w = [int(v) for v in np.frombuffer((GOLD / "witness.wtns").read_bytes()[-128:], dtype="<u8")[::4]]
    assert w == [1, 11210000, 1121, 10000]
    c2 = RC.circuit("BN128", CASES.one_constraint("BN128"))
    assert clean(RC.check(c2, w))
    p = RC.PRIMES["BN128"]
    (f,) = RC.check(c2, [1, 11210001, 1121, 10000])["findings"]
    assert (int(f["a"]), int(f["b"]), int(f["c"])) == (p - 1121, 10000, p - 11210001)


@pytest.mark.parametrize("kind,signal,expect", [
    ("cmuladd", 0, ("cmuladd", 0, 0)), ("cmuladd", 11, ("cmuladd", 0, 2)),
    ("poseidon", 0, ("poseidon12", 0, (0, 0))), ("poseidon", 371, ("poseidon12", 0, (29, 11))), ("poseidon", 15 * 12 + 5, ("poseidon12", 0, (14, 5))),
    ("evpol4", 0, ("evpol4", 0, 0)), ("evpol4", 20, ("evpol4", 0, 2))])
def test_ref_names_the_broken_gate_output(kind, signal, expect):
    b, w = CIRC.with_custom(kind)
    circ = RC.circuit("GL", b)
    sig = circ["uses"][0][1]
    rep = RC.check(circ, CASES.corrupt(w, sig[signal]))
    (f,) = rep["findings"]
    k, use, pos = expect
    assert f["kind"] == k and f["use"] == use and rep["n_failing"][k] == 1
    assert ((f["row"], f["column"]) if k == "poseidon12" else f["position"]) == pos
    if signal in (11, 371, 20, 15 * 12 + 5):                                # a wrong output: the finding names that wire and its value
        assert f["wire"] == sig[signal] and int(f["value"]) == (w[sig[signal]] + 1) % REF.P and int(f["expected"]) == w[sig[signal]]


@pytest.mark.parametrize("use", [0, 1])
def test_ref_fft4_both_types_and_second_use_only(use):
    b, w = CIRC.with_custom("fft4")
    circ = RC.circuit("GL", b)
    sig = circ["uses"][use][1]
    (f,) = RC.check(circ, CASES.corrupt(w, sig[0]))["findings"]             # an input: every output of that use moves, the first is named
    assert (f["kind"], f["use"], f["position"]) == ("fft4", use, 0)
    (f,) = RC.check(circ, CASES.corrupt(w, sig[23]))["findings"]
    assert (f["kind"], f["use"], f["position"], f["wire"]) == ("fft4", use, 11, sig[23])


def test_sym_parser_and_lines():
    text = "1,1,0,main.out\n2,2,0,main.a\n3,-1,0,main.gone\n4,2,0,main.alias\n5,3,1,main.sub.b,with,commas\n\nnot a line\n"
    names = zkgpu_prove.read_sym(text)
    assert names == {1: "main.out", 2: "main.a", 3: "main.sub.b,with,commas"}
    f = {"kind": "constraint", "index": 7, "a": "2", "b": "3", "c": "5", "wires": {"a": [[2, "1"]], "b": [[3, "1"], [9, "4"]], "c": []}}
    line = zkgpu_prove.wtns_finding_line(f, names)
    assert line.startswith("constraint 7:") and "1*w2 (main.a)" in line and "4*w9" in line and "w9 (" not in line
    assert "w2 (" not in zkgpu_prove.wtns_finding_line(f)
    g = {"kind": "poseidon12", "use": 2, "row": 14, "column": 5, "wire": 3, "expected": "8", "value": "9"}
    assert "row 14 column 5" in zkgpu_prove.wtns_finding_line(g, names) and "main.sub.b" in zkgpu_prove.wtns_finding_line(g, names)
    assert "wire 0 holds 2" in zkgpu_prove.wtns_finding_line({"kind": "one_wire", "value": "2"})


def test_parser_accepts_the_new_flags():
    ap = zkgpu_prove.build_parser()
    a = ap.parse_args(["wtns_check", "-c", "GL", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--sym", "c.sym", "--report", "o.json", "--max-findings", "3"])
    assert (a.curve_type, a.circuit_file, a.wtns, a.sym, a.report, a.max_findings) == ("GL", "c.r1cs", "w.wtns", "c.sym", "o.json", 3) and a.fn is zkgpu_prove.wtns_check
    a = ap.parse_args(["groth16_prove", "--r1cs", "c.r1cs", "-w", "w.wtns", "--check-witness"])
    assert a.check_witness is True
    assert ap.parse_args(["groth16_prove", "--r1cs", "c.r1cs", "-w", "w.wtns"]).check_witness is False
    a = ap.parse_args(["compressor12_exec", "--wtns", "w.wtns", "--check-witness", "c.r1cs"])
    assert a.check_witness == "c.r1cs"
    assert ap.parse_args(["compressor12_exec", "--wtns", "w.wtns"]).check_witness is None


def test_header_declares_the_six_prototypes():
    h = (ROOT / "include" / "zkgpu.h").read_text()
    assert re.search(r"typedef\s+struct\s+zk_r1cs_check\s+zk_r1cs_check_t\s*;", h)
    for proto in (r"zk_r1cs_check_t\s*\*\s*zk_r1cs_check_new\s*\(\s*const char\s*\*\s*field\s*,\s*const void\s*\*\s*r1cs\s*,\s*size_t\s+len\s*\)",
                  r"int\s+zk_r1cs_check_info\s*\(\s*const zk_r1cs_check_t\s*\*[^)]*uint32_t\s*\*\s*n_wires[^)]*uint64_t\s*\*\s*n_constraints[^)]*uint64_t\s*\*\s*n_custom_uses[^)]*uint32_t\s*\*\s*n_public\s*\)",
                  r"char\s*\*\s*zk_r1cs_check_run\s*\(\s*zk_r1cs_check_t\s*\*[^)]*const void\s*\*\s*witness[^)]*uint64_t\s+n_values[^)]*uint32_t\s+max_findings\s*\)",
                  r"char\s*\*\s*zk_r1cs_check_run_dev\s*\(\s*zk_r1cs_check_t\s*\*[^)]*const void\s*\*\s*d_witness[^)]*uint64_t\s+n_values[^)]*uint32_t\s+max_findings\s*\)",
                  r"int\s+zk_r1cs_check_free\s*\(\s*zk_r1cs_check_t\s*\*"):
        assert re.search(proto, h), proto
