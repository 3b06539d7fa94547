"""The surface of the PLONK prover's R1CS import without a GPU: the header declares the entry points and the package binds
them; zk_plonk_<curve>_r1cs_new + _tables give the tables of the plain-integer model (tests/plonk_r1cs_ref.py) ARRAY FOR ARRAY on every
circuit of test_plonk_r1cs_ref.py, both fields, with no device present; every refusal of the host comes back with its text; the two new
forms of the command-line tool parse and their exclusive groups hold."""
import importlib, pathlib, re, struct, sys, types

import numpy as np
import pytest

import plonk_r1cs_ref as model
import r1cs_check_cases as cases
from plonk_r1cs_ref import FIELDS, circuits

ROOT = pathlib.Path(__file__).resolve().parent.parent
ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
ENTRY_POINTS = ["zk_plonk_r1cs_wave_min_terms"] + ["zk_plonk_%s_r1cs_%s" % (c, f) for c in ABI.values() for f in ("new", "info", "tables", "extend_dev", "free")]


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


def test_header_declares_and_package_binds_the_entry_points(zk, plonk):
    code = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "zkgpu.h").read_text(), flags=re.S)
    lib = zk.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in zk.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define\s+ZK_PLONK_R1CS_INFO_WORDS\s+%d\b" % len(plonk.R1CS_INFO), code)
    assert zk.R1csCircuit is plonk.R1csCircuit and zk.extend_witness is plonk.extend_witness and issubclass(plonk.R1csCircuit, plonk.Circuit)
    assert lib.zk_plonk_r1cs_wave_min_terms() >= 2


@pytest.mark.parametrize("field", FIELDS)
def test_the_librarys_tables_are_the_models_array_for_array(plonk, field):
    ints = lambda words: [plonk.int_of(w) for w in words]
    for name, data, w, _ in circuits(field):
        m = model.Compiled(data, field)
        t = m.tables()
        c = plonk.R1csCircuit(data, field)
        try:
            lens = [len(x) for _, x in m.segments]
            assert c.info == {"n_wires": m.n_wires, "n_public": m.n_public, "n_constraints": m.n_constraints, "n_gates": m.n_gates, "n_aux": m.n_aux,
                              "n_segments": len(lens), "max_segment_terms": max(lens or [0]), "n_segment_terms": sum(lens)}, name
            assert (c.n_vars, c.n_wires, c.n_aux, c.public, c.n_gates, c.n_public) == (m.n_vars, m.n_wires, m.n_aux, m.public, m.n_gates, m.n_public), name
            for k in model.SELECTORS:
                assert c.gates[k].shape == (m.n_gates, 4) and c.gates[k].dtype == np.uint64 and ints(c.gates[k]) == t[k], (name, k)
            for k in model.WIRES:
                assert c.gates[k].dtype == np.uint32 and c.gates[k].tolist() == t[k], (name, k)
            assert c.origin.dtype == np.uint32 and c.origin.tolist() == t["origin"], name
            s = c.segments
            assert s["seg_first"].tolist() == t["seg_first"] and s["seg_ptr"].tolist() == t["seg_ptr"] and s["seg_wire"].tolist() == t["seg_wire"], name
            assert ints(s["seg_coef"]) == t["seg_coef"], name
            # and it is the Circuit of that table: the public rows in front, padded to n = 2^k >= 8
            plain = plonk.Circuit(m.n_vars, m.public, m.gates, field)
            assert c.n == plain.n and all(np.array_equal(c.sel[k], plain.sel[k]) for k in model.SELECTORS) and all(np.array_equal(c.wire[k], plain.wire[k]) for k in "abc"), name
        finally:
            c.free()
        c.free()                                                                      # twice is harmless


def _header_with(data, n_wires):
    """the same file with another wire count in its header (section 1 comes first in what the test writer makes)"""
    at = 12 + 12 + 4 + 32
    assert data[12:16] == struct.pack("<I", 1)
    return data[:at] + struct.pack("<I", n_wires) + data[at + 4:]


@pytest.mark.parametrize("field", FIELDS)
def test_refusals_on_the_host(zk, plonk, field):
    p = model.R[field]
    other = "BLS12381" if field == "BN128" else "BN128"
    with pytest.raises(plonk.ZkError, match="prime is not the scalar field"):
        plonk.R1csCircuit(cases.one_constraint(other), field)
    with pytest.raises(plonk.ZkError, match="constraint 0: wire 4, the file has 4 wires"):
        plonk.R1csCircuit(cases.write(field, 4, [([(4, 1)], [(2, 1)], [(3, 1)])]), field)
    with pytest.raises(plonk.ZkError, match="constraint 1 is 0 = k with k not zero"):
        plonk.R1csCircuit(cases.write(field, 4, [([(1, 1)], [(2, 1)], [(3, 1)]), ([], [], [(0, 5)])]), field)
    with pytest.raises(plonk.ZkError, match="constraint 0 is 0 = k with k not zero"):
        plonk.R1csCircuit(cases.write(field, 4, [([(0, 1)], [(1, 2), (0, 3)], [(1, 2)])]), field)
    c = plonk.R1csCircuit(cases.write(field, 4, [([(0, 1)], [(1, 2), (0, 3)], [(1, 2), (0, 3)])]), field)      # 0 = 0 emits nothing
    assert c.n_gates == 0 and c.n == 8
    c.free()
    # a table whose variable ids would not fit 32 bits: 2^32 - 1 wires and one fold
    big = _header_with(cases.write(field, 8, [([(1, 1), (2, 1), (3, 1)], [(4, 1)], [(5, 1)])]), 0xFFFFFFFF)
    with pytest.raises(plonk.ZkError, match="a variable id has 32 bits"):
        plonk.R1csCircuit(big, field)
    with pytest.raises(model.Refused, match="32 bits"):
        model.Compiled(big, field)
    with pytest.raises(plonk.ZkError, match="Invalid magic number"):
        plonk.R1csCircuit(b"r1cx" + cases.one_constraint(field)[4:], field)
    with pytest.raises(plonk.ZkError, match='unknown curve "GL"'):
        plonk.R1csCircuit(cases.one_constraint(field), "GL")
    lib = zk.lib()
    assert not getattr(lib, "zk_plonk_%s_r1cs_new" % ABI[field])(None, 0) and "null input" in lib.zk_last_error().decode()
    info = np.zeros(8, np.uint64)
    assert getattr(lib, "zk_plonk_%s_r1cs_info" % ABI[field])(None, zk._ptr(info)) != 0 and "null handle" in lib.zk_last_error().decode()
    c = plonk.R1csCircuit(cases.one_constraint(field), field)
    try:
        assert getattr(lib, "zk_plonk_%s_r1cs_info" % ABI[other])(c._h, zk._ptr(info)) != 0 and "another field" in lib.zk_last_error().decode()
        assert getattr(lib, "zk_plonk_%s_r1cs_extend_dev" % ABI[field])(c._h, None, None) != 0 and "null argument" in lib.zk_last_error().decode()
        # the witness, before any device work: extend_witness and prove alike (the key's device arrays are never read)
        key = types.SimpleNamespace(curve=field, n=c.n, log_n=c.log_n, circuit=c, kzg=None)
        good = [1, 6, 2, 3]
        for call in (lambda w: plonk.extend_witness(c, w), lambda w: plonk.prove(key, w)):
            with pytest.raises(plonk.ZkError, match="the witness has 3 values, the .r1cs has 4 wires"):
                call(good[:3])
            with pytest.raises(plonk.ZkError, match="the witness has 5 values, the .r1cs has 4 wires"):
                call(cases.wtns_bytes(field, good + [0]))
            with pytest.raises(plonk.ZkError, match="witness value 2 is not below the scalar field's modulus"):
                call([1, 6, p, 3])
            with pytest.raises(plonk.ZkError, match="witness value 0 is 2: wire 0 of a circom witness is the constant 1"):
                call([2, 6, 2, 3])
            with pytest.raises(plonk.ZkError, match="the file is not a witness over %s" % field):
                call(cases.wtns_bytes(other, good))
        with pytest.raises(plonk.ZkError, match="extend_witness takes an R1csCircuit"):
            plonk.extend_witness(plonk.Circuit(c.n_vars, c.public, c.gates, field), good)
    finally:
        c.free()


def test_cli_parses_the_two_new_forms():
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_plonk")
    ap = cli.build_parser()
    a = ap.parse_args(["plonk_setup", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "-v", "vk.json"])
    assert (a.cmd, a.r1cs, a.circuit, a.vk) == ("plonk_setup", "c.r1cs", None, "vk.json")
    a = ap.parse_args(["plonk_setup", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])
    assert (a.r1cs, a.circuit) == (None, "c.npz")
    a = ap.parse_args(["plonk_prove", "-c", "BN128", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--proof", "proof.json", "--public", "public.json"])
    assert (a.cmd, a.r1cs, a.wtns, a.circuit, a.witness, a.proof, a.public) == ("plonk_prove", "c.r1cs", "w.wtns", None, None, "proof.json", "public.json")
    tail = ["--proof", "p.json", "--public", "x.json"]
    for bad in (["plonk_setup", "--ptau", "f", "-v", "vk.json"],                                                   # none given
                ["plonk_setup", "--ptau", "f", "-v", "vk.json", "--circuit", "c.npz", "--r1cs", "c.r1cs"],         # both given
                ["plonk_prove", "--ptau", "f", "--wtns", "w.wtns"] + tail,
                ["plonk_prove", "--ptau", "f", "--r1cs", "c.r1cs"] + tail,
                ["plonk_prove", "--ptau", "f", "--r1cs", "c.r1cs", "--circuit", "c.npz", "--wtns", "w.wtns"] + tail,
                ["plonk_prove", "--ptau", "f", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--witness", "w.bin"] + tail):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    for mixed in (["plonk_prove", "--ptau", "f", "--r1cs", "c.r1cs", "--witness", "w.bin"] + tail, ["plonk_prove", "--ptau", "f", "--circuit", "c.npz", "--wtns", "w.wtns"] + tail):
        with pytest.raises(SystemExit):
            cli.main(mixed)                                                           # --circuit goes with --witness, --r1cs with --wtns: refused before a file is opened
    assert [cli.smallest_power(n) for n in (30, 31, 32, 54, 6150)] == [4, 4, 5, 5, 12]
    text = (ROOT / "README.md").read_text()
    assert "plonk_setup --ptau pot.ptau --r1cs c.r1cs" in text and "plonk_prove --ptau pot.ptau --r1cs c.r1cs --wtns w.wtns" in text
