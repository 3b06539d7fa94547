"""pil_verify without a GPU: the reference checker (tests/pil_check_ref.py) on the inputs the GPU tests corrupt, the check programs
zk_pil_check_new generates and assembles (one `check1` per polynomial identity), its error messages, the command line."""
import copy
import json
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
D = ROOT / "tests" / "golden" / "starky_data"
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))

import pil_check_ref as REF

FIXTURES = {"fib": ("fib.pil.json", "fib.const", "fib.cm"), "fib.gl": ("fib.pil.json.gl", "fib.const.gl", "fib.cm.gl"),
            "plookup": ("plookup.pil.json", "plookup.const", "plookup.cm"), "pe": ("pe.pil.json", "pe.const", "pe.cm"),
            "connection": ("connection.pil.json", "connection.const", "connection.cm")}
INPUTS = list(FIXTURES) + ["poseidong"]


def load_input(name):
    """-> (pil dict, constants, trace) of a fixture, or of tools/poseidong.py at nbits = 10"""
    if name == "poseidong":
        import poseidong as PG
        return PG.pil(10), np.asarray(PG.consts(10), dtype=np.uint64).reshape(-1), np.asarray(PG.trace(10, None, PG.FIRST_ZERO, seed=10), dtype=np.uint64).reshape(-1)
    p, c, m = FIXTURES[name]
    return json.load(open(D / p)), np.fromfile(D / c, dtype="<u8"), np.fromfile(D / m, dtype="<u8")


@pytest.fixture(scope="module")
def zk():
    import eigen_zkvm_amd
    return eigen_zkvm_amd


def _stark(zk):
    import importlib
    return importlib.import_module("eigen_zkvm_amd.stark")


@pytest.mark.parametrize("name", INPUTS)
def test_reference_checker_finds_nothing_on_the_clean_inputs(name):
    pil, const, cm = load_input(name)
    rep = REF.check(pil, const, cm)
    assert rep["findings"] == []
    assert rep["n"] == 1024
    assert rep["checked"]["polIdentities"] == len(pil["polIdentities"])


def test_reference_checker_sees_a_flipped_cell():
    pil, const, cm = load_input("fib")
    bad = cm.copy(); bad[2 * 77] ^= 1
    f = REF.check(pil, const, bad)["findings"]
    assert f and all(x["kind"] == "identity" and x["fileName"] == "fibonacci.pil" for x in f)
    assert min(int(x["first_row"]) for x in f) == 76                         # row 76 reads row 77 through `next`


@pytest.mark.parametrize("name", INPUTS)
def test_check_programs_assemble_without_a_gpu(zk, name):
    pil, _, _ = load_input(name)
    chk = zk.PilCheck(pil)
    listing = chk.listing()
    lines = [l.split() for l in listing.splitlines() if l and not l.startswith(";")]
    n_check = sum(1 for l in lines if l[1] == "check1")
    assert n_check == len(pil["polIdentities"])
    assert sorted(l[2] for l in lines if l[1] == "check1") == sorted("id%d" % k for k in range(n_check))
    if name == "fib":
        assert n_check == 5
    if name in ("plookup", "pe", "connection"):
        assert n_check == 0 and "check1" not in listing
    assert chk.n == 1024
    chk.free()


def test_package_exports_pilcheck(zk):
    assert zk.PilCheck is _stark(zk).PilCheck
    for sym in ("zk_pil_check_new", "zk_pil_check_listing", "zk_pil_check_run", "zk_pil_check_run_dev", "zk_pil_check_free"):
        assert sym in zk.EXPORTS and hasattr(zk.lib(), sym)


def test_public_assembler_does_not_know_check1(zk):
    """the instruction is internal to the checker: zk_program_assemble and zk_program_compile reject its opcode as any unknown op"""
    code = [zk.instr(zk.OP_COPY, zk.opnd(zk.OPND_TMP, 0), zk.opnd(zk.OPND_NUMBER, value=1)),
            zk.instr(64, zk.opnd(zk.OPND_MEM, 0, stride=1), zk.opnd(zk.OPND_TMP, 0), zk.opnd(zk.OPND_TMP, 0))]
    for mode in ("bytecode", "jit"):
        with pytest.raises(zk.ZkError):
            zk.Program(code, mode=mode)


def _error(zk, pil):
    with pytest.raises(zk.ZkError) as e:
        zk.PilCheck(pil)
    return str(e.value)


def test_errors_have_their_messages(zk):
    pil, const, cm = load_input("fib")
    chk = zk.PilCheck(pil)
    with pytest.raises(zk.ZkError, match="the trace has 512 rows, the PIL's polDeg is 1024"):
        chk.run(const[:512 * pil["nConstants"]], cm[:512 * pil["nCommitments"]], n_rows=512)
    chk.free()

    bad = copy.deepcopy(pil); bad["polIdentities"][2]["e"] = len(pil["expressions"])
    assert "expression id out of range" in _error(zk, bad)
    bad = copy.deepcopy(pil); bad["expressions"][1] = {"op": "exp", "deg": 1, "id": 99}
    assert "expression id out of range" in _error(zk, bad)

    for name, key in (("plookup", "plookupIdentities"), ("pe", "permutationIdentities")):
        p2, _, _ = load_input(name)
        bad = copy.deepcopy(p2); bad[key][0]["f"] = bad[key][0]["f"][:-1]
        assert "%s[0]: f and t differ in length" % key in _error(zk, bad)
    p2, _, _ = load_input("connection")
    bad = copy.deepcopy(p2); bad["connectionIdentities"][0]["pols"].pop()
    assert "connectionIdentities[0]: pols and connections differ in length" in _error(zk, bad)

    bad = copy.deepcopy(pil)
    for r in bad["references"].values():
        r["polDeg"] = 1000
    assert "polDeg 1000 is not a power of two" in _error(zk, bad)
    bad = copy.deepcopy(pil); next(iter(bad["references"].values()))["polDeg"] = 2048
    assert "differ in polDeg" in _error(zk, bad)


def test_cli_parser():
    import zkgpu_prove as Z
    ap = Z.build_parser()
    a = ap.parse_args(["pil_verify", "-p", "c.pil.json", "--o", "c.const", "--m", "c.cm", "--report", "out.json"])
    assert (a.piljson, a.const_pols, a.cm_pols, a.report, a.fn) == ("c.pil.json", "c.const", "c.cm", "out.json", Z.pil_verify)
    assert ap.parse_args(["pil_verify", "-p", "c.pil.json", "--o", "c.const", "--m", "c.cm"]).report is None
    argv = ["stark_prove", "-s", "ss.json", "-p", "c.pil.json", "--o", "c.const", "--m", "c.cm", "--i", "zkin.json"]
    plain, checked = vars(ap.parse_args(argv)), vars(ap.parse_args(argv + ["--check-trace"]))
    assert plain.pop("check_trace") is False and checked.pop("check_trace") is True
    assert plain == checked
    assert plain == {"cmd": "stark_prove", "stark_struct": "ss.json", "piljson": "c.pil.json", "norm_stage": False, "skip_main": False, "agg_stage": False,
                     "const_pols": "c.const", "cm_pols": "c.cm", "circom_file": None, "zkin": "zkin.json",
                     "prover_addr": "273030697313060285579891744179749754319274977764", "program": None, "no_verify": False, "eval": "jit",
                     "fn": Z.stark_prove}


def test_finding_lines():
    import zkgpu_prove as Z
    pil, const, cm = load_input("fib")
    bad = cm.copy(); bad[2 * 77] ^= 1
    for f in REF.check(pil, const, bad)["findings"]:
        assert Z.finding_line(f).startswith("fibonacci.pil:%d: identity %d: " % (f["line"], f["index"]))
