"""tools/zkgpu_plonk.py from a circom circuit, through its files: plonk_setup --r1cs, plonk_prove --r1cs --wtns and plonk_verify on the
reference project's multiplier.r1cs with the witness of tests/golden/groth16/witness.wtns ([1, 11210000, 1121, 10000], n = 8).  Exit codes:
0 on the good path, 1 for a witness that breaks the constraint, which is named.  The vk.json is the one plonk_setup --circuit writes for the
saved gate table of the same circuit.  The tool is the subject, so it runs as a process."""
import importlib, json, pathlib, subprocess, sys

import pytest

import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_plonk.py")]
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args):
    p = subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def test_setup_prove_verify_from_the_r1cs_and_the_wtns(zk, tmp_path):
    cv = "BN128"
    plonk = importlib.import_module("eigen_zkvm_amd.plonk")
    r1cs, wtns = GOLDEN / "plonk" / "multiplier.r1cs", GOLDEN / "groth16" / "witness.wtns"
    ptau = tmp_path / "f.ptau"
    ptau.write_bytes(make_test_ptau.build_ptau(zk, cv, 4, 0x1234567, 5, 7))                       # 31 powers: 3n + 6 = 30 for n = 8
    rc, out = _run("plonk_setup", "--ptau", ptau, "--r1cs", r1cs, "-v", tmp_path / "vk.json")
    assert rc == 0 and "1 constraints -> 1 gates, 0 auxiliaries; n = 2^3 rows need 3n + 6 = 30 powers (a file of power 4 has them)" in out, out
    assert "1 gates and 1 public input(s) in n = 2^3 rows" in out, out
    # the same key from the saved gate table of the same circuit
    c = plonk.R1csCircuit(r1cs.read_bytes(), cv)
    c.save(tmp_path / "c.npz")
    c.free()
    rc, out = _run("plonk_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk_table.json", "--no-check-srs")
    assert rc == 0, out
    assert (tmp_path / "vk.json").read_text() == (tmp_path / "vk_table.json").read_text()
    rc, out = _run("plonk_prove", "--ptau", ptau, "--r1cs", r1cs, "--wtns", wtns, "--proof", tmp_path / "proof.json", "--public", tmp_path / "public.json", "--no-check-srs")
    assert rc == 0 and "plonk_prove:" in out, out
    assert json.loads((tmp_path / "public.json").read_text()) == ["11210000"]
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("plonk_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, "--no-check-srs")
    assert rc == 0 and "1 proof(s) accepted" in out, out
    (tmp_path / "bad.wtns").write_bytes(cases.wtns_bytes(cv, [1, 11210001, 1121, 10000]))         # the output wire + 1
    rc, out = _run("plonk_prove", "--ptau", ptau, "--r1cs", r1cs, "--wtns", tmp_path / "bad.wtns", "--proof", tmp_path / "p2.json", "--public", tmp_path / "x2.json",
                   "--no-check-srs")
    assert rc == 1 and "witness does not satisfy gate 0 (constraint 0 of the .r1cs)" in out and not (tmp_path / "p2.json").exists(), out
    rc, out = _run("plonk_prove", "--ptau", ptau, "--r1cs", r1cs, "--witness", wtns, "--proof", tmp_path / "p3.json", "--public", tmp_path / "x3.json")
    assert rc == 2 and "--circuit goes with --witness, --r1cs with --wtns" in out, out             # refused by the parser, before a file is opened
