"""tools/zkgpu_prove.py wtns_check, groth16_prove --check-witness and compressor12_exec --check-witness in fresh child processes:
exit codes, printed lines, the report file, and that a bad witness stops the command before anything else is read or written."""
import importlib
import json
import pathlib
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import c12_setup_circuits as CIRC  # noqa: E402
import c12_setup_ref as REF  # noqa: E402
import groth16 as G  # noqa: E402
import r1cs_check_cases as CASES  # noqa: E402
import r1cs_check_ref as RC  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


def run(*args):
    return subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_wtns_check_lines_report_and_exit_codes(tmp_path):
    b, w = CIRC.with_custom("poseidon")
    circ = RC.circuit("GL", b)
    sig = circ["uses"][0][1]
    bad = CASES.corrupt(CASES.corrupt(w, sig[15 * 12 + 5]), len(circ["constraints"]) + 6)     # a Poseidon12 state and the output of the last sum
    expected = RC.check(circ, bad)
    assert [f["kind"] for f in expected["findings"]][-1] == "poseidon12" and expected["n_failing"]["constraint"] >= 1
    r1cs, good_w, bad_w, sym, rep = (tmp_path / n for n in ("c.r1cs", "good.wtns", "bad.wtns", "c.sym", "rep.json"))
    r1cs.write_bytes(b); good_w.write_bytes(CASES.wtns_bytes("GL", w)); bad_w.write_bytes(CASES.wtns_bytes("GL", bad))
    sym.write_text("".join("%d,%d,0,main.s%d\n" % (i, i, i) for i in range(1, len(w))) + "9999,-1,0,main.gone\n%d,%d,0,main.second_name\n" % (len(w), sig[15 * 12 + 5]))
    a = run("wtns_check", "-c", "GL", "--r1cs", r1cs, "--wtns", good_w, "--report", rep)
    assert a.returncode == 0, a.stderr
    assert "zkgpu_prove: %s satisfies %s (%d constraints, 1 custom-gate uses)" % (good_w, r1cs, len(circ["constraints"])) in a.stdout
    assert json.loads(rep.read_text()) == RC.check(circ, w)
    c = run("wtns_check", "-c", "GL", "--r1cs", r1cs, "--wtns", bad_w, "--report", rep)
    assert c.returncode == 1 and "satisfies" not in c.stdout, c.stderr
    assert json.loads(rep.read_text()) == expected
    lines = c.stdout.strip().splitlines()
    assert len(lines) == len(expected["findings"]) and lines[-1].startswith("poseidon12 use 0: row 14 column 5, w%d holds" % sig[15 * 12 + 5])
    assert lines[0].startswith("constraint %d:" % expected["findings"][0]["index"]) and "(main." not in c.stdout
    d = run("wtns_check", "-c", "GL", "--r1cs", r1cs, "--wtns", bad_w, "--sym", sym, "--max-findings", "1")
    assert d.returncode == 1
    lines = d.stdout.strip().splitlines()
    assert len(lines) == 2 and "w%d (main.s%d) holds" % (sig[15 * 12 + 5], sig[15 * 12 + 5]) in lines[-1] and "(main.s" in lines[0] and "second_name" not in d.stdout


def test_groth16_prove_check_witness(zk, tmp_path):
    assert zk.lib().zk_device_count() >= 1
    zk.init(0)
    p = RC.PRIMES["BN128"]
    r, w = G.synthetic_r1cs(p, 6, seed=4)
    b = REF.write_r1cs(r["n_wires"], r["n_pub_out"], r["n_pub_in"], r["n_prv_in"], r["constraints"], field_size=32, prime=p)
    r1cs, wt, bad_wt, pk, vk, pub, proof, proof2 = (tmp_path / n for n in ("c.r1cs", "w.wtns", "bad.wtns", "g16.key", "vk.json", "public_input.json", "proof.json", "proof2.json"))
    bad = CASES.corrupt(w, len(w) - 2, p=p)                                 # the output of the last product
    expected = RC.check(RC.circuit("BN128", b), bad)
    assert expected["n_failing"]["constraint"] == 1
    r1cs.write_bytes(b); wt.write_bytes(CASES.wtns_bytes("BN128", w)); bad_wt.write_bytes(CASES.wtns_bytes("BN128", bad))
    # a bad witness: findings, exit 1, no proof -- and the key file does not exist, so it was never opened
    a = run("groth16_prove", "-c", "BN128", "--r1cs", r1cs, "-w", bad_wt, "-p", tmp_path / "no_such.key", "--public-input", pub, "--proof", proof, "--check-witness")
    assert a.returncode == 1 and "constraint %d:" % expected["findings"][0]["index"] in a.stderr, (a.stdout, a.stderr)
    assert not proof.exists() and not pub.exists() and "no_such.key" not in a.stderr
    # a good witness: the flag changes nothing.  The command line draws r and s itself, so the two proofs differ; both must verify
    assert run("groth16_setup", "-c", "BN128", "--r1cs", r1cs, "-p", pk, "-v", vk).returncode == 0
    args = ["groth16_prove", "-c", "BN128", "--r1cs", r1cs, "-w", wt, "-p", pk, "--public-input", pub]
    c = run(*args, "--proof", proof, "--check-witness")
    assert c.returncode == 0, c.stderr
    pub_with = pub.read_text()
    d = run(*args, "--proof", proof2)
    assert d.returncode == 0, d.stderr
    assert pub.read_text() == pub_with
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    key = dev.Groth16VerifyingKey("BN128", vk.read_text())
    assert key.verify(proof.read_text(), pub_with) == dev.ACCEPTED and key.verify(proof2.read_text(), pub_with) == dev.ACCEPTED
    key.free()


def test_compressor12_exec_check_witness(tmp_path):
    b, w = CIRC.with_cmuladd()
    circ = RC.circuit("GL", b)
    bad = CASES.corrupt(w, circ["uses"][0][1][11])
    f = lambda n: str(tmp_path / n)
    (tmp_path / "c.r1cs").write_bytes(b); (tmp_path / "w.wtns").write_bytes(CASES.wtns_bytes("GL", w)); (tmp_path / "bad.wtns").write_bytes(CASES.wtns_bytes("GL", bad))
    files = ["--p", f("c.pil"), "--e", f("c.exec")]
    assert run("compressor12_setup", "--r", f("c.r1cs"), "--c", f("c.const"), "--force_n_bits", "8", *files).returncode == 0
    a = run("compressor12_exec", "--wtns", f("bad.wtns"), "--m", f("c.cm"), "--check-witness", f("c.r1cs"), *files)
    assert a.returncode == 1 and "cmuladd use 0: output 2" in a.stderr and not (tmp_path / "c.cm").exists(), (a.stdout, a.stderr)
    c = run("compressor12_exec", "--wtns", f("w.wtns"), "--m", f("c.cm"), "--check-witness", f("c.r1cs"), *files)
    assert c.returncode == 0 and (tmp_path / "c.cm").stat().st_size == (1 << 8) * 12 * 8, c.stderr
