"""tools/zkgpu_prove.py groth16_key_check, groth16_prove --check-key and groth16_setup --check-key in fresh child processes: exit
codes, printed lines, the report file, and that a damaged key stops the prover before the witness is touched or a proof written."""
import json, pathlib, subprocess, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
import key_check_cases as KC  # noqa: E402
import key_check_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


def run(*args):
    return subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_setup_check_key_then_key_check_then_prove_check_key(orc, tmp_path):
    g = G.Groth16Oracle(orc, "bn254")
    r1cs, w = KC.circuit(g.r, 20)
    c, pk, bad_pk, vk, rep, wt, proof, pub = (tmp_path / n for n in ("c.r1cs", "g16.key", "bad.key", "vk.json", "rep.json", "w.wtns", "proof.json", "public_input.json"))
    c.write_bytes(g.r1cs_bytes(r1cs)); wt.write_bytes(g.wtns_bytes(w))
    a = run("groth16_setup", "-c", "BN128", "--r1cs", c, "-p", pk, "-v", vk, "--check-key")
    assert a.returncode == 0 and "the key passes groth16_key_check" in a.stdout, a.stderr
    b = run("groth16_key_check", "-c", "BN128", "--r1cs", c, "-p", pk, "-v", vk, "--report", rep)
    assert b.returncode == 0 and "is a well-formed key of" in b.stdout and "not checked against the circuit's polynomials" in b.stdout, b.stderr
    report = json.loads(rep.read_text())
    assert report["findings"] == [] and report["n_wires"] == r1cs["n_wires"]
    pb = pk.read_bytes()
    bad = KC.set_point("BN128", KC.off_curve("BN128", KC.off_curve("BN128", pb, "a", 3), "a", 5), "l", 2, None)
    bad_pk.write_bytes(bad)
    want = K.report("BN128", c.read_bytes(), bad, b_indices=[])
    d = run("groth16_key_check", "-c", "BN128", "--r1cs", c, "-p", bad_pk, "--report", rep)
    assert d.returncode == 1 and "well-formed" not in d.stdout, d.stderr
    assert d.stdout.strip().splitlines() == [K.finding_line(f) for f in want["findings"]]
    assert d.stdout.strip().splitlines() == ["infinity: section l: 1 point, first at index 2", "not_on_curve: section a: 2 points, first at index 3"]
    assert json.loads(rep.read_text())["findings"] == want["findings"]
    # a check that was skipped is said on the terminal too, after the findings and before the exit
    bad_pk.write_bytes(KC.set_point("BN128", pb, "b_g2", 1, KC.twist_point_outside_subgroup("BN128")))
    want = K.report("BN128", c.read_bytes(), bad_pk.read_bytes(), b_indices=[])
    s = run("groth16_key_check", "-c", "BN128", "--r1cs", c, "-p", bad_pk)
    assert s.returncode == 1 and want["skipped"], s.stderr
    assert s.stdout.strip().splitlines() == [K.finding_line(f) for f in want["findings"]] + [K.skipped_line(x) for x in want["skipped"]]
    assert s.stdout.strip().splitlines()[-1] == "skipped: g1_g2_mismatch of b: an invalid point"
    bad_pk.write_bytes(bad)
    e = run("groth16_key_check", "-c", "BLS12381", "--r1cs", c, "-p", pk)
    assert e.returncode == 1 and "prime is not the scalar field" in e.stderr
    f = run("groth16_prove", "-c", "BN128", "--r1cs", c, "-w", tmp_path / "absent.wtns", "-p", bad_pk, "--proof", proof, "--public-input", pub, "--check-key")
    assert f.returncode == 1 and "not_on_curve: section a" in f.stderr and not proof.exists() and not pub.exists()   # the witness file was never opened
    h = run("groth16_prove", "-c", "BN128", "--r1cs", c, "-w", wt, "-p", pk, "--proof", proof, "--public-input", pub, "--check-key", "--verify", vk)
    assert h.returncode == 0 and proof.exists(), h.stderr
