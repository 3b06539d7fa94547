"""tools/zkgpu_prove.py groth16_setup -> groth16_prove -> groth16_verify in fresh child processes, both curves
(`zkit groth16_verify`, zkit/src/main.rs:221-230)."""
import json, pathlib, subprocess, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


def run(*args):
    return subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("cv,tag", [("bn254", "BN128"), ("bls12_381", "BLS12381")])
def test_setup_prove_verify_round_trip(orc, tmp_path, cv, tag):
    g = G.Groth16Oracle(orc, cv)
    r1cs_d, wit = G.synthetic_r1cs(g.r, 6, seed=4)
    r1cs, wtns, pk, vk, pub, proof, proof2 = (tmp_path / n for n in ("c.r1cs", "w.wtns", "g16.key", "vk.json", "public_input.json", "proof.json", "proof2.json"))
    r1cs.write_bytes(g.r1cs_bytes(r1cs_d)); wtns.write_bytes(g.wtns_bytes(wit))
    a = run("groth16_setup", "-c", tag, "--r1cs", r1cs, "-p", pk, "-v", vk)
    assert a.returncode == 0, a.stderr
    b = run("groth16_prove", "-c", tag, "--r1cs", r1cs, "-w", wtns, "-p", pk, "--public-input", pub, "--proof", proof)
    assert b.returncode == 0, b.stderr
    c = run("groth16_verify", "-c", tag, "-v", vk, "--public-input", pub, "--proof", proof)
    assert c.returncode == 0 and "accepted" in c.stdout, c.stderr
    # the command line draws r and s itself: a proof written under --verify is a different, equally valid one
    d = run("groth16_prove", "-c", tag, "--r1cs", r1cs, "-w", wtns, "-p", pk, "--public-input", pub, "--proof", proof2, "--verify", vk)
    assert d.returncode == 0, d.stderr
    assert run("groth16_verify", "-c", tag, "-v", vk, "--public-input", pub, "--proof", proof2).returncode == 0
    vals = json.loads(pub.read_text())
    vals[0] = str((int(vals[0]) + 1) % g.r)
    bad = tmp_path / "tampered.json"; bad.write_text(json.dumps(vals))
    e = run("groth16_verify", "-c", tag, "-v", vk, "--public-input", bad, "--proof", proof)
    assert e.returncode != 0 and "verify failed" in (e.stderr + e.stdout) and "equation" in (e.stderr + e.stdout)


def test_groth16_verify_help_shows_zkits_flags():
    out = subprocess.run(CLI + ["groth16_verify", "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("-c", "-v", "--public-input", "--proof"):
        assert flag in out.stdout
