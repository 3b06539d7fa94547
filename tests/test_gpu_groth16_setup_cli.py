"""tools/zkgpu_prove.py groth16_setup, then groth16_prove on its output, as two child processes (`zkit groth16_setup` /
`groth16_prove`, zkit/src/main.rs:185-217): the proof the second writes verifies against the key the first wrote."""
import json, pathlib, re, subprocess, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


def test_groth16_setup_help_shows_zkits_flags():
    out = subprocess.run(CLI + ["groth16_setup", "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    # the option lines of argparse's help: indented, the flag first, then a metavar, a comma (an alias) or the end of the line
    shown = set(re.findall(r"^\s+(--?[A-Za-z][\w-]*)(?=[ ,]|$)", out.stdout, flags=re.M))
    assert {"-c", "--r1cs", "-p", "-v", "-t"} <= shown, shown


@pytest.mark.gpu
@pytest.mark.parametrize("hexed", [False, True])
def test_groth16_setup_then_prove_round_trip(orc, tmp_path, hexed):
    sys.path.insert(0, str(ROOT / "oracle"))
    import groth16 as G
    import pairing as PG
    g = G.Groth16Oracle(orc, "bls12_381")
    r1cs = ROOT / "tests" / "golden" / "groth16" / "mycircuit_bls12381.r1cs"
    wtns = tmp_path / "witness.wtns"; wtns.write_bytes(g.wtns_bytes([1, 33, 3, 11]))
    pk, vk, proof, pub = (tmp_path / n for n in ("g16.key", "verification_key.json", "proof.json", "public_input.json"))
    a = subprocess.run(CLI + ["groth16_setup", "-c", "BLS12381", "--r1cs", str(r1cs), "-p", str(pk), "-v", str(vk)] + (["-t"] if hexed else []),
                       capture_output=True, text=True, timeout=600)
    assert a.returncode == 0, a.stderr
    b = subprocess.run(CLI + ["groth16_prove", "-c", "BLS12381", "--r1cs", str(r1cs), "-w", str(wtns), "-p", str(pk), "--public-input", str(pub), "--proof", str(proof)],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr
    v = json.loads(vk.read_text()); js = json.loads(proof.read_text())
    assert v["vk_alpha_1"]["x"].startswith("0x") == hexed
    i = lambda s: int(s, 0)
    g1 = lambda p: (i(p["x"]), i(p["y"]))
    g2 = lambda p: (i(p["x"][0]), i(p["x"][1]), i(p["y"][0]), i(p["y"][1]))
    vki = dict(alpha_g1=g1(v["vk_alpha_1"]), beta_g2=g2(v["vk_beta_2"]), gamma_g2=g2(v["vk_gamma_2"]), delta_g2=g2(v["vk_delta_2"]), ic=[g1(p) for p in v["IC"]])
    pr = dict(a=g1(js["pi_a"]), b=g2(js["pi_b"]), c=g1(js["pi_c"]))
    public = [int(x) for x in json.loads(pub.read_text())]
    assert public == [33]
    assert PG.BLS12_381.groth16_verify(vki, pr, public)
    assert not PG.BLS12_381.groth16_verify(vki, pr, [34])
