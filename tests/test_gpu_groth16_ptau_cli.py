"""tools/zkgpu_prove.py groth16_setup --ptau, groth16_contribute and groth16_contribution_check as child processes, end to end on the
n_mul = 40 circuit: exit codes and the flags that exclude each other.  That circuit has a wire no row mentions, whose `l` point is
infinity -- the one finding groth16_key_check has for any key of it (bellman's reader refuses the point) -- so the `--check-key` pass on a
contributed key is shown on the reference's own circuit, where every wire is used."""
import pathlib, random, struct, subprocess, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


def _run(*args):
    return subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def test_no_check_srs_without_a_file_is_refused():
    out = _run("groth16_setup", "--r1cs", "nothing.r1cs", "--no-check-srs")
    assert out.returncode != 0 and "--no-check-srs" in out.stderr and "--ptau" in out.stderr


def test_help_shows_the_new_commands_and_flags():
    out = _run("groth16_setup", "--help")
    assert out.returncode == 0 and "--ptau" in out.stdout and "--no-check-srs" in out.stdout
    assert _run("groth16_contribute", "--help").returncode == 0 and _run("groth16_contribution_check", "--help").returncode == 0
    assert _run("groth16_contribute", "-c", "BN128", "-p", "in.key").returncode == 2       # -o is required


@pytest.mark.gpu
def test_setup_from_file_contribute_check_end_to_end(zk, orc, tmp_path):
    sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
    import groth16 as G
    import make_test_ptau as MP
    zk.init(0)
    g = G.Groth16Oracle(orc, "bn254"); rng = random.Random(40)
    r1cs, _ = G.synthetic_r1cs(g.r, 40, seed=5)
    rf = tmp_path / "c.r1cs"; rf.write_bytes(g.r1cs_bytes(r1cs))
    td = [rng.randrange(1, g.r) for _ in range(3)]
    b = MP.build_ptau(zk, "BN128", g.circuit(r1cs)["log_m"], *td)
    pt = tmp_path / "c.ptau"; pt.write_bytes(b)
    k0, k1, k2, vk0, vk1 = (tmp_path / n for n in ("k0.key", "k1.key", "k2.key", "vk0.json", "vk1.json"))
    a = _run("groth16_setup", "-c", "BN128", "--r1cs", rf, "-p", k0, "-v", vk0, "--ptau", pt)
    assert a.returncode == 0, a.stderr
    assert "well-formed powers-of-tau file" in a.stdout and "delta = 1" in a.stdout
    assert k0.read_bytes() == g.params_bytes(g.setup(r1cs, *td, 1, 1))
    # a damaged file: findings on stderr, exit 1, no key -- unless the check is switched off
    o, sid = 12, 0
    while sid != 4:                                                        # the payload of section 4
        sid, sz = struct.unpack_from("<IQ", b, o)
        o += 12 + (sz if sid != 4 else 0)
    bad = bytearray(b)
    bad[o + 64:o + 128] = b[o + 128:o + 192]                               # alphaTauG1[1] := alphaTauG1[2]
    pb = tmp_path / "bad.ptau"; pb.write_bytes(bytes(bad))
    kb = tmp_path / "kb.key"
    c = _run("groth16_setup", "-c", "BN128", "--r1cs", rf, "-p", kb, "-v", tmp_path / "vkb.json", "--ptau", pb)
    assert c.returncode == 1 and "not_powers: section alphaTauG1" in c.stderr and not kb.exists()
    c = _run("groth16_setup", "-c", "BN128", "--r1cs", rf, "-p", kb, "-v", tmp_path / "vkb.json", "--ptau", pb, "--no-check-srs")
    assert c.returncode == 0 and kb.exists() and kb.read_bytes() != k0.read_bytes()
    # contributions
    d = _run("groth16_contribute", "-c", "BN128", "-p", k0, "-o", k1, "-v", vk1, "--check")
    assert d.returncode == 0, d.stderr
    assert k1.read_bytes() != k0.read_bytes() and len(k1.read_bytes()) == len(k0.read_bytes())
    e = _run("groth16_key_check", "-c", "BN128", "--r1cs", rf, "-p", k1, "-v", vk1)    # the unused wire, and nothing else: vk1 is k1's
    assert e.returncode == 1 and e.stdout.strip().splitlines() == ["infinity: section l: 1 point, first at index %d" % (r1cs["n_wires"] - 4)], e.stdout + e.stderr
    assert _run("groth16_contribute", "-c", "BN128", "-p", k1, "-o", k2).returncode == 0
    f = _run("groth16_contribution_check", "-c", "BN128", "--old", k0, "--new", k2)
    assert f.returncode == 0 and "nothing else changed" in f.stdout, f.stdout + f.stderr
    # a key that is not a contribution of the other: exit 1 with the finding
    f = _run("groth16_contribution_check", "-c", "BN128", "--old", k0, "--new", kb)
    assert f.returncode == 1 and "changed: section" in f.stdout
    f = _run("groth16_contribution_check", "-c", "BN128", "--old", k0, "--new", tmp_path / "missing.key")
    assert f.returncode == 1 and "zkgpu_prove:" in f.stderr


@pytest.mark.gpu
def test_check_key_passes_on_a_contributed_key_of_the_reference_circuit(zk, orc, tmp_path):
    sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
    import groth16 as G
    import make_test_ptau as MP
    zk.init(0)
    g = G.Groth16Oracle(orc, "bls12_381"); rng = random.Random(41)
    rf = ROOT / "tests" / "golden" / "groth16" / "mycircuit_bls12381.r1cs"
    log_m = g.circuit(G.read_r1cs(rf.read_bytes())[1])["log_m"]
    pt = tmp_path / "c.ptau"; pt.write_bytes(MP.build_ptau(zk, "BLS12381", log_m + 1, *[rng.randrange(1, g.r) for _ in range(3)]))
    wtns = tmp_path / "witness.wtns"; wtns.write_bytes(g.wtns_bytes([1, 33, 3, 11]))
    k0, k1, vk0, vk1 = (tmp_path / n for n in ("k0.key", "k1.key", "vk0.json", "vk1.json"))
    a = _run("groth16_setup", "-c", "BLS12381", "--r1cs", rf, "-p", k0, "-v", vk0, "--ptau", pt, "--check-key")
    assert a.returncode == 0 and "passes groth16_key_check" in a.stdout, a.stdout + a.stderr
    assert _run("groth16_contribute", "-c", "BLS12381", "-p", k0, "-o", k1, "-v", vk1, "--check").returncode == 0
    e = _run("groth16_key_check", "-c", "BLS12381", "--r1cs", rf, "-p", k1, "-v", vk1)
    assert e.returncode == 0 and "well-formed key" in e.stdout, e.stdout + e.stderr
    e = _run("groth16_key_check", "-c", "BLS12381", "--r1cs", rf, "-p", k1, "-v", vk0)        # the old verification key no longer fits
    assert e.returncode == 1 and "vk_mismatch: vk_delta_2" in e.stdout
    b = _run("groth16_prove", "-c", "BLS12381", "--r1cs", rf, "-w", wtns, "-p", k1, "--public-input", tmp_path / "pub.json", "--proof", tmp_path / "proof.json",
             "--check-key", "--verify", vk1)
    assert b.returncode == 0, b.stdout + b.stderr
