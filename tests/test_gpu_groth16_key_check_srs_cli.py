"""tools/zkgpu_prove.py groth16_key_check --ptau in fresh child processes: exit codes, the printed lines, the three reports under --report,
and that without --ptau the command says and returns what it did before the option existed."""
import importlib, json, pathlib, random, subprocess, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
import make_test_ptau as MP  # noqa: E402
import key_check_cases as KC  # noqa: E402
import key_check_srs_ref as KS  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


def run(*args):
    return subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_key_check_with_and_without_ptau(zk, orc, tmp_path):
    zk.init(0)
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    g = G.Groth16Oracle(orc, "bn254"); rng = random.Random(3)
    r1cs, _ = KC.circuit(g.r, 20)                                           # no wire without a row: the key's own check has nothing to say
    rb = g.r1cs_bytes(r1cs)
    c, pot, pk, bad_pk, rep = (tmp_path / n for n in ("c.r1cs", "pot.ptau", "g16.key", "bad.key", "rep.json"))
    c.write_bytes(rb)
    pot.write_bytes(MP.build_ptau(zk, "BN128", g.circuit(r1cs)["log_m"], *(rng.randrange(1, g.r) for _ in range(3))))
    srs = dev.Srs("BN128", pot)
    pb, _ = dev.keygen("BN128", rb, srs=srs)
    srs.free()
    pb = dev.contribute("BN128", pb, rng.randrange(2, g.r))
    k = KS.layout(g, pb)["b_g1"][0] // 2
    bad = KC.doubled("BN128", KC.doubled("BN128", pb, "b_g1", k), "b_g2", k)
    pk.write_bytes(pb); bad_pk.write_bytes(bad)
    wire = KS.wires(g, r1cs)["b_g1"][k]

    a = run("groth16_key_check", "-c", "BN128", "--r1cs", c, "-p", pk, "--ptau", pot, "--report", rep)
    assert a.returncode == 0 and "is a key of %s over %s (" % (c, pot) in a.stdout and "mismatch" not in a.stdout, (a.stdout, a.stderr)
    reports = json.loads(rep.read_text())
    assert sorted(reports) == ["key_check", "key_check_srs", "srs_check"]
    assert all(r["findings"] == [] and not any(r["counts"].values()) for r in reports.values())
    assert reports["key_check"]["n_wires"] == r1cs["n_wires"] and reports["srs_check"]["power"] == reports["key_check_srs"]["power"]

    b = run("groth16_key_check", "-c", "BN128", "--r1cs", c, "-p", bad_pk, "--ptau", pot, "--no-check-srs", "--report", rep)
    assert b.returncode == 1, (b.stdout, b.stderr)
    assert b.stdout.strip().splitlines() == [dev.key_check_srs_line(dict(kind="query_mismatch", section=s, first_index=k, wire=wire)) for s in ("b_g1", "b_g2")]
    assert b.stdout.startswith("query_mismatch: section b_g1 ")
    reports = json.loads(rep.read_text())
    assert reports["srs_check"] is None and reports["key_check"]["findings"] == [] and reports["key_check_srs"]["counts"] == dict(query_mismatch=2, vk_mismatch=0)

    # without --ptau: the line and the exit status of the command as it was, on both keys; and --no-check-srs alone is refused
    for key in (pk, bad_pk):
        own = dev.key_check("BN128", rb, key.read_bytes())
        assert own["findings"] == []
        d = run("groth16_key_check", "-c", "BN128", "--r1cs", c, "-p", key, "--report", rep)
        assert d.returncode == 0, (d.stdout, d.stderr)
        assert d.stdout == ("zkgpu_prove: %s is a well-formed key of %s (%d G1 and %d G2 points, %d pairs; h, l, ic, a are not checked against the circuit's polynomials)\n"
                            % (key, c, own["checked"]["g1_points"], own["checked"]["g2_points"], own["checked"]["pairs"]))
        assert json.loads(rep.read_text()) == own
    e = run("groth16_key_check", "-c", "BN128", "--r1cs", c, "-p", pk, "--no-check-srs")
    assert e.returncode != 0 and "--no-check-srs" in e.stderr
