"""tools/zkgpu_fflonk.py end to end through its files: fflonk_setup, fflonk_prove, fflonk_verify at n = 16 from a gate table, their exit
codes, a tampered public.json, a witness that breaks a gate and a file too small; then the same three commands from multiplier.r1cs and its
.wtns, whose vk.json must equal the one made from the saved table of the same circuit.  The tool is the subject, so it runs as a process; the
file is made with a known tau by tools/make_test_ptau.py and passes the tool's own check of it."""
import importlib, json, pathlib, subprocess, sys

import pytest

import plonk_ref as ref
import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_fflonk.py")]
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def ptau(zk, tmp_path_factory):
    p = tmp_path_factory.mktemp("fflonk_cli") / "f.ptau"
    p.write_bytes(make_test_ptau.build_ptau(zk, "BN128", 7, 0x1234567, 5, 7))          # 255 powers: 9n + 18 = 162 for n = 16
    return p


def _run(*args):
    p = subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def test_setup_prove_verify_through_the_files(zk, tmp_path, ptau):
    cv = "BN128"
    r = ref.R[cv]
    fflonk = importlib.import_module("eigen_zkvm_amd.fflonk")
    n_vars, public, gates, wit = ref.chain(3, r)
    fflonk.Circuit(n_vars, public, gates, cv).save(tmp_path / "c.npz")
    (tmp_path / "w.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    rc, out = _run("fflonk_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk.json")
    assert rc == 0 and "14 gates and 1 public input(s) in n = 2^4 rows" in out, out
    assert "n = 2^4 = 16 rows need 9n + 18 = 162 powers (a file of power 7 has them)" in out, out
    vk = json.loads((tmp_path / "vk.json").read_text())
    assert (vk["protocol"], vk["curve"], vk["log_n"], vk["n_public"], sorted(vk["C0"])) == ("fflonk-shplonk", cv, 4, 1, ["x", "y"]) and "commitments" not in vk
    rc, out = _run("fflonk_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w.bin", "--proof", tmp_path / "proof.json",
                   "--public", tmp_path / "public.json", "--no-check-srs")
    assert rc == 0 and "fflonk_prove:" in out, out
    assert json.loads((tmp_path / "public.json").read_text()) == [str(wit[-1])]
    proof = json.loads((tmp_path / "proof.json").read_text())
    assert len(proof["values"]) == 15 and all(k in proof for k in ("C1", "C2", "W1", "W2"))
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("fflonk_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, pair, "--no-check-srs")
    assert rc == 0 and "2 proof(s) accepted" in out, out
    (tmp_path / "bad.json").write_text(json.dumps([str((wit[-1] + 1) % r)]))                      # a tampered public.json
    bad = "%s:%s" % (tmp_path / "proof.json", tmp_path / "bad.json")
    rc, out = _run("fflonk_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, bad, "--no-check-srs")
    assert rc == 1 and out.count("fflonk_verify:") == 1 and "proof.json: the opening that carries the identities does not hold" in out, out
    wit[5] = (wit[5] + 1) % r                                                                     # a witness that breaks a gate
    (tmp_path / "w2.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    rc, out = _run("fflonk_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w2.bin", "--proof", tmp_path / "p2.json",
                   "--public", tmp_path / "x2.json", "--no-check-srs")
    assert rc == 1 and "witness does not satisfy gate" in out and not (tmp_path / "p2.json").exists(), out
    ptau2 = tmp_path / "small.ptau"                                                               # 127 powers: fewer than 9n + 18 = 162
    ptau2.write_bytes(make_test_ptau.build_ptau(zk, cv, 6, 0x1234567, 5, 7))
    rc, out = _run("fflonk_setup", "--ptau", ptau2, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk2.json", "--no-check-srs")
    assert rc == 1 and "the file holds 127 G1 powers" in out and "a file of power 7 has them" in out and not (tmp_path / "vk2.json").exists(), out


def test_the_three_commands_from_an_r1cs_and_its_wtns(zk, tmp_path, ptau):
    cv = "BN128"
    fflonk = importlib.import_module("eigen_zkvm_amd.fflonk")
    r1cs = ROOT / "tests" / "golden" / "plonk" / "multiplier.r1cs"
    w = [1, 11210000, 1121, 10000]
    (tmp_path / "w.wtns").write_bytes(cases.wtns_bytes(cv, w))
    rc, out = _run("fflonk_setup", "--ptau", ptau, "--r1cs", r1cs, "-v", tmp_path / "vk.json", "--no-check-srs")
    assert rc == 0 and "1 constraints -> " in out and "n = 2^3 = 8 rows need 9n + 18 = 90 powers (a file of power 6 has them)" in out, out
    c = fflonk.R1csCircuit(r1cs.read_bytes(), cv)                                                 # the table the import made, saved, through --circuit
    c.save(tmp_path / "c.npz")
    c.free()
    rc, out = _run("fflonk_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk_table.json", "--no-check-srs")
    assert rc == 0, out
    assert (tmp_path / "vk.json").read_text() == (tmp_path / "vk_table.json").read_text()
    rc, out = _run("fflonk_prove", "--ptau", ptau, "--r1cs", r1cs, "--wtns", tmp_path / "w.wtns", "--proof", tmp_path / "proof.json", "--public", tmp_path / "public.json",
                   "--no-check-srs")
    assert rc == 0 and "fflonk_prove:" in out, out
    assert json.loads((tmp_path / "public.json").read_text()) == [str(w[1])]
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("fflonk_verify", "-v", tmp_path / "vk_table.json", "--ptau", ptau, pair, "--no-check-srs")
    assert rc == 0 and "1 proof(s) accepted" in out, out
    (tmp_path / "bad.wtns").write_bytes(cases.wtns_bytes(cv, [1, 11210001, 1121, 10000]))
    rc, out = _run("fflonk_prove", "--ptau", ptau, "--r1cs", r1cs, "--wtns", tmp_path / "bad.wtns", "--proof", tmp_path / "p2.json", "--public", tmp_path / "x2.json",
                   "--no-check-srs")
    assert rc == 1 and "witness does not satisfy gate 0 (constraint 0 of the .r1cs)" in out and not (tmp_path / "p2.json").exists(), out
