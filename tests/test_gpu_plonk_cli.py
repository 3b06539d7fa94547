"""tools/zkgpu_plonk.py end to end through its files at n = 16: plonk_setup, plonk_prove, plonk_verify, their exit codes, a tampered
public.json and a witness that breaks a gate.  The tool is the subject, so it runs as a process; the file is made with a known tau by
tools/make_test_ptau.py and passes the tool's own check of it."""
import importlib, json, pathlib, subprocess, sys

import pytest

import plonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_plonk.py")]
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args):
    p = subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def test_setup_prove_verify_through_the_files(zk, tmp_path):
    cv = "BN128"
    r = ref.R[cv]
    plonk = importlib.import_module("eigen_zkvm_amd.plonk")
    n_vars, public, gates, wit = ref.chain(3, r)
    plonk.Circuit(n_vars, public, gates, cv).save(tmp_path / "c.npz")
    (tmp_path / "w.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    ptau = tmp_path / "f.ptau"
    ptau.write_bytes(make_test_ptau.build_ptau(zk, cv, 5, 0x1234567, 5, 7))
    rc, out = _run("plonk_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk.json")
    assert rc == 0 and "14 gates and 1 public input(s) in n = 2^4 rows" in out, out
    vk = json.loads((tmp_path / "vk.json").read_text())
    assert (vk["curve"], vk["log_n"], vk["n_public"], sorted(vk["commitments"])) == (cv, 4, 1, sorted(plonk.FIXED_NAMES))
    rc, out = _run("plonk_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w.bin", "--proof", tmp_path / "proof.json",
                   "--public", tmp_path / "public.json", "--no-check-srs")
    assert rc == 0 and "plonk_prove:" in out, out
    assert json.loads((tmp_path / "public.json").read_text()) == [str(wit[-1])]
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("plonk_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, pair, "--no-check-srs")
    assert rc == 0 and "2 proof(s) accepted" in out, out
    (tmp_path / "bad.json").write_text(json.dumps([str((wit[-1] + 1) % r)]))                      # a tampered public.json
    bad = "%s:%s" % (tmp_path / "proof.json", tmp_path / "bad.json")
    rc, out = _run("plonk_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, bad, "--no-check-srs")
    assert rc == 1 and out.count("plonk_verify:") == 1 and "proof.json: the identity or the pairing equation does not hold" in out, out
    wit[5] = (wit[5] + 1) % r                                                                     # a witness that breaks a gate
    (tmp_path / "w2.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    rc, out = _run("plonk_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w2.bin", "--proof", tmp_path / "p2.json",
                   "--public", tmp_path / "x2.json", "--no-check-srs")
    assert rc == 1 and "witness does not satisfy gate" in out and not (tmp_path / "p2.json").exists(), out
    ptau2 = tmp_path / "small.ptau"                                                               # 31 powers: fewer than 3n + 6 = 54
    ptau2.write_bytes(make_test_ptau.build_ptau(zk, cv, 4, 0x1234567, 5, 7))
    rc, out = _run("plonk_setup", "--ptau", ptau2, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk2.json", "--no-check-srs")
    assert rc == 1 and "the file holds 31 G1 powers" in out and not (tmp_path / "vk2.json").exists(), out
