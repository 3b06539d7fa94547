"""tools/zkgpu_fflonk_lookup.py end to end through its files at n = 16: fflonk_lookup_setup, fflonk_lookup_prove, fflonk_lookup_verify, their
exit codes, a tampered public.json, a witness whose looked-up tuple is no row of the table, and a key of this tool
under tools/zkgpu_plonk_lookup.py and tools/zkgpu_fflonk.py.  The tool is the subject, so it runs as a process; the file is made with a known
tau by tools/make_test_ptau.py."""
import importlib, json, pathlib, subprocess, sys

import pytest

import plonk_lookup_ref as lref
import plonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_fflonk_lookup.py")]
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args, cli=CLI):
    p = subprocess.run(cli + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def test_setup_prove_verify_through_the_files(zk, tmp_path):
    cv = "BN128"
    r = ref.R[cv]
    fl = importlib.import_module("eigen_zkvm_amd.fflonk_lookup")
    n_vars, public, gates, table, wit = lref.lookup_chain(1, r)
    fl.LookupCircuit(n_vars, public, gates, table, cv).save(tmp_path / "c.npz")
    (tmp_path / "w.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    ptau = tmp_path / "f.ptau"
    ptau.write_bytes(make_test_ptau.build_ptau(zk, cv, 7, 0x1234567, 5, 7))
    rc, out = _run("fflonk_lookup_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk.json")
    assert rc == 0 and "10 gates and 1 public input(s) in n = 2^4 rows" in out and "a table of 5 rows, 4 of the gates look a row up" in out, out
    assert "fflonk_lookup_setup: n = 2^4 = 16 rows need 8n + 8 = 136 powers (a file of power 7 has them)" in out, out
    vk = json.loads((tmp_path / "vk.json").read_text())
    assert (vk["protocol"], vk["curve"], vk["log_n"], vk["n_public"]) == ("fflonk-shplonk-lookup", cv, 4, 1) and "C0" in vk and "C0L" in vk and "commitments" not in vk
    rc, out = _run("fflonk_lookup_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w.bin", "--proof", tmp_path / "proof.json",
                   "--public", tmp_path / "public.json", "--no-check-srs")
    assert rc == 0 and "fflonk_lookup_prove:" in out, out
    assert json.loads((tmp_path / "public.json").read_text()) == [str(wit[public[0]])]
    proof = json.loads((tmp_path / "proof.json").read_text())
    assert proof["protocol"] == "fflonk-shplonk-lookup" and len(proof["values"]) == 22 and all(k in proof for k in fl.POINT_NAMES)
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("fflonk_lookup_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, pair, "--no-check-srs")
    assert rc == 0 and "2 proof(s) accepted" in out, out
    (tmp_path / "bad.json").write_text(json.dumps([str((wit[public[0]] + 1) % r)]))             # a tampered public.json
    bad = "%s:%s" % (tmp_path / "proof.json", tmp_path / "bad.json")
    rc, out = _run("fflonk_lookup_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, bad, "--no-check-srs")
    assert rc == 1 and out.count("fflonk_lookup_verify:") == 1 and "proof.json: the opening that carries the identities does not hold" in out, out
    wit[-1] = (wit[-1] + 2) % r                                                                   # the last looked-up c: no row of the table
    (tmp_path / "w2.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    rc, out = _run("fflonk_lookup_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w2.bin", "--proof", tmp_path / "p2.json",
                   "--public", tmp_path / "x2.json", "--no-check-srs")
    assert rc == 1 and "witness does not satisfy lookup at row" in out and "is not a row of the table" in out and not (tmp_path / "p2.json").exists(), out
    rc, out = _run("fflonk_lookup_setup", "--ptau", ptau, "--r1cs", tmp_path / "c.r1cs", "-v", tmp_path / "vk3.json")
    assert rc == 1 and "takes no --r1cs" in out and len(out.strip().splitlines()) == 1, out
    # the two nearest provers' tools refuse this tool's key, with their own words
    for tool, cmd in (("zkgpu_plonk_lookup.py", "plonk_lookup_verify"), ("zkgpu_fflonk.py", "fflonk_verify")):
        rc, out = _run(cmd, "-v", tmp_path / "vk.json", "--ptau", ptau, pair, "--no-check-srs", cli=[sys.executable, str(ROOT / "tools" / tool)])
        assert rc != 0 and "not a verification key of this prover" in out, out
