"""tools/zkgpu_fflonk_lookup_tagged.py end to end on a saved TAGGED circuit at n = 16: fflonk_lookup_tagged_setup prints the
sizes and the tables, fflonk_lookup_tagged_prove and fflonk_lookup_tagged_verify run on its files, a witness whose range-checked row holds a
tuple of the XOR table exits 1 with the row and the table named, and a plain (single-table) .npz, --r1cs and a key of
tools/zkgpu_fflonk_lookup.py are each refused with one line.  The tool is the subject, so it runs as a process; the file is made with a known
tau."""
import importlib, json, pathlib, subprocess, sys

import pytest

import plonk_lookup_ref as lref
import plonk_lookup_tagged_ref as tref
import plonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_fflonk_lookup_tagged.py")]
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args, cli=CLI):
    p = subprocess.run(cli + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def test_setup_prove_verify_on_a_saved_tagged_circuit(zk, tmp_path):
    cv = "BN128"
    r = ref.R[cv]
    flt = importlib.import_module("eigen_zkvm_amd.fflonk_lookup_tagged")
    n_vars, public, gates, tables, wit = tref.tagged_chain(1, r)
    # the range-checked 1 sits in a, a variable of its own in b (0 in the good witness): b = 1 makes the row (1, 1, 0), an XOR row
    g = max(i for i, q in enumerate(gates["qK"]) if q == 1)
    wit = list(wit) + [0]
    gates["b"][g] = n_vars
    flt.LookupCircuit(n_vars + 1, public, gates, curve=cv, tables=tables).save(tmp_path / "c.npz")
    (tmp_path / "w.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    ptau = tmp_path / "f.ptau"
    ptau.write_bytes(make_test_ptau.build_ptau(zk, cv, 7, 0x1234567, 5, 7))
    rc, out = _run("fflonk_lookup_tagged_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk.json")
    assert rc == 0 and "12 gates and 1 public input(s) in n = 2^4 rows" in out and "2 tagged tables of 2, 5 rows (7 in all), 6 of the gates look a row up" in out, out
    assert "fflonk_lookup_tagged_setup: n = 2^4 = 16 rows need 8n + 8 = 136 powers (a file of power 7 has them)" in out, out
    vk = json.loads((tmp_path / "vk.json").read_text())
    assert (vk["protocol"], vk["curve"], vk["log_n"], vk["n_public"]) == ("fflonk-shplonk-lookup-tagged", cv, 4, 1) and "C0" in vk and "C0L" in vk and "commitments" not in vk
    rc, out = _run("fflonk_lookup_tagged_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w.bin", "--proof", tmp_path / "proof.json",
                   "--public", tmp_path / "public.json", "--no-check-srs")
    assert rc == 0 and "fflonk_lookup_tagged_prove:" in out, out
    assert json.loads((tmp_path / "public.json").read_text()) == [str(wit[public[0]])]
    proof = json.loads((tmp_path / "proof.json").read_text())
    assert proof["protocol"] == "fflonk-shplonk-lookup-tagged" and len(proof["values"]) == 23 and all(k in proof for k in flt.POINT_NAMES)
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("fflonk_lookup_tagged_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, pair, "--no-check-srs")
    assert rc == 0 and "2 proof(s) accepted" in out, out
    (tmp_path / "bad.json").write_text(json.dumps([str((wit[public[0]] + 1) % r)]))             # a tampered public.json
    bad = "%s:%s" % (tmp_path / "proof.json", tmp_path / "bad.json")
    rc, out = _run("fflonk_lookup_tagged_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, bad, "--no-check-srs")
    assert rc == 1 and out.count("fflonk_lookup_tagged_verify:") == 1 and "proof.json: the opening that carries the identities does not hold" in out, out
    wit[-1] = 1                                                                            # (1, 1, 0) under the range table's tag
    (tmp_path / "w2.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    rc, out = _run("fflonk_lookup_tagged_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w2.bin", "--proof", tmp_path / "p2.json",
                   "--public", tmp_path / "x2.json", "--no-check-srs")
    row = len(public) + g
    assert rc == 1 and "witness does not satisfy lookup at row %d (1 rows): (a, b, c) is not a row of table 1" % row in out and not (tmp_path / "p2.json").exists(), out
    # the three refusals, one line each
    rc, out = _run("fflonk_lookup_tagged_setup", "--ptau", ptau, "--r1cs", tmp_path / "c.r1cs", "-v", tmp_path / "vk3.json")
    assert rc == 1 and "takes no --r1cs" in out and len(out.strip().splitlines()) == 1, out
    n_vars1, public1, gates1, table1, _ = lref.lookup_chain(1, r)
    flt.LookupCircuit(n_vars1, public1, gates1, table1, cv).save(tmp_path / "plain.npz")
    rc, out = _run("fflonk_lookup_tagged_setup", "--ptau", ptau, "--circuit", tmp_path / "plain.npz", "-v", tmp_path / "vk4.json", "--no-check-srs")
    assert rc == 1 and "the circuit has one untagged table" in out and "fflonk_lookup.py proves a circuit of one table" in out and len(out.strip().splitlines()) == 1, out
    assert not (tmp_path / "vk4.json").exists()
    rc, out = _run("fflonk_lookup_setup", "--ptau", ptau, "--circuit", tmp_path / "plain.npz", "-v", tmp_path / "vk1.json", "--no-check-srs",
                   cli=[sys.executable, str(ROOT / "tools" / "zkgpu_fflonk_lookup.py")])
    assert rc == 0, out
    rc, out = _run("fflonk_lookup_tagged_verify", "-v", tmp_path / "vk1.json", "--ptau", ptau, pair, "--no-check-srs")
    assert rc == 1 and 'not a verification key of this prover (protocol "fflonk-shplonk-lookup"): fflonk_lookup.py proves and verifies it' in out, out
    assert len(out.strip().splitlines()) == 1 and out.startswith("zkgpu_fflonk_lookup_tagged: "), out
    # and that tool refuses this tool's key, with its own words
    rc, out = _run("fflonk_lookup_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, "--no-check-srs", cli=[sys.executable, str(ROOT / "tools" / "zkgpu_fflonk_lookup.py")])
    assert rc != 0 and 'not a verification key of this prover (protocol "fflonk-shplonk-lookup-tagged")' in out, out
