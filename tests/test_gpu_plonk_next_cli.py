"""tools/zkgpu_plonk_next.py end to end: plonk_next_setup, plonk_next_prove and plonk_next_verify on a saved gate table with
chains at n = 16 and on an .r1cs with its .wtns, with their exit codes; a witness that breaks a next-row relation exits 1 with its row; and
the two tools refuse each other's keys and proofs.  The tool is the subject, so it runs as a process; the file is made with a known tau."""
import importlib, json, pathlib, subprocess, sys

import pytest

import plonk_next_ref as nref
import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_plonk_next.py")]
PLONK_CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_plonk.py")]
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args, cli=CLI):
    p = subprocess.run(cli + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def test_the_three_commands_on_files_and_the_two_tools_at_each_others_door(zk, tmp_path):
    cv = "BN128"
    r = nref.R[cv]
    pn = importlib.import_module("eigen_zkvm_amd.plonk_next")
    n_vars, public, gates, wit = nref.running_sums([(i + 2, 100 + i) for i in range(5)], r)
    circuit = pn.NextCircuit(n_vars, public, gates, cv)
    circuit.save(tmp_path / "c.npz")
    (tmp_path / "w.bin").write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))
    ptau = tmp_path / "f.ptau"
    ptau.write_bytes(make_test_ptau.build_ptau(zk, cv, 5, 0x1234567, 5, 7))
    rc, out = _run("plonk_next_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "vk.json")
    assert rc == 0 and "10 gates and 1 public input(s) in n = 2^4 rows" in out, out
    vk = json.loads((tmp_path / "vk.json").read_text())
    assert (vk["protocol"], vk["curve"], vk["log_n"], vk["n_public"], sorted(vk["commitments"])) == ("plonk-shplonk-next", cv, 4, 1, sorted(pn.NEXT_FIXED_NAMES))
    rc, out = _run("plonk_next_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w.bin", "--proof", tmp_path / "proof.json",
                   "--public", tmp_path / "public.json", "--no-check-srs")
    assert rc == 0 and "plonk_next_prove:" in out, out
    proof = json.loads((tmp_path / "proof.json").read_text())
    assert proof["protocol"] == "plonk-shplonk-next" and len(proof["values"]) == 16
    assert json.loads((tmp_path / "public.json").read_text()) == [str(wit[public[0]])]
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("plonk_next_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, pair, "--no-check-srs")
    assert rc == 0 and "2 proof(s) accepted" in out, out
    (tmp_path / "x2.json").write_text(json.dumps([str((wit[public[0]] + 1) % r)]))
    rc, out = _run("plonk_next_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, "%s:%s" % (tmp_path / "proof.json", tmp_path / "x2.json"), "--no-check-srs")
    assert rc == 1 and out.count("plonk_next_verify:") == 1 and "the identity or the pairing equation does not hold" in out, out
    # a chain's auxiliary wrong: the row before the one it stands in, through its next-row term
    row = 1 + min(i for i, q in enumerate(gates["qN"]) if q)
    v = gates["c"][row]                                                                     # gate `row` is table row 1 + row: the c after the first chain row
    bad = list(wit)
    bad[v] = (bad[v] + 1) % r
    (tmp_path / "w2.bin").write_bytes(b"".join(x.to_bytes(32, "little") for x in bad))
    rc, out = _run("plonk_next_prove", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "--witness", tmp_path / "w2.bin", "--proof", tmp_path / "p2.json",
                   "--public", tmp_path / "x3.json", "--no-check-srs")
    assert rc == 1 and "plonk next: witness does not satisfy gate %d (2 rows)" % row in out and not (tmp_path / "p2.json").exists(), out
    # the other tool's key and proof here, this tool's there: one line each, exit 1
    plonk = importlib.import_module("eigen_zkvm_amd.plonk")
    pcircuit = plonk.Circuit(n_vars, public, {k: v for k, v in gates.items() if k != "qN"}, cv)
    pcircuit.save(tmp_path / "pc.npz")
    rc, out = _run("plonk_setup", "--ptau", ptau, "--circuit", tmp_path / "pc.npz", "-v", tmp_path / "pvk.json", "--no-check-srs", cli=PLONK_CLI)
    assert rc == 0, out
    rc, out = _run("plonk_next_verify", "-v", tmp_path / "pvk.json", "--ptau", ptau, pair, "--no-check-srs")
    assert rc == 1 and out.strip() == 'zkgpu_plonk_next: plonk next: not a verification key of this prover (protocol "plonk-shplonk")', out
    rc, out = _run("plonk_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, "--no-check-srs", cli=PLONK_CLI)
    assert rc != 0 and 'plonk: not a verification key of this prover (protocol "plonk-shplonk-next")' in out, out
    rc, out = _run("plonk_verify", "-v", tmp_path / "pvk.json", "--ptau", ptau, pair, "--no-check-srs", cli=PLONK_CLI)
    assert rc != 0 and 'plonk: not a proof of this prover on BN128 (protocol "plonk-shplonk-next"' in out, out
    rc, out = _run("plonk_setup", "--ptau", ptau, "--circuit", tmp_path / "c.npz", "-v", tmp_path / "no.json", "--no-check-srs", cli=PLONK_CLI)
    assert rc == 1 and "holds a next-row selector qN: it is a circuit of plonk_next.py" in out and not (tmp_path / "no.json").exists(), out


def test_setup_and_prove_from_an_r1cs_and_its_wtns(zk, tmp_path):
    cv = "BN128"
    data, w, long_row, cw = cases.shapes(cv)
    m = nref.Compiled(data, cv)
    (tmp_path / "c.r1cs").write_bytes(data)
    (tmp_path / "w.wtns").write_bytes(cases.wtns_bytes(cv, w))
    ptau = tmp_path / "f.ptau"
    ptau.write_bytes(make_test_ptau.build_ptau(zk, cv, 11, 0x7654321, 5, 7))
    rc, out = _run("plonk_next_setup", "--ptau", ptau, "--r1cs", tmp_path / "c.r1cs", "-v", tmp_path / "vk.json", "--no-check-srs")
    assert rc == 0 and "8 constraints -> %d gates, %d auxiliaries; n = 2^10 rows need 3n + 7 = 3079 powers (a file of power 11 has them)" % (m.n_gates, m.n_aux) in out, out
    rc, out = _run("plonk_next_prove", "--ptau", ptau, "--r1cs", tmp_path / "c.r1cs", "--wtns", tmp_path / "w.wtns", "--proof", tmp_path / "proof.json",
                   "--public", tmp_path / "public.json", "--no-check-srs")
    assert rc == 0 and "n = 2^10" in out, out
    pair = "%s:%s" % (tmp_path / "proof.json", tmp_path / "public.json")
    rc, out = _run("plonk_next_verify", "-v", tmp_path / "vk.json", "--ptau", ptau, pair, "--no-check-srs")
    assert rc == 0 and "1 proof(s) accepted" in out, out
    (tmp_path / "bad.wtns").write_bytes(cases.wtns_bytes(cv, cases.corrupt(w, cw, p=m.p)))
    rc, out = _run("plonk_next_prove", "--ptau", ptau, "--r1cs", tmp_path / "c.r1cs", "--wtns", tmp_path / "bad.wtns", "--proof", tmp_path / "p2.json",
                   "--public", tmp_path / "x2.json", "--no-check-srs")
    assert rc == 1 and "(constraint %d of the .r1cs)" % long_row in out and not (tmp_path / "p2.json").exists(), out
