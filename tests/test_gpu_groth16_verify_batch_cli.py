"""tools/zkgpu_prove.py groth16_verify --batch LIST.json in fresh child processes, both curves: a good list is one line with the
count and exit 0; a list with bad entries names each of them with its verdict and exits as the single-proof command does."""
import importlib, json, pathlib, subprocess, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


@pytest.mark.parametrize("cv,tag", [("bn254", "BN128"), ("bls12_381", "BLS12381")])
def test_batch_list(zk, orc, tmp_path, cv, tag):
    zk.init(0)
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    g = G.Groth16Oracle(orc, cv)
    r1cs, wit = G.synthetic_r1cs(g.r, 6, n_pub=2, seed=9)
    rb = g.r1cs_bytes(r1cs)
    pb, vk_json = dev.keygen(tag, rb)
    S = dev.Groth16Setup(tag, rb, pb)
    (tmp_path / "vk.json").write_text(vk_json)
    sub = tmp_path / "proofs"; sub.mkdir()
    pub = [str(int(w)) for w in wit[1:3]]
    for k in range(5):
        js, _ = S.prove(g.fr_array(wit), r=5 + k, s=50 + k)
        (sub / ("proof%d.json" % k)).write_text(json.dumps(js)); (sub / ("public%d.json" % k)).write_text(json.dumps(pub))
    S.free()
    pairs = [["proofs/proof%d.json" % k, "proofs/public%d.json" % k] for k in range(5)]
    (tmp_path / "good.json").write_text(json.dumps(pairs))
    (sub / "tampered.json").write_text(json.dumps([pub[0], str((int(pub[1]) + 1) % g.r)]))
    (sub / "short.json").write_text(json.dumps(pub[:1]))
    bad = list(pairs); bad[1] = [pairs[1][0], "proofs/tampered.json"]; bad[3] = [pairs[3][0], "proofs/short.json"]
    (tmp_path / "bad.json").write_text(json.dumps(bad))
    run = lambda lst: subprocess.run(CLI + ["groth16_verify", "-c", tag, "-v", str(tmp_path / "vk.json"), "--batch", str(tmp_path / lst)],
                                     capture_output=True, text=True, timeout=300)
    a = run("good.json")
    assert a.returncode == 0 and "all 5 proofs" in a.stdout and "accepted" in a.stdout, a.stdout + a.stderr
    b = run("bad.json")
    out = b.stdout + b.stderr
    assert b.returncode == 1 and "verify failed: 2 of 5" in out, out
    assert "proof 1 (proofs/proof1.json): the verification equation does not hold" in out
    assert "proof 3 (proofs/proof3.json): wrong number of public inputs" in out
    assert "proof 0" not in out and "proof 2" not in out and "proof 4" not in out
