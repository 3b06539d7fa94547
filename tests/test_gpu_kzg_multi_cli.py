"""tools/zkgpu_kzg.py at several points, end to end on a power-6 file with a known tau: kzg_open with two --poly / --at groups writes one
multi_opening.json, kzg_verify accepts it beside a single-point opening, and a tampered file exits 1 with the line that names it.  The tool is
the subject, so it runs as a process; one curve, the other differs in the library alone (test_gpu_kzg_multi.py)."""
import importlib, json, pathlib, subprocess, sys
import pytest

import kzg_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_kzg.py")]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args):
    p = subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def _write_poly(path, vals):
    path.write_bytes(b"".join(v.to_bytes(32, "little") for v in vals))


def test_open_two_groups_verify_and_tamper(zk, tmp_path):
    cv = "BN128"
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    r = ref.R[cv]
    f1 = tmp_path / "a.ptau"
    f1.write_bytes(make_test_ptau.build_ptau(zk, cv, 6, 0x1234567, 5, 7))
    p1, p2 = [(3 * i * i + 1) % r for i in range(40)], [r - 1 - i for i in range(100)]
    _write_poly(tmp_path / "p1.bin", p1); _write_poly(tmp_path / "p2.bin", p2)
    w = ref.root_of_unity(cv, 3)
    s1, s2 = [5, 5 * w % r], [5, 0x77, r - 2]
    rc, out = _run("kzg_open", "--ptau", f1, "--poly", tmp_path / "p1.bin", "--at", ",".join(hex(p) for p in s1), "--poly", tmp_path / "p2.bin", "--at",
                   ",".join(str(p) for p in s2), "-o", tmp_path / "m.json", "--no-check-srs")
    assert rc == 0 and "2 polynomial(s) at 5 point(s)" in out, out
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["protocol"] == "kzg-multi" and m["sets"] == [[str(p) for p in s1], [str(p) for p in s2]]
    assert m["values"] == [[str(ref.horner(p1, s, r)) for s in s1], [str(ref.horner(p2, s, r)) for s in s2]]
    cs = [kzg.point_from_json(c, cv) for c in m["commitments"]]
    gamma = kzg.challenges_of(cv, cs, [s1, s2], [[int(y) for y in ys] for ys in m["values"]])
    assert int(m["gamma"]) == gamma and int(m["z"]) == kzg.challenge_z(cv, gamma, kzg.point_from_json(m["W1"], cv), avoid=s1 + s2)
    # beside a single-point opening
    rc, out = _run("kzg_open", "--ptau", f1, "--poly", tmp_path / "p1.bin", "--at", "0x99", "-o", tmp_path / "o1.json", "--no-check-srs")
    assert rc == 0, out
    rc, out = _run("kzg_verify", "--ptau", f1, tmp_path / "o1.json", tmp_path / "m.json", "--no-check-srs")
    assert rc == 0 and "2 opening(s) accepted" in out, out
    # one value moved
    bad = json.loads(json.dumps(m)); y = m["values"][1][2]
    bad["values"][1][2] = y[:-1] + ("1" if y[-1] != "1" else "2")
    (tmp_path / "bad.json").write_text(json.dumps(bad))
    rc, out = _run("kzg_verify", "--ptau", f1, tmp_path / "m.json", tmp_path / "bad.json", tmp_path / "o1.json", "--no-check-srs")
    assert rc == 1 and out.count("kzg_verify:") == 1 and "bad.json: the pairing equation does not hold" in out, out
    # a point that is not below r: named directly, nothing is hashed
    big = json.loads(json.dumps(m)); big["sets"][0][1] = str(int(m["sets"][0][1]) + r)
    (tmp_path / "big.json").write_text(json.dumps(big))
    rc, out = _run("kzg_verify", "--ptau", f1, tmp_path / "big.json", "--no-check-srs")
    assert rc == 1 and "big.json: z or y is not below r" in out, out
    # an --at that does not follow its --poly
    rc, out = _run("kzg_open", "--ptau", f1, "--poly", tmp_path / "p1.bin", "--poly", tmp_path / "p2.bin", "--at", "1,2", "-o", tmp_path / "x.json", "--no-check-srs")
    assert rc != 0 and "one --at Z1,Z2,.. after every --poly" in out and not (tmp_path / "x.json").exists(), out
