"""tools/zkgpu_kzg.py end to end on a power-6 file with a known tau, both curves: kzg_commit -> kzg_open -> kzg_verify exits 0, and each way
of spoiling it exits 1 with the line the tool's text documents.  The tool is the subject, so it runs as a process."""
import hashlib, importlib, json, pathlib, subprocess, sys
import pytest

import kzg_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_kzg.py")]
CURVES = ("BN128", "BLS12381")


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args):
    p = subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def _write_poly(path, vals):
    path.write_bytes(b"".join(v.to_bytes(32, "little") for v in vals))


@pytest.mark.parametrize("cv", CURVES)
def test_commit_open_verify_and_refusals(zk, tmp_path, cv):
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    r = ref.R[cv]
    f1, f2 = tmp_path / "a.ptau", tmp_path / "b.ptau"
    f1.write_bytes(make_test_ptau.build_ptau(zk, cv, 6, 0x1234567, 5, 7))
    f2.write_bytes(make_test_ptau.build_ptau(zk, cv, 6, 0x7654321, 5, 7))
    p1, p2 = [(3 * i * i + 1) % r for i in range(40)], [r - 1 - i for i in range(100)]
    _write_poly(tmp_path / "p1.bin", p1); _write_poly(tmp_path / "p2.bin", p2)
    z = 0xABCDEF0123
    # one polynomial, the file's own check included once
    rc, out = _run("kzg_commit", "--ptau", f1, "--poly", tmp_path / "p1.bin", "-o", tmp_path / "c1.json")
    assert rc == 0, out
    rc, out = _run("kzg_open", "-c", cv, "--ptau", f1, "--poly", tmp_path / "p1.bin", "--at", hex(z), "-o", tmp_path / "o1.json", "--no-check-srs")
    assert rc == 0, out
    o1 = json.loads((tmp_path / "o1.json").read_text())
    assert o1["commitments"][0] == json.loads((tmp_path / "c1.json").read_text())["commitment"]
    assert o1["values"] == [str(ref.horner(p1, z, r))]
    # two polynomials: gamma is the documented hash
    rc, out = _run("kzg_open", "--ptau", f1, "--poly", tmp_path / "p1.bin", "--poly", tmp_path / "p2.bin", "--at", z, "-o", tmp_path / "o2.json", "--no-check-srs")
    assert rc == 0, out
    o2 = json.loads((tmp_path / "o2.json").read_text())
    enc = [kzg.point_from_json(c, cv) for c in o2["commitments"]]
    h = hashlib.sha256(cv.encode("ascii") + enc[0] + enc[1] + z.to_bytes(32, "little")).digest()
    assert int(o2["gamma"]) == int.from_bytes(h, "big") % r
    assert o2["values"] == [str(ref.horner(p1, z, r)), str(ref.horner(p2, z, r))]
    rc, out = _run("kzg_verify", "--ptau", f1, tmp_path / "o1.json", tmp_path / "o2.json", "--no-check-srs")
    assert rc == 0 and "2 opening(s) accepted" in out, out
    # a flipped digit of y
    bad = dict(o1); y = o1["values"][0]
    bad["values"] = [y[:-1] + ("1" if y[-1] != "1" else "2")]
    (tmp_path / "bad.json").write_text(json.dumps(bad))
    rc, out = _run("kzg_verify", "--ptau", f1, tmp_path / "o2.json", tmp_path / "bad.json", "--no-check-srs")
    assert rc == 1 and out.count("kzg_verify:") == 1 and "bad.json: the pairing equation does not hold" in out, out
    # a several-polynomial opening with a value that is not below r: named directly, nothing is folded
    big = dict(o2); big["values"] = [o2["values"][0], str(int(o2["values"][1]) + r)]
    (tmp_path / "big.json").write_text(json.dumps(big))
    rc, out = _run("kzg_verify", "--ptau", f1, tmp_path / "big.json", tmp_path / "o1.json", "--no-check-srs")
    assert rc == 1 and out.count("kzg_verify:") == 1 and "big.json: z or y is not below r" in out, out
    # an opening made over another file
    rc, out = _run("kzg_verify", "--ptau", f2, tmp_path / "o1.json", "--no-check-srs")
    assert rc == 1 and "o1.json: the pairing equation does not hold" in out, out
    # a value >= r in p.bin
    _write_poly(tmp_path / "p3.bin", [1, 2, r, 4])
    rc, out = _run("kzg_commit", "--ptau", f1, "--poly", tmp_path / "p3.bin", "-o", tmp_path / "c3.json", "--no-check-srs")
    assert rc == 1 and "p3.bin: value 2 is not below the scalar field's modulus" in out and not (tmp_path / "c3.json").exists(), out
