"""tools/zkgpu_poly.py end to end on small files, both curves: the three commands, their exit codes, the non-divisible case and a product
that does not close.  The tool is the subject, so it runs as a process."""
import pathlib, subprocess, sys
import pytest

import frpoly_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = [sys.executable, str(ROOT / "tools" / "zkgpu_poly.py")]
CURVES = ("BN128", "BLS12381")


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


def _run(*args):
    p = subprocess.run(CLI + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def _write(path, vals):
    path.write_bytes(b"".join(v.to_bytes(32, "little") for v in vals))


def _read(path):
    b = path.read_bytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


@pytest.mark.parametrize("cv", CURVES)
def test_poly_mul_and_divmod_zh(tmp_path, cv):
    r = ref.R[cv]
    a, zh = [(5 * i * i + 3) % r for i in range(21)], [r - 1] + [0] * 7 + [1]           # X^8 - 1
    _write(tmp_path / "a.bin", a); _write(tmp_path / "zh.bin", zh)
    rc, out = _run("poly_mul", "-c", cv, "--poly", tmp_path / "a.bin", "--poly", tmp_path / "zh.bin", "-o", tmp_path / "t.bin")
    assert rc == 0 and "21 x 9 coefficients -> 29" in out, out
    t = _read(tmp_path / "t.bin")
    assert t == ref.poly_mul(a, zh, r)
    rc, out = _run("poly_divmod_zh", "-c", cv, "--poly", tmp_path / "t.bin", "--log-n", 3, "-o", tmp_path / "q.bin", "--rem", tmp_path / "r.bin")
    assert rc == 0 and "exactly" in out, out
    assert _read(tmp_path / "q.bin") == a and _read(tmp_path / "r.bin") == [0] * 8
    t[2] = (t[2] + 1) % r; t[5] = (t[5] + 9) % r                                         # not divisible any more
    _write(tmp_path / "t2.bin", t)
    rc, out = _run("poly_divmod_zh", "-c", cv, "--poly", tmp_path / "t2.bin", "--log-n", 3, "-o", tmp_path / "q2.bin", "--rem", tmp_path / "r2.bin")
    assert rc == 1 and "does not divide" in out and "2 non-zero remainder coefficient(s), the first at X^2" in out, out
    assert (_read(tmp_path / "q2.bin"), _read(tmp_path / "r2.bin")) == ref.divmod_zh(t, 3, r)
    _write(tmp_path / "big.bin", [r])                                                    # a value that is not below r
    rc, out = _run("poly_mul", "-c", cv, "--poly", tmp_path / "big.bin", "--poly", tmp_path / "a.bin", "-o", tmp_path / "x.bin")
    assert rc == 1 and "value 0 is not below the scalar field's modulus" in out, out


@pytest.mark.parametrize("cv", CURVES)
def test_grand_product(tmp_path, cv):
    r = ref.R[cv]
    num = [(7 * i + 1) % r for i in range(100)]
    den = num[37:] + num[:37]
    _write(tmp_path / "n.bin", num); _write(tmp_path / "d.bin", den)
    rc, out = _run("grand_product", "-c", cv, "--num", tmp_path / "n.bin", "--den", tmp_path / "d.bin", "-o", tmp_path / "z.bin")
    assert rc == 0 and "closes over 100 rows" in out, out
    assert (_read(tmp_path / "z.bin"), 1) == ref.grand_product(num, den, r)
    num[50] += 1
    _write(tmp_path / "n2.bin", num)
    rc, out = _run("grand_product", "-c", cv, "--num", tmp_path / "n2.bin", "--den", tmp_path / "d.bin", "-o", tmp_path / "z2.bin")
    want_z, want_last = ref.grand_product(num, den, r)
    assert rc == 1 and "does NOT close" in out and str(want_last) in out, out
    assert _read(tmp_path / "z2.bin") == want_z
    den[3] = 0
    _write(tmp_path / "d2.bin", den)
    rc, out = _run("grand_product", "-c", cv, "--num", tmp_path / "n.bin", "--den", tmp_path / "d2.bin", "-o", tmp_path / "z3.bin")
    assert rc == 1 and "the denominator of row 3 is zero" in out and not (tmp_path / "z3.bin").exists(), out
