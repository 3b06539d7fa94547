"""compressor12_setup -> compressor12_exec --wtns -> stark_prove -> stark_verify as four commands on files (tools/zkgpu_prove.py)."""
import json, pathlib, struct, subprocess, sys
import pytest

import c12_setup_ref as REF
import c12_setup_circuits as CC
from test_gpu_c12_setup import stark_struct

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent


def wtns_gl(w):
    """the .wtns container with 8-byte field elements"""
    head = struct.pack("<I", 8) + REF.P.to_bytes(8, "little") + struct.pack("<I", len(w))
    body = b"".join(int(v).to_bytes(8, "little") for v in w)
    return b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, len(head)) + head + struct.pack("<IQ", 2, len(body)) + body


def test_setup_exec_prove_verify_on_files(zk, tmp_path):
    r1cs, w = CC.plain_circuit()
    f = lambda n: str(tmp_path / n)
    (tmp_path / "c.r1cs").write_bytes(r1cs); (tmp_path / "c.wtns").write_bytes(wtns_gl(w))
    (tmp_path / "ss.json").write_text(json.dumps(stark_struct(8)))
    run = lambda *args: subprocess.run([sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")] + list(args), capture_output=True, text=True, timeout=300)
    files = ["--p", f("c.pil"), "--e", f("c.exec")]
    for args in (["compressor12_setup", "--r", f("c.r1cs"), "--c", f("c.const"), "--force_n_bits", "8", "--pil-json", f("c.pil.json")] + files,
                 ["compressor12_exec", "--wtns", f("c.wtns"), "--m", f("c.cm")] + files,
                 ["stark_prove", "-s", f("ss.json"), "-p", f("c.pil.json"), "--o", f("c.const"), "--m", f("c.cm"), "--i", f("zkin.json"), "--eval", "bytecode"],
                 ["stark_verify", "-s", f("ss.json"), "-p", f("c.pil.json"), "--o", f("c.const"), "--i", f("zkin.json")]):
        r = run(*args)
        assert r.returncode == 0, (args[0], r.stdout, r.stderr)
    assert (tmp_path / "c.const").stat().st_size == (1 << 8) * 31 * 8
    assert (tmp_path / "c.cm").stat().st_size == (1 << 8) * 12 * 8
    assert [int(x) for x in json.loads((tmp_path / "zkin.json").read_text())["publics"]] == w[1:4]
