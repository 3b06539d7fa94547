"""tools/zkgpu_ceremony.py end to end on the device: ptau_new -> ptau_contribute --check -> ptau_beacon -> ptau_verify, the result through
`zkgpu_prove.py groth16_setup --ptau`, key_contribute twice -> key_verify, and the exit status and the finding line on a file whose
transcript was tampered with.  The secrets here come from the operating system, so nothing can be compared byte for byte: that is
tests/test_gpu_ptau_ceremony.py's and tests/test_gpu_key_transcript.py's part."""
import json, pathlib, subprocess, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tests"))
import groth16 as G  # noqa: E402
import ceremony_ref as CR  # noqa: E402
CER = [sys.executable, str(ROOT / "tools" / "zkgpu_ceremony.py")]
PROVE = [sys.executable, str(ROOT / "tools" / "zkgpu_prove.py")]


def _run(cmd, *args):
    return subprocess.run(cmd + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def test_a_ceremony_from_the_command_line_to_a_key(orc, tmp_path):
    g = G.Groth16Oracle(orc, "bn254")
    r1cs, _ = G.synthetic_r1cs(g.r, 4, seed=5)
    power = g.circuit(r1cs)["log_m"]
    rf = tmp_path / "c.r1cs"; rf.write_bytes(g.r1cs_bytes(r1cs))
    p0, p1, p2, rep = (tmp_path / n for n in ("p0.ptau", "p1.ptau", "p2.ptau", "rep.json"))
    a = _run(CER, "ptau_new", "-c", "BN128", "--power", power, "-o", p0)
    assert a.returncode == 0 and "tau = alpha = beta = 1" in a.stdout, a.stderr
    a = _run(CER, "ptau_contribute", "-c", "BN128", "-i", p0, "-o", p1, "--check")
    assert a.returncode == 0 and "contribution 1" in a.stdout and "1 contribution(s): ok" in a.stdout, a.stderr
    a = _run(CER, "ptau_beacon", "-i", p1, "-o", p2, "--seed", "ab" * 32, "--iter-log", 4)
    assert a.returncode == 0, a.stderr
    a = _run(CER, "ptau_verify", "-c", "BN128", p2, "--report", rep)
    assert a.returncode == 0 and "2 contribution(s): ok" in a.stdout, a.stdout + a.stderr
    r = json.loads(rep.read_text())
    assert r["contributions"] == 2 and not r["findings"] and not r["file"]["findings"]
    b1, b2 = p1.read_bytes(), p2.read_bytes()
    assert b1 != b2 and len(b2) - len(b1) == CR.rec_bytes(64)              # the contribution moved the points; the beacon added its record
    # the existing setup takes the file as it is, transcript and all
    k, vk = tmp_path / "k.key", tmp_path / "vk.json"
    a = _run(PROVE, "groth16_setup", "-c", "BN128", "--r1cs", rf, "-p", k, "-v", vk, "--ptau", p2)
    assert a.returncode == 0 and k.exists() and "well-formed powers-of-tau file" in a.stdout, a.stderr
    # one byte of the first record's tau response: exit 1, one line per finding
    recs = CR.parse(CR.section(b2, CR.SECTION), 64)
    z = recs[0]["z"][0]
    recs[0]["z"][0] = bytes([z[0] ^ 1]) + z[1:]
    CR.rehash(recs, 32, power)
    bad = tmp_path / "bad.ptau"; bad.write_bytes(CR.replace_section(b2, CR.SECTION, CR.serialize(recs)))
    a = _run(CER, "ptau_verify", bad)
    lines = [ln for ln in a.stdout.splitlines() if ln.startswith("ptau transcript:")]
    assert a.returncode == 1 and lines[0] == "ptau transcript: contribution 1: no valid proof of knowledge of the tau factor", a.stdout + a.stderr
    assert len(lines) == 4 and "4 finding(s)" in a.stdout                  # and the beacon's three proofs, whose challenges hang on the hash that moved
    assert _run(CER, "ptau_beacon", "-i", p1, "-o", tmp_path / "x.ptau", "--seed", "abc", "--iter-log", 1).returncode != 0
    # phase 2: two contributions to the key's delta, each with its proof, then the whole chain
    k1, k2, t = tmp_path / "k1.key", tmp_path / "k2.key", tmp_path / "key.transcript"
    a = _run(CER, "key_contribute", "-c", "BN128", "-p", k, "-o", k1, "--transcript", t)
    assert a.returncode == 0 and t.exists(), a.stderr
    a = _run(CER, "key_contribute", "-c", "BN128", "-p", k1, "-o", k2, "--transcript", t, "-v", tmp_path / "vk2.json")
    assert a.returncode == 0 and json.loads((tmp_path / "vk2.json").read_text())["protocol"] == "groth16", a.stderr
    a = _run(CER, "key_verify", "-c", "BN128", "--initial", k, "--final", k2, "--transcript", t)
    assert a.returncode == 0 and "2 contribution(s)" in a.stdout and a.stdout.rstrip().endswith(": ok"), a.stdout + a.stderr
    a = _run(CER, "key_verify", "-c", "BN128", "--initial", k, "--final", k1, "--transcript", t)
    assert a.returncode == 1 and "key transcript: the transcript does not end at the final key (delta_g1)" in a.stdout, a.stdout + a.stderr
    assert _run(CER, "key_contribute", "-c", "BN128", "-p", k, "-o", tmp_path / "x.key", "--transcript", t).returncode != 0   # the transcript ends at k2, not at k
