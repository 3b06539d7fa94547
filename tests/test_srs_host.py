"""The powers-of-tau reader (csrc/groth16_srs.hip.h zk_srs_open) on the host, no GPU: the committed file
tests/golden/groth16/test_bn128_power3.ptau (tools/make_test_ptau.py wrote it; its trapdoor is in the .json beside it) opens, every way
of damaging the container is refused by name, and a setup asked of a file that is too small fails before any device work.
No file written by snarkjs has met this reader: the layout is restated from its writer."""
import importlib, json, pathlib, struct, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
GOLDEN = ROOT / "tests" / "golden" / "groth16" / "test_bn128_power3.ptau"
R_BN = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


def _sections(b):
    """[(id, offset of the section's 12-byte head, payload size)]"""
    n = struct.unpack_from("<I", b, 8)[0]
    o, out = 12, []
    for _ in range(n):
        sid, sz = struct.unpack_from("<IQ", b, o)
        out.append((sid, o, sz)); o += 12 + sz
    assert o == len(b)
    return out


def test_golden_file_opens(zk, dev):
    td = json.loads(GOLDEN.with_name(GOLDEN.name + ".json").read_text())
    assert td["curve"] == "BN128" and td["power"] == 3
    b = GOLDEN.read_bytes()
    assert [(s, z) for s, _, z in _sections(b)] == [(1, 44), (2, 15 * 64), (3, 8 * 128), (4, 8 * 64), (5, 8 * 64), (6, 128)]
    s = dev.Srs("BN128", GOLDEN)
    assert (s.power, s.ceremony_power) == (3, 3)
    s.free(); s.free()
    lib = zk.lib()
    h = lib.zk_srs_open(b"BN128", str(GOLDEN).encode())
    assert h and lib.zk_srs_free(h) == 0


def test_an_ignored_section_is_walked_over(dev, tmp_path):
    b = GOLDEN.read_bytes()
    extra = struct.pack("<IQ", 7, 5) + b"hello"                           # contributions: not read
    p = tmp_path / "extra.ptau"
    p.write_bytes(b[:8] + struct.pack("<I", 7) + b[12:12 + 12 + 44] + extra + b[12 + 12 + 44:])
    assert dev.Srs("BN128", p).power == 3


def _damaged():
    b = GOLDEN.read_bytes()
    sec = {s: (o, z) for s, o, z in _sections(b)}
    drop = lambda sid: b[:8] + struct.pack("<I", 5) + b[12:sec[sid][0]] + b[sec[sid][0] + 12 + sec[sid][1]:]
    o4, z4 = sec[4]
    short4 = b[:o4] + struct.pack("<IQ", 4, z4 - 64) + b[o4 + 12:o4 + 12 + z4 - 64] + b[o4 + 12 + z4:]
    o1 = sec[1][0] + 12
    return [("magic", b"ptbu" + b[4:], "Invalid magic number"),
            ("version", b[:4] + struct.pack("<I", 2) + b[8:], "Unsupported version"),
            ("modulus", b[:o1 + 4] + bytes([b[o1 + 4] ^ 2]) + b[o1 + 5:], "prime is not the base field"),
            ("scalar modulus", b[:o1 + 4] + R_BN.to_bytes(32, "little") + b[o1 + 36:], "prime is not the base field"),
            ("missing tauG2", drop(3), r"section 3 \(tauG2\) is missing"),
            ("missing betaG2", drop(6), r"section 6 \(betaG2\) is missing"),
            ("short alphaTauG1", short4, r"section 4 \(alphaTauG1\) has 448 bytes, power 3 needs 512"),
            ("power against sizes", b[:o1 + 36] + struct.pack("<I", 4) + b[o1 + 40:], r"section 2 \(tauG1\) has 960 bytes, power 4 needs 1984"),
            ("truncated", b[:-9], "truncated file"),
            ("truncated head", b[:10], "truncated file")]


@pytest.mark.parametrize("what,data,msg", _damaged(), ids=[d[0] for d in _damaged()])
def test_each_damage_is_refused_by_name(zk, dev, tmp_path, what, data, msg):
    p = tmp_path / "bad.ptau"
    p.write_bytes(data)
    with pytest.raises(zk.ZkError, match=msg):
        dev.Srs("BN128", p)
    assert not zk.lib().zk_srs_open(b"BN128", str(p).encode())
    assert zk.lib().zk_last_error().decode().startswith("ptau")


def test_other_curve_unknown_curve_missing_file(zk, dev, tmp_path):
    with pytest.raises(zk.ZkError, match="prime is not the base field of BLS12381"):
        dev.Srs("BLS12381", GOLDEN)
    with pytest.raises(zk.ZkError, match="unknown curve"):
        dev.Srs("BN254", GOLDEN)
    with pytest.raises(zk.ZkError, match="cannot open"):
        dev.Srs("BN128", tmp_path / "nothing.ptau")


def test_setup_refuses_a_file_too_small_before_any_device_work(zk, dev, orc):
    import groth16 as G
    g = G.Groth16Oracle(orc, "bn254")
    r1cs, _ = G.synthetic_r1cs(g.r, 12, seed=5)
    assert g.circuit(r1cs)["log_m"] == 4
    s = dev.Srs("BN128", GOLDEN)
    with pytest.raises(zk.ZkError, match="the file has power 3.*need power 4"):
        dev.keygen("BN128", g.r1cs_bytes(r1cs), srs=s, check_srs=False)
    with pytest.raises(zk.ZkError, match="exclude each other"):
        dev.keygen("BN128", g.r1cs_bytes(r1cs), [3, 5, 7, 1, 1], srs=s)
    s2 = dev.Srs("BN128", GOLDEN)
    rb = (ROOT / "tests" / "golden" / "groth16" / "mycircuit_bls12381.r1cs").read_bytes()
    with pytest.raises(zk.ZkError, match="prime is not the scalar field"):
        dev.keygen("BN128", rb, srs=s2, check_srs=False)
    with pytest.raises(zk.ZkError, match="opened for BN128"):
        dev.keygen("BLS12381", rb, srs=s2, check_srs=False)
