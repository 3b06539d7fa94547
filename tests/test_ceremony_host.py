"""The host side of the powers-of-tau ceremony, no GPU: zk_srs_new's file read back through zk_srs_open, the transcript's layout and hash
chain pinned by a record of known factors and nonces (tests/ceremony_ref.py builds it on the oracle's CPU curve), the library's parser
(csrc/ceremony_host.h) against that record and against truncated and mis-versioned sections, and the command line's arguments."""
import importlib, pathlib, struct, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import groth16 as G  # noqa: E402
import make_test_ptau as MP  # noqa: E402
import ceremony_ref as CR  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
# the chain hash of the record test_reference_record_has_the_pinned_hash_chain builds, per curve
PINNED = {"BN128": "22ffd8594df01fa9039e7f751457418e80e56953b0af54188364725eb1c5e537", "BLS12381": "b830f3fb8397dbb13cadb7f5701cce9ff7d9ff94d87355fb7ce2977917a21c3e"}
H0 = {"BN128": "38989ebc90fcea292f43f0bcbc29b5b1a650b8dfa98a6aa163c395eace0c68b6", "BLS12381": "bce2ede74d23e0a5950de26bc3ebd8382af3599b3a36af4ace7286c7ce2152af"}


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


@pytest.fixture(scope="module")
def g16(orc):
    return {tag: G.Groth16Oracle(orc, cv) for cv, tag in CURVES}


def _gens(g):
    b = lambda p: bytes(memoryview(p.astype("<u8")))
    return b(g.g1.generator()), b(g.g2.generator())


@pytest.mark.parametrize("power", (0, 3))
@pytest.mark.parametrize("cv,tag", CURVES)
def test_new_file_is_all_generators_with_an_empty_transcript(zk, dev, g16, tmp_path, cv, tag, power):
    p = tmp_path / "new.ptau"
    dev.srs_new(tag, power, p)
    g1, g2 = _gens(g16[tag])
    n = 1 << power
    want = MP.container(tag, power, {2: g1 * (2 * n - 1), 3: g2 * n, 4: g1 * n, 5: g1 * n, 6: g2})
    want = want[:8] + struct.pack("<I", 7) + want[12:] + struct.pack("<IQII", CR.SECTION, 8, 1, 0)
    assert p.read_bytes() == want
    srs = dev.Srs(tag, p)
    assert (srs.power, srs.ceremony_power, srs.transcript_count()) == (power, power, 0)
    srs.free()
    with pytest.raises(zk.ZkError, match="out of range"):
        dev.srs_new(tag, 29, tmp_path / "big.ptau")
    with pytest.raises(zk.ZkError, match="unknown curve"):
        dev.srs_new("BN254", 1, tmp_path / "x.ptau")


def _record(g16, tag):
    cv = CR.Curve(g16[tag], tag)
    g1, _ = _gens(g16[tag])
    h0 = CR.chain_start(CR.B1[tag] // 2, 3)
    return h0, g1, CR.make_record(cv, h0, [g1] * 3, (0x1234567, 0x2345678, 0x3456789), (0x1111, 0x2222, 0x3333))


@pytest.mark.parametrize("cv,tag", CURVES)
def test_reference_record_has_the_pinned_hash_chain(zk, dev, g16, tmp_path, cv, tag):
    h0, g1, rec = _record(g16, tag)
    b1 = CR.B1[tag]
    assert h0.hex() == H0[tag] and rec["hash"].hex() == PINNED[tag]
    assert len(rec["body"]) + 32 == CR.rec_bytes(b1) == 168 + 6 * b1
    cvr = CR.Curve(g16[tag], tag)
    assert CR.check(cvr, [rec], b1 // 2, 3, g1) == []
    # the Schnorr equation by hand for one proof: [z] B = R + [c] Q
    c = CR.challenge(h0, 1, g1, rec["img"][1], rec["R"][1])
    z = int.from_bytes(rec["z"][1], "little")
    assert z == (0x2222 + c * 0x2345678) % CR.R[tag] and c < 2**128
    assert cvr.mul(g1, z) == cvr.lin2(rec["R"][1], 1, rec["img"][1], c)
    # the round trip of the layout, and the library's parser on the same bytes
    payload = CR.serialize([rec])
    back = CR.parse(payload, b1)[0]
    assert all(back[k] == rec[k] for k in ("kind", "iter_log", "seed", "img", "R", "z", "hash", "body"))
    new = tmp_path / "new.ptau"
    dev.srs_new(tag, 3, new)
    one = tmp_path / "one.ptau"
    one.write_bytes(CR.replace_section(new.read_bytes(), CR.SECTION, payload))
    srs = dev.Srs(tag, one)
    assert srs.transcript_count() == 1
    srs.free()
    assert CR.beacon_scalars(bytes(32), 0)[0] == int.from_bytes(CR.sha(CR.sha(bytes(32)), b"\0"), "little") % 2**253


BAD = {
    "short": (lambda p: p[:6], "truncated section"),
    "version": (lambda p: struct.pack("<I", 2) + p[4:], "Unsupported version"),
    "cut": (lambda p: p[:-1], "truncated section"),
    "count": (lambda p: p[:4] + struct.pack("<I", 2) + p[8:], "truncated section"),
    "tail": (lambda p: p + b"\0", "behind the last record"),
    "kind": (lambda p: p[:8] + struct.pack("<I", 2) + p[12:], "unknown kind"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_parser_refuses_truncated_and_misversioned_transcripts(zk, dev, g16, tmp_path, what):
    tag = "BN128"
    _, _, rec = _record(g16, tag)
    edit, text = BAD[what]
    payload = edit(CR.serialize([rec]))
    with pytest.raises(CR.TranscriptError, match=text):
        CR.parse(payload, CR.B1[tag])
    new = tmp_path / "new.ptau"
    dev.srs_new(tag, 3, new)
    bad = tmp_path / "bad.ptau"
    bad.write_bytes(CR.replace_section(new.read_bytes(), CR.SECTION, payload))
    srs = dev.Srs(tag, bad)                                                # the sections the setup reads are whole: the file opens
    with pytest.raises(zk.ZkError, match=text):
        srs.transcript_count()
    srs.free()


def test_a_file_cut_inside_the_transcript_does_not_open(zk, dev, tmp_path):
    new = tmp_path / "new.ptau"
    dev.srs_new("BN128", 1, new)
    cut = tmp_path / "cut.ptau"
    cut.write_bytes(new.read_bytes()[:-3])
    with pytest.raises(zk.ZkError, match="truncated"):
        dev.Srs("BN128", cut)


def test_command_line_arguments(tmp_path):
    import zkgpu_ceremony as ZC
    ap = ZC.build_parser()
    a = ap.parse_args(["ptau_new", "-c", "BLS12381", "--power", "12", "-o", "a.ptau"])
    assert (a.curve, a.power, a.out, a.fn) == ("BLS12381", 12, "a.ptau", ZC.ptau_new)
    a = ap.parse_args(["ptau_contribute", "-c", "BN128", "-i", "a.ptau", "-o", "b.ptau", "--check"])
    assert (a.curve, a.inp, a.out, a.check, a.fn) == ("BN128", "a.ptau", "b.ptau", True, ZC.ptau_contribute)
    a = ap.parse_args(["ptau_beacon", "-i", "b.ptau", "-o", "c.ptau", "--seed", "00" * 32, "--iter-log", "10"])
    assert (a.curve, a.seed, a.iter_log, a.fn) == (None, "00" * 32, 10, ZC.ptau_beacon)
    a = ap.parse_args(["ptau_verify", "-c", "BN128", "c.ptau", "--report", "r.json"])
    assert (a.file, a.report, a.fn) == ("c.ptau", "r.json", ZC.ptau_verify)
    a = ap.parse_args(["key_contribute", "-c", "BN128", "-p", "a.key", "-o", "b.key", "--transcript", "t.bin", "-v", "vk.json"])
    assert (a.pk_file, a.out_file, a.transcript, a.vk_file, a.fn) == ("a.key", "b.key", "t.bin", "vk.json", ZC.key_contribute)
    a = ap.parse_args(["key_verify", "-c", "BLS12381", "--initial", "a.key", "--final", "b.key", "--transcript", "t.bin"])
    assert (a.curve, a.initial, a.final, a.fn) == ("BLS12381", "a.key", "b.key", ZC.key_verify)
    for argv in (["key_contribute", "-c", "BN128", "-p", "a.key", "-o", "b.key", "--transcript", "t", "--delta", "5"], ["key_verify", "-c", "BN128", "--initial", "a"],
                 ["ptau_new", "--power", "3", "-o", "x"], ["ptau_contribute", "-i", "a", "-o", "b", "--tau", "5"], ["ptau_beacon", "-i", "a", "-o", "b"]):
        with pytest.raises(SystemExit):                                    # no curve for a new file; no flag takes a secret; a beacon needs its seed
            ap.parse_args(argv)
    # without -c the curve is the one the file's header names
    import importlib
    import eigen_zkvm_amd  # noqa: F401
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    for tag in ("BN128", "BLS12381"):
        dev.srs_new(tag, 0, tmp_path / "n.ptau")
        assert ZC.curve_of_file(tmp_path / "n.ptau") == tag
    assert ZC.main(["ptau_new", "-c", "BN128", "--power", "2", "-o", str(tmp_path / "m.ptau")]) == 0
    assert (tmp_path / "m.ptau").stat().st_size > 0
