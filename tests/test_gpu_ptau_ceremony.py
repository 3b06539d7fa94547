"""A powers-of-tau ceremony on the device (csrc/groth16_ceremony.hip.h, ceremony_impl.hip.h, ceremony_host.h; zk_srs_new, zk_srs_contribute,
zk_srs_verify): with the factors given, a contributed file is byte for byte the file tools/make_test_ptau.py builds for the product
trapdoor (points are affine and canonical: no tolerance), its transcript passes the library's check and the plain-Python one
(tests/ceremony_ref.py), and every corruption is reported with its contribution and factor.
Sizes: ZK_SRS_CHUNK=64 in a child process cuts powers 7 and 8 (255 and 511 tauG1 points) into chunks that end inside a 64-lane launch and
inside the 256-lane way out; powers 0 and 3 are the file without a tauG1[1] and the golden file's size."""
import importlib, json, os, pathlib, random, struct, subprocess, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import groth16 as G  # noqa: E402
import make_test_ptau as MP  # noqa: E402
import ceremony_ref as CR  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
SEED = bytes(range(32))
GOLDEN = ROOT / "tests" / "golden" / "groth16" / "test_bn128_power3.ptau"


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def g16(orc):
    return {tag: G.Groth16Oracle(orc, cv) for cv, tag in CURVES}


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


def _secrets(tag, seed, n=1):
    rng = random.Random(seed)
    out = [tuple(rng.randrange(1, CR.R[tag]) for _ in range(3)) for _ in range(n)]
    return out[0] if n == 1 else out


def _body(b):
    """sections 2..6 of a container, by id"""
    return {sid: b[o:o + size] for sid, o, size in CR.sections(b) if 2 <= sid <= 6}


def _findings(rep):
    return sorted(((f["kind"], f.get("contribution"), f.get("which")) for f in rep["findings"]), key=lambda t: (t[0], t[1] or 0, t[2] or ""))


def _verify(dev, tag, path):
    srs = dev.Srs(tag, path)
    try:
        return srs.verify(seed=SEED, max_findings=64)
    finally:
        srs.free()


def _ref_findings(g16, tag, b):
    b1 = CR.B1[tag]
    power = struct.unpack_from("<I", CR.section(b, 1), 4 + b1 // 2)[0]
    body = _body(b)
    cv = CR.Curve(g16[tag], tag)
    gen = g16[tag].g1.generator()
    gen1 = cv._bytes(gen)
    imgs = (body[2][b1:2 * b1] if power else None, body[4][:b1], body[5][:b1])
    return CR.check(cv, CR.parse(CR.section(b, CR.SECTION), b1), b1 // 2, power, gen1, imgs)


def test_contribution_to_the_golden_file_is_the_product_trapdoor(zk, g16, dev, tmp_path):
    td = json.loads((GOLDEN.parent / (GOLDEN.name + ".json")).read_text())
    tau, alpha, beta = int(td["tau"]), int(td["alpha"]), int(td["beta"])
    t, a, b = _secrets("BN128", 1)
    r = CR.R["BN128"]
    srs = dev.Srs("BN128", GOLDEN)
    assert srs.transcript_count() == -1
    srs.contribute(tmp_path / "c.ptau", secrets=(t, a, b)); srs.free()
    got = (tmp_path / "c.ptau").read_bytes()
    assert _body(got) == _body(MP.build_ptau(zk, "BN128", 3, tau * t % r, alpha * a % r, beta * b % r))
    rep = _verify(dev, "BN128", tmp_path / "c.ptau")
    # the golden file has no transcript: the record proves the factors over the file's own images, a chain that does not start at G1,
    # and that is what the check says -- about every factor, and nothing else
    assert not rep["file"]["findings"] and rep["contributions"] == 1
    assert _findings(rep) == [("pok_invalid", 1, w) for w in ("alpha", "beta", "tau")] == _ref_findings(g16, "BN128", got)


CHILD = """
import importlib, sys
sys.path.insert(0, %r)
import eigen_zkvm_amd as zk
zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")
tag, power, new, out = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
dev.srs_new(tag, power, new)
srs = dev.Srs(tag, new)
assert srs.power == power and srs.transcript_count() == 0
srs.contribute(out, secrets=tuple(int(v) for v in sys.argv[5:8]))
"""


@pytest.mark.parametrize("power", (0, 3, 7, 8))
@pytest.mark.parametrize("cv,tag", CURVES)
def test_contribution_to_a_new_file_in_small_chunks(zk, g16, dev, tmp_path, cv, tag, power):
    t, a, b = _secrets(tag, 10 + power)
    env = dict(os.environ, ZK_SRS_CHUNK="64")
    subprocess.run([sys.executable, "-c", CHILD % str(ROOT), tag, str(power), str(tmp_path / "new.ptau"), str(tmp_path / "c.ptau"), str(t), str(a), str(b)],
                   check=True, env=env, timeout=120)
    got = (tmp_path / "c.ptau").read_bytes()
    assert _body(got) == _body(MP.build_ptau(zk, tag, power, t, a, b))
    rep = _verify(dev, tag, tmp_path / "c.ptau")
    assert rep["contributions"] == 1 and not rep["findings"] and not rep["file"]["findings"], rep
    assert _ref_findings(g16, tag, got) == []


@pytest.fixture(scope="module")
def chain(zk, dev, tmp_path_factory):
    """per curve: new -> two contributions -> a beacon at power 3; (path, bytes, the product trapdoor)"""
    out = {}
    d = tmp_path_factory.mktemp("chain")
    for _, tag in CURVES:
        r = CR.R[tag]
        p = [d / ("%s_%d.ptau" % (tag, i)) for i in range(4)]
        dev.srs_new(tag, 3, p[0])
        td = [1, 1, 1]
        beacon = (bytes(range(7, 39)), 3)
        steps = _secrets(tag, 77, 2) + [tuple(CR.beacon_scalars(*beacon))]
        for i, s in enumerate(steps):
            srs = dev.Srs(tag, p[i])
            if i < 2: srs.contribute(p[i + 1], secrets=s)
            else: srs.contribute(p[i + 1], beacon=beacon)
            srs.free()
            td = [x * y % r for x, y in zip(td, s)]
        out[tag] = (p[3], p[3].read_bytes(), td)
    return out


@pytest.mark.parametrize("cv,tag", CURVES)
def test_two_contributions_and_a_beacon_equal_the_product_trapdoor(zk, g16, dev, chain, cv, tag):
    path, b, td = chain[tag]
    assert _body(b) == _body(MP.build_ptau(zk, tag, 3, *td))
    rep = _verify(dev, tag, path)
    assert rep["contributions"] == 3 and not rep["findings"] and not rep["file"]["findings"], rep
    assert _ref_findings(g16, tag, b) == []
    recs = CR.parse(CR.section(b, CR.SECTION), CR.B1[tag])
    assert [r["kind"] for r in recs] == [0, 0, 1] and recs[2]["iter_log"] == 3 and recs[2]["seed"] == bytes(range(7, 39))
    # the key from the contributed file is the trapdoor key for (tau, alpha, beta, 1, 1): a transcript does not disturb the setup
    g = g16[tag]
    r1cs, _ = G.synthetic_r1cs(g.r, 4, seed=5)
    rb = g.r1cs_bytes(r1cs)
    assert g.circuit(r1cs)["log_m"] <= 3
    srs = dev.Srs(tag, path)
    pb, vk = dev.keygen(tag, rb, srs=srs)
    srs.free()
    assert (pb, vk) == dev.keygen(tag, rb, td + [1, 1])


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def _tampered(tag, b, what):
    b1 = CR.B1[tag]
    recs = CR.parse(CR.section(b, CR.SECTION), b1)
    rehash = True
    if what == "z": recs[2]["z"][1] = _flip(recs[2]["z"][1], 5)
    elif what == "z_earlier": recs[1]["z"][1] = _flip(recs[1]["z"][1], 5)
    elif what == "R": recs[2]["R"][0] = _flip(recs[2]["R"][0], 9)
    elif what == "image": recs[2]["img"][2] = _flip(recs[2]["img"][2], 3)
    elif what == "seed": recs[2]["seed"] = _flip(recs[2]["seed"], 0)
    elif what == "hash": recs[1]["hash"] = _flip(recs[1]["hash"], 31); rehash = False
    elif what == "removed": del recs[1]; rehash = False
    elif what == "swapped": recs[0], recs[1] = recs[1], recs[0]; rehash = False
    if rehash: CR.rehash(recs, b1 // 2, 3)
    return CR.replace_section(b, CR.SECTION, CR.serialize(recs))


# A forger who edits a field recomputes the hashes behind it (CR.rehash), so the edits to fields are looked for in the last record, where
# nothing follows; "z_earlier" shows what the chain does to the records that do follow: their challenges hang on the hash that moved.
EXPECT = {
    "z": [("pok_invalid", 3, "alpha")],
    "z_earlier": [("pok_invalid", 2, "alpha")] + [("pok_invalid", 3, w) for w in ("alpha", "beta", "tau")],
    "R": [("pok_invalid", 3, "tau")],
    # the last image is also what the beacon recomputes and what the file must hold
    "image": [("beacon_mismatch", 3, "beta"), ("image_mismatch", 3, "beta"), ("pok_invalid", 3, "beta")],
    "seed": [("beacon_mismatch", 3, w) for w in ("alpha", "beta", "tau")],
    "hash": [("chain_hash", 2, None)],
    # the beacon moves up: its chain hash, its challenges and its bases are the first record's, not the second's
    "removed": [("beacon_mismatch", 2, w) for w in ("alpha", "beta", "tau")] + [("chain_hash", 2, None)] + [("pok_invalid", 2, w) for w in ("alpha", "beta", "tau")],
    "swapped": None,
}


@pytest.mark.parametrize("what", sorted(EXPECT))
@pytest.mark.parametrize("cv,tag", CURVES)
def test_a_tampered_transcript_is_reported_where_it_was_tampered_with(g16, dev, chain, tmp_path, cv, tag, what):
    _, b, _ = chain[tag]
    bad = _tampered(tag, b, what)
    (tmp_path / "bad.ptau").write_bytes(bad)
    rep = _verify(dev, tag, tmp_path / "bad.ptau")
    got = _findings(rep)
    assert not rep["file"]["findings"]
    assert got == _ref_findings(g16, tag, bad), rep["findings"]
    if EXPECT[what] is not None:
        assert got == EXPECT[what]
    else:                                                                  # the chain parts at the first record and every proof behind it loses its base
        assert all(("chain_hash", i, None) in got for i in (1, 2, 3))
        assert all(("pok_invalid", i, w) in got for i in (1, 2, 3) for w in CR.WHICH)


@pytest.mark.parametrize("cv,tag", CURVES)
def test_a_replaced_point_arrives_under_file_and_a_reset_file_under_image_mismatch(zk, g16, dev, chain, tmp_path, cv, tag):
    _, b, td = chain[tag]
    b1 = CR.B1[tag]
    o2 = [o for sid, o, _ in CR.sections(b) if sid == 2][0]
    bad = b[:o2 + 3 * b1] + b[o2 + 2 * b1:o2 + 3 * b1] + b[o2 + 4 * b1:]                # tauG1[3] := tauG1[2]
    (tmp_path / "p.ptau").write_bytes(bad)
    rep = _verify(dev, tag, tmp_path / "p.ptau")
    assert not rep["findings"] and [(f["kind"], f["section"]) for f in rep["file"]["findings"]] == [("not_powers", "tauG1")]
    # the reset attack: a fresh file of a trapdoor its maker knows, dressed in the honest file's transcript
    known = MP.build_ptau(zk, tag, 3, 5, 7, 11)
    forged = known[:8] + struct.pack("<I", 7) + known[12:]
    t = CR.section(b, CR.SECTION)
    forged += struct.pack("<IQ", CR.SECTION, len(t)) + t
    (tmp_path / "f.ptau").write_bytes(forged)
    rep = _verify(dev, tag, tmp_path / "f.ptau")
    assert not rep["file"]["findings"]
    assert _findings(rep) == [("image_mismatch", 3, w) for w in ("alpha", "beta", "tau")] == _ref_findings(g16, tag, forged)
    # and the file make_test_ptau writes has no transcript at all
    (tmp_path / "k.ptau").write_bytes(known)
    rep = _verify(dev, tag, tmp_path / "k.ptau")
    assert _findings(rep) == [("no_transcript", None, None)] and not rep["file"]["findings"]
    assert dev.srs_verify_lines(rep) == ["ptau transcript: the file has no transcript of contributions (section 64)"]
