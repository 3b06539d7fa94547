"""Contributions to a key's delta with proofs of knowledge (csrc/groth16_ceremony.hip.h; zk_groth16_params_contribute_pok,
zk_groth16_key_transcript_check): a chain of three passes, the key still is its circuit's over the powers-of-tau file, and the attack the
transcript exists for -- the delta = 1 key scaled by a known k, presented as the successor of the current key -- passes the transcript-less
contribution_check and fails here.  The transcript's layout and hashes are restated below with hashlib."""
import hashlib, importlib, pathlib, random, struct, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
import make_test_ptau as MP  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
SEED = bytes(range(32))
HEAD = 48


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


def _recs(tag, t):
    """(header, [records]) of a key transcript; a record: key hash | delta_g1 | R | z | chain hash"""
    b1 = MP.CURVES[tag]["n8"] * 2
    rb = 96 + 2 * b1
    assert t[:4] == b"zkgk" and struct.unpack_from("<III", t, 4) == (1, b1 // 2, (len(t) - HEAD) // rb) and (len(t) - HEAD) % rb == 0
    return t[:HEAD], [t[HEAD + i * rb:HEAD + (i + 1) * rb] for i in range((len(t) - HEAD) // rb)]


def _join(head, recs):
    return head[:12] + struct.pack("<I", len(recs)) + head[16:] + b"".join(recs)


def _rehash(tag, head, recs):
    """the chain recomputed over the records as they stand"""
    prev = hashlib.sha256(b"zkgpu key transcript v1" + struct.pack("<I", MP.CURVES[tag]["n8"]) + head[16:48]).digest()
    out = []
    for r in recs:
        prev = hashlib.sha256(b"zkgpu key rec v1" + prev + r[:-32]).digest()
        out.append(r[:-32] + prev)
    return out


@pytest.fixture(scope="module")
def chain(zk, dev, orc, tmp_path_factory):
    """per curve: the delta = 1 key of a small circuit over a file of known trapdoor, three contributions with known deltas"""
    out = {}
    d = tmp_path_factory.mktemp("keys")
    for cv, tag in CURVES:
        g = G.Groth16Oracle(orc, cv)
        rng = random.Random(41)
        r1cs, _ = G.synthetic_r1cs(g.r, 6, seed=5)
        rb = g.r1cs_bytes(r1cs)
        p = d / (tag + ".ptau")
        p.write_bytes(MP.build_ptau(zk, tag, g.circuit(r1cs)["log_m"], *[rng.randrange(1, g.r) for _ in range(3)]))
        srs = dev.Srs(tag, p)
        keys = [dev.keygen(tag, rb, srs=srs)[0]]
        deltas = [rng.randrange(1, g.r) for _ in range(3)]
        t = b""
        for dl in deltas:
            k, t = dev.contribute_pok(tag, keys[-1], t, delta=dl)
            keys.append(k)
        out[tag] = dict(g=g, rb=rb, srs=srs, keys=keys, t=t, deltas=deltas)
    yield out
    for v in out.values():
        v["srs"].free()


def _kinds(rep):
    return sorted((f["kind"], f.get("contribution")) for f in rep["findings"])


@pytest.mark.parametrize("cv,tag", CURVES)
def test_three_contributions_pass_and_the_key_is_still_its_circuits(dev, chain, cv, tag):
    c = chain[tag]
    rep = dev.key_transcript_check(tag, c["keys"][0], c["keys"][3], c["t"], seed=SEED)
    assert rep["contributions"] == 3 and not rep["findings"] and not rep["keys"]["findings"], rep
    assert dev.key_transcript_lines(rep) == []
    # the same keys as the plain contribution gives for the same deltas: the proof is beside the key, not in it
    assert c["keys"][1] == dev.contribute(tag, c["keys"][0], delta=c["deltas"][0])
    head, recs = _recs(tag, c["t"])
    assert head[16:] == hashlib.sha256(c["keys"][0]).digest() and [r[:32] for r in recs] == [hashlib.sha256(k).digest() for k in c["keys"][1:]]
    assert _rehash(tag, head, recs) == recs
    rep = dev.key_check_srs(tag, c["rb"], c["keys"][3], c["srs"], seed=SEED)
    assert not rep["findings"] and not rep["skipped"], rep
    # a transcript continues only from the key it ends at
    with pytest.raises(Exception, match="does not end at this key"):
        dev.contribute_pok(tag, c["keys"][1], c["t"], delta=5)


@pytest.mark.parametrize("cv,tag", CURVES)
def test_the_reset_attack_passes_the_ratio_check_and_fails_the_transcript(dev, chain, cv, tag):
    c = chain[tag]
    k = 0x1234567
    # the delta = 1 key scaled by a known k, with an honest proof of knowledge of k -- over the initial delta_g1, the only base k fits
    forged, t_forged = dev.contribute_pok(tag, c["keys"][0], b"", delta=k)
    assert forged == dev.contribute(tag, c["keys"][0], delta=k)
    # the hole: as a successor of the current key it passes the check that has no transcript
    assert not dev.contribution_check(tag, c["keys"][2], forged, seed=SEED)["findings"]
    # with a transcript the forger has to continue the chain of two records, and the proof does not fit the current delta_g1
    head, recs = _recs(tag, c["t"])
    graft = _rehash(tag, head, recs[:2] + _recs(tag, t_forged)[1])
    rep = dev.key_transcript_check(tag, c["keys"][0], forged, _join(head, graft), seed=SEED)
    assert _kinds(rep) == [("pok_invalid", 3)] and not rep["keys"]["findings"], rep
    assert dev.key_transcript_lines(rep) == ["key transcript: contribution 3: no valid proof of knowledge of the ratio of the two deltas"]


@pytest.mark.parametrize("cv,tag", CURVES)
def test_tampered_transcripts_and_wrong_keys(dev, chain, cv, tag):
    c = chain[tag]
    head, recs = _recs(tag, c["t"])
    b1 = MP.CURVES[tag]["n8"] * 2
    flip = lambda r, at: r[:at] + bytes([r[at] ^ 1]) + r[at + 1:]
    check = lambda a, b, t: _kinds(dev.key_transcript_check(tag, a, b, t, seed=SEED))
    k0, k1, k2, k3 = c["keys"]
    z = _rehash(tag, head, recs[:2] + [flip(recs[2], 32 + 2 * b1 + 3)])
    assert check(k0, k3, _join(head, z)) == [("pok_invalid", 3)]
    assert check(k0, k3, _join(head, [recs[0], flip(recs[1], len(recs[1]) - 1), recs[2]])) == [("chain_hash", 2)]
    # another initial key: its hash is not the header's, and the first proof's base is not its delta_g1
    assert check(k1, k3, c["t"]) == [("initial_key_mismatch", None), ("pok_invalid", 1)]
    assert check(k0, k2, c["t"]) == [("final_key_mismatch", None)]
    assert check(k0, k2, _join(head, recs[:2])) == []                      # the chain is whole at every length
    with pytest.raises(Exception, match="truncated"):
        dev.key_transcript_check(tag, k0, k3, c["t"][:-1])
    with pytest.raises(Exception, match="Unsupported version"):
        dev.key_transcript_check(tag, k0, k3, c["t"][:4] + struct.pack("<I", 2) + c["t"][8:])
