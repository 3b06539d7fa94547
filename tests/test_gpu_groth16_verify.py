"""Groth16 verification on the device (csrc/pairing.hip; eigen_zkvm_amd.groth16.Groth16VerifyingKey): the reference's own proof
fixture, keys and proofs made here on both curves, the oracle's verdicts, every malformed-input verdict, batches, handles.
`zkit groth16_verify`, groth16/src/api.rs:302-341."""
import importlib, json, pathlib, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
import pairing as PG  # noqa: E402
import pairing_constants as pc  # noqa: E402

GOLD = ROOT / "tests" / "golden" / "groth16"
CURVES = (("bn254", "BN128", pc.BN254, PG.BN254), ("bls12_381", "BLS12381", pc.BLS12_381, PG.BLS12_381))
TD = [0x1234567, 0x2345678, 0x3456789, 0x456789a, 0x56789ab]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


@pytest.fixture(scope="module")
def made(orc, dev):
    """per (curve, n_pub): a key made on the device for a synthetic circuit, one proof of it, its public inputs"""
    out = {}
    for cv, tag, C, O in CURVES:
        g = G.Groth16Oracle(orc, cv)
        for n_pub in (1, 3):
            r1cs, wit = G.synthetic_r1cs(g.r, 6, n_pub=n_pub, seed=7 + n_pub)
            rb = g.r1cs_bytes(r1cs)
            pb, vk_json = dev.keygen(tag, rb, TD)
            S = dev.Groth16Setup(tag, rb, pb)
            js, pts = S.prove(g.fr_array(wit), r=12345, s=67890)
            S.free()
            out[(tag, n_pub)] = dict(vk_json=vk_json, proof=js, pts=np.array(pts), pub=[int(w) for w in wit[1:1 + n_pub]])
    return out


def _vk_ints(vk_json):
    v = json.loads(vk_json); i = lambda s: int(s, 0)
    g1 = lambda p: (i(p["x"]), i(p["y"])); g2 = lambda p: (i(p["x"][0]), i(p["x"][1]), i(p["y"][0]), i(p["y"][1]))
    return dict(alpha_g1=g1(v["vk_alpha_1"]), beta_g2=g2(v["vk_beta_2"]), gamma_g2=g2(v["vk_gamma_2"]), delta_g2=g2(v["vk_delta_2"]), ic=[g1(p) for p in v["IC"]])


def _proof_ints(js):
    return dict(a=(int(js["pi_a"]["x"]), int(js["pi_a"]["y"])), c=(int(js["pi_c"]["x"]), int(js["pi_c"]["y"])),
                b=tuple(int(js["pi_b"][k][c]) for k in "xy" for c in (0, 1)))


def test_reference_fixture_accepted_and_rejected(dev):
    """independent of the oracle: the reference's own proof.json, verification_key.json and public input [33]"""
    C = pc.BN254
    vk = dev.Groth16VerifyingKey("BN128", (GOLD / "verification_key.json").read_text())
    proof = json.loads((GOLD / "proof.json").read_text())
    assert vk.n_public == 1
    assert vk.verify(proof, [33]) == dev.ACCEPTED
    assert vk.verify(json.dumps(proof), '["33"]') == dev.ACCEPTED and vk.verify(proof, ["0x21"]) == dev.ACCEPTED
    assert vk.verify(proof, [34]) == dev.REJECTED
    cg = C.g1_add((int(proof["pi_c"]["x"]), int(proof["pi_c"]["y"])), C.g1)              # C + G: on the curve, wrong
    bad = dict(proof, pi_c={"x": str(cg[0]), "y": str(cg[1])})
    assert vk.verify(bad, [33]) == dev.REJECTED


def test_bls12_381_setup_prove_verify_through_the_public_api(dev):
    rb = (GOLD / "mycircuit_bls12381.r1cs").read_bytes()
    pb, vk_json = dev.keygen("BLS12381", rb)
    S = dev.Groth16Setup("BLS12381", rb, pb)
    w33 = np.array([[1, 0, 0, 0], [33, 0, 0, 0], [3, 0, 0, 0], [11, 0, 0, 0]], dtype=np.uint64)   # ONE, out c, in a, in b: 3 x 11
    js, pts = S.prove(w33)
    vk = dev.Groth16VerifyingKey("BLS12381", vk_json)
    assert vk.verify(js, [33]) == dev.ACCEPTED and vk.verify(js, [34]) == dev.REJECTED
    # witness.wtns itself holds 1121 x 10000 = 11210000 (its header names BN254's scalar field; the values are the circuit's on either curve)
    w = dev.wtns_values((GOLD / "witness.wtns").read_bytes(), "BN128")
    js2, _ = S.prove(w)
    assert vk.verify(js2, [11210000]) == dev.ACCEPTED and vk.verify(js2, [33]) == dev.REJECTED and vk.verify(js, [11210000]) == dev.REJECTED
    assert list(vk.verify_batch(pts, [[33]])) == [dev.ACCEPTED]                          # prover to verifier without JSON


@pytest.mark.parametrize("n_pub", [1, 3])
@pytest.mark.parametrize("cv,tag,C,O", CURVES, ids=[c[1] for c in CURVES])
def test_verdict_equals_oracle(dev, made, cv, tag, C, O, n_pub):
    m = made[(tag, n_pub)]
    vk = dev.Groth16VerifyingKey(tag, m["vk_json"])
    wrong = ([0, C.r - 1, 5] * 2)[:n_pub]                                                # the input values 0 and r - 1
    assert vk.verify(m["proof"], m["pub"]) == dev.ACCEPTED and vk.verify(m["proof"], wrong) == dev.REJECTED
    if n_pub == 3:                                                                       # the oracle costs seconds: once per curve
        assert O.groth16_verify(_vk_ints(m["vk_json"]), _proof_ints(m["proof"]), m["pub"]) is True
        assert O.groth16_verify(_vk_ints(m["vk_json"]), _proof_ints(m["proof"]), wrong) is False


def _f2sqrt(C, a):
    """a square root in Fq2 for q = 3 mod 4 (Adj-Rodriguez-Henriquez), or None"""
    q = C.q
    a1 = C.f2pow(a, (q - 3) // 4); x0 = C.f2mul(a1, a); alpha = C.f2mul(a1, x0)
    x = C.f2mul((0, 1), x0) if alpha == (q - 1, 0) else C.f2mul(C.f2pow(C.f2add((1, 0), alpha), (q - 1) // 2), x0)
    return x if C.f2mul(x, x) == (a[0] % q, a[1] % q) else None


@pytest.mark.parametrize("cv,tag,C,O", CURVES, ids=[c[1] for c in CURVES])
def test_malformed_inputs(dev, made, cv, tag, C, O):
    m = made[(tag, 1)]
    vk = dev.Groth16VerifyingKey(tag, m["vk_json"])
    p = m["proof"]
    assert vk.verify(p, [C.r]) == dev.INPUT_NOT_CANONICAL and vk.verify(p, [C.r + m["pub"][0]]) == dev.INPUT_NOT_CANONICAL
    assert vk.verify(p, [2**256]) == dev.INPUT_NOT_CANONICAL
    assert vk.verify(p, []) == dev.INPUT_COUNT and vk.verify(p, m["pub"] + [1]) == dev.INPUT_COUNT
    off = dict(p, pi_a={"x": p["pi_a"]["x"], "y": str((int(p["pi_a"]["y"]) + 1) % C.q)})
    assert vk.verify(off, m["pub"]) == dev.NOT_ON_CURVE
    offb = dict(p, pi_b={"x": p["pi_b"]["x"], "y": [p["pi_b"]["y"][1], p["pi_b"]["y"][0]]})
    assert vk.verify(offb, m["pub"]) == dev.NOT_ON_CURVE
    x = (1, 0)                                                                           # a twist point outside the subgroup
    while True:
        x = (x[0] + 1, 1)
        y = _f2sqrt(C, C.f2add(C.f2mul(x, C.f2mul(x, x)), C.bt))
        if y is not None and C.g2_mul(C.r, (x, y)) is not None: break
    out = dict(p, pi_b={"x": [str(x[0]), str(x[1])], "y": [str(y[0]), str(y[1])]})
    assert vk.verify(out, m["pub"]) == dev.NOT_IN_SUBGROUP
    inf = dict(p, pi_c={"x": "0", "y": "1"})                                             # infinity contributes 1: well formed, wrong
    assert vk.verify(inf, m["pub"]) == dev.REJECTED
    out = vk.verify_batch(np.concatenate([m["pts"], m["pts"]]), [m["pub"], m["pub"] + [2]])
    assert list(out) == [dev.ACCEPTED, dev.INPUT_COUNT]


@pytest.mark.parametrize("cv,tag,C,O", CURVES, ids=[c[1] for c in CURVES])
def test_batch_of_11_and_handles(dev, made, cv, tag, C, O):
    m, m3 = made[(tag, 1)], made[(tag, 3)]
    vk = dev.Groth16VerifyingKey(tag, m["vk_json"])
    pubs = [list(m["pub"]) for _ in range(11)]
    for i in (0, 5, 10): pubs[i] = [(m["pub"][0] + 1 + i) % C.r]
    want = [0 if i in (0, 5, 10) else 1 for i in range(11)]
    pts = np.concatenate([m["pts"]] * 11)
    assert list(vk.verify_batch(pts, pubs)) == want
    vk3 = dev.Groth16VerifyingKey(tag, m3["vk_json"])                                    # a second handle alive
    assert list(vk3.verify_batch(m3["pts"], [m3["pub"]])) == [1]
    assert list(vk.verify_batch(pts, pubs)) == want and list(vk3.verify_batch(m["pts"], [m3["pub"]])) == [0]
    vk3.free()
    assert list(vk.verify_batch(m["pts"], [m["pub"]])) == [1]


def test_key_errors(dev, made):
    from eigen_zkvm_amd import ZkError
    v = json.loads(made[("BN128", 1)]["vk_json"])
    v["vk_gamma_2"]["x"][0] = str(int(v["vk_gamma_2"]["x"][0]) + 1)
    with pytest.raises(ZkError, match="not on its curve"):
        dev.Groth16VerifyingKey("BN128", json.dumps(v))
    with pytest.raises(ZkError, match="curve"):
        dev.Groth16VerifyingKey("BLS12381", made[("BN128", 1)]["vk_json"])
