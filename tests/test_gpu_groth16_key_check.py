"""groth16_key_check on the device (csrc/groth16.hip, csrc/key_check_impl.hip.h; through the C ABI) against the plain-Python checker
(tests/key_check_ref.py): keys made on the device with a fixed trapdoor, untouched and with one corruption at a time; every finding
identical, with the fixed seed and with the operating system's randomness in every case.  The oracle's pairing costs 1.2 s (BN254) to
1.9 s (BLS12-381) a pair, so only the tiny key has every b pair tied by it (test_every_b_pair_by_the_oracle); for the 65 pairs of the
small keys the reference ties those at the indices a case touches (and 0, the middle, the last).  The keys large enough for their b sums
to leave the small-n path of the sums (4096 points), one per curve, have none of their points classified by the reference -- they are
the device's own and the small keys cover every class."""
import importlib, json, pathlib, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
import key_check_cases as KC  # noqa: E402
import key_check_ref as K  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
TD = [0x1234567, 0x89abcdef1, 0x2468ace, 0x13579bdf, 0xfedcba987]
SEED = bytes(range(32))


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


@pytest.fixture(scope="module")
def g16(orc):
    return {cv: G.Groth16Oracle(orc, cv) for cv, _ in CURVES}


@pytest.fixture(scope="module")
def keys(dev, g16):
    """(tag, size) -> (r1cs bytes, key bytes, verification_key.json); tiny: 3 or 4 b pairs; small: 100 products, 64 < wires < 200; large: 4420 b pairs"""
    out = {}
    for cv, tag in CURVES:
        g = g16[cv]
        r1cs, _ = KC.circuit(g.r, 100)
        assert 64 < r1cs["n_wires"] < 200
        rb = g.r1cs_bytes(r1cs)
        out[(tag, "small")] = (rb,) + tuple(dev.keygen(tag, rb, TD))
        for size, n_mul in (("tiny", 4), ("large", 7000)):
            rb = g.r1cs_bytes(KC.circuit(g.r, n_mul)[0])
            out[(tag, size)] = (rb,) + tuple(dev.keygen(tag, rb, TD))
    return out


def b_idx(tag, pb, extra=()):
    n = KC.layout(tag, pb)["b_g1"][0]
    return sorted({0, n // 2, n - 1, *[i % n for i in extra]})


def agree(dev, tag, rb, pb, vk=None, extra=(), sections=None, seeds=(SEED, None)):
    want = K.report(tag, rb, pb, vk_json=vk, b_indices=b_idx(tag, pb, extra), classify_sections=sections)
    for sd in seeds:
        got = dev.key_check(tag, rb, pb, vk_json=vk, seed=sd)
        assert got == want, (got, want)
    return want


@pytest.mark.parametrize("cv,tag", CURVES)
def test_untouched_key_is_clean_and_reports_agree(dev, keys, cv, tag):
    rb, pb, vk = keys[(tag, "small")]
    rep = agree(dev, tag, rb, pb, vk)
    assert rep["findings"] == [] and not any(rep["counts"].values()) and rep["skipped"] == []
    assert dev.key_check(tag, rb, pb, seed=SEED) == dev.key_check(tag, rb, pb, seed=SEED)      # a fixed seed: the same report twice


@pytest.mark.parametrize("cv,tag", CURVES)
def test_sizes_truncation_other_circuit_other_curve(dev, zk, g16, keys, cv, tag):
    rb, pb, vk = keys[(tag, "small")]
    rep = agree(dev, tag, rb, KC.truncate(tag, pb, "h", 3))
    assert [(f["kind"], f["section"]) for f in rep["findings"]] == [("size", "h")]
    rep = agree(dev, tag, rb, KC.truncate(tag, pb, "b_g2", 1))
    assert rep["skipped"] and rep["skipped"][0]["section"] == "b"
    other, _ = KC.circuit(g16[cv].r, 60, seed=9)
    rep = agree(dev, tag, g16[cv].r1cs_bytes(other), pb)
    assert rep["counts"]["size"] >= 3
    if tag == "BN128":                                                      # the other curve's size: the existing parse error
        rb2, _, _ = keys[("BLS12381", "small")]
        with pytest.raises(ValueError) as e: K.report("BLS12381", rb2, pb)
        with pytest.raises(zk.ZkError, match=str(e.value)): dev.key_check("BLS12381", rb2, pb)
        assert str(e.value).startswith("proving key: ")


@pytest.mark.parametrize("cv,tag", CURVES)
def test_damaged_points(dev, keys, cv, tag):
    rb, pb, vk = keys[(tag, "small")]
    for section, i in (("h", 0), ("l", -1), ("a", 63), ("a", 64)):
        rep = agree(dev, tag, rb, KC.off_curve(tag, pb, section, i))
        n = KC.layout(tag, pb)[section][0]
        assert rep["findings"] == [dict(kind="not_on_curve", section=section, n_points=1, first_index=i % n)]
    both = KC.off_curve(tag, KC.off_curve(tag, pb, "a", 64), "a", 63)
    assert agree(dev, tag, rb, both)["findings"] == [dict(kind="not_on_curve", section="a", n_points=2, first_index=63)]
    rep = agree(dev, tag, rb, KC.set_point(tag, pb, "b_g2", 5, KC.twist_point_outside_subgroup(tag)))
    assert rep["findings"] == [dict(kind="not_in_subgroup", section="b_g2", n_points=1, first_index=5)] and rep["skipped"][0]["section"] == "b"
    rep = agree(dev, tag, rb, KC.set_point(tag, pb, "l", 7, None))
    assert rep["findings"] == [dict(kind="infinity", section="l", n_points=1, first_index=7)]
    # two classes whose sections come in the other order than their kinds: the report lists kind by kind, infinity (in l) before not_on_curve (in h)
    rep = agree(dev, tag, rb, KC.set_point(tag, KC.off_curve(tag, pb, "h", 2), "l", 7, None))
    assert rep["findings"] == [dict(kind="infinity", section="l", n_points=1, first_index=7), dict(kind="not_on_curve", section="h", n_points=1, first_index=2)]
    three = KC.set_point(tag, KC.set_point(tag, KC.off_curve(tag, pb, "ic", 0), "a", 9, None), "b_g2", 5, KC.twist_point_outside_subgroup(tag))
    rep = agree(dev, tag, rb, three)
    assert [(f["kind"], f["section"]) for f in rep["findings"]] == [("infinity", "a"), ("not_on_curve", "ic"), ("not_in_subgroup", "b_g2")]
    q = K.CURVES[tag].q
    c = list(KC.get_point(tag, pb, "ic", 1)); c[0] = q + 5                 # (x + q would reach the encoding's flag bits on BN254)
    rep = agree(dev, tag, rb, KC.set_point(tag, pb, "ic", 1, c))
    assert rep["findings"][0] == dict(kind="coordinate_range", section="ic", n_points=1, first_index=1)


@pytest.mark.parametrize("cv,tag", CURVES)
def test_b_halves_that_disagree(dev, keys, cv, tag):
    rb, pb, vk = keys[(tag, "small")]
    n = KC.layout(tag, pb)["b_g1"][0]
    for idx in ([0], [n - 1], [n // 2], [n // 2, n - 1]):
        bad = pb
        for i in idx: bad = KC.doubled(tag, bad, "b_g1", i)
        rep = agree(dev, tag, rb, bad)
        assert rep["findings"] == [dict(kind="g1_g2_mismatch", section="b", first_index=idx[0])]


@pytest.mark.parametrize("cv,tag", CURVES)
def test_every_b_pair_by_the_oracle(dev, keys, cv, tag):
    """the tiny key: the reference ties EVERY b pair with the oracle's pairing (b_indices=None) and finds the first failing index itself"""
    rb, pb, vk = keys[(tag, "tiny")]
    n = KC.layout(tag, pb)["b_g1"][0]
    assert 2 <= n <= 6                                                      # few enough to pair every one of them
    want = K.report(tag, rb, KC.doubled(tag, pb, "b_g1", n - 1))
    assert want["findings"] == [dict(kind="g1_g2_mismatch", section="b", first_index=n - 1)]
    for sd in (SEED, None):
        assert dev.key_check(tag, rb, KC.doubled(tag, pb, "b_g1", n - 1), seed=sd) == want


@pytest.mark.parametrize("damaged", [False, True])
@pytest.mark.parametrize("cv,tag", CURVES)
def test_b_sums_beyond_the_small_path_of_the_sums(dev, keys, cv, tag, damaged):
    """4420 b points: the sums split their scalars (msm_impl.hip.h, n >= 4096) and the bisection runs a dozen steps.  The
    reference classifies no point of this key (minutes in Python; the device made them, and the small keys carry every class) and ties
    the pairs at the two indices the case touches."""
    rb, pb, vk = keys[(tag, "large")]
    n = KC.layout(tag, pb)["b_g1"][0]
    assert n >= 4096
    idx = [n // 2, n - 1]
    bad = pb
    if damaged:
        for i in idx: bad = KC.doubled(tag, bad, "b_g1", i)
    want = K.report(tag, rb, bad, b_indices=idx, classify_sections=())
    assert want["findings"] == ([dict(kind="g1_g2_mismatch", section="b", first_index=idx[0])] if damaged else [])
    for sd in (SEED, None):
        assert dev.key_check(tag, rb, bad, seed=sd) == want


@pytest.mark.parametrize("cv,tag", CURVES)
def test_beta_and_the_verification_key_file(dev, keys, cv, tag):
    rb, pb, vk = keys[(tag, "small")]
    rep = agree(dev, tag, rb, KC.doubled(tag, pb, "beta_g1", 0), vk)
    assert [(f["kind"], f.get("section"), f.get("field")) for f in rep["findings"]] == [("g1_g2_mismatch", "beta", None), ("vk_mismatch", None, "vk_beta_1")]
    js = json.loads(vk)
    other = json.loads(keys[(tag, "small")][2]); C = K.CURVES[tag]
    d2 = C.coords(C.mul(C.gen[1], 77), 1)
    other["vk_delta_2"] = {"x": [str(d2[0]), str(d2[1])], "y": [str(d2[2]), str(d2[3])]}
    rep = agree(dev, tag, rb, pb, json.dumps(other))
    assert rep["findings"] == [dict(kind="vk_mismatch", field="vk_delta_2")] and js["vk_delta_2"] != other["vk_delta_2"]
    lines = [dev.key_check_line(f) for f in rep["findings"]]
    assert lines == [K.finding_line(f) for f in rep["findings"]]
