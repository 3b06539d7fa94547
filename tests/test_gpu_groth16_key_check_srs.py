"""groth16_key_check --ptau on the device (csrc/key_check_srs.hip.h, key_check_srs_impl.hip.h; through the C ABI): is this key a key for
this circuit over this powers-of-tau file?  Files come from tools/make_test_ptau.py with known tau, alpha, beta, so the yardstick is
exact: tests/key_check_srs_ref.py builds the CPU oracle's key for the trapdoor and compares point by point; the device, which sees no
trapdoor, must name the same sections, first indices and wires.  The seed is fixed.

n_mul = 6: the smallest domain; 40: a wire no row mentions (infinity in l) and an aux wire without A-density (the a map is not the
identity); 300: 512 rows, so the row kernel crosses a 256-lane block and has padding rows."""
import importlib, pathlib, random, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
import make_test_ptau as MP  # noqa: E402
import key_check_cases as KC  # noqa: E402
import key_check_srs_ref as KS  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
SEED = bytes(range(32))
CLEAN = dict(query_mismatch=0, vk_mismatch=0)


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def g16(orc):
    return {cv: G.Groth16Oracle(orc, cv) for cv, _ in CURVES}


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


@pytest.fixture(scope="module")
def ptau(zk, dev, g16, tmp_path_factory):
    """(tag, power, which) -> (path, bytes, (tau, alpha, beta)); which = 1: another tau and alpha, the same beta.  Made once each"""
    made = {}
    d = tmp_path_factory.mktemp("ptau")

    def get(tag, power, which=0):
        if (tag, power, which) not in made:
            rng = random.Random(7000 + power + (100 if tag == "BN128" else 0))
            td = tuple(rng.randrange(1, MP.CURVES[tag]["r"]) for _ in range(3))
            if which: td = (td[0] + 1, td[1] + 1, td[2])
            b = MP.build_ptau(zk, tag, power, *td)
            p = d / ("%s_%d_%d.ptau" % (tag, power, which))
            p.write_bytes(b)
            made[(tag, power, which)] = (p, b, td)
        return made[(tag, power, which)]
    return get


@pytest.fixture(scope="module")
def contributed(dev, g16, ptau):
    """per curve: n_mul = 40, the key from the file after two contributions -> (r1cs, r1cs bytes, key bytes, delta, log_m)"""
    out = {}
    for cv, tag in CURVES:
        g = g16[cv]; rng = random.Random(31)
        r1cs, _ = G.synthetic_r1cs(g.r, 40, seed=5)
        rb = g.r1cs_bytes(r1cs)
        log_m = g.circuit(r1cs)["log_m"]
        srs = dev.Srs(tag, ptau(tag, log_m)[0])
        pb, _ = dev.keygen(tag, rb, srs=srs, check_srs=False)
        srs.free()
        d1, d2 = rng.randrange(2, g.r), rng.randrange(2, g.r)
        out[tag] = (r1cs, rb, dev.contribute(tag, dev.contribute(tag, pb, d1), d2), d1 * d2 % g.r, log_m)
    return out


def check(dev, tag, rb, pb, path, **kw):
    srs = dev.Srs(tag, path)
    try:
        return dev.key_check_srs(tag, rb, pb, srs, seed=SEED, **kw)
    finally:
        srs.free()


def clean(rep):
    return rep["findings"] == [] and rep["skipped"] == [] and rep["counts"] == CLEAN


# ---- 1. accepted keys ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
@pytest.mark.parametrize("n_mul", [6, 40, 300])
def test_keys_of_the_circuit_over_the_file_are_accepted(g16, dev, ptau, cv, tag, n_mul):
    g = g16[cv]; rng = random.Random(n_mul)
    r1cs, _ = G.synthetic_r1cs(g.r, n_mul, seed=5)
    rb = g.r1cs_bytes(r1cs)
    cir = g.circuit(r1cs)
    log_m = cir["log_m"]
    if n_mul == 300: assert 256 < len(cir["rows"]) < 512
    for power in (log_m, log_m + 2):                                        # (a) the key from the file
        path, _, td = ptau(tag, power)
        srs = dev.Srs(tag, path)
        pb, _ = dev.keygen(tag, rb, srs=srs, check_srs=False)
        rep = dev.key_check_srs(tag, rb, pb, srs, seed=SEED)
        srs.free()
        assert clean(rep), rep
        assert (rep["curve"], rep["power"], rep["domain_log"], rep["n_wires"], rep["n_public"]) == (tag, power, log_m, r1cs["n_wires"], cir["num_inputs"] - 1)
        assert rep["checked"]["row_sums"] == 3 and rep["checked"]["transforms"] == 6 and rep["checked"]["pairs"] == 6
    if n_mul == 40:
        assert KS.split_key(g, pb)["l"][-1][0] & 0x40                      # the wire no row mentions: infinity in l
    path, _, td = ptau(tag, log_m + 2)                                      # (b) after two contributions, against the larger file
    pb2 = dev.contribute(tag, dev.contribute(tag, pb, rng.randrange(2, g.r)), rng.randrange(2, g.r))
    assert pb2 != pb and clean(check(dev, tag, rb, pb2, path))
    gamma, delta = rng.randrange(2, g.r), rng.randrange(2, g.r)             # (c) any gamma and delta: the key of a trapdoor with the file's tau, alpha, beta
    pb3, _ = dev.keygen(tag, rb, list(td) + [gamma, delta])
    assert clean(check(dev, tag, rb, pb3, path))
    assert check(dev, tag, rb, pb3, path) == check(dev, tag, rb, pb3, path)  # a fixed seed: the same report twice


def test_the_reference_circuit_fixture(g16, dev, ptau):
    g = g16["bls12_381"]
    rb = (ROOT / "tests" / "golden" / "groth16" / "mycircuit_bls12381.r1cs").read_bytes()
    _prime, r1cs = G.read_r1cs(rb)
    path, _, _td = ptau("BLS12381", g.circuit(r1cs)["log_m"])
    srs = dev.Srs("BLS12381", path)
    pb, _ = dev.keygen("BLS12381", rb, srs=srs)
    srs.free()
    assert clean(check(dev, "BLS12381", rb, dev.contribute("BLS12381", pb, 12345), path))
    rep = check(dev, "BLS12381", rb, dev.contribute("BLS12381", pb, 12345), path, max_findings=0)
    assert clean(rep)


# ---- 2. what groth16_key_check cannot see -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
def test_b_altered_consistently_in_both_groups(g16, dev, ptau, cv, tag):
    """b_g1[k] and b_g2[k] doubled: the two halves still agree, so the key's own check is silent; against circuit and file both are wrong"""
    g = g16[cv]
    for r1cs in (KC.circuit(g.r, 40)[0], G.synthetic_r1cs(g.r, 40, seed=5)[0]):   # without and with the wire no row mentions
        rb = g.r1cs_bytes(r1cs)
        path, _, td = ptau(tag, g.circuit(r1cs)["log_m"])
        srs = dev.Srs(tag, path)
        pb, _ = dev.keygen(tag, rb, srs=srs, check_srs=False)
        srs.free()
        n = KS.layout(g, pb)["b_g1"][0]
        k = n // 2
        bad = KC.doubled(tag, KC.doubled(tag, pb, "b_g1", k), "b_g2", k)
        assert bad != pb and len(bad) == len(pb)
        own = dev.key_check(tag, rb, bad, seed=SEED)
        if r1cs["n_wires"] == KC.circuit(g.r, 40)[0]["n_wires"]:
            assert own["findings"] == [] and not any(own["counts"].values())
        assert own == dev.key_check(tag, rb, pb, seed=SEED)                 # nothing the untouched key does not have
        rep = check(dev, tag, rb, bad, path)
        wire = KS.wires(g, r1cs)["b_g1"][k]
        assert rep["findings"] == [dict(kind="query_mismatch", section="b_g1", first_index=k, wire=wire),
                                   dict(kind="query_mismatch", section="b_g2", first_index=k, wire=wire)]
        assert rep["counts"] == dict(query_mismatch=2, vk_mismatch=0) and rep["skipped"] == []
        want = KS.report(g, r1cs, bad, td + (1, 1))
        assert (rep["findings"], rep["counts"]) == (want["findings"], want["counts"])
        assert clean(check(dev, tag, rb, pb, path))


# ---- 3. every section, against the yardstick ------------------------------------------------------------------------------------------
def _alpha_of(g, file_bytes):
    """alphaTauG1[0] of a file as a key encodes it"""
    n = int.from_bytes(file_bytes[8:12], "little")
    o = 12
    for _ in range(n):
        sid, sz = int.from_bytes(file_bytes[o:o + 4], "little"), int.from_bytes(file_bytes[o + 4:o + 12], "little")
        if sid == 4: return g.enc_point(g.g1, np.frombuffer(file_bytes[o + 12:o + 12 + 16 * g.nl], dtype="<u8").astype(np.uint64))
        o += 12 + sz
    raise AssertionError("no section 4")


SECTION_CASES = ["a first", "a middle", "a last", "l first", "l middle", "l last", "h first", "h middle", "h last", "ic", "other circuit", "other file", "alpha of the other file"]


@pytest.mark.parametrize("cv,tag", CURVES)
@pytest.mark.parametrize("case", SECTION_CASES)
def test_one_section_at_a_time_against_the_yardstick(g16, dev, ptau, contributed, cv, tag, case):
    """corruptions by points that are on the curve and in the subgroup: the point classes stay silent"""
    g = g16[cv]
    r1cs, rb, pb, delta, log_m = contributed[tag]
    path, _, td = ptau(tag, log_m)
    L = KS.layout(g, pb)
    key, against, trapdoor = pb, path, td + (1, delta)
    what, _, where = case.partition(" ")
    if what in ("a", "l"):
        n = L[what][0] - (1 if what == "l" else 0)                           # l: the last entry is the infinity of the unused wire
        k = {"first": 0, "middle": n // 2, "last": L[what][0] - 1}[where]
        src = (k + 1) % n
        assert KS.get(g, pb, what, src) != KS.get(g, pb, what, k) and not KS.get(g, pb, what, src)[0] & 0x40
        key = KS.put(g, pb, what, k, KS.get(g, pb, what, src))
    elif what == "h":
        n = L["h"][0]
        i = {"first": 0, "middle": n // 2, "last": n - 2}[where]
        key = KS.swap(g, pb, "h", i, i + 1)
    elif what == "ic":
        key = KS.put(g, pb, "ic", 1, KS.get(g, pb, "ic", 2))
    elif case == "other circuit":                                           # one coefficient of one constraint changed
        cons = list(r1cs["constraints"])
        a, b, c = cons[10]
        cons[10] = ([(a[0][0], (a[0][1] + 1) % g.r)] + list(a[1:]), b, c)
        other = dict(r1cs, constraints=cons)
        srs = dev.Srs(tag, path)
        key, _ = dev.keygen(tag, g.r1cs_bytes(other), srs=srs, check_srs=False)
        srs.free()
        key = dev.contribute(tag, key, delta)
        assert len(key) == len(pb)
    elif case == "other file":
        against, _, td2 = ptau(tag, log_m, 1)
        trapdoor = td2 + (1, delta)
    else:
        key = KS.put(g, pb, "alpha_g1", 0, _alpha_of(g, ptau(tag, log_m, 1)[1]))
    assert key != pb or against != path
    rep = check(dev, tag, rb, key, against)
    want = KS.report(g, r1cs, key, trapdoor)
    assert want["findings"], case
    assert (rep["findings"], rep["counts"]) == (want["findings"], want["counts"]), (case, rep, want)
    assert rep["skipped"] == []
    for f in rep["findings"]:
        assert dev.key_check_srs_line(f).startswith(f["kind"])
    if what in ("a", "l", "h"):
        assert [f["section"] for f in rep["findings"]] == [what]
    if case == "alpha of the other file":
        assert rep["findings"] == [dict(kind="vk_mismatch", field="alpha_g1")]
    if case == "other file":
        assert [f["section"] for f in rep["findings"] if f["kind"] == "query_mismatch"] == list(KS.SECTIONS) and rep["counts"]["vk_mismatch"] == 1


# ---- 4. skips and errors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
def test_skipped_sections_and_refusals(zk, g16, dev, ptau, contributed, cv, tag):
    g = g16[cv]
    r1cs, rb, pb, delta, log_m = contributed[tag]
    path, _, td = ptau(tag, log_m)
    n_l = KS.layout(g, pb)["l"][0]
    moved = KS.put(g, pb, "l", 2, KS.get(g, pb, "l", 3))
    want = KS.report(g, r1cs, moved, td + (1, delta))["findings"]
    assert want == [dict(kind="query_mismatch", section="l", first_index=2, wire=g.circuit(r1cs)["num_inputs"] + 2)] and n_l > 4
    # a point off the curve: its section is not compared, the others are
    rep = check(dev, tag, rb, KC.off_curve(tag, moved, "a", 3), path)
    assert rep["skipped"] == [dict(check="query_mismatch", section="a", reason="an invalid point")]
    assert rep["findings"] == want and rep["counts"] == dict(query_mismatch=1, vk_mismatch=0)
    # a wrong length
    rep = check(dev, tag, rb, KC.truncate(tag, moved, "h", 1), path)
    assert rep["skipped"] == [dict(check="query_mismatch", section="h", reason="a wrong length")]
    assert rep["findings"] == want
    # delta_g2 off its curve: what is paired against it cannot be compared
    rep = check(dev, tag, rb, KC.off_curve(tag, pb, "delta_g2", 0), path)
    assert [s["section"] for s in rep["skipped"]] == ["l", "h"] and rep["findings"] == []
    with pytest.raises(zk.ZkError, match=r"the file has power %d, the circuit's \d+ rows need power %d" % (log_m - 1, log_m)):
        check(dev, tag, rb, pb, ptau(tag, log_m - 1)[0])
    other = "BLS12381" if tag == "BN128" else "BN128"
    with pytest.raises(zk.ZkError, match="the powers-of-tau file was opened for " + other):
        srs = dev.Srs(other, ptau(other, 3)[0])
        try:
            dev.key_check_srs(tag, rb, pb, srs, seed=SEED)
        finally:
            srs.free()
    with pytest.raises(zk.ZkError, match="truncated|trailing"):
        check(dev, tag, rb, pb[:-3], path)
