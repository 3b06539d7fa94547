"""A Groth16 key from a powers-of-tau file (csrc/groth16_srs.hip.h over csrc/ecntt.hip), contributions to it and the two checks, both
curves.  The yardstick is exact: a file built from known tau, alpha, beta (tools/make_test_ptau.py) must give, byte for byte, the key the
CPU reference's generate_parameters restatement and zk_groth16_keygen_new give for the trapdoor (tau, alpha, beta, 1, 1), and after a
contribution delta' the key for (tau, alpha, beta, 1, delta')."""
import importlib, json, pathlib, random, struct, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
import make_test_ptau as MP  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
SEED = bytes(range(32))


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
    """(tag, power) -> (path, bytes, (tau, alpha, beta)); one file per curve and power, made once"""
    made = {}
    d = tmp_path_factory.mktemp("ptau")

    def get(tag, power):
        if (tag, power) not in made:
            rng = random.Random(9000 + power + (100 if tag == "BN128" else 0))
            td = tuple(rng.randrange(1, MP.CURVES[tag]["r"]) for _ in range(3))
            b = MP.build_ptau(zk, tag, power, *td)
            p = d / ("%s_%d.ptau" % (tag, power))
            p.write_bytes(b)
            made[(tag, power)] = (p, b, td)
        return made[(tag, power)]
    return get


def _sections(b):
    """{id: (payload offset, size)}"""
    n = struct.unpack_from("<I", b, 8)[0]
    o, out = 12, {}
    for _ in range(n):
        sid, sz = struct.unpack_from("<IQ", b, o)
        out[sid] = (o + 12, sz); o += 12 + sz
    return out


def _queries(g, pb):
    """the byte ranges of a Parameters file: {name: (count, offset, point bytes)} and the offsets of delta_g1, delta_g2"""
    vk, o = g.vk_from_bytes(pb)
    s1, s2 = 16 * g.nl, 32 * g.nl
    q = {"delta_g1": (1, 2 * s1 + 2 * s2, s1), "delta_g2": (1, 3 * s1 + 2 * s2, s2)}
    for name, sz in (("h", s1), ("l", s1), ("a", s1), ("b_g1", s1), ("b_g2", s2)):
        n = struct.unpack(">I", pb[o:o + 4])[0]; o += 4
        q[name] = (n, o, sz); o += n * sz
    assert o == len(pb)
    return q


def _put(pb, q, name, i, data):
    n, o, sz = q[name]
    return pb[:o + i * sz] + data + pb[o + i * sz + len(data):]


def _get(pb, q, name, i, count=1):
    n, o, sz = q[name]
    return pb[o + i * sz:o + (i + count) * sz]


# ---- 1. the key, byte for byte ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
@pytest.mark.parametrize("n_mul", [6, 40, 300])
def test_key_from_file_matches_oracle_and_trapdoor_keygen(g16, dev, ptau, cv, tag, n_mul):
    g = g16[cv]
    r1cs, _wit = G.synthetic_r1cs(g.r, n_mul, seed=5)
    rb = g.r1cs_bytes(r1cs)
    log_m = g.circuit(r1cs)["log_m"]
    for power in (log_m, log_m + 2):
        path, _, (tau, alpha, beta) = ptau(tag, power)
        td = [tau, alpha, beta, 1, 1]
        srs = dev.Srs(tag, path)
        assert srs.power == power
        pb, vk = dev.keygen(tag, rb, srs=srs)
        _, vk_hex = dev.keygen(tag, rb, srs=srs, to_hex=True, check_srs=False)
        srs.free()
        P = g.setup(r1cs, *td)
        if n_mul == 40:
            assert sum(p is None for p in P["l"]) == 1                      # the unused wire: infinity comes out of the column sums
        exp = g.params_bytes(P)
        assert len(pb) == len(exp) and pb == exp
        pb_td, vk_td = dev.keygen(tag, rb, td)
        assert pb == pb_td and vk == vk_td
        assert vk_hex == dev.keygen(tag, rb, td, to_hex=True)[1]


@pytest.mark.parametrize("cv,tag", CURVES)
def test_key_from_file_at_2_12_rows_device_against_device(g16, dev, ptau, cv, tag):
    import groth16_bench as GB
    g = g16[cv]
    rb, _wit, _ni, _nw = GB.make_circuit(g.r, 12)
    path, _, (tau, alpha, beta) = ptau(tag, 12)
    srs = dev.Srs(tag, path)
    ms = []
    pb, vk = dev.keygen(tag, rb, srs=srs, check_srs=False, timing=ms)
    srs.free()
    assert len(ms) == 5 and all(v >= 0 for v in ms)
    pb_td, vk_td = dev.keygen(tag, rb, [tau, alpha, beta, 1, 1])
    assert pb == pb_td and vk == vk_td


# ---- 2. the reference's own circuit: file -> key -> contribution -> proof -> verifier -------------------------------------------------------
def test_reference_r1cs_fixture_from_file_to_accepted_proof(zk, g16, dev, ptau):
    g = g16["bls12_381"]; rng = random.Random(4)
    rb = (ROOT / "tests" / "golden" / "groth16" / "mycircuit_bls12381.r1cs").read_bytes()
    _prime, r1cs = G.read_r1cs(rb)
    log_m = g.circuit(r1cs)["log_m"]
    path, _, (tau, alpha, beta) = ptau("BLS12381", log_m)
    srs = dev.Srs("BLS12381", path)
    pb0, _ = dev.keygen("BLS12381", rb, srs=srs)
    srs.free()
    delta = rng.randrange(1, g.r)
    pb = dev.contribute("BLS12381", pb0, delta)
    P = g.setup(r1cs, tau, alpha, beta, 1, delta)
    assert pb == g.params_bytes(P)
    wit = [1, 33, 3, 11]                                                    # ONE, out c, in a, in b: 3 x 11
    rr, ss = rng.randrange(g.r), rng.randrange(g.r)
    S = dev.Groth16Setup("BLS12381", rb, pb)
    js, pts = S.prove(g.fr_array(wit), rr, ss)
    S.free()
    exp = g.expected_proof(P, wit, rr, ss); nl = g.nl
    assert np.array_equal(pts[:2 * nl], exp["a"]) and np.array_equal(pts[2 * nl:6 * nl], exp["b"]) and np.array_equal(pts[6 * nl:], exp["c"])
    # the verification key of the contributed key: the head of its bytes, rendered as the command-line tool renders it
    import zkgpu_prove
    vk = dev.Groth16VerifyingKey("BLS12381", zkgpu_prove._vk_json_of_key("BLS12381", pb))
    assert vk.verify(js, [33]) == dev.ACCEPTED
    assert vk.verify(js, [34]) == dev.REJECTED
    vk.free()


# ---- 3. contributions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
def test_contributions_match_the_oracle_key_for_the_product_of_deltas(g16, dev, ptau, cv, tag):
    g = g16[cv]; rng = random.Random(12)
    r1cs, _ = G.synthetic_r1cs(g.r, 40, seed=5)                             # has an unused wire: infinity in l goes through the product
    rb = g.r1cs_bytes(r1cs)
    path, _, (tau, alpha, beta) = ptau(tag, g.circuit(r1cs)["log_m"])
    srs = dev.Srs(tag, path)
    pb0, _ = dev.keygen(tag, rb, srs=srs)
    srs.free()
    d1, d2 = rng.randrange(1, g.r), rng.randrange(1, g.r)
    keep = bytes(pb0)
    pb1 = dev.contribute(tag, pb0, d1)
    assert pb0 == keep                                                     # the input buffer is unchanged
    assert pb1 == g.params_bytes(g.setup(r1cs, tau, alpha, beta, 1, d1))
    pb2 = dev.contribute(tag, pb1, d2)
    assert pb2 == g.params_bytes(g.setup(r1cs, tau, alpha, beta, 1, d1 * d2 % g.r))
    assert dev.contribute(tag, pb0, 1) == pb0
    a, b = dev.contribute(tag, pb0), dev.contribute(tag, pb0)              # delta from the operating system: another one every time
    assert a != b and a != pb0 and len(a) == len(pb0)
    assert not dev.contribution_check(tag, pb0, a, seed=SEED)["findings"]
    for bad in (0, g.r):
        with pytest.raises(Exception, match="non-zero canonical"):
            dev.contribute(tag, pb0, bad)
    with pytest.raises(Exception, match="truncated|trailing"):
        dev.contribute(tag, pb0[:-3], d1)


# ---- 4. the check of the file -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
def test_srs_check_names_the_damaged_section_and_the_setup_refuses(zk, g16, dev, ptau, tmp_path, cv, tag):
    g = g16[cv]
    r1cs, _ = G.synthetic_r1cs(g.r, 6, seed=5)
    rb = g.r1cs_bytes(r1cs)
    power = g.circuit(r1cs)["log_m"]
    path, b, _td = ptau(tag, power)
    srs = dev.Srs(tag, path)
    rep = srs.check(seed=SEED)
    srs.free()
    n = 1 << power
    assert rep["findings"] == [] and rep["skipped"] == [] and not any(rep["counts"].values())
    assert rep["checked"]["g1_points"] == 4 * n - 1 and rep["checked"]["g2_points"] == n + 1 and rep["power"] == power
    sec = _sections(b)
    s1, s2 = 16 * g.nl, 32 * g.nl
    pt = lambda sid, i, sz: b[sec[sid][0] + i * sz:sec[sid][0] + (i + 1) * sz]
    put = lambda sid, i, data: b[:sec[sid][0] + i * len(data)] + data + b[sec[sid][0] + (i + 1) * len(data):]
    beta_g2 = np.frombuffer(pt(6, 0, s2), dtype="<u8")
    twice = dev.mul_scalar(zk.DevArray.from_host(beta_g2.astype(np.uint64)), 2, tag, "g2").to_host().astype("<u8").tobytes()
    x = bytearray(pt(3, 1, s2)); x[0] ^= 1
    cases = [("swapped", put(2, 2, pt(2, 5, s1))[:sec[2][0] + 5 * s1] + pt(2, 2, s1) + b[sec[2][0] + 6 * s1:], "not_powers", "tauG1"),
             ("replaced", put(4, 3, pt(2, 4, s1)), "not_powers", "alphaTauG1"),
             ("doubled", put(6, 0, twice), "beta_mismatch", "betaG2"),
             ("off the curve", put(3, 1, bytes(x)), "not_on_curve", "tauG2")]
    for what, data, kind, section in cases:
        assert len(data) == len(b) and data != b, what
        p = tmp_path / "bad.ptau"
        p.write_bytes(data)
        srs = dev.Srs(tag, p)
        rep = srs.check(seed=SEED)
        assert {"kind": kind, "section": section}.items() <= rep["findings"][0].items(), (what, rep)
        assert all(f["section"] == section for f in rep["findings"]), (what, rep)
        assert dev.srs_check_line(rep["findings"][0]).startswith(kind)
        with pytest.raises(zk.ZkError, match="fails its check: " + kind):
            dev.keygen(tag, rb, srs=srs)
        srs.free()


# ---- 5. the check of a contribution ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
def test_contribution_check_reports_what_was_changed(g16, dev, ptau, cv, tag):
    g = g16[cv]; rng = random.Random(21)
    r1cs, _ = G.synthetic_r1cs(g.r, 40, seed=5)
    rb = g.r1cs_bytes(r1cs)
    path, _, _td = ptau(tag, g.circuit(r1cs)["log_m"])
    srs = dev.Srs(tag, path)
    base, _ = dev.keygen(tag, rb, srs=srs, check_srs=False)
    srs.free()
    k1, k2 = dev.contribute(tag, base, rng.randrange(2, g.r)), dev.contribute(tag, base, rng.randrange(2, g.r))
    q = _queries(g, base)
    for old, new in ((base, k1), (k1, dev.contribute(tag, k1, rng.randrange(2, g.r))), (base, base)):
        rep = dev.contribution_check(tag, old, new, seed=SEED)
        assert rep["findings"] == [] and rep["skipped"] == [] and not any(rep["counts"].values())
    nl_, nh_ = q["l"][0], q["h"][0]
    cases = [("l by another scalar", _put(k1, q, "l", 0, _get(k2, q, "l", 0, nl_)), "not_scaled", "l"),
             ("h swapped", _put(_put(k1, q, "h", 0, _get(k1, q, "h", 1)), q, "h", 1, _get(k1, q, "h", 0)), "not_scaled", "h"),
             ("a altered", _put(k1, q, "a", 0, _get(k1, q, "a", 1)), "changed", "a"),
             ("two deltas", _put(k1, q, "delta_g2", 0, _get(k2, q, "delta_g2", 0)), "delta_mismatch", "delta")]
    assert nl_ > 2 and nh_ > 2
    for what, new, kind, section in cases:
        assert len(new) == len(k1) and new != k1, what
        rep = dev.contribution_check(tag, base, new, seed=SEED)
        hit = [f for f in rep["findings"] if f["kind"] == kind and f["section"] == section]
        assert hit, (what, rep)
        assert rep["counts"][kind] >= 1 and dev.contribution_check_line(hit[0]).startswith(kind)
        if kind != "delta_mismatch":
            assert len(rep["findings"]) == 1, (what, rep)
    x = bytearray(_get(k1, q, "h", 3)); x[-1] ^= 1                          # y changed: the point leaves the curve
    rep = dev.contribution_check(tag, base, _put(k1, q, "h", 3, bytes(x)), seed=SEED)
    assert rep["findings"][0]["kind"] == "not_on_curve" and rep["findings"][0]["section"] == "h" and rep["findings"][0]["first_index"] == 3
    assert rep["skipped"] and rep["skipped"][0]["section"] == "h"
