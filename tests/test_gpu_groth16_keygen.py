"""Groth16 key generation on the device (csrc/fixedbase_impl.hip.h, groth16_keygen_impl.hip.h; through the C ABI) against the
oracle's generate_parameters restatement (oracle/groth16.py) -- byte for byte -- and against the pairing verifier: a key made
here, a proof made with it, accepted.  `zkit groth16_setup`, groth16/src/api.rs:42-66."""
import ctypes as C
import importlib, json, pathlib, random, struct, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
CURVES = (("bn254", "BN128"), ("bls12_381", "BLS12381"))
WINDOW_BITS = 8                                                            # fixedbase_impl.hip.h FB_W


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


def _pairing(cv):
    import pairing as PG
    return PG.BN254 if cv == "bn254" else PG.BLS12_381


def _vk_ints(vk_json):
    """verification_key.json (decimal or 0x strings) -> the integer tuples the pairing verifier takes"""
    v = json.loads(vk_json)
    i = lambda s: int(s, 0)
    g1 = lambda p: (i(p["x"]), i(p["y"]))
    g2 = lambda p: (i(p["x"][0]), i(p["x"][1]), i(p["y"][0]), i(p["y"][1]))
    return dict(alpha_g1=g1(v["vk_alpha_1"]), beta_g1=g1(v["vk_beta_1"]), beta_g2=g2(v["vk_beta_2"]), gamma_g2=g2(v["vk_gamma_2"]),
                delta_g1=g1(v["vk_delta_1"]), delta_g2=g2(v["vk_delta_2"]), ic=[g1(p) for p in v["IC"]])


def _proof_ints(js):
    return dict(a=(int(js["pi_a"]["x"]), int(js["pi_a"]["y"])), c=(int(js["pi_c"]["x"]), int(js["pi_c"]["y"])),
                b=(int(js["pi_b"]["x"][0]), int(js["pi_b"]["x"][1]), int(js["pi_b"]["y"][0]), int(js["pi_b"]["y"][1])))


def _queries(g, pb):
    """the byte ranges of a Parameters file: (vk dict, {name: (count, offset, point bytes)})"""
    vk, o = g.vk_from_bytes(pb)
    s1, s2 = 16 * g.nl, 32 * g.nl
    q = {}
    for name, sz in (("h", s1), ("l", s1), ("a", s1), ("b_g1", s1), ("b_g2", s2)):
        n = struct.unpack(">I", pb[o:o + 4])[0]; o += 4
        q[name] = (n, o, sz); o += n * sz
    assert o == len(pb)
    return vk, q


# ---- 1. the fixed-base kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["g1", "g2"])
@pytest.mark.parametrize("cv,tag", CURVES)
def test_mul_generator_fr_matches_oracle(zk, g16, cv, tag, group):
    g = g16[cv]; r = g.r; cur = g.g2 if group == "g2" else g.g1
    rng = random.Random(11)
    ks = [0, 1, 2, r - 1, r - 2]
    for k in range(WINDOW_BITS, r.bit_length(), WINDOW_BITS):             # every window boundary
        ks += [v for v in (1 << k, (1 << k) - 1) if v < r]
    ks += [rng.randrange(r) for _ in range(200)]
    got = zk.mul_generator_fr(zk.DevArray.from_host(g.fr_array(ks).reshape(-1)), cv, group=group).to_host().reshape(len(ks), -1)
    Gen = cur.generator()
    for k, row in zip(ks, got):
        exp = g.mul(cur, Gen, k)
        assert np.array_equal(row, np.zeros_like(row) if exp is None else exp), hex(k)


@pytest.mark.parametrize("group", ["g1", "g2"])
@pytest.mark.parametrize("cv,tag", CURVES)
def test_mul_generator_fr_batch_of_2_20(zk, g16, cv, tag, group):
    """a full-size batch: sampled points against the oracle, and the whole batch through its sum -- sum_i [k_i]G = [sum_i k_i]G"""
    g = g16[cv]; r = g.r; cur = g.g2 if group == "g2" else g.g1
    n = 1 << 20
    rng = np.random.default_rng(20)
    k = np.concatenate([rng.integers(0, 2**64, size=(n, 3), dtype=np.uint64), rng.integers(0, r >> 192, size=(n, 1), dtype=np.uint64)], axis=1)   # top word below r's: k < r
    d_pts = zk.mul_generator_fr(zk.DevArray.from_host(k.reshape(-1)), cv, group=group)
    pw = g.nl * (4 if group == "g2" else 2)
    Gen = cur.generator()
    ks = g.fr_ints(k)
    pts = d_pts.to_host().reshape(n, pw)
    for i in (0, 1, 255, 256, 65537, n // 2, n - 2, n - 1):
        assert np.array_equal(pts[i], g.mul(cur, Gen, ks[i])), i
    ones = np.zeros((n, 4), np.uint64); ones[:, 0] = 1
    out = zk.msm_g1_dev(d_pts, zk.DevArray.from_host(ones.reshape(-1)), n, cv, group=group).to_host()
    assert int(out[pw]) & 0xFFFFFFFF == 0
    assert np.array_equal(out[:pw], g.mul(cur, Gen, sum(ks) % r))


# ---- 2. the key, byte for byte ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
@pytest.mark.parametrize("n_mul", [6, 40, 300])
def test_key_matches_oracle_byte_for_byte(g16, dev, cv, tag, n_mul):
    g = g16[cv]; rng = random.Random(500 + n_mul)
    r1cs, _wit = G.synthetic_r1cs(g.r, n_mul, seed=5)
    td = [rng.randrange(1, g.r) for _ in range(5)]
    P = g.setup(r1cs, *td)
    if n_mul == 40:
        assert sum(p is None for p in P["l"]) == 1                          # the unused wire: the infinity encoding is in the file
    exp = g.params_bytes(P)
    pb, vk_dec = dev.keygen(tag, g.r1cs_bytes(r1cs), td)
    assert len(pb) == len(exp) and pb == exp
    _, vk_hex = dev.keygen(tag, g.r1cs_bytes(r1cs), td, to_hex=True)
    vk = P["vk"]
    want = dict(alpha_g1=g.g1.affine_ints(vk["alpha_g1"]), beta_g1=g.g1.affine_ints(vk["beta_g1"]), beta_g2=g.g2.affine_ints(vk["beta_g2"]),
                gamma_g2=g.g2.affine_ints(vk["gamma_g2"]), delta_g1=g.g1.affine_ints(vk["delta_g1"]), delta_g2=g.g2.affine_ints(vk["delta_g2"]),
                ic=[g.g1.affine_ints(p) for p in vk["ic"]])
    for text, hexed in ((vk_dec, False), (vk_hex, True)):
        js = json.loads(text)
        assert list(js) == ["protocol", "curve", "vk_alpha_1", "vk_beta_1", "vk_beta_2", "vk_gamma_2", "vk_delta_1", "vk_delta_2", "IC"]
        assert js["protocol"] == "groth16" and js["curve"] == tag
        assert js["vk_alpha_1"]["x"].startswith("0x") == hexed
        got = _vk_ints(text)
        assert {k: tuple(v) if k != "ic" else [tuple(p) for p in v] for k, v in want.items()} == got


# ---- 3. the reference's own circuit ----------------------------------------------------------------------------------------------
def test_reference_r1cs_fixture_setup_prove_verify(g16, dev):
    g = g16["bls12_381"]
    rb = (ROOT / "tests" / "golden" / "groth16" / "mycircuit_bls12381.r1cs").read_bytes()
    pb, vk_json = dev.keygen("BLS12381", rb)
    S = dev.Groth16Setup("BLS12381", rb, pb)
    js, _ = S.prove(g.fr_array([1, 33, 3, 11]))                            # ONE, out c, in a, in b: 3 x 11
    S.free()
    PG = _pairing("bls12_381")
    assert PG.groth16_verify(_vk_ints(vk_json), _proof_ints(js), [33])
    assert not PG.groth16_verify(_vk_ints(vk_json), _proof_ints(js), [34])


# ---- 4. the full chain at size, trapdoor unknown ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
def test_setup_prove_verify_at_2_16_rows(zk, g16, dev, cv, tag):
    import groth16_bench as GB
    g = g16[cv]
    rb, wit, ni, n_wires = GB.make_circuit(g.r, 16)
    pb, vk_json = dev.keygen(tag, rb)
    S = dev.Groth16Setup(tag, rb, pb)
    assert S.domain_log == 16
    js, _ = S.prove(zk.DevArray.from_host(wit.reshape(-1)))
    S.free()
    pub = g.fr_ints(wit[1:ni])
    PG = _pairing(cv)
    assert PG.groth16_verify(_vk_ints(vk_json), _proof_ints(js), pub)
    assert not PG.groth16_verify(_vk_ints(vk_json), _proof_ints(js), [(pub[0] + 1) % g.r] + pub[1:])
    pb2, vk2 = dev.keygen(tag, rb)
    assert pb2 != pb and vk2 != vk_json and len(pb2) == len(pb)           # a fresh trapdoor every time


# ---- 5. structure at size, trapdoor known -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,tag", CURVES)
def test_key_structure_at_2_16_rows(g16, dev, cv, tag):
    import groth16_bench as GB
    g = g16[cv]; r = g.r; rng = random.Random(16)
    log_rows = 16; m = 1 << log_rows
    rb, _wit, ni, n_wires = GB.make_circuit(r, log_rows)
    tau, alpha, beta, gamma, delta = td = [rng.randrange(1, r) for _ in range(5)]
    pb, _ = dev.keygen(tag, rb, td)
    vk, q = _queries(g, pb)
    na, nb = GB.density(rb, ni, n_wires)
    assert (q["h"][0], q["l"][0], q["a"][0], q["b_g1"][0], q["b_g2"][0]) == (m - 1, n_wires - ni, na, nb, nb)
    assert len(vk["ic"]) == ni
    G1 = g.g1.generator()
    zt_dinv = (pow(tau, m, r) - 1) * pow(delta, -1, r) % r
    n, o, sz = q["h"]
    for i in (0, 1, 2, 12345, m // 2, m - 3, m - 2):
        assert pb[o + i * sz:o + (i + 1) * sz] == g.enc_point(g.g1, g.mul(g.g1, G1, pow(tau, i, r) * zt_dinv)), i
    assert np.array_equal(vk["alpha_g1"], g.mul(g.g1, G1, alpha)) and np.array_equal(vk["delta_g2"], g.mul(g.g2, g.g2.generator(), delta))


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_keygen_errors(zk, g16, dev):
    g = g16["bn254"]; r = g.r
    r1cs, _ = G.synthetic_r1cs(r, 6, seed=3)
    rb = g.r1cs_bytes(r1cs)
    td = [3, 5, 7, 11, 13]
    for i, name in enumerate(("tau", "alpha", "beta", "gamma", "delta")):
        bad = list(td); bad[i] = 0
        with pytest.raises(zk.ZkError, match=name + " is zero"):
            dev.keygen("BN128", rb, bad)
    log_m = g.circuit(r1cs)["log_m"]
    with pytest.raises(zk.ZkError, match=r"tau\^m = 1"):
        dev.keygen("BN128", rb, [g.omega(log_m)] + td[1:])                  # a root of unity of the domain: t(tau) = 0
    with pytest.raises(zk.ZkError, match=r"tau\^m = 1"):
        dev.keygen("BN128", rb, [1] + td[1:])
    with pytest.raises(zk.ZkError, match="unknown curve"):
        dev.keygen("BN254", rb, td)
    lib = zk.lib(); err = lambda: lib.zk_last_error().decode()
    buf = np.frombuffer(rb, np.uint8)
    assert not lib.zk_groth16_keygen_new(b"BN254", buf.ctypes.data, buf.size, None) and "unknown curve" in err()
    with pytest.raises(zk.ZkError, match="Invalid magic number"):
        dev.keygen("BN128", b"xxxx" + rb[4:], td)
    with pytest.raises(zk.ZkError, match="prime is not the scalar field"):
        dev.keygen("BLS12381", rb, td)
    with pytest.raises(zk.ZkError, match="truncated"):
        dev.keygen("BN128", rb[:-9], td)
    # a buffer that is too small: an error, and nothing written
    tdw = g.fr_array(td).reshape(-1)
    h = lib.zk_groth16_keygen_new(b"BN128", buf.ctypes.data, buf.size, tdw.ctypes.data)
    assert h
    n = lib.zk_groth16_keygen_params_size(h)
    out = np.full(n, 0xA5, np.uint8)
    assert lib.zk_groth16_keygen_params(h, out.ctypes.data, n - 1) != 0 and "buffer" in err()
    assert (out == 0xA5).all()
    assert lib.zk_groth16_keygen_params(h, out.ctypes.data, n) == 0
    assert out.tobytes() == g.params_bytes(g.setup(r1cs, *td))
    lib.zk_groth16_keygen_free(h)
