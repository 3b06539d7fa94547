"""What the C ABI does with a curve, pinned: which curve strings each Groth16 entry point takes and the exact text of every refusal,
and how many bytes the host-staged sums and pairings write per curve and group.  The expectations are literals that state what
the library did before the curves moved into one table (csrc/curve.h); nothing here is derived from that table."""
import ctypes as C
import importlib, pathlib, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402

NAMES = [b"BN128", b"BLS12381", b"bn254", b"bls12_381", b"BN254", b"", None]
# name -> the curve whose material the call gets (only the reference's names reach the material of setup / keygen / wtns)
REFERENCE = {b"BN128": "bn254", b"BLS12381": "bls12_381"}
WITH_ABI = {**REFERENCE, b"bn254": "bn254", b"bls12_381": "bls12_381"}
GROTH16_REFUSAL = {b"bn254": 'groth16: unknown curve "bn254" (BN128 | BLS12381)', b"bls12_381": 'groth16: unknown curve "bls12_381" (BN128 | BLS12381)',
                   b"BN254": 'groth16: unknown curve "BN254" (BN128 | BLS12381)', b"": 'groth16: unknown curve "" (BN128 | BLS12381)',
                   None: 'groth16: unknown curve "" (BN128 | BLS12381)'}
PAIRING_REFUSAL = {b"BN254": "pairing: unknown curve 'BN254' (BN128 | BLS12381)", b"": "pairing: unknown curve '' (BN128 | BLS12381)",
                   None: "pairing: null curve"}
POINT_BYTES = {("bn254", "g1"): 64, ("bls12_381", "g1"): 96, ("bn254", "g2"): 128, ("bls12_381", "g2"): 192}
GT_BYTES = {"bn254": 384, "bls12_381": 576}
GUARD = 64                                                                 # bytes of 0xA5 behind every output buffer


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def material(zk, orc):
    """per curve: the one-constraint circuit c = a * b (the shape of tests/golden/groth16/mycircuit_bls12381.r1cs), a key made for it
    with a fixed trapdoor, its verification key and a witness file"""
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    out = {}
    for cv, tag in (("bn254", "BN128"), ("bls12_381", "BLS12381")):
        g = G.Groth16Oracle(orc, cv)
        r1cs = g.r1cs_bytes(dict(n_wires=4, n_pub_out=1, n_pub_in=0, n_prv_in=2, constraints=[([(2, 1)], [(3, 1)], [(1, 1)])]))
        params, vk_json = dev.keygen(tag, r1cs, [3, 5, 7, 11, 13])
        out[cv] = dict(r1cs=np.frombuffer(r1cs, np.uint8), params=np.frombuffer(params, np.uint8), vk=vk_json.encode(),
                       wtns=np.frombuffer(g.wtns_bytes([1, 33, 3, 11]), np.uint8))
    return out


def _err(zk):
    return zk.lib().zk_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_setup_new_curve_names(zk, material, name):
    lib = zk.lib(); m = material[REFERENCE.get(name, "bn254")]
    h = lib.zk_groth16_setup_new(name, m["r1cs"].ctypes.data, m["r1cs"].size, m["params"].ctypes.data, m["params"].size)
    if name in REFERENCE:
        assert h, _err(zk)
        assert lib.zk_groth16_setup_free(h) == 0
    else:
        assert not h and _err(zk) == GROTH16_REFUSAL[name]


@pytest.mark.parametrize("name", NAMES)
def test_keygen_new_curve_names(zk, material, name):
    lib = zk.lib(); m = material[REFERENCE.get(name, "bn254")]
    td = np.zeros((5, 4), np.uint64); td[:, 0] = [3, 5, 7, 11, 13]
    h = lib.zk_groth16_keygen_new(name, m["r1cs"].ctypes.data, m["r1cs"].size, td.ctypes.data)
    if name in REFERENCE:
        assert h, _err(zk)
        assert lib.zk_groth16_keygen_params_size(h) == m["params"].size
        assert lib.zk_groth16_keygen_free(h) == 0
    else:
        assert not h and _err(zk) == GROTH16_REFUSAL[name]


@pytest.mark.parametrize("name", NAMES)
def test_wtns_payload_curve_names(zk, material, name):
    lib = zk.lib(); m = material[REFERENCE.get(name, "bn254")]
    off, n = C.c_uint64(0), C.c_uint64(0)
    rc = lib.zk_groth16_wtns_payload(m["wtns"].ctypes.data, m["wtns"].size, name, C.byref(off), C.byref(n))
    if name in REFERENCE:
        assert rc == 0, _err(zk)
        assert (off.value, n.value) == (m["wtns"].size - 4 * 32, 4)
    else:
        assert rc != 0 and _err(zk) == GROTH16_REFUSAL[name]


@pytest.mark.parametrize("name", NAMES)
def test_vk_new_curve_names(zk, material, name):
    lib = zk.lib(); m = material[WITH_ABI.get(name, "bn254")]
    h = lib.zk_groth16_vk_new(name, m["vk"])
    if name in WITH_ABI:
        assert h, _err(zk)
        n_pub, pb, gb = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        assert lib.zk_groth16_vk_info(h, C.byref(n_pub), C.byref(pb), C.byref(gb)) == 0
        cv = WITH_ABI[name]
        assert (n_pub.value, pb.value, gb.value) == (1, 2 * POINT_BYTES[cv, "g1"] + POINT_BYTES[cv, "g2"], GT_BYTES[cv])
        assert lib.zk_groth16_vk_free(h) == 0
    else:
        assert not h and _err(zk) == PAIRING_REFUSAL[name]


def _point(zk, cv, group, k):
    """[k]G in the layout of the sums, as bytes"""
    sc = np.zeros(4, np.uint64); sc[0] = k
    return zk.mul_generator_fr(zk.DevArray.from_host(sc), cv, group=group).to_host().view(np.uint8)


@pytest.mark.parametrize("cv,group", sorted(POINT_BYTES))
def test_host_msm_writes_one_point(zk, cv, group):
    lib = zk.lib(); pb = POINT_BYTES[cv, group]
    fn = getattr(lib, "zk_msm_%s_%s" % (group, cv))
    base = _point(zk, cv, group, 5)
    assert base.size == pb and base[-8:].any()
    one = np.zeros(4, np.uint64); one[0] = 1
    # the empty sum: the point's bytes zeroed, the flag set, nothing behind them touched (null inputs are fine when n = 0)
    out = np.full(pb + GUARD, 0xA5, np.uint8); inf = C.c_int(-1)
    assert fn(None, None, 0, out.ctypes.data, C.byref(inf)) == 0, _err(zk)
    assert inf.value == 1 and not out[:pb].any() and (out[pb:] == 0xA5).all()
    # one point, scalar 1: the point itself
    out = np.full(pb + GUARD, 0xA5, np.uint8); inf = C.c_int(-1)
    assert fn(base.ctypes.data, one.ctypes.data, 1, out.ctypes.data, C.byref(inf)) == 0, _err(zk)
    assert inf.value == 0 and np.array_equal(out[:pb], base) and (out[pb:] == 0xA5).all()


@pytest.mark.parametrize("cv", sorted(GT_BYTES))
def test_host_pairing_writes_one_gt(zk, cv):
    lib = zk.lib(); gb = GT_BYTES[cv]
    p, q = _point(zk, cv, "g1", 2), _point(zk, cv, "g2", 3)
    out = np.full(gb + GUARD, 0xA5, np.uint8)
    assert getattr(lib, "zk_pairing_" + cv)(p.ctypes.data, q.ctypes.data, 1, out.ctypes.data, 1) == 0, _err(zk)
    assert (out[gb:] == 0xA5).all()
    # the same pair through the device entry point, whose buffers have the exact sizes
    d_p, d_q = zk.DevArray.from_host(p.view(np.uint64)), zk.DevArray.from_host(q.view(np.uint64))
    d_gt = zk.DevArray(gb // 8, zero=True)
    assert getattr(lib, "zk_pairing_%s_dev" % cv)(d_p.ptr, d_q.ptr, 1, d_gt.ptr, 1, 0) == 0, _err(zk)
    want = d_gt.to_host().view(np.uint8)
    assert want.any() and np.array_equal(out[:gb], want)
