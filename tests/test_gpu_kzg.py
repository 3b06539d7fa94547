"""KZG commitments over a powers-of-tau file with a KNOWN tau (tools/make_test_ptau.py): commit, open, open_many, verify through the package's
Kzg (csrc/kzg.hip), byte for byte.  With tau known every point the library makes has a scalar the reference (tests/kzg_ref.py) computes:
commit(p) = [p(tau)] G and W = [(p(tau) - y) / (tau - z)] G, made here by the fixed-base kernel tests/test_gpu_groth16_keygen.py holds to the
CPU oracle.  The file's power is the smallest at which 2T + 1 coefficients fit (T = zk_kzg_tile_elems()); one file per curve, built once."""
import importlib, pathlib, random, sys
import numpy as np
import pytest

import kzg_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

CURVES = ("BN128", "BLS12381")
ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
Q = {c: make_test_ptau.CURVES[c]["q"] for c in CURVES}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
SEED = bytes(range(32))
ACCEPTED, REJECTED, NOT_CANONICAL, NOT_ON_CURVE, NOT_IN_SUBGROUP = 1, 0, -1, -3, -4


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def kzg():
    return importlib.import_module("eigen_zkvm_amd.kzg")


@pytest.fixture(scope="module")
def tile(zk):
    return int(zk.lib().zk_kzg_tile_elems())


@pytest.fixture(scope="module")
def files(zk, tile, tmp_path_factory):
    """{curve: (path, power)}: 2^(power + 1) - 1 >= 2T + 1"""
    power = (2 * tile + 1).bit_length() - 1
    assert (2 << power) - 1 >= 2 * tile + 1
    d = tmp_path_factory.mktemp("kzg")
    out = {}
    for cv in CURVES:
        p = d / (cv + ".ptau")
        p.write_bytes(make_test_ptau.build_ptau(zk, cv, power, TAU[cv], 5, 7))
        out[cv] = (p, power)
    return out


@pytest.fixture(scope="module")
def handles(kzg, files):
    g16 = importlib.import_module("eigen_zkvm_amd.groth16")
    hs = {}
    for cv in CURVES:
        srs = g16.Srs(cv, files[cv][0])
        hs[cv] = (kzg.Kzg(srs), srs)
    yield {cv: h for cv, (h, _) in hs.items()}
    for h, srs in hs.values():
        h.free(); srs.free()


def gen_mul(zk, cv, ks):
    """[k] G for each k, as bytes in the layout of the sums (zero: all zero)"""
    k = np.array([[(v >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in ks], dtype=np.uint64)
    pts = zk.mul_generator_fr(zk.DevArray.from_host(k.reshape(-1)), ABI[cv]).to_host()
    b = pts.astype("<u8").tobytes()
    pb = len(b) // len(ks)
    return [b[i * pb:(i + 1) * pb] for i in range(len(ks))]


def _poly(rng, n, r):
    return [rng.randrange(r) for _ in range(n)]


@pytest.mark.parametrize("cv", CURVES)
def test_commit_is_p_of_tau_times_g(zk, handles, tile, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(1)
    assert k.max_coeffs == (2 << k.power) - 1 >= 2 * tile + 1
    polys = [_poly(rng, n, r) for n in (1, 2, 5, 65, tile + 1, 2 * tile + 1)]
    want = gen_mul(zk, cv, [ref.horner(p, TAU[cv], r) for p in polys])
    for p, w in zip(polys, want):
        assert k.commit(p) == w, len(p)


@pytest.mark.parametrize("cv", CURVES)
def test_open_is_the_quotient_at_tau(zk, handles, tile, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(2)
    cases = [(_poly(rng, n, r), z) for n in (2, 5, 65, tile + 1, 2 * tile + 1) for z in (rng.randrange(r), 0)]
    want = gen_mul(zk, cv, [ref.witness_scalar(p, z, TAU[cv], r) for p, z in cases])
    for (p, z), w in zip(cases, want):
        y, W = k.open(p, z)
        assert y == ref.horner(p, z, r) == k.eval(p, z)
        assert W == w, (len(p), z)


@pytest.mark.parametrize("cv", CURVES)
def test_degenerate_polynomials(zk, handles, cv):
    k, r = handles[cv], ref.R[cv]
    inf = bytes(k.point_bytes)
    g1, g9 = gen_mul(zk, cv, [1, 9])
    assert k.commit([]) == inf and k.commit([0, 0, 0]) == inf and k.commit([9]) == g9
    assert k.open([], 3) == (0, inf) and k.open([9], 3) == (9, inf)
    assert k.verify([(g9, 3, 9, inf)]) == (ACCEPTED, None)                  # a constant: W at infinity
    p = [r - TAU[cv], 1]                                                    # X - tau: p(tau) = 0
    assert k.commit(p) == inf
    y, W = k.open(p, 12345)
    assert y == (12345 - TAU[cv]) % r and W == g1
    assert k.verify([(inf, 12345, y, W)]) == (ACCEPTED, None)
    assert k.verify([]) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_commit_evals_equals_commit(kzg, handles, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(3)
    g16 = importlib.import_module("eigen_zkvm_amd.groth16")
    for log_n in (0, 1, 2, 6, k.power):
        p = _poly(rng, 1 << log_n, r)
        if log_n <= 6:
            evals = ref.ntt(p, cv)                                          # the reference's own transform
        else:
            evals = kzg.from_mont(g16.fr_ntt(kzg.to_mont(p, cv), cv), cv)   # the scalar-field transform test_gpu_groth16.py holds to the oracle
        assert k.commit_evals(evals) == k.commit(p), log_n


@pytest.mark.parametrize("cv", CURVES)
def test_open_many_is_open_of_the_fold(zk, handles, tile, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(4)
    for lens in ((7,), (300, 3), (tile + 1, 1, 64, 2 * tile + 1, 5)):
        polys = [_poly(rng, n, r) for n in lens]
        z, gamma = rng.randrange(r), rng.randrange(r)
        f = ref.fold_polys(polys, gamma, r)
        ys, W = k.open_many(polys, z, gamma)
        assert ys == [ref.horner(p, z, r) for p in polys]
        assert (ref.fold_values(ys, gamma, r), W) == k.open(f, z)
        cs = [k.commit(p) for p in polys]
        C = k.fold_commitments(cs, gamma)
        assert C == k.commit(f)
        assert k.verify([(C, z, k.fold_values(ys, gamma), W)]) == (ACCEPTED, None)
    inf = bytes(k.point_bytes)
    assert k.fold_commitments([inf, inf], 5) == inf


def _openings(k, rng, r, m, points=None):
    """m honest openings (C, z, y, W) of short random polynomials"""
    out = []
    for j in range(m):
        p = _poly(rng, rng.randrange(1, 40), r)
        z = points[j % len(points)] if points else rng.randrange(r)
        y, W = k.open(p, z)
        out.append((k.commit(p), z, y, W))
    return out


@pytest.mark.parametrize("cv", CURVES)
def test_verify_accepts_honest_batches(handles, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(5)
    for m in (1, 2, 17):
        assert k.verify(_openings(k, rng, r, m)) == (ACCEPTED, None)
        assert k.verify(_openings(k, rng, r, m, points=[rng.randrange(r)]), seed=SEED) == (ACCEPTED, None)   # one point for all
    ops = _openings(k, rng, r, 3)
    assert k.verify(ops + ops, locate=False) == (ACCEPTED, None)            # the same openings twice: equal points in one sum


def _off_subgroup_point(cv):
    """a point of BLS12-381's curve outside the subgroup of order r, Montgomery bytes: the cofactor is about 2^126, so the first x that gives a
    point does"""
    q = Q[cv]
    x = 5
    while True:
        a = (x * x * x + 4) % q
        y = pow(a, (q + 1) // 4, q)
        if y * y % q == a:
            break
        x += 1
    n8 = 48
    return b"".join(((v << (8 * n8)) % q).to_bytes(n8, "little") for v in (x, y))


@pytest.mark.parametrize("cv", CURVES)
def test_verify_refuses_and_names_the_opening(zk, handles, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(6)
    good = _openings(k, rng, r, 5)
    other = gen_mul(zk, cv, [0xABCDEF])[0]
    at = 3
    C, z, y, W = good[at]
    off_curve = bytes([C[0] ^ 1]) + C[1:]
    cases = [("y + 1", (C, z, (y + 1) % r, W), REJECTED), ("z + 1", (C, (z + 1) % r, y, W), REJECTED), ("another W", (C, z, y, other), REJECTED),
             ("C off the curve", (off_curve, z, y, W), NOT_ON_CURVE), ("W off the curve", (C, z, y, off_curve), NOT_ON_CURVE),
             ("y >= r", (C, z, y + r, W), NOT_CANONICAL), ("z >= r", (C, z + r, y, W), NOT_CANONICAL)]
    if cv == "BLS12381":
        cases.append(("W outside the subgroup", (C, z, y, _off_subgroup_point(cv)), NOT_IN_SUBGROUP))
        cases.append(("C outside the subgroup", (_off_subgroup_point(cv), z, y, W), NOT_IN_SUBGROUP))
    for name, bad, code in cases:
        batch = good[:at] + [bad] + good[at + 1:]
        assert k.verify(batch) == (code, at), name
        assert k.verify(batch, seed=SEED, locate=False) == (REJECTED, None), name
        assert k.verify([bad]) == (code, 0), name
    assert k.verify(good) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_two_wrong_openings_that_cancel_without_weights(zk, handles, cv):
    """y_1 + d and y_2 - d: the unweighted sum of the two equations still holds, the weighted one does not"""
    k, r, rng = handles[cv], ref.R[cv], random.Random(7)
    polys = [_poly(rng, 9, r), _poly(rng, 4, r)]
    zs = [rng.randrange(r), rng.randrange(r)]
    d = rng.randrange(1, r)
    scal, ops = [], []
    for p, z, dy in zip(polys, zs, (d, r - d)):
        y, W = k.open(p, z)
        ops.append((k.commit(p), z, (y + dy) % r, W))
        scal.append((ref.horner(p, TAU[cv], r), z, (y + dy) % r, ref.witness_scalar(p, z, TAU[cv], r)))
    assert ref.batch_holds(scal, [1, 1], TAU[cv], r) and not ref.batch_holds(scal, [1, 2], TAU[cv], r)
    assert not ref.opening_holds(*scal[0], TAU[cv], r)
    assert k.verify(ops, seed=SEED) == (REJECTED, 0)
    assert k.verify(ops) == (REJECTED, 0)


@pytest.mark.parametrize("cv", CURVES)
def test_plain_sums_without_window_tables(kzg, handles, files, tile, cv, monkeypatch):
    """ZK_KZG_NO_TABLES (read when a handle is made): commitments and openings through the plain multi-scalar sum are the same bytes"""
    g16 = importlib.import_module("eigen_zkvm_amd.groth16")
    k, r, rng = handles[cv], ref.R[cv], random.Random(8)
    monkeypatch.setenv("ZK_KZG_NO_TABLES", "1")
    srs = g16.Srs(cv, files[cv][0])
    plain = kzg.Kzg(srs)
    srs.free()
    try:
        for n in (1, 65, tile + 1):
            p, z = _poly(rng, n, r), rng.randrange(r)
            assert plain.commit(p) == k.commit(p)
            assert plain.open(p, z) == k.open(p, z)
    finally:
        plain.free()


@pytest.mark.parametrize("cv", CURVES)
def test_sizes_are_refused_with_a_message(kzg, handles, files, cv):
    g16 = importlib.import_module("eigen_zkvm_amd.groth16")
    srs = g16.Srs(cv, files[cv][0])
    try:
        with pytest.raises(kzg.ZkError, match="holds %d powers in G1" % ((2 << srs.power) - 1)):
            kzg.Kzg(srs, (2 << srs.power))
        small = kzg.Kzg(srs, 8)
        try:
            assert small.max_coeffs == 8 and len(small.commit([1] * 8)) == small.point_bytes
            with pytest.raises(kzg.ZkError, match="exceeds the 8 powers the handle holds"):
                small.commit([1] * 9)
            with pytest.raises(kzg.ZkError, match="exceeds the 8 powers the handle holds"):
                small.open([1] * 9, 2)
            with pytest.raises(kzg.ZkError, match="exceeds"):
                small.commit_evals([1] * 16)
        finally:
            small.free()
    finally:
        srs.free()
