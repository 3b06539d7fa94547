"""Several polynomials at several points in one two-point proof through the package's Kzg.open_multi / verify_multi
(csrc/kzg.hip: zk_kzg_multi_begin .. finish, zk_kzg_multi_verify), over the power-12 file with a KNOWN tau that test_gpu_kzg.py uses.  With tau
known, W1 and W2 have scalars the reference (tests/kzg_multi_ref.py: successive division, not the device's partial fractions) computes, and the
points are compared byte for byte with [scalar] G from the fixed-base kernel.  Everything is exact: no tolerance anywhere."""
import importlib, pathlib, random, sys
import numpy as np
import pytest

import kzg_ref as ref
import kzg_multi_ref as mref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

CURVES = ("BN128", "BLS12381")
ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
SEED = bytes(range(32))
ACCEPTED, REJECTED, NOT_CANONICAL, INPUT_COUNT, NOT_ON_CURVE = 1, 0, -1, -2, -3


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
    power = (2 * tile + 1).bit_length() - 1
    assert (2 << power) - 1 >= 2 * tile + 1
    d = tmp_path_factory.mktemp("kzg_multi")
    out = {}
    for cv in CURVES:
        p = d / (cv + ".ptau")
        p.write_bytes(make_test_ptau.build_ptau(zk, cv, power, TAU[cv], 5, 7))
        out[cv] = p
    return out


@pytest.fixture(scope="module")
def handles(kzg, files):
    g16 = importlib.import_module("eigen_zkvm_amd.groth16")
    hs = {}
    for cv in CURVES:
        srs = g16.Srs(cv, files[cv])
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


def _points(rng, n, r, start=()):
    s = list(start)
    while len(s) < n:
        p = rng.randrange(r)
        if p not in s:
            s.append(p)
    return s


def _honest(k, rng, r, lens=(9, 4, 12), sizes=(2, 3, 2), shared=1):
    """one honest proof (commitments, sets, values, gamma, z, W1, W2) of short random polynomials, and the polynomials"""
    common = _points(rng, shared, r)
    sets = [_points(rng, ns, r, common[:ns]) for ns in sizes]
    polys = [_poly(rng, n, r) for n in lens]
    cs = [k.commit(p) for p in polys]
    values, W1, W2, gamma, z = k.open_multi(polys, sets, commitments=cs)
    return (cs, sets, values, gamma, z, W1, W2), polys


def _scalars(cv, polys, proof):
    """the proof in the exponent: (c_i, sets, values, gamma, z, w1, w2) from the reference"""
    r = ref.R[cv]
    _, sets, values, gamma, z, _, _ = proof
    _, w1, w2 = mref.open_scalars(polys, sets, gamma, z, TAU[cv], r)
    return [ref.horner(p, TAU[cv], r) for p in polys], sets, values, gamma, z, w1, w2


def _shapes(rng, r, T):
    """(lengths, sets): lengths 1, 2, |S|, |S| + 1, 65, T + 1, 2T + 1; sets of 1, 2, 3, 8, 16 points; disjoint, overlapping and identical sets;
    the points 0 and 1"""
    big = _points(rng, 16, r)
    same = _points(rng, 3, r)
    return [((1, 2, 3, 4, 65), [_points(rng, n, r) for n in (1, 2, 3, 3, 8)]),                  # disjoint
            ((T + 1, 2 * T + 1, 17), [big[3:5], big, list(reversed(big))]),                     # a subset, and the same 16 points in another order
            ((5, 9, 1), [[0, 1], _points(rng, 3, r, (1, 0)), [0]]),
            ((6, 7), [same, same]),
            ((40,), [_points(rng, 8, r)])]


@pytest.mark.parametrize("cv", CURVES)
def test_w1_and_w2_are_the_reference_scalars_times_g(zk, kzg, handles, tile, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x51 + len(cv))
    proofs = []
    for lens, sets in _shapes(rng, r, tile):
        polys = [_poly(rng, n, r) for n in lens]
        cs = [k.commit(p) for p in polys]
        values, W1, W2, gamma, z = k.open_multi(polys, sets, commitments=cs)
        assert gamma == kzg.challenges_of(cv, cs, sets, values) and z == kzg.challenge_z(cv, gamma, W1, avoid=[p for s in sets for p in s])
        want_values, w1, w2 = mref.open_scalars(polys, sets, gamma, z, TAU[cv], r)
        assert values == want_values, lens
        assert [W1, W2] == gen_mul(zk, cv, [w1, w2]), lens
        assert mref.proof_holds([ref.horner(p, TAU[cv], r) for p in polys], sets, values, gamma, z, w1, w2, TAU[cv], r)
        proofs.append((cs, sets, values, gamma, z, W1, W2))
        assert k.verify_multi([proofs[-1]]) == (ACCEPTED, None), lens
    assert k.verify_multi(proofs, seed=SEED) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_the_fflonk_shape(zk, kzg, handles, cv):
    """f = sum_i f_i(X^4) X^i (interleave) opened at the 4 fourth roots h w^j of x = h^4: f(h w^j) = sum_i f_i(x) (h w^j)^i, so the f_i(x) come
    back from the 4 values by an inverse transform of size 4 on the host"""
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x52 + len(cv))
    parts = [_poly(rng, n, r) for n in (40, 33, 40, 7)]
    f = kzg.interleave(parts, cv)
    assert f == mref.interleave(parts)
    h, w = rng.randrange(1, r), ref.root_of_unity(cv, 2)
    x = pow(h, 4, r)
    roots = [h * pow(w, j, r) % r for j in range(4)]
    values, W1, W2, gamma, z = k.open_multi([f], [roots])
    for i, p in enumerate(parts):
        got = sum(pow(w, -i * j % 4, r) * values[0][j] for j in range(4)) * pow(4 * pow(h, i, r), -1, r) % r
        assert got == ref.horner(p, x, r), i
    _, w1, w2 = mref.open_scalars([f], [roots], gamma, z, TAU[cv], r)
    assert [W1, W2] == gen_mul(zk, cv, [w1, w2])
    assert k.verify_multi([([k.commit(f)], [roots], values, gamma, z, W1, W2)]) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_every_polynomial_its_own_interpolant(zk, handles, cv):
    """n_i <= |S_i| everywhere: q = 0, W1 is infinity, and the proof still verifies"""
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x53 + len(cv))
    proof, polys = _honest(k, rng, r, lens=(2, 3, 1, 0), sizes=(2, 4, 1, 2), shared=0)
    assert proof[5] == bytes(k.point_bytes)
    _, _, _, _, _, w1, w2 = _scalars(cv, polys, proof)
    assert w1 == 0 and proof[6] == gen_mul(zk, cv, [w2])[0]
    assert k.verify_multi([proof]) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_one_polynomial_at_one_point_is_the_single_opening(handles, cv):
    """k = 1, |S| = 1: gamma^0 a_s = 1, so q is the single-point quotient and W1 is Kzg.open's witness"""
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x54 + len(cv))
    p, s = _poly(rng, 70, r), rng.randrange(r)
    values, W1, W2, gamma, z = k.open_multi([p], [[s]])
    y, W = k.open(p, s)
    assert values == [[y]] and W1 == W
    C = k.commit(p)
    assert k.verify([(C, s, y, W1)]) == (ACCEPTED, None)
    assert k.verify_multi([([C], [[s]], values, gamma, z, W1, W2)]) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_honest_batches(handles, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x55 + len(cv))
    proofs = [_honest(k, rng, r)[0] for _ in range(5)]
    for m in (1, 2, 5):
        assert k.verify_multi(proofs[:m]) == (ACCEPTED, None)
        assert k.verify_multi(proofs[:m], seed=SEED, locate=False) == (ACCEPTED, None)
    assert k.verify_multi([]) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_the_device_form_gives_the_same_verdicts(zk, handles, cv):
    """zk_kzg_multi_verify_dev over the same bytes in device memory; an accepted batch leaves first_bad = m"""
    import ctypes as C
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x59 + len(cv))
    good = [_honest(k, rng, r)[0] for _ in range(2)]
    moved = [[(good[1][2][0][0] + 1) % r] + list(good[1][2][0][1:])] + [list(v) for v in good[1][2][1:]]
    seed = np.frombuffer(SEED, dtype=np.uint8)
    for batch, want in ((good, (ACCEPTED, 2)), ([good[0], good[1][:2] + (moved,) + good[1][3:]], (REJECTED, 1))):
        buf = np.frombuffer(b"".join(k.pack_multi(p) for p in batch), dtype="<u8").astype(np.uint64)
        d = zk.DevArray.from_host(buf)
        verdict, first = C.c_int(0), C.c_uint64(0)
        try:
            zk._check(zk.lib().zk_kzg_multi_verify_dev(k._h, d.ptr, 8 * buf.size, len(batch), seed.ctypes.data, C.byref(verdict), C.byref(first), None))
        finally:
            d.free()
        assert (verdict.value, first.value) == want
        assert k.verify_multi(batch, seed=SEED)[0] == want[0]


@pytest.mark.parametrize("cv", CURVES)
def test_a_wrong_proof_is_refused_and_named(zk, handles, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x56 + len(cv))
    good = [_honest(k, rng, r)[0] for _ in range(4)]
    at = 2
    cs, sets, values, gamma, z, W1, W2 = good[at]
    other = gen_mul(zk, cv, [0xABCDEF])[0]
    off_curve = bytes([cs[0][0] ^ 1]) + cs[0][1:]

    def values_with(i, j, v):
        out = [list(ys) for ys in values]
        out[i][j] = v
        return out
    cases = [("a value off by one", (cs, sets, values_with(1, 2, (values[1][2] + 1) % r), gamma, z, W1, W2), REJECTED),
             ("another W1", (cs, sets, values, gamma, z, other, W2), REJECTED),
             ("another W2", (cs, sets, values, gamma, z, W1, other), REJECTED),
             ("another commitment", ([cs[0], other, cs[2]], sets, values, gamma, z, W1, W2), REJECTED),
             ("two sets swapped", (cs, [sets[2], sets[1], sets[0]], values, gamma, z, W1, W2), REJECTED),
             ("gamma + 1", (cs, sets, values, (gamma + 1) % r, z, W1, W2), REJECTED),
             ("z + 1", (cs, sets, values, gamma, (z + 1) % r, W1, W2), REJECTED),
             ("z in T", (cs, sets, values, gamma, sets[1][1], W1, W2), INPUT_COUNT),
             ("a repeated point", (cs, [[sets[0][0], sets[0][0]], sets[1], sets[2]], values, gamma, z, W1, W2), INPUT_COUNT),
             ("a value >= r", (cs, sets, values_with(0, 0, values[0][0] + r), gamma, z, W1, W2), NOT_CANONICAL),
             ("a point >= r", (cs, [[sets[0][0] + r, sets[0][1]], sets[1], sets[2]], values, gamma, z, W1, W2), NOT_CANONICAL),
             ("a commitment off the curve", ([off_curve, cs[1], cs[2]], sets, values, gamma, z, W1, W2), NOT_ON_CURVE),
             ("W2 off the curve", (cs, sets, values, gamma, z, W1, off_curve), NOT_ON_CURVE)]
    assert sets[0] != sets[2]
    for name, bad, code in cases:
        batch = good[:at] + [bad] + good[at + 1:]
        assert k.verify_multi(batch) == (code, at), name
        assert k.verify_multi(batch, seed=SEED, locate=False) == (REJECTED, None), name
        assert k.verify_multi([bad]) == (code, 0), name
    assert k.verify_multi(good) == (ACCEPTED, None)


@pytest.mark.parametrize("cv", CURVES)
def test_two_wrong_proofs_that_cancel_without_weights(handles, cv):
    """a value of each of two proofs is moved so that the two defects add up to zero: the unweighted sum of the two equations still holds,
    the weighted one does not"""
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x57 + len(cv))
    tau = TAU[cv]
    (p0, polys0), (p1, polys1) = _honest(k, rng, r), _honest(k, rng, r)
    s0, s1 = _scalars(cv, polys0, p0), _scalars(cv, polys1, p1)

    def defect(s, d):
        """the equation's left side minus its right side, in the exponent, with the first value moved by d: linear in d"""
        cs, sets, values, gamma, z, w1, w2 = s
        moved = [[(values[0][0] + d) % r] + list(values[0][1:])] + [list(v) for v in values[1:]]
        return (mref.verifier_f(cs, sets, moved, gamma, z, w1, r) + z * w2 - tau * w2) % r, moved
    assert defect(s0, 0)[0] == 0 and defect(s1, 0)[0] == 0
    d0 = rng.randrange(1, r)
    e0, moved0 = defect(s0, d0)
    d1 = -e0 * pow(defect(s1, 1)[0], -1, r) % r
    e1, moved1 = defect(s1, d1)
    assert e0 != 0 and (e0 + e1) % r == 0
    bad_s = [s0[:2] + (moved0,) + s0[3:], s1[:2] + (moved1,) + s1[3:]]
    assert mref.batch_holds(bad_s, [1, 1], tau, r) and not mref.batch_holds(bad_s, [1, 2], tau, r)
    bad = [p0[:2] + (moved0,) + p0[3:], p1[:2] + (moved1,) + p1[3:]]
    assert k.verify_multi(bad, seed=SEED) == (REJECTED, 0)
    assert k.verify_multi(bad) == (REJECTED, 0)
    assert k.verify_multi([bad[1]]) == (REJECTED, 0)


@pytest.mark.parametrize("cv", CURVES)
def test_refusals_carry_their_text(kzg, handles, files, cv):
    k, r, rng = handles[cv], ref.R[cv], random.Random(0x58 + len(cv))
    p, q = _poly(rng, 9, r), _poly(rng, 5, r)
    pts = _points(rng, 17, r)
    for polys, sets, text in (([], [], "no polynomials"),
                              ([p, q], [[1, 2], []], "set 1 is empty"),
                              ([p], [pts], r"set 0 has 17 points, more than ZK_KZG_MULTI_MAX_POINTS \(16\)"),
                              ([p, q], [[1], [2, r]], "a point of set 1 is not below the scalar field's modulus"),
                              ([p, q], [[1, 2], [3, 4, 3]], "set 1 repeats a point"),
                              ([p], [[1], [2]], "1 polynomials, 2 sets")):
        with pytest.raises(kzg.ZkError, match=text):
            k.multi_begin(polys, sets)
    g16 = importlib.import_module("eigen_zkvm_amd.groth16")
    srs = g16.Srs(cv, files[cv])
    small = kzg.Kzg(srs, 8)
    srs.free()
    try:
        with pytest.raises(kzg.ZkError, match="exceeds the 8 powers the handle holds"):
            small.multi_begin([p], [[1, 2]])
    finally:
        small.free()
    m = k.multi_begin([p, q], [[1, 2], [2, 3]])
    try:
        assert m.values == [[ref.horner(p, 1, r), ref.horner(p, 2, r)], [ref.horner(q, 2, r), ref.horner(q, 3, r)]]
        with pytest.raises(kzg.ZkError, match="finish comes once, after the quotient"):
            m.finish(5)
        with pytest.raises(kzg.ZkError, match="gamma is not below the scalar field's modulus"):
            m.quotient(r)
        m.quotient(7)
        with pytest.raises(kzg.ZkError, match="the quotient comes once, after begin"):
            m.quotient(7)
        for z in (1, 2, 3):
            with pytest.raises(kzg.ZkError, match="z is one of the opening points"):
                m.finish(z)
        with pytest.raises(kzg.ZkError, match="z is not below the scalar field's modulus"):
            m.finish(r)
        assert len(m.finish(4)) == k.point_bytes                             # a refusal leaves the stage where it was
    finally:
        m.free()
