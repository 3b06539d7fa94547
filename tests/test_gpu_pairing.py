"""The device pairing (csrc/pairing.hip, through eigen_zkvm_amd.groth16.pairing) against oracle/pairing.py and against its own
algebra.  Oracle pairings cost seconds: at most two per curve per test."""
import importlib, pathlib, random, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import pairing as PG  # noqa: E402
import pairing_constants as pc  # noqa: E402

CURVES = {"BN128": (pc.BN254, PG.BN254, 4), "BLS12381": (pc.BLS12_381, PG.BLS12_381, 6)}


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


def _mont(C, nl, v): return [((v << (64 * nl)) % C.q >> (64 * i)) & (2**64 - 1) for i in range(nl)]
def enc_g1(C, nl, P): return np.zeros(2 * nl, np.uint64) if P is None else np.array(_mont(C, nl, P[0]) + _mont(C, nl, P[1]), dtype=np.uint64)
def enc_g2(C, nl, Q): return np.zeros(4 * nl, np.uint64) if Q is None else np.array(sum((_mont(C, nl, c) for xy in Q for c in xy), []), dtype=np.uint64)
def gt_ints(row, nl): return [sum(int(row[j, i]) << (64 * i) for i in range(nl)) for j in range(12)]


def to_flat(O, gt):
    """coefficients of w^k over Fq2 -> the oracle's flat basis, u = w^6 - xi0"""
    flat = [0] * 12
    for k in range(6):
        flat[k] = (gt[2 * k] - O.xi0 * gt[2 * k + 1]) % O.Q; flat[k + 6] = gt[2 * k + 1]
    return flat


def pair(dev, tag, pairs, final_exp=True):
    C, _, nl = CURVES[tag]
    g1 = np.concatenate([enc_g1(C, nl, P) for P, _ in pairs]); g2 = np.concatenate([enc_g2(C, nl, Q) for _, Q in pairs])
    out = dev.pairing(g1, g2, tag, final_exp=final_exp)
    return [gt_ints(out[i], nl) for i in range(len(pairs))]


def f12(gt): return [(gt[2 * k], gt[2 * k + 1]) for k in range(6)]
ONE = [1] + [0] * 11


@pytest.mark.parametrize("tag", list(CURVES))
def test_matches_oracle_on_generators_and_a_random_pair(dev, tag):
    C, O, nl = CURVES[tag]
    rng = random.Random(11)
    a, b = rng.randrange(1, C.r), rng.randrange(1, C.r)
    pairs = [(C.g1, C.g2), (C.g1_mul(a, C.g1), C.g2_mul(b, C.g2))]
    got = pair(dev, tag, pairs)
    for (P, Q), g in zip(pairs, got):
        want = O.pairing((Q[0][0], Q[0][1], Q[1][0], Q[1][1]), P)
        if tag == "BLS12381": want = want.inverse()          # the oracle does not conjugate for the negative curve parameter
        assert to_flat(O, g) == want.c


@pytest.mark.parametrize("tag", list(CURVES))
def test_miller_value_then_oracle_exponent(dev, tag):
    C, O, nl = CURVES[tag]
    Q = C.g2_mul(3, C.g2)
    f, e = pair(dev, tag, [(C.g1, Q)], final_exp=False)[0], pair(dev, tag, [(C.g1, Q)])[0]
    assert (O.F12(to_flat(O, f)) ** O.final_exp).c == to_flat(O, e)


@pytest.mark.parametrize("tag", list(CURVES))
def test_bilinear_inverse_and_infinity(dev, tag):
    C, _, nl = CURVES[tag]
    M = pc.Model(C)
    a = random.Random(5).randrange(2, C.r)
    P, Q = C.g1, C.g2
    aP, aQ, negP = C.g1_mul(a, P), C.g2_mul(a, Q), (P[0], C.q - P[1])
    e = pair(dev, tag, [(aP, Q), (P, aQ), (P, Q), (negP, Q), (None, Q), (P, None), (None, None)])
    assert e[0] == e[1] != ONE and e[0] != e[2]
    assert f12(e[0]) == M.pow(f12(e[2]), a)                                # e([a]P, Q) = e(P, Q)^a
    assert M.mul(f12(e[2]), f12(e[3])) == M.one()                          # e(P, Q) e(-P, Q) = 1
    assert e[4] == ONE and e[5] == ONE and e[6] == ONE
    assert M.pow(f12(e[2]), C.r) == M.one()


@pytest.mark.parametrize("tag", list(CURVES))
def test_batches_of_1_and_9_equal_single_calls(dev, tag):
    C, _, nl = CURVES[tag]
    pairs = [(C.g1_mul(i + 2, C.g1), C.g2_mul(2 * i + 3, C.g2)) for i in range(9)]      # a workgroup holds 8 pairings
    pairs[4] = (None, pairs[4][1])
    batch = pair(dev, tag, pairs)
    for i in (0, 4, 7, 8):
        assert pair(dev, tag, [pairs[i]])[0] == batch[i]
    assert len({tuple(x) for x in batch}) == 9


@pytest.mark.parametrize("tag", list(CURVES))
def test_nine_random_pairs_equal_the_model_miller_value_and_its_exponentiation(dev, tag):
    """[a]G1, [b]G2 with a, b uniform below r: the value miller_kernel leaves is pairing_constants.Model.miller's exactly (the same line
    scalings), and Model.final_exp of it is the full call.  Milliseconds on the host, where the oracle costs seconds."""
    C, _, nl = CURVES[tag]
    M = pc.Model(C)
    rng = random.Random(254 + nl)
    pairs = [(C.g1_mul(rng.randrange(C.r), C.g1), C.g2_mul(rng.randrange(C.r), C.g2)) for _ in range(9)]
    f, e = pair(dev, tag, pairs, final_exp=False), pair(dev, tag, pairs)
    for i, pq in enumerate(pairs):
        assert f12(f[i]) == M.miller([pq]), f"pair {i}: the Miller value"
        assert M.final_exp(f12(f[i])) == f12(e[i]), f"pair {i}: the exponentiation"
