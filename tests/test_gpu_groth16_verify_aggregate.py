"""n Groth16 proofs in one randomised pairing check (csrc/pairing.hip groth16_verify_aggregate_dev) and its three
kernels: the Fq12 product reduction (pairing_product), the per-point scalar product (mul_scalars) and, through the verdicts, the
weighted input sums.  The per-proof path (verify_batch) and the per-pair pairing are pinned by the oracle elsewhere
(test_gpu_groth16_verify.py, test_gpu_pairing.py); here the oracle is asked for one pairing per curve and for the curve arithmetic.

Product reduction, final_exp=False: the product of the Miller values is compared EXACTLY (Fq12 arithmetic is exact and the output
canonical), which implies equality after any exponentiation; one size is also taken through Model.final_exp."""
import importlib, os, pathlib, random, subprocess, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
import key_check_ref as K  # noqa: E402
import pairing as PG  # noqa: E402
import pairing_constants as pc  # noqa: E402

CURVES = {"BN128": ("bn254", pc.BN254, PG.BN254, 4), "BLS12381": ("bls12_381", pc.BLS12_381, PG.BLS12_381, 6)}
TAGS = list(CURVES)
TD = [0x1234567, 0x2345678, 0x3456789, 0x456789a, 0x56789ab]
SEED = bytes(range(32))
# the product reduction's constants (csrc/pairing_impl.hip.h)
PR_GROUPS = 8                  # PR_GROUPS: groups of a wave
PR_PROD_BLOCK = 64             # PR_PROD_BLOCK = PR_GROUPS * PR_PROD_SHARE: more items open a second block and with it the second level
PRODUCT_SIZES = (1, PR_GROUPS - 1, PR_GROUPS, PR_GROUPS + 1, PR_PROD_BLOCK, PR_PROD_BLOCK + 1)   # the last needs every level


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


def _mont(q, nl, v): return [((v << (64 * nl)) % q >> (64 * i)) & (2**64 - 1) for i in range(nl)]


def enc(tag, p, g):
    """a key_check_ref point (None = infinity) -> the Montgomery words of the sums' layout"""
    KC, nl = K.CURVES[tag], CURVES[tag][3]
    if p is None: return np.zeros((4 if g else 2) * nl, np.uint64)
    return np.array(sum((_mont(KC.q, nl, c) for c in KC.coords(p, g)), []), dtype=np.uint64)


def gt_ints(row, nl): return [sum(int(row[j, i]) << (64 * i) for i in range(nl)) for j in range(12)]
def f12(gt): return [(gt[2 * k], gt[2 * k + 1]) for k in range(6)]


def to_flat(O, gt):
    flat = [0] * 12
    for k in range(6):
        flat[k] = (gt[2 * k] - O.xi0 * gt[2 * k + 1]) % O.Q; flat[k + 6] = gt[2 * k + 1]
    return flat


# ---- 1. the product reduction ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_pool(dev):
    """per curve: 65 pairs tiled from five distinct ones (two of them with a point at infinity), their per-pair values with and
    without the final exponentiation, computed once"""
    out = {}
    for tag in TAGS:
        KC, nl = K.CURVES[tag], CURVES[tag][3]
        P, Q = KC.gen
        kinds = [(KC.mul(P, 5), KC.mul(Q, 7)), (KC.mul(P, 11), Q), (None, KC.mul(Q, 3)), (KC.mul(P, 2), KC.mul(Q, 9)), (KC.mul(P, 13), None)]
        pairs = [kinds[i % 5] for i in range(PR_PROD_BLOCK + 1)]
        g1 = np.concatenate([enc(tag, p, 0) for p, _ in pairs]); g2 = np.concatenate([enc(tag, q, 1) for _, q in pairs])
        vals = {fe: [f12(gt_ints(row, nl)) for row in dev.pairing(g1, g2, tag, final_exp=fe)] for fe in (True, False)}
        out[tag] = (g1.reshape(len(pairs), -1), g2.reshape(len(pairs), -1), vals)
    return out


@pytest.mark.parametrize("final_exp", [True, False], ids=["exp", "miller"])
@pytest.mark.parametrize("tag", TAGS)
def test_product_equals_the_python_product_of_single_pairings(dev, pair_pool, tag, final_exp):
    _, C, _, nl = CURVES[tag]
    M = pc.Model(C)
    g1, g2, vals = pair_pool[tag]
    want, acc = {0: M.one()}, M.one()
    for i, v in enumerate(vals[final_exp]):
        acc = M.mul(acc, v); want[i + 1] = acc
    for n in (0,) + PRODUCT_SIZES:
        got = f12(gt_ints(dev.pairing_product(g1[:n], g2[:n], tag, final_exp=final_exp), nl))
        assert got == want[n], (tag, n, final_exp)
    if not final_exp:                                                      # and through the exponent, once
        n = PR_GROUPS + 1
        assert M.final_exp(want[n]) == f12(gt_ints(dev.pairing_product(g1[:n], g2[:n], tag), nl))


@pytest.mark.parametrize("tag", TAGS)
def test_product_of_three_pairs_is_the_generators_pairing_to_the_sum(dev, tag):
    """prod e([a_i]G1, [b_i]G2) = e(G1, G2)^(sum a_i b_i), e(G1, G2) from the oracle (one pairing)"""
    _, C, O, nl = CURVES[tag]
    KC = K.CURVES[tag]
    rng = random.Random(31)
    ab = [(rng.randrange(1, C.r), rng.randrange(1, C.r)) for _ in range(3)]
    g1 = np.concatenate([enc(tag, KC.mul(KC.gen[0], a), 0) for a, _ in ab]); g2 = np.concatenate([enc(tag, KC.mul(KC.gen[1], b), 1) for _, b in ab])
    got = gt_ints(dev.pairing_product(g1, g2, tag), nl)
    e = O.pairing(KC.coords(KC.gen[1], 1), KC.coords(KC.gen[0], 0))
    if tag == "BLS12381": e = e.inverse()                                  # the oracle does not conjugate for the negative curve parameter
    assert to_flat(O, got) == (e ** (sum(a * b for a, b in ab) % C.r)).c


# ---- 2. the per-point scalar product -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["g1", "g2"])
@pytest.mark.parametrize("tag", TAGS)
def test_mul_scalars_against_the_oracle(zk, dev, orc, tag, group):
    cv, C, _, nl = CURVES[tag]
    o = G.Groth16Oracle(orc, cv)
    oc = o.g2 if group else o.g1
    KC, rng = K.CURVES[tag], random.Random(17 + group)
    gen = o.point_from_ints(KC.coords(KC.gen[group], group))
    points = [gen, o.mul(oc, gen, rng.randrange(1, C.r)), None]
    scalars = [0, 1, 2, C.r - 1, 2**127, 2**128 - 1, rng.randrange(2**250, C.r)]
    pw = (4 if group else 2) * nl
    words = lambda p: np.zeros(pw, np.uint64) if p is None else np.asarray(p, np.uint64).reshape(-1)
    want = {(i, j): words(o.mul(oc, p, k)) for i, p in enumerate(points) for j, k in enumerate(scalars)}
    n_max = 257
    idx = [(t % 3, (t // 3 + t) % 7) for t in range(n_max)]               # every (point, scalar) pair occurs within the first 63
    assert len(set(idx[:63])) == 21
    for n in (1, 63, 64, 65, 257):
        d = zk.DevArray.from_host(np.concatenate([words(points[i]) for i, _ in idx[:n]]))
        got = dev.mul_scalars(d, [scalars[j] for _, j in idx[:n]], tag, "g2" if group else "g1").to_host().reshape(n, pw)
        for t, (i, j) in enumerate(idx[:n]):
            assert np.array_equal(got[t], want[(i, j)]), (tag, group, n, t, i, j)


# ---- 3 - 5. the aggregate check ---------------------------------------------------------------------------------------------------
def mul_circuit(r, n_pub):
    """wires: ONE, n_pub outputs, private a and b, three more products.  out_j = (a + j) b; t0 = a a, t1 = t0 b, t2 = t1 t1.
    -> (r1cs, witness(a, b)): any outputs a test wants, 0 and r - 1 among them, under one key"""
    ia, ib, it = 1 + n_pub, 2 + n_pub, 3 + n_pub
    cons = [(sorted(([(0, j)] if j else []) + [(ia, 1)]), [(ib, 1)], [(1 + j, 1)]) for j in range(n_pub)]
    cons += [([(ia, 1)], [(ia, 1)], [(it, 1)]), ([(it, 1)], [(ib, 1)], [(it + 1, 1)]), ([(it + 1, 1)], [(it + 1, 1)], [(it + 2, 1)])]
    def witness(a, b):
        t0 = a * a % r; t1 = t0 * b % r
        return [1] + [(a + j) * b % r for j in range(n_pub)] + [a, b, t0, t1, t1 * t1 % r]
    return dict(n_wires=6 + n_pub, n_pub_out=n_pub, n_pub_in=0, n_prv_in=2, constraints=cons), witness


def _proof_points(tag, js):
    a = ((int(js["pi_a"]["x"]), 0), (int(js["pi_a"]["y"]), 0)); c = ((int(js["pi_c"]["x"]), 0), (int(js["pi_c"]["y"]), 0))
    b = tuple((int(js["pi_b"][k][0]), int(js["pi_b"][k][1])) for k in "xy")
    return a, b, c


def build_made(dev, orc, n_pubs):
    """per (curve, n_pub): a key made on the device and four distinct honest proofs: dict(A, B, C points, pub, words)"""
    out = {}
    for tag in TAGS:
        cv, C = CURVES[tag][0], CURVES[tag][1]
        g = G.Groth16Oracle(orc, cv)
        for n_pub in n_pubs:
            r1cs, witness = mul_circuit(C.r, n_pub)
            rb = g.r1cs_bytes(r1cs)
            pb, vk_json = dev.keygen(tag, rb, TD)
            S = dev.Groth16Setup(tag, rb, pb)
            proofs = []
            for k, (a, b) in enumerate([(0, 5), (C.r - 1, 1), (12345, 678), (C.r - 2, C.r - 3)]):   # outputs 0 (a = 0), r - 1 ((r - 1) 1)
                w = witness(a, b)
                js, pts = S.prove(g.fr_array(w), r=1000 + k, s=2000 + k)
                A, B, Cc = _proof_points(tag, js)
                words = np.array(pts, np.uint64).reshape(-1)
                assert np.array_equal(words, np.concatenate([enc(tag, A, 0), enc(tag, B, 1), enc(tag, Cc, 0)]))
                proofs.append(dict(A=A, B=B, C=Cc, pub=w[1:1 + n_pub], words=words))
            S.free()
            if n_pub: assert proofs[0]["pub"][0] == 0 and proofs[1]["pub"][0] == C.r - 1
            out[(tag, n_pub)] = dict(vk_json=vk_json, vk=dev.Groth16VerifyingKey(tag, vk_json), proofs=proofs)
    return out


@pytest.fixture(scope="module")
def made(dev, orc):
    return build_made(dev, orc, (1, 3))


def with_points(tag, p, **kw):
    """a copy of a proof with points replaced (A=, B=, C=: key_check_ref points or raw word arrays) or inputs (pub=)"""
    q = dict(p); q.update(kw)
    part = lambda v, g: v if isinstance(v, np.ndarray) else enc(tag, v, g)
    q["words"] = np.concatenate([part(q["A"], 0), part(q["B"], 1), part(q["C"], 0)])
    return q


def run(vk, items, **kw):
    return vk.verify_aggregate(np.concatenate([p["words"] for p in items]), [p["pub"] for p in items], **kw)


def per_proof(vk, items):
    return [int(v) for v in vk.verify_batch(np.concatenate([p["words"] for p in items]), [p["pub"] for p in items])]


def first_bad(verdicts):
    return next(((v, i) for i, v in enumerate(verdicts) if v != 1), (1, None))


@pytest.mark.parametrize("n_pub", [1, 3])
@pytest.mark.parametrize("tag", TAGS)
def test_honest_batches_are_accepted(dev, made, tag, n_pub):
    m = made[(tag, n_pub)]
    for n in (0, 1, 2, 7, 8, 9, 64, 65):
        items = [m["proofs"][i % 4] for i in range(n)]                    # (from n = 2 on with the inputs 0 and r - 1)
        if n: assert run(m["vk"], items, seed=SEED) == (dev.ACCEPTED, None), (tag, n_pub, n)
        else: assert m["vk"].verify_aggregate(np.zeros(0, np.uint64), [], seed=SEED) == (dev.ACCEPTED, None)
    items = [m["proofs"][i % 4] for i in range(9)]
    assert run(m["vk"], items) == (dev.ACCEPTED, None)                     # the operating system's weights
    assert run(m["vk"], items, seed=SEED, locate=False) == (dev.ACCEPTED, None)


def test_no_public_inputs(dev, orc):
    m = build_made(dev, orc, (0,))
    for tag in TAGS:
        vk, pr = m[(tag, 0)]["vk"], m[(tag, 0)]["proofs"]
        assert per_proof(vk, pr) == [1, 1, 1, 1] and run(vk, pr, seed=SEED) == (dev.ACCEPTED, None)
        bad = pr[:2] + [with_points(tag, pr[2], C=pr[3]["C"])] + pr[3:]
        assert run(vk, bad, seed=SEED) == (dev.REJECTED, 2)


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import zkgpu_loader
zk = zkgpu_loader.load(); zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")
d = np.load(sys.argv[2], allow_pickle=True).item()
for tag, e in d.items():
    vk = dev.Groth16VerifyingKey(tag, e["vk_json"])
    assert vk.verify_aggregate(e["good"], e["pub"], seed=bytes(range(32))) == (dev.ACCEPTED, None), tag
    assert vk.verify_aggregate(e["bad"], e["pub"], seed=bytes(range(32))) == (dev.REJECTED, 16), tag
    whole = dev.pairing_product(e["g1"], e["g2"], tag)
    assert np.array_equal(whole, e["product"]), tag
print("child ok")
"""


def test_chunk_borders_in_a_fresh_process(dev, made, pair_pool, tmp_path):
    """ZK_VERIFY_AGG_CHUNK is read once: 17 proofs and 17 pairs in chunks of 8 (8 + 8 + 1), the running product carried across"""
    d = {}
    for tag in TAGS:
        m = made[(tag, 3)]
        items = [m["proofs"][i % 4] for i in range(17)]
        bad = items[:16] + [with_points(tag, items[16], C=items[15]["C"])]
        g1, g2, _ = pair_pool[tag]
        d[tag] = dict(vk_json=m["vk_json"], good=np.concatenate([p["words"] for p in items]), bad=np.concatenate([p["words"] for p in bad]),
                      pub=[p["pub"] for p in items], g1=g1[:17], g2=g2[:17], product=dev.pairing_product(g1[:17], g2[:17], tag))
    np.save(tmp_path / "in.npy", d, allow_pickle=True)
    (tmp_path / "child.py").write_text(_CHILD)
    env = dict(os.environ, ZK_VERIFY_AGG_CHUNK="8")
    r = subprocess.run([sys.executable, str(tmp_path / "child.py"), str(ROOT / "tests"), str(tmp_path / "in.npy")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("tag", TAGS)
def test_one_wrong_proof_is_located(dev, made, tag):
    m = made[(tag, 3)]
    KC = K.CURVES[tag]
    n = 10
    for at in (0, 7, 8, n - 1):
        items = [m["proofs"][i % 4] for i in range(n)]
        items[at] = with_points(tag, items[at], C=KC.add(items[at]["C"], KC.gen[0]))   # C + G: in the subgroup, wrong
        assert run(m["vk"], items, seed=SEED) == (dev.REJECTED, at), (tag, at)
        assert run(m["vk"], items, seed=SEED, locate=False) == (dev.REJECTED, None)
    items = [m["proofs"][i % 4] for i in range(n)]
    items[4] = with_points(tag, items[4], pub=[(items[4]["pub"][0] + 1) % KC.r] + items[4]["pub"][1:])
    assert run(m["vk"], items, seed=SEED) == (dev.REJECTED, 4)


@pytest.mark.parametrize("tag", TAGS)
def test_random_mixtures_agree_with_the_per_proof_path(dev, made, tag):
    KC = K.CURVES[tag]
    rng = random.Random(2024)
    for b in range(12):
        n_pub = (1, 3)[b % 2]
        m = made[(tag, n_pub)]
        n = rng.randrange(1, 17)
        items = []
        for i in range(n):
            p = m["proofs"][rng.randrange(4)]
            kind = rng.randrange(8) if b % 3 else 0                        # every third batch is all good
            if kind == 1: p = with_points(tag, p, A=KC.mul(p["A"], 2))
            elif kind == 2: p = with_points(tag, p, pub=[rng.randrange(KC.r) for _ in range(n_pub)])
            elif kind == 3: p = with_points(tag, p, C=KC.neg(p["C"]))
            items.append(p)
        want = first_bad(per_proof(m["vk"], items))
        assert run(m["vk"], items, seed=bytes([b] * 32)) == want, (tag, b)
        assert run(m["vk"], items, seed=bytes([b] * 32), locate=False)[0] == (dev.ACCEPTED if want[0] == 1 else dev.REJECTED)


def _vk_points(tag, vk_json):
    import json
    v = json.loads(vk_json); i = lambda s: int(s, 0)
    g1 = lambda p: ((i(p["x"]), 0), (i(p["y"]), 0)); g2 = lambda p: ((i(p["x"][0]), i(p["x"][1])), (i(p["y"][0]), i(p["y"][1])))
    return dict(alpha=g1(v["vk_alpha_1"]), beta=g2(v["vk_beta_2"]), gamma=g2(v["vk_gamma_2"]), delta=g2(v["vk_delta_2"]), ic=[g1(p) for p in v["IC"]])


@pytest.mark.parametrize("tag", TAGS)
def test_errors_that_cancel_without_weights_are_refused(dev, made, tag):
    """C_i + D and C_j - D: each proof fails alone, the plain product of the two equations holds (shown with pairing_product), and the
    weighted one must not, whatever the seed.  Then the same with the error in the inputs: x + d and x - d under one (A, B, C)."""
    KC, nl = K.CURVES[tag], CURVES[tag][3]
    m = made[(tag, 1)]
    vk, pr, V = m["vk"], m["proofs"], _vk_points(tag, m["vk_json"])
    D = KC.mul(KC.gen[0], 0xabcdef)
    def plain_product_is_one(items):
        g1, g2 = [], []
        for p in items:
            X = KC.add(V["ic"][0], KC.mul(V["ic"][1], p["pub"][0]))
            for a, b in ((p["A"], p["B"]), (X, KC.neg(V["gamma"])), (p["C"], KC.neg(V["delta"])), (V["alpha"], KC.neg(V["beta"]))):
                g1.append(enc(tag, a, 0)); g2.append(enc(tag, b, 1))
        return gt_ints(dev.pairing_product(np.concatenate(g1), np.concatenate(g2), tag), nl) == [1] + [0] * 11
    assert plain_product_is_one([pr[2], pr[3]])                            # (the harness itself: two honest proofs)
    pair_c = [with_points(tag, pr[2], C=KC.add(pr[2]["C"], D)), with_points(tag, pr[3], C=KC.add(pr[3]["C"], KC.neg(D)))]
    d = 77
    pair_x = [with_points(tag, pr[2], pub=[(pr[2]["pub"][0] + d) % KC.r]), with_points(tag, pr[2], pub=[(pr[2]["pub"][0] - d) % KC.r])]
    for pair in (pair_c, pair_x):
        assert per_proof(vk, pair) == [0, 0] and plain_product_is_one(pair)
        for s in (1, 2, 3):
            assert run(vk, pair, seed=bytes([s] * 32)) == (dev.REJECTED, 0), (tag, s)
            assert run(vk, [pr[0]] + pair + [pr[1]], seed=bytes([s] * 32)) == (dev.REJECTED, 1)
    assert run(vk, pair_c) == (dev.REJECTED, 0)                            # and with the operating system's weights


def _outside_subgroup(KC, g):
    x = 1
    while True:
        p = KC.lift_x((x, 1 if g else 0), g); x += 1
        if p and KC.classify(KC.coords(p, g), g) == "not_in_subgroup": return p


@pytest.mark.parametrize("tag", TAGS)
def test_malformed_input_gets_the_per_proof_code_and_index(dev, made, tag):
    KC = K.CURVES[tag]
    m = made[(tag, 3)]
    vk, pr = m["vk"], m["proofs"]
    off = lambda p, g: (p[0], KC.fadd(p[1], (1, 0)))                       # y + 1: off the curve
    cases = [("A off the curve", dict(A=off(pr[1]["A"], 0)), dev.NOT_ON_CURVE),
             ("B off the curve", dict(B=off(pr[1]["B"], 1)), dev.NOT_ON_CURVE),
             ("C off the curve", dict(C=off(pr[1]["C"], 0)), dev.NOT_ON_CURVE),
             ("B outside the subgroup", dict(B=_outside_subgroup(KC, 1)), dev.NOT_IN_SUBGROUP),
             ("an input equal to r", dict(pub=[pr[1]["pub"][0], KC.r, pr[1]["pub"][2]]), dev.INPUT_NOT_CANONICAL),
             ("A all zero", dict(A=None), dev.REJECTED)]
    if tag == "BLS12381":
        cases += [("A outside the subgroup", dict(A=_outside_subgroup(KC, 0)), dev.NOT_IN_SUBGROUP),
                  ("C outside the subgroup", dict(C=_outside_subgroup(KC, 0)), dev.NOT_IN_SUBGROUP)]
    for k, (what, change, code) in enumerate(cases):
        n = 9
        at = (3 * k + 1) % n
        items = [pr[i % 4] for i in range(n)]
        items[at] = with_points(tag, pr[1], **change)
        want = per_proof(vk, items)
        assert want == [1] * at + [code] + [1] * (n - at - 1), what
        assert run(vk, items, seed=SEED) == (code, at), what
        assert run(vk, items, seed=SEED, locate=False) == (dev.REJECTED, None), what
    # two kinds in one batch: the first in order is reported, with its own code
    items = [pr[i % 4] for i in range(6)]
    items[4] = with_points(tag, pr[0], A=off(pr[0]["A"], 0)); items[2] = with_points(tag, pr[2], pub=[KC.r + 5, 1, 2])
    assert run(vk, items, seed=SEED) == (dev.INPUT_NOT_CANONICAL, 2)
    # settled on the host, as verify_batch does: a wrong number of inputs
    items = [pr[0], dict(pr[1], pub=pr[1]["pub"] + [1]), pr[2]]
    assert run(vk, items, seed=SEED) == (dev.INPUT_COUNT, 1) and first_bad(per_proof(vk, items)) == (dev.INPUT_COUNT, 1)
