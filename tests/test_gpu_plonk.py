"""eigen_zkvm_amd.plonk end to end on the device against tests/plonk_ref.py, over powers-of-tau files with a KNOWN tau (as
test_gpu_kzg_multi.py builds them): with fixed blinders and with none, the device's proof equals the reference's BYTE FOR BYTE -- its points
are [scalar] G of the reference's scalars from the fixed-base kernel, its values the reference's integers.  The circuits are the chain
x^3 + x + 5 = y of plonk_ref.chain at n = 8 (the tightest degree: 3n + 6 = 30 of 32 coefficients), 16 and 4096 (more than one tile of the
grand product's scan) on BN128 and n = 16 on BLS12381.  Then batches, random blinders, every rejection at n = 16, and the prover's refusals.
Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import plonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
POWER = {"BN128": 13, "BLS12381": 5}                    # 4n - 1 powers for n = 4096 and n = 16: at least 3n + 6
STEPS = {8: 1, 16: 3, 4096: 1023}
SEED = bytes(range(32))
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(9)]
ACCEPTED, REJECTED, NOT_CANONICAL = 1, 0, -1
SIZES = [("BN128", 8), ("BN128", 16), ("BN128", 4096), ("BLS12381", 16)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


@pytest.fixture(scope="module")
def handles(zk, tmp_path_factory):
    g16, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    d = tmp_path_factory.mktemp("plonk")
    hs = {}
    for cv in POWER:
        p = d / (cv + ".ptau")
        p.write_bytes(make_test_ptau.build_ptau(zk, cv, POWER[cv], TAU[cv], 5, 7))
        srs = g16.Srs(cv, p)
        hs[cv] = kzg.Kzg(srs)
        srs.free()
    yield hs
    for h in hs.values():
        h.free()


class Points:
    """[k] G as bytes in the layout of the sums, remembered"""

    def __init__(self, zk, cv):
        self.zk, self.cv, self.seen = zk, cv, {}

    def __call__(self, k):
        if k not in self.seen:
            w = np.array([(k >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
            self.seen[k] = self.zk.mul_generator_fr(self.zk.DevArray.from_host(w), ABI[self.cv]).to_host().astype("<u8").tobytes()
        return self.seen[k]


@pytest.fixture(scope="module")
def world(zk, plonk, handles):
    """per (curve, n): the circuit, its witness, the device key and the reference, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(cv, n):
        if (cv, n) not in made:
            n_vars, public, gates, wit = ref.chain(STEPS[n], ref.R[cv])
            circuit = plonk.Circuit(n_vars, public, gates, cv)
            assert circuit.n == n
            made[(cv, n)] = (circuit, wit, plonk.PlonkKey(handles[cv], circuit), ref.Reference(cv, n_vars, public, gates, TAU[cv], points[cv]))
        return made[(cv, n)]
    get.points = points
    yield get
    for _, _, key, _ in made.values():
        key.free()


@pytest.mark.parametrize("blind", (BLIND, [0] * 9), ids=("blinded", "unblinded"))
@pytest.mark.parametrize("cv,n", SIZES)
def test_the_device_proof_is_the_reference_proof_byte_for_byte(zk, plonk, handles, world, cv, n, blind):
    circuit, wit, key, R = world(cv, n)
    if n == 4096:
        assert n > zk.lib().zk_frpoly_tile_elems()                                   # the grand product spans more than one tile
    assert key.vk.commitments == R.vk_points and (key.k1, key.k2) == R.t.k[1:] and key.vk.digest == R.vkd
    want = R.prove(wit, blind)
    proof, publics = plonk.prove(key, wit, blinding=blind)
    assert publics == want["publics"] == [wit[-1]]
    assert proof["values"] == want["values"]
    for name in plonk.POINT_NAMES:
        assert proof[name] == want["proof"][name], name
    assert plonk.proof_to_bytes(proof) == plonk.proof_to_bytes(want["proof"])
    assert plonk.challenges(key.vk, publics, proof) == want["challenges"]
    assert plonk.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    assert plonk.verify(key.vk, [publics], [proof], seed=SEED, locate=False) == (ACCEPTED, None)
    if any(blind):                                                                    # the blinders reach every commitment they should
        plain = R.prove(wit, [0] * 9)
        assert all(plain["proof"][k] != proof[k] for k in ("A", "B", "C", "Z", "T"))


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_keys_and_proofs_go_through_json(plonk, handles, world, cv):
    circuit, wit, key, R = world(cv, 16)
    proof, publics = plonk.prove(key, wit, blinding=BLIND)
    vk = plonk.vk_from_json(plonk.vk_to_json(key.vk))
    assert (vk.curve, vk.log_n, vk.n_public, vk.k1, vk.k2, vk.commitments, vk.digest) == (cv, 4, 1, key.k1, key.k2, key.vk.commitments, key.vk.digest)
    back = plonk.proof_from_json(plonk.proof_to_json(proof, cv), cv)
    assert back == proof
    assert plonk.verify(vk, [publics], [back], kzg=handles[cv]) == (ACCEPTED, None)
    with pytest.raises(plonk.ZkError, match="verify needs the Kzg handle"):
        plonk.verify(vk, [publics], [back])


def test_batches_and_random_blinders(plonk, world):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    made = [plonk.prove(key, wit) for _ in range(3)]                                 # blinders from `secrets`
    proofs, publics = [p for p, _ in made], [x for _, x in made]
    assert plonk.verify(key.vk, publics, proofs) == (ACCEPTED, None)
    assert plonk.verify(key.vk, publics, proofs, seed=SEED) == (ACCEPTED, None)
    for name in ("A", "B", "C", "Z", "T", "W1", "W2"):
        assert len({p[name] for p in proofs}) == 3, name                             # every commitment moves with the blinders
    for i in (8, 9, 10, 11, 12, 13):                                                  # and every value of a, b, c, t, Z
        assert len({p["values"][i] for p in proofs}) == 3, i
    assert len({tuple(p["values"][:8]) for p in proofs}) == 3                        # (the fixed polynomials' values move with zeta)
    # one bad proof in the batch is named, wherever it stands and whichever way it is bad
    moved = dict(proofs[1], values=proofs[1]["values"][:12] + [(proofs[1]["values"][12] + 1) % r] + proofs[1]["values"][13:])
    other_w = dict(proofs[1], W2=proofs[0]["W2"])
    for at in range(3):
        for bad, code in ((moved, REJECTED), (other_w, REJECTED)):
            batch = proofs[:at] + [bad] + proofs[at + 1:]
            assert plonk.verify(key.vk, publics, batch) == (code, at), at
            assert plonk.verify(key.vk, publics, batch, seed=SEED, locate=False) == (REJECTED, None), at
    # a pairing failure before a host refusal is the first bad one
    assert plonk.verify(key.vk, publics, [other_w, proofs[1], moved]) == (REJECTED, 0)
    assert plonk.verify(key.vk, publics, [proofs[0], moved, other_w]) == (REJECTED, 1)


def test_rejections(zk, plonk, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r, vk = R.r, key.vk
    proof, publics = plonk.prove(key, wit, blinding=BLIND)
    assert plonk.verify(vk, [publics], [proof]) == (ACCEPTED, None)
    for i in range(14):                                                               # each of the 14 values + 1
        bad = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert plonk.verify(vk, [publics], [bad]) == (REJECTED, 0), i
    other = world.points[cv](0xABCDEF)
    for name in plonk.POINT_NAMES:                                                    # each of the 7 points replaced by another valid point
        assert plonk.verify(vk, [publics], [dict(proof, **{name: other})]) == (REJECTED, 0), name
    assert plonk.verify(vk, [[(publics[0] + 1) % r]], [proof]) == (REJECTED, 0)       # the public input + 1
    # the same gates with one wire moved to a fresh variable: another sigma, another key
    n_vars, public, gates, _ = ref.chain(STEPS[16], r)
    gates = {k: list(v) for k, v in gates.items()}
    gates["b"][5] = n_vars
    key2 = plonk.PlonkKey(handles[cv], plonk.Circuit(n_vars + 1, public, gates, cv))
    try:
        assert key2.vk.commitments[:5] == vk.commitments[:5] and key2.vk.commitments[5:] != vk.commitments[5:]
        assert plonk.verify(key2.vk, [publics], [proof]) == (REJECTED, 0)
    finally:
        key2.free()
    _, wit8, key8, _ = world(cv, 8)                                                   # the other circuit size
    assert plonk.verify(key8.vk, [publics], [proof]) == (REJECTED, 0)
    proof8, publics8 = plonk.prove(key8, wit8, blinding=BLIND)
    assert plonk.verify(vk, [publics8], [proof8]) == (REJECTED, 0) and plonk.verify(key8.vk, [publics8], [proof8]) == (ACCEPTED, None)
    for i in (0, 11, 13):                                                             # a value equal to r
        assert plonk.verify(vk, [publics], [dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])]) == (NOT_CANONICAL, 0), i
    assert plonk.verify(vk, [[r]], [proof]) == (NOT_CANONICAL, 0)
    with pytest.raises(plonk.ZkError, match="a proof holds 14 values"):               # truncated
        plonk.verify(vk, [publics], [dict(proof, values=proof["values"][:13])])
    with pytest.raises(plonk.ZkError, match="a proof is"):
        plonk.proof_from_bytes(plonk.proof_to_bytes(proof)[:-32], handles[cv].point_bytes)
    with pytest.raises(plonk.ZkError, match="point T of the proof is 63 bytes"):
        plonk.verify(vk, [publics], [dict(proof, T=proof["T"][:-1])])
    # the prover takes the opening's gamma' from the KZG layer's default transcript instead of the chained one: an honest opening under
    # challenges the verifier does not derive.  The verifier uses its own and refuses
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    loose, _ = plonk.prove(key, wit, blinding=BLIND, self_check=False, _opening_transcript=kzg.challenges_of)
    assert loose["values"] == proof["values"] and all(loose[k] == proof[k] for k in ("A", "B", "C", "Z", "T")) and loose["W1"] != proof["W1"]
    ch = plonk.challenges(vk, publics, loose)
    _, tup = plonk.host_check(vk, publics, loose)
    cs, sets, vals = tup[:3]
    g = kzg.challenges_of(cv, cs, sets, vals)
    z = kzg.challenge_z(cv, g, loose["W1"], avoid=sets[12])
    assert handles[cv].verify_multi([(cs, sets, vals, g, z, loose["W1"], loose["W2"])]) == (ACCEPTED, None)      # sound under ITS challenges
    assert g != ch["gamma_open"] and plonk.verify(vk, [publics], [loose]) == (REJECTED, 0)
    # and a proof that carries its prover's challenges along is not believed either
    assert plonk.verify(vk, [publics], [dict(loose, gamma_open=g, z_open=z)]) == (REJECTED, 0)


def test_the_prover_refuses_a_bad_witness(plonk, world):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    bad = list(wit)
    bad[5] = (bad[5] + 1) % r                                                         # one variable wrong
    rows = R.gates_hold(R.wires_of(bad), [bad[-1]])
    assert rows
    with pytest.raises(plonk.ZkError, match=r"witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
        plonk.prove(key, bad, blinding=BLIND)
    bad = list(wit)
    bad[-1] = (bad[-1] + 1) % r                                                       # the public input: its own row holds, the gate that made it does not
    rows = R.gates_hold(R.wires_of(bad), [bad[-1]])
    with pytest.raises(plonk.ZkError, match=r"witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
        plonk.prove(key, bad, blinding=BLIND)
    # wire values that satisfy every gate but break a copy: row 2 is x + x - 2x = 0 for any x
    wires = R.wires_of(wit)
    for k in "abc":
        wires[k][2] = (wires[k][2] + 9) % r
    assert not R.gates_hold(wires, [wit[-1]])
    with pytest.raises(plonk.ZkError, match="the permutation product does not close"):
        plonk.prove(key, wit, blinding=BLIND, _wires=[wires[k] for k in "abc"])
    proof, _ = plonk.prove(key, wit, blinding=BLIND, _wires=[R.wires_of(wit)[k] for k in "abc"])        # the hook itself is sound
    assert proof == R.prove(wit, BLIND)["proof"]
