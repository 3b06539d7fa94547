"""eigen_zkvm_amd.fflonk end to end on the device against tests/fflonk_ref.py, over powers-of-tau files with a KNOWN tau (as
test_gpu_plonk.py builds them): with fixed blinders and with none, the device's proof equals the reference's BYTE FOR BYTE -- its points are
[scalar] G of the reference's scalars from the fixed-base kernel, its values the reference's integers.  The circuits are the chain
x^3 + x + 5 = y of plonk_ref.chain at n = 8 (the tightest degree: T2's 3n + 6 = 30 of 32 coefficients), 16 and 512 (a file of power 12 holds
9 x 512 + 18 powers) on BN128 and n = 16 on BLS12381.  Then batches, random blinders, every rejection at n = 16, and the prover's refusals.
Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import fflonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
POWER = {"BN128": 12, "BLS12381": 7}                    # 2^(power + 1) - 1 powers: at least 9n + 18 for n = 512 and n = 16
STEPS = {8: 1, 16: 3, 512: 127}
SEED = bytes(range(32))
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(9)]
ACCEPTED, REJECTED, NOT_CANONICAL = 1, 0, -1
SIZES = [("BN128", 8), ("BN128", 16), ("BN128", 512), ("BLS12381", 16)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def fflonk(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk")


@pytest.fixture(scope="module")
def handles(zk, tmp_path_factory):
    g16, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    d = tmp_path_factory.mktemp("fflonk")
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
def world(zk, fflonk, handles):
    """per (curve, n): the circuit, its witness, the device key and the reference, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(cv, n):
        if (cv, n) not in made:
            n_vars, public, gates, wit = ref.chain(STEPS[n], ref.R[cv])
            circuit = fflonk.Circuit(n_vars, public, gates, cv)
            assert circuit.n == n
            made[(cv, n)] = (circuit, wit, fflonk.FflonkKey(handles[cv], circuit), ref.Reference(cv, n_vars, public, gates, TAU[cv], points[cv]))
        return made[(cv, n)]
    get.points = points
    yield get
    for _, _, key, _ in made.values():
        key.free()


@pytest.mark.parametrize("blind", (BLIND, [0] * 9), ids=("blinded", "unblinded"))
@pytest.mark.parametrize("cv,n", SIZES)
def test_the_device_proof_is_the_reference_proof_byte_for_byte(zk, fflonk, handles, world, cv, n, blind):
    circuit, wit, key, R = world(cv, n)
    assert handles[cv].max_coeffs >= fflonk.required_powers(n)
    assert key.vk.c0 == R.C0 and (key.k1, key.k2) == R.t.k[1:] and key.vk.digest == R.vkd
    assert not hasattr(key, "commitments")                                            # one point, not eight
    want = R.prove(wit, blind)
    proof, publics = fflonk.prove(key, wit, blinding=blind)
    assert publics == want["publics"] == [wit[-1]]
    assert proof["values"] == want["values"]
    for name in fflonk.POINT_NAMES:
        assert proof[name] == want["proof"][name], name
    assert fflonk.proof_to_bytes(proof) == fflonk.proof_to_bytes(want["proof"])
    assert fflonk.challenges(key.vk, publics, proof) == want["challenges"]
    assert fflonk.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    assert fflonk.verify(key.vk, [publics], [proof], seed=SEED, locate=False) == (ACCEPTED, None)
    if any(blind):                                                                    # the blinders reach both commitments
        plain = R.prove(wit, [0] * 9)
        assert all(plain["proof"][k] != proof[k] for k in ("C1", "C2"))


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_keys_and_proofs_go_through_json_and_bytes(fflonk, handles, world, cv):
    circuit, wit, key, R = world(cv, 16)
    proof, publics = fflonk.prove(key, wit, blinding=BLIND)
    for vk in (fflonk.vk_from_json(fflonk.vk_to_json(key.vk)), fflonk.vk_from_bytes(fflonk.vk_to_bytes(key.vk))):
        assert (vk.curve, vk.log_n, vk.n_public, vk.k1, vk.k2, vk.c0, vk.digest) == (cv, 4, 1, key.k1, key.k2, key.vk.c0, key.vk.digest)
        back = fflonk.proof_from_json(fflonk.proof_to_json(proof, cv), cv)
        assert back == proof == fflonk.proof_from_bytes(fflonk.proof_to_bytes(proof), handles[cv].point_bytes)
        assert fflonk.verify(vk, [publics], [back], kzg=handles[cv]) == (ACCEPTED, None)
        with pytest.raises(fflonk.ZkError, match="verify needs the Kzg handle"):
            fflonk.verify(vk, [publics], [back])


def test_batches_and_random_blinders(fflonk, world):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    made = [fflonk.prove(key, wit) for _ in range(3)]                                # blinders from `secrets`
    proofs, publics = [p for p, _ in made], [x for _, x in made]
    assert fflonk.verify(key.vk, publics, proofs) == (ACCEPTED, None)
    assert fflonk.verify(key.vk, publics, proofs, seed=SEED) == (ACCEPTED, None)
    for name in fflonk.POINT_NAMES:
        assert len({p[name] for p in proofs}) == 3, name                             # every point moves with the blinders
    for i in range(8, 15):                                                            # and every value of a, b, c, Z, T1, T2
        assert len({p["values"][i] for p in proofs}) == 3, i
    # one bad proof in the batch is named, wherever it stands and whichever way it is bad
    moved = dict(proofs[1], values=proofs[1]["values"][:12] + [(proofs[1]["values"][12] + 1) % r] + proofs[1]["values"][13:])
    other_w = dict(proofs[1], W2=proofs[0]["W2"])
    for at in range(3):
        for bad in (moved, other_w):
            batch = proofs[:at] + [bad] + proofs[at + 1:]
            assert fflonk.verify(key.vk, publics, batch) == (REJECTED, at), at
            assert fflonk.verify(key.vk, publics, batch, seed=SEED, locate=False) == (REJECTED, None), at
    big = dict(proofs[2], values=[r] + proofs[2]["values"][1:])                       # a pairing failure before a host refusal is the first bad one
    assert fflonk.verify(key.vk, publics, [proofs[0], moved, big]) == (REJECTED, 1)
    assert fflonk.verify(key.vk, publics, [proofs[0], proofs[1], big]) == (NOT_CANONICAL, 2)


def test_rejections(zk, fflonk, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r, vk = R.r, key.vk
    proof, publics = fflonk.prove(key, wit, blinding=BLIND)
    assert fflonk.verify(vk, [publics], [proof]) == (ACCEPTED, None)
    for i in range(15):                                                               # each of the 15 values + 1
        bad = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert fflonk.verify(vk, [publics], [bad]) == (REJECTED, 0), i
    other = world.points[cv](0xABCDEF)
    for name in fflonk.POINT_NAMES:                                                   # each of the 4 points replaced by another valid point
        assert fflonk.verify(vk, [publics], [dict(proof, **{name: other})]) == (REJECTED, 0), name
    assert fflonk.verify(vk, [[(publics[0] + 1) % r]], [proof]) == (REJECTED, 0)      # the public input + 1
    assert fflonk.verify(fflonk.VerifyingKey(cv, vk.log_n, vk.n_public, vk.k1, vk.k2, other, handles[cv]), [publics], [proof]) == (REJECTED, 0)       # another [C0]
    # the same gates with one wire moved to a fresh variable: another sigma, another key
    n_vars, public, gates, _ = ref.chain(STEPS[16], r)
    gates = {k: list(v) for k, v in gates.items()}
    gates["b"][5] = n_vars
    key2 = fflonk.FflonkKey(handles[cv], fflonk.Circuit(n_vars + 1, public, gates, cv))
    try:
        assert key2.vk.c0 != vk.c0
        assert fflonk.verify(key2.vk, [publics], [proof]) == (REJECTED, 0)
    finally:
        key2.free()
    _, wit8, key8, _ = world(cv, 8)                                                   # the other circuit size
    assert fflonk.verify(key8.vk, [publics], [proof]) == (REJECTED, 0)
    proof8, publics8 = fflonk.prove(key8, wit8, blinding=BLIND)
    assert fflonk.verify(vk, [publics8], [proof8]) == (REJECTED, 0) and fflonk.verify(key8.vk, [publics8], [proof8]) == (ACCEPTED, None)
    for i in (0, 11, 14):                                                             # a value equal to r
        assert fflonk.verify(vk, [publics], [dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])]) == (NOT_CANONICAL, 0), i
    assert fflonk.verify(vk, [[r]], [proof]) == (NOT_CANONICAL, 0)
    with pytest.raises(fflonk.ZkError, match="a proof holds 15 values"):              # truncated
        fflonk.verify(vk, [publics], [dict(proof, values=proof["values"][:14])])
    with pytest.raises(fflonk.ZkError, match="a proof is"):
        fflonk.proof_from_bytes(fflonk.proof_to_bytes(proof)[:-32], handles[cv].point_bytes)
    with pytest.raises(fflonk.ZkError, match="point C2 of the proof is 63 bytes"):
        fflonk.verify(vk, [publics], [dict(proof, C2=proof["C2"][:-1])])
    with pytest.raises(fflonk.ZkError, match="2 public inputs, the verification key has 1"):
        fflonk.verify(vk, [publics * 2], [proof])
    # the prover takes the opening's gamma' from the KZG layer's default transcript instead of the chained one: an honest opening under
    # challenges the verifier does not derive.  The verifier uses its own and refuses
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    loose, _ = fflonk.prove(key, wit, blinding=BLIND, self_check=False, _opening_transcript=kzg.challenges_of)
    assert loose["values"] == proof["values"] and all(loose[k] == proof[k] for k in ("C1", "C2")) and loose["W1"] != proof["W1"]
    ch = fflonk.challenges(vk, publics, loose)
    _, tup = fflonk.host_check(vk, publics, loose)
    cs, sets, vals = tup[:3]
    g = kzg.challenges_of(cv, cs, sets, vals)
    z = kzg.challenge_z(cv, g, loose["W1"], avoid=[p for s in sets for p in s])
    assert handles[cv].verify_multi([(cs, sets, vals, g, z, loose["W1"], loose["W2"])]) == (ACCEPTED, None)      # sound under ITS challenges
    assert g != ch["gamma_open"] and fflonk.verify(vk, [publics], [loose]) == (REJECTED, 0)
    # and a proof that carries its prover's challenges along is not believed either
    assert fflonk.verify(vk, [publics], [dict(loose, gamma_open=g, z_open=z)]) == (REJECTED, 0)


def test_the_prover_refuses_a_bad_witness_and_a_small_file(zk, fflonk, handles, world, tmp_path):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    bad = list(wit)
    bad[5] = (bad[5] + 1) % r                                                         # one variable wrong
    rows = R.gates_hold(R.wires_of(bad), [bad[-1]])
    assert rows
    with pytest.raises(fflonk.ZkError, match=r"witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
        fflonk.prove(key, bad, blinding=BLIND)
    bad = list(wit)
    bad[-1] = (bad[-1] + 1) % r                                                       # the public input: its own row holds, the gate that made it does not
    rows = R.gates_hold(R.wires_of(bad), [bad[-1]])
    with pytest.raises(fflonk.ZkError, match=r"witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
        fflonk.prove(key, bad, blinding=BLIND)
    # wire values that satisfy every gate but break a copy: row 2 is x + x - 2x = 0 for any x
    wires = R.wires_of(wit)
    for k in "abc":
        wires[k][2] = (wires[k][2] + 9) % r
    assert not R.gates_hold(wires, [wit[-1]])
    with pytest.raises(fflonk.ZkError, match="the permutation product does not close"):
        fflonk.prove(key, wit, blinding=BLIND, _wires=[wires[k] for k in "abc"])
    proof, _ = fflonk.prove(key, wit, blinding=BLIND, _wires=[R.wires_of(wit)[k] for k in "abc"])       # the hook itself is sound
    assert proof == R.prove(wit, BLIND)["proof"]
    # a file too small: power 6 holds 127 powers, fewer than 9n + 18 = 162
    kzg, g16 = importlib.import_module("eigen_zkvm_amd.kzg"), importlib.import_module("eigen_zkvm_amd.groth16")
    path = tmp_path / "small.ptau"
    path.write_bytes(make_test_ptau.build_ptau(zk, "BN128", 6, TAU["BN128"], 5, 7))
    srs = g16.Srs("BN128", path)
    small = kzg.Kzg(srs)
    srs.free()
    try:
        with pytest.raises(fflonk.ZkError, match=r"the file holds 127 G1 powers, n = 16 rows need 9n \+ 18 = 162 \(a file of power 7 has them\)"):
            fflonk.FflonkKey(small, circuit)
    finally:
        small.free()
