"""eigen_zkvm_amd.plonk_next end to end on the device against tests/plonk_next_ref.py, over powers-of-tau files with a KNOWN
tau: with fixed blinders and with none, the device's proof equals the model's BYTE FOR BYTE.  The circuits are plonk_next_ref.running_sums: a
chain that crosses rows and lands in a closing gate at n = 8 (the tightest degree: 3n + 7 = 31 of 32 coefficients), the same and a second
chain that lands in a row of its own at n = 16 and n = 256 on BN128 and at n = 16 on BLS12381.  Then a plonk.Circuit table proved here with
q_N = 0, a batch with one bad proof located, every rejection at n = 16, the prover's refusals -- a witness that breaks only a next-row
relation named by its row -- and the two provers refusing each other's keys and proofs.  Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import plonk_next_ref as nref
import plonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
POWER = {"BN128": 9, "BLS12381": 5}                     # 4n - 1 powers for n = 256 and n = 16: at least 3n + 7
TERMS = {8: (3, False), 16: (5, True), 256: (249, True)}        # n -> (terms of the sum, the sum twice)
SEED = bytes(range(32))
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(10)]
ACCEPTED, REJECTED, NOT_CANONICAL = 1, 0, -1
SIZES = [("BN128", 8), ("BN128", 16), ("BN128", 256), ("BLS12381", 16)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def pn(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_next")


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


@pytest.fixture(scope="module")
def handles(zk, tmp_path_factory):
    g16, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    d = tmp_path_factory.mktemp("plonk_next")
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


def circuit_of(cv, n):
    r = nref.R[cv]
    m, twice = TERMS[n]
    return nref.running_sums([(r - 1 - 3 * i, 1000 + 7 * i) for i in range(m)], r, twice=twice)


@pytest.fixture(scope="module")
def world(zk, pn, handles):
    """per (curve, n): the circuit, its witness, the device key and the model, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(cv, n):
        if (cv, n) not in made:
            n_vars, public, gates, wit = circuit_of(cv, n)
            circuit = pn.NextCircuit(n_vars, public, gates, cv)
            assert circuit.n == n and circuit.sel["qN"].any()
            made[(cv, n)] = (circuit, wit, pn.NextKey(handles[cv], circuit), nref.Reference(cv, n_vars, public, gates, TAU[cv], points[cv]))
        return made[(cv, n)]
    get.points = points
    yield get
    for _, _, key, _ in made.values():
        key.free()


@pytest.mark.parametrize("blind", (BLIND, [0] * 10), ids=("blinded", "unblinded"))
@pytest.mark.parametrize("cv,n", SIZES)
def test_the_device_proof_is_the_model_proof_byte_for_byte(zk, pn, handles, world, cv, n, blind):
    circuit, wit, key, R = world(cv, n)
    assert key.vk.commitments == R.vk_points and len(R.vk_points) == 9 and (key.k1, key.k2) == R.t.k[1:] and key.vk.digest == R.vkd
    want = R.prove(wit, blind)
    proof, publics = pn.prove(key, wit, blinding=blind)
    assert publics == want["publics"] == [wit[circuit.public[0]]]
    assert len(proof["values"]) == 16 and proof["values"] == want["values"]
    for name in pn.POINT_NAMES:
        assert proof[name] == want["proof"][name], name
    assert pn.proof_to_bytes(proof) == pn.proof_to_bytes(want["proof"])
    assert pn.challenges(key.vk, publics, proof) == want["challenges"]
    assert pn.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    assert pn.verify(key.vk, [publics], [proof], seed=SEED, locate=False) == (ACCEPTED, None)
    if any(blind):                                                                    # the blinders reach every commitment they should
        plain = R.prove(wit, [0] * 10)
        assert all(plain["proof"][k] != proof[k] for k in ("A", "B", "C", "Z", "T"))
        assert plain["values"][15] != proof["values"][15] and plain["values"][11] != proof["values"][11]    # c at both points


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_a_plonk_circuit_table_proves_here_with_qN_zero(pn, plonk, handles, world, cv):
    r = ref.R[cv]
    n_vars, public, gates, wit = ref.chain(3, r)
    circuit = plonk.Circuit(n_vars, public, gates, cv)                                 # plonk.py's own class: no qN anywhere
    key = pn.NextKey(handles[cv], circuit)
    try:
        R = nref.Reference(cv, n_vars, public, gates, TAU[cv], world.points[cv])
        assert key.vk.commitments == R.vk_points and R.fixed_tau["qN"] == 0
        want = R.prove(wit, BLIND)
        proof, publics = pn.prove(key, wit, blinding=BLIND)
        assert proof == want["proof"] and proof["values"][8] == 0                      # q_N(zeta) = 0
        assert pn.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
        pkey = plonk.PlonkKey(handles[cv], circuit)                                    # the same table under plonk.py: the same 8 commitments, another protocol
        try:
            assert pkey.vk.commitments == key.vk.commitments[:8] and pkey.vk.digest != key.vk.digest
        finally:
            pkey.free()
    finally:
        key.free()


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_keys_and_proofs_go_through_json_and_the_two_provers_refuse_each_others(pn, plonk, handles, world, cv):
    circuit, wit, key, R = world(cv, 16)
    proof, publics = pn.prove(key, wit, blinding=BLIND)
    vk = pn.vk_from_json(pn.vk_to_json(key.vk))
    assert (vk.curve, vk.log_n, vk.n_public, vk.k1, vk.k2, vk.commitments, vk.digest) == (cv, 4, 1, key.k1, key.k2, key.vk.commitments, key.vk.digest)
    back = pn.proof_from_json(pn.proof_to_json(proof, cv), cv)
    assert back == proof and pn.proof_from_bytes(pn.proof_to_bytes(proof), handles[cv].point_bytes) == proof
    assert pn.verify(vk, [publics], [back], kzg=handles[cv]) == (ACCEPTED, None)
    with pytest.raises(pn.ZkError, match="verify needs the Kzg handle"):
        pn.verify(vk, [publics], [back])
    # real keys and proofs of either prover at the other's door
    n_vars, public, gates, pw = ref.chain(3, ref.R[cv])
    pkey = plonk.PlonkKey(handles[cv], plonk.Circuit(n_vars, public, gates, cv))
    try:
        pproof, ppublics = plonk.prove(pkey, pw, blinding=BLIND[:9])
        with pytest.raises(pn.ZkError, match='^plonk next: not a verification key of this prover \\(protocol "plonk-shplonk"\\)$'):
            pn.vk_from_json(plonk.vk_to_json(pkey.vk))
        with pytest.raises(pn.ZkError, match='^plonk: not a verification key of this prover \\(protocol "plonk-shplonk-next"\\)$'):
            plonk.vk_from_json(pn.vk_to_json(key.vk))
        with pytest.raises(pn.ZkError, match='^plonk next: not a proof of this prover on %s \\(protocol "plonk-shplonk"' % cv):
            pn.proof_from_json(plonk.proof_to_json(pproof, cv), cv)
        with pytest.raises(pn.ZkError, match='^plonk: not a proof of this prover on %s \\(protocol "plonk-shplonk-next"' % cv):
            plonk.proof_from_json(pn.proof_to_json(proof, cv), cv)
        with pytest.raises(pn.ZkError, match="plonk next: a proof holds 16 values, not 14"):
            pn.verify(key.vk, [ppublics], [pproof])
        with pytest.raises(pn.ZkError, match="plonk: a proof holds 14 values, not 16"):
            plonk.verify(pkey.vk, [publics], [proof])
        with pytest.raises(pn.ZkError, match="plonk: the circuit has a next-row selector qN"):
            plonk.PlonkKey(handles[cv], circuit)
    finally:
        pkey.free()


def test_a_batch_of_three_with_one_bad_proof_located(pn, world):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    made = [pn.prove(key, wit) for _ in range(3)]                                    # blinders from `secrets`
    proofs, publics = [p for p, _ in made], [x for _, x in made]
    assert pn.verify(key.vk, publics, proofs) == (ACCEPTED, None)
    assert pn.verify(key.vk, publics, proofs, seed=SEED) == (ACCEPTED, None)
    for name in pn.POINT_NAMES:
        assert len({p[name] for p in proofs}) == 3, name                             # every commitment moves with the blinders
    for i in range(9, 16):                                                            # and every value of a, b, c, t, Z, Z(zeta w), c(zeta w)
        assert len({p["values"][i] for p in proofs}) == 3, i
    v = proofs[1]["values"]
    moved = dict(proofs[1], values=v[:15] + [(v[15] + 1) % r])                       # c(zeta w): the host's identity refuses it
    other_w = dict(proofs[1], W2=proofs[0]["W2"])                                     # the pairing check refuses it
    for at in range(3):
        for bad in (moved, other_w):
            batch = proofs[:at] + [bad] + proofs[at + 1:]
            assert pn.verify(key.vk, publics, batch) == (REJECTED, at), at
            assert pn.verify(key.vk, publics, batch, seed=SEED, locate=False) == (REJECTED, None), at
    assert pn.verify(key.vk, publics, [other_w, proofs[1], moved]) == (REJECTED, 0)
    assert pn.verify(key.vk, publics, [proofs[0], moved, other_w]) == (REJECTED, 1)


def test_rejections(zk, pn, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r, vk = R.r, key.vk
    proof, publics = pn.prove(key, wit, blinding=BLIND)
    assert pn.verify(vk, [publics], [proof]) == (ACCEPTED, None)
    for i in range(16):                                                               # each of the 16 values + 1
        bad = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert pn.verify(vk, [publics], [bad]) == (REJECTED, 0), i
    swapped = list(proof["values"])
    swapped[11], swapped[15] = swapped[15], swapped[11]                               # c(zeta) and c(zeta w) exchanged
    assert pn.verify(vk, [publics], [dict(proof, values=swapped)]) == (REJECTED, 0)
    other = world.points[cv](0xABCDEF)
    for name in pn.POINT_NAMES:                                                       # each of the 7 points replaced by another valid point
        assert pn.verify(vk, [publics], [dict(proof, **{name: other})]) == (REJECTED, 0), name
    assert pn.verify(vk, [[(publics[0] + 1) % r]], [proof]) == (REJECTED, 0)          # the public input + 1
    # the same table with one q_N taken out: another ninth commitment, another key
    n_vars, public, gates, _ = circuit_of(cv, 16)
    gates = {k: list(v) for k, v in gates.items()}
    at = max(i for i, q in enumerate(gates["qN"]) if q)
    gates["qN"][at] = 0
    key2 = pn.NextKey(handles[cv], pn.NextCircuit(n_vars, public, gates, cv))
    try:
        assert key2.vk.commitments[:8] == vk.commitments[:8] and key2.vk.commitments[8] != vk.commitments[8]
        assert pn.verify(key2.vk, [publics], [proof]) == (REJECTED, 0)
        with pytest.raises(pn.ZkError, match=r"plonk next: witness does not satisfy gate %d \(1 rows\)" % (1 + at)):     # that row's sum no longer leaves through q_N
            pn.prove(key2, wit, blinding=BLIND)
    finally:
        key2.free()
    _, wit8, key8, _ = world(cv, 8)                                                   # the other circuit size
    assert pn.verify(key8.vk, [publics], [proof]) == (REJECTED, 0)
    proof8, publics8 = pn.prove(key8, wit8, blinding=BLIND)
    assert pn.verify(vk, [publics8], [proof8]) == (REJECTED, 0) and pn.verify(key8.vk, [publics8], [proof8]) == (ACCEPTED, None)
    for i in (0, 8, 11, 15):                                                          # a value equal to r
        assert pn.verify(vk, [publics], [dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])]) == (NOT_CANONICAL, 0), i
    assert pn.verify(vk, [[r]], [proof]) == (NOT_CANONICAL, 0)
    with pytest.raises(pn.ZkError, match="a proof holds 16 values"):                  # truncated
        pn.verify(vk, [publics], [dict(proof, values=proof["values"][:15])])
    with pytest.raises(pn.ZkError, match="a proof is"):
        pn.proof_from_bytes(pn.proof_to_bytes(proof)[:-32], handles[cv].point_bytes)
    with pytest.raises(pn.ZkError, match="point T of the proof is 63 bytes"):
        pn.verify(vk, [publics], [dict(proof, T=proof["T"][:-1])])
    # the prover takes the opening's gamma' from the KZG layer's default transcript instead of the chained one: an honest opening under
    # challenges the verifier does not derive.  The verifier uses its own and refuses
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    loose, _ = pn.prove(key, wit, blinding=BLIND, self_check=False, _opening_transcript=kzg.challenges_of)
    assert loose["values"] == proof["values"] and all(loose[k] == proof[k] for k in ("A", "B", "C", "Z", "T")) and loose["W1"] != proof["W1"]
    ch = pn.challenges(vk, publics, loose)
    _, tup = pn.host_check(vk, publics, loose)
    cs, sets, vals = tup[:3]
    g = kzg.challenges_of(cv, cs, sets, vals)
    z = kzg.challenge_z(cv, g, loose["W1"], avoid=sets[13])
    assert handles[cv].verify_multi([(cs, sets, vals, g, z, loose["W1"], loose["W2"])]) == (ACCEPTED, None)      # sound under ITS challenges
    assert g != ch["gamma_open"] and pn.verify(vk, [publics], [loose]) == (REJECTED, 0)


def test_the_prover_refuses_a_bad_witness_and_names_the_row(pn, world):
    circuit, wit, key, R = world("BN128", 16)
    r, t = R.r, R.t
    x = [wit[circuit.public[0]]]
    chain_rows = [i for i in range(t.n) if t.sel["qN"][i]]
    # an auxiliary of the first chain wrong: it stands in c of one row alone (q_O = 1 there) and is read from the row before it
    i = chain_rows[0]
    v = t.wire["c"][i + 1]
    bad = list(wit)
    bad[v] = (bad[v] + 1) % r
    rows = R.gates_hold(R.wires_of(bad), x)
    assert rows == [i, i + 1]
    with pytest.raises(pn.ZkError, match=r"plonk next: witness does not satisfy gate %d \(2 rows\)" % i):
        pn.prove(key, bad, blinding=BLIND)
    # the value that lands in a row of its own (every selector zero there): ONLY the next-row relation of the row before it breaks, and
    # the gate that reads it elsewhere
    land = [j + 1 for j in chain_rows if j + 1 not in chain_rows][1]
    assert all(t.sel[k][land] == 0 for k in nref.SELECTORS)
    wires = R.wires_of(wit)
    wires["c"][land] = (wires["c"][land] + 5) % r                                     # the column value alone, by the hook: no other gate sees it
    assert R.gates_hold(wires, x) == [land - 1]
    with pytest.raises(pn.ZkError, match=r"plonk next: witness does not satisfy gate %d \(1 rows\)" % (land - 1)):
        pn.prove(key, wit, blinding=BLIND, _wires=[wires[k] for k in "abc"])
    bad = list(wit)
    bad[circuit.public[0]] = (bad[circuit.public[0]] + 1) % r                         # the public input: its own row holds, the gates that read it do not
    rows = R.gates_hold(R.wires_of(bad), [bad[circuit.public[0]]])
    with pytest.raises(pn.ZkError, match=r"witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
        pn.prove(key, bad, blinding=BLIND)
    # wire values that satisfy every gate but break a copy: the landing row's a is variable 0 under a zero selector
    wires = R.wires_of(wit)
    wires["a"][land] = 77
    assert not R.gates_hold(wires, x)
    with pytest.raises(pn.ZkError, match="the permutation product does not close"):
        pn.prove(key, wit, blinding=BLIND, _wires=[wires[k] for k in "abc"])
    proof, _ = pn.prove(key, wit, blinding=BLIND, _wires=[R.wires_of(wit)[k] for k in "abc"])        # the hook itself is sound
    assert proof == R.prove(wit, BLIND)["proof"]
    with pytest.raises(pn.ZkError, match="plonk next: blinding takes ten integers"):
        pn.prove(key, wit, blinding=BLIND[:9])
