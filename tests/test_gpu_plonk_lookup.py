"""eigen_zkvm_amd.plonk_lookup end to end on the device against tests/plonk_lookup_ref.py, over powers-of-tau files with a
KNOWN tau: with fixed blinders and with none, the device's proof equals the reference's BYTE FOR BYTE.  The circuits are plonk_ref's chain
with AND-table lookups (a duplicated table row, duplicated lookups) at n = 8 and 16, a range check whose 256-row table alone forces n = 256,
and n = 4096 (more than one tile of the running sum) on BN128, and n = 16 on BLS12381.  Then a circuit that selects no row, batches with
random blinders, every rejection at n = 16, the prover's refusals, and the two provers refusing each other.  Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import plonk_lookup_ref as lref
import plonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
POWER = {"BN128": 13, "BLS12381": 5}                    # 4n - 1 powers for n = 4096 and n = 16: at least 3n + 6
SEED = bytes(range(32))
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(14)]
ACCEPTED, REJECTED, NOT_CANONICAL = 1, 0, -1
SIZES = [("BN128", 8), ("BN128", 16), ("BN128", 256), ("BN128", 4096), ("BLS12381", 16)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def pl(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_lookup")


@pytest.fixture(scope="module")
def handles(zk, tmp_path_factory):
    g16, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    d = tmp_path_factory.mktemp("plonk_lookup")
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


def _circuit_of(cv, n):
    """(n_vars, public, gates, table, witness) for the n rows the tests name"""
    r = ref.R[cv]
    if n == 256:                                                                           # three range checks; the table alone forces n
        gates = {k: [0, 0, 0] for k in ref.SELECTORS}
        gates.update(a=[1, 2, 3], b=[0, 0, 0], c=[0, 0, 0], qK=[1, 1, 1])
        return 4, [1], gates, [(v, 0, 0) for v in range(256)], [0, 200, 7, 255]
    steps, lookups = {8: (0, None), 16: (1, None), 4096: (1000, 60)}[n]
    return lref.lookup_chain(steps, r, lookups=lookups)


@pytest.fixture(scope="module")
def world(zk, pl, handles):
    """per (curve, n): the circuit, its witness, the device key and the reference, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(cv, n):
        if (cv, n) not in made:
            n_vars, public, gates, table, wit = _circuit_of(cv, n)
            circuit = pl.LookupCircuit(n_vars, public, gates, table, cv)
            assert circuit.n == n
            made[(cv, n)] = (circuit, wit, pl.LookupKey(handles[cv], circuit), lref.Reference(cv, n_vars, public, gates, table, TAU[cv], points[cv]))
        return made[(cv, n)]
    get.points = points
    yield get
    for _, _, key, _ in made.values():
        key.free()


@pytest.mark.parametrize("blind", (BLIND, [0] * 14), ids=("blinded", "unblinded"))
@pytest.mark.parametrize("cv,n", SIZES)
def test_the_device_proof_is_the_reference_proof_byte_for_byte(zk, pl, handles, world, cv, n, blind):
    circuit, wit, key, R = world(cv, n)
    if n == 4096:
        assert n > zk.lib().zk_frpoly_tile_elems()                                         # the running sum spans more than one tile
    assert key.vk.commitments == R.vk_points and (key.k1, key.k2) == R.t.k[1:] and key.vk.digest == R.vkd
    want = R.prove(wit, blind)
    proof, publics = pl.prove(key, wit, blinding=blind)
    assert publics == want["publics"]
    assert proof["values"] == want["values"]
    for name in pl.POINT_NAMES:
        assert proof[name] == want["proof"][name], name
    assert pl.proof_to_bytes(proof) == pl.proof_to_bytes(want["proof"])
    assert pl.challenges(key.vk, publics, proof) == want["challenges"]
    assert pl.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    assert pl.verify(key.vk, [publics], [proof], seed=SEED, locate=False) == (ACCEPTED, None)
    if any(blind):                                                                         # the blinders reach every commitment they should
        plain = R.prove(wit, [0] * 14)
        assert all(plain["proof"][k] != proof[k] for k in ("A", "B", "C", "M", "Z", "Phi", "T"))


def test_a_circuit_that_selects_no_row(zk, pl, handles, world):
    """qK all zero under zero blinders: m and phi are zero, [M] and [Phi] the point at infinity, which the KZG layer allows"""
    cv = "BN128"
    n_vars, public, gates, table, wit = _circuit_of(cv, 16)
    gates = dict(gates, qK=[0] * len(gates["qK"]))
    key = pl.LookupKey(handles[cv], pl.LookupCircuit(n_vars, public, gates, table, cv))
    try:
        R = lref.Reference(cv, n_vars, public, gates, table, TAU[cv], world.points[cv])
        proof, publics = pl.prove(key, wit, blinding=[0] * 14)
        infinity = bytes(handles[cv].point_bytes)
        assert proof["M"] == infinity and proof["Phi"] == infinity and proof["A"] != infinity
        assert pl.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
        assert proof == R.prove(wit, [0] * 14)["proof"]
        bad = list(wit)                                                                    # nothing is selected, so nothing is looked up
        bad[-1] = (bad[-1] + 1) % R.r
        assert pl.verify(key.vk, *[[x] for x in pl.prove(key, bad)[::-1]]) == (ACCEPTED, None)
    finally:
        key.free()


def test_keys_and_proofs_go_through_json(pl, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    proof, publics = pl.prove(key, wit, blinding=BLIND)
    vk = pl.vk_from_json(pl.vk_to_json(key.vk))
    assert (vk.curve, vk.log_n, vk.n_public, vk.k1, vk.k2, vk.commitments, vk.digest) == (cv, 4, 1, key.k1, key.k2, key.vk.commitments, key.vk.digest)
    back = pl.proof_from_json(pl.proof_to_json(proof, cv), cv)
    assert back == proof
    assert pl.verify(vk, [publics], [back], kzg=handles[cv]) == (ACCEPTED, None)
    with pytest.raises(pl.ZkError, match="verify needs the Kzg handle"):
        pl.verify(vk, [publics], [back])


def test_batches_and_random_blinders(pl, world):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    made = [pl.prove(key, wit) for _ in range(3)]                                          # blinders from `secrets`
    proofs, publics = [p for p, _ in made], [x for _, x in made]
    assert pl.verify(key.vk, publics[:1], proofs[:1]) == (ACCEPTED, None)
    assert pl.verify(key.vk, publics, proofs) == (ACCEPTED, None)
    assert pl.verify(key.vk, publics, proofs, seed=SEED) == (ACCEPTED, None)
    for name in pl.POINT_NAMES:
        assert len({p[name] for p in proofs}) == 3, name                                   # every commitment moves with the blinders
    for i in range(12, 21):                                                                # and every value of a, b, c, t, M, Z, Phi
        assert len({p["values"][i] for p in proofs}) == 3, i
    moved = dict(proofs[1], values=proofs[1]["values"][:19] + [(proofs[1]["values"][19] + 1) % r] + proofs[1]["values"][20:])
    other_w = dict(proofs[1], W2=proofs[0]["W2"])
    for at in range(3):
        for bad in (moved, other_w):
            batch = proofs[:at] + [bad] + proofs[at + 1:]
            assert pl.verify(key.vk, publics, batch) == (REJECTED, at), at
            assert pl.verify(key.vk, publics, batch, seed=SEED, locate=False) == (REJECTED, None), at


def test_rejections(zk, pl, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r, vk = R.r, key.vk
    proof, publics = pl.prove(key, wit, blinding=BLIND)
    assert pl.verify(vk, [publics], [proof]) == (ACCEPTED, None)
    for i in range(21):                                                                    # each of the 21 values + 1
        bad = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert pl.verify(vk, [publics], [bad]) == (REJECTED, 0), i
    other = world.points[cv](0xABCDEF)
    for name in pl.POINT_NAMES:                                                            # each of the 9 points replaced by another valid point
        assert pl.verify(vk, [publics], [dict(proof, **{name: other})]) == (REJECTED, 0), name
    assert pl.verify(vk, [[(publics[0] + 1) % r]], [proof]) == (REJECTED, 0)               # the public input + 1
    # the same gates over another table: other commitments to t1 .. t3, another key
    n_vars, public, gates, table, _ = _circuit_of(cv, 16)
    key2 = pl.LookupKey(handles[cv], pl.LookupCircuit(n_vars, public, gates, table + [(2, 3, 4)], cv))
    try:
        assert key2.vk.commitments[:9] == vk.commitments[:9] and all(a != b for a, b in zip(key2.vk.commitments[9:], vk.commitments[9:]))
        assert pl.verify(key2.vk, [publics], [proof]) == (REJECTED, 0)
    finally:
        key2.free()
    _, wit8, key8, _ = world(cv, 8)                                                        # the other circuit size
    assert pl.verify(key8.vk, [publics], [proof]) == (REJECTED, 0)
    for i in (0, 11, 16, 20):                                                              # a value equal to r
        assert pl.verify(vk, [publics], [dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])]) == (NOT_CANONICAL, 0), i
    assert pl.verify(vk, [[r]], [proof]) == (NOT_CANONICAL, 0)
    with pytest.raises(pl.ZkError, match="a proof holds 21 values"):                       # truncated
        pl.verify(vk, [publics], [dict(proof, values=proof["values"][:20])])
    with pytest.raises(pl.ZkError, match="a proof is"):
        pl.proof_from_bytes(pl.proof_to_bytes(proof)[:-32], handles[cv].point_bytes)
    with pytest.raises(pl.ZkError, match="point Phi of the proof is 63 bytes"):
        pl.verify(vk, [publics], [dict(proof, Phi=proof["Phi"][:-1])])


def test_the_two_provers_refuse_each_other(pl, handles, world):
    cv = "BN128"
    plonk = importlib.import_module("eigen_zkvm_amd.plonk")
    circuit, wit, key, R = world(cv, 16)
    proof, publics = pl.prove(key, wit, blinding=BLIND)
    n_vars, public, gates, _, _ = _circuit_of(cv, 16)
    pkey = plonk.PlonkKey(handles[cv], plonk.Circuit(n_vars, public, gates, cv))           # the same gates without their lookups
    try:
        pproof, ppublics = plonk.prove(pkey, wit, blinding=BLIND[:9])
        assert ppublics == publics and pkey.vk.commitments == key.vk.commitments[:8] and pkey.vk.digest != key.vk.digest
        with pytest.raises(pl.ZkError, match="plonk lookup: the proof holds no M, Phi"):
            pl.verify(key.vk, [ppublics], [pproof])
        with pytest.raises(pl.ZkError, match="plonk: a proof holds 14 values, not 21"):
            plonk.verify(pkey.vk, [publics], [proof])
        with pytest.raises(pl.ZkError, match='plonk lookup: not a proof of this prover on BN128 \\(protocol "plonk-shplonk"'):
            pl.proof_from_json(plonk.proof_to_json(pproof, cv), cv)
        with pytest.raises(pl.ZkError, match='plonk: not a proof of this prover on BN128 \\(protocol "plonk-shplonk-lookup"'):
            plonk.proof_from_json(pl.proof_to_json(proof, cv), cv)
        with pytest.raises(pl.ZkError, match='plonk lookup: not a verification key of this prover \\(protocol "plonk-shplonk"\\)'):
            pl.vk_from_json(plonk.vk_to_json(pkey.vk))
        with pytest.raises(pl.ZkError, match='plonk: not a verification key of this prover \\(protocol "plonk-shplonk-lookup"\\)'):
            plonk.vk_from_json(pl.vk_to_json(key.vk))
        # a plonk proof dressed up with the two missing points and seven more values is no proof here either: other challenges
        dressed = dict(pproof, M=proof["M"], Phi=proof["Phi"], values=pproof["values"][:8] + proof["values"][8:12] + pproof["values"][8:12] + proof["values"][16:17] +
                       pproof["values"][12:] + proof["values"][19:])
        assert pl.verify(key.vk, [publics], [dressed]) == (REJECTED, 0)
    finally:
        pkey.free()


def test_the_prover_refuses_a_bad_witness(pl, world):
    circuit, wit, key, R = world("BN128", 16)
    r, n = R.r, R.t.n
    wires = R.wires_of(wit)
    looked = [i for i in range(n) if R.qk[i]]
    # a selected row outside the table: the variable of a looked-up c, moved.  Lookup rows have all-zero selectors, so every gate still holds
    twice = next(v for v in set(circuit.wire["c"][looked].tolist()) if circuit.wire["c"][looked].tolist().count(v) == 2)
    bad = list(wit)
    bad[twice] = (bad[twice] + 2) % r
    assert not R.gates_hold(R.wires_of(bad), [bad[circuit.public[0]]])
    missing = R.multiplicities(R.wires_of(bad))[1]
    assert len(missing) == 2
    with pytest.raises(pl.ZkError, match=r"plonk lookup: witness does not satisfy lookup at row %d \(2 rows\): \(a, b, c\) is not a row of the table" % missing[0]):
        pl.prove(key, bad, blinding=BLIND)
    # a gate failure is still named first
    both = list(bad)
    both[5] = (both[5] + 1) % r
    rows = R.gates_hold(R.wires_of(both), [both[circuit.public[0]]])
    assert rows
    with pytest.raises(pl.ZkError, match=r"witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
        pl.prove(key, both, blinding=BLIND)
    # the hook _wires skips nothing: the same row is named
    bw = R.wires_of(bad)
    with pytest.raises(pl.ZkError, match=r"does not satisfy lookup at row %d \(2 rows\)" % missing[0]):
        pl.prove(key, wit, blinding=BLIND, _wires=[bw[k] for k in "abc"])
    # multiplicities with one count moved to another row: the sum does not close
    m, _ = R.multiplicities(wires)
    j = next(i for i, c in enumerate(m) if c)
    moved = list(m)
    moved[j] -= 1
    moved[next(k for k in range(n) if R.rows[k] != R.rows[j])] += 1
    with pytest.raises(pl.ZkError, match="plonk lookup: the lookup sum does not close"):
        pl.prove(key, wit, blinding=BLIND, _multiplicities=moved)
    proof, _ = pl.prove(key, wit, blinding=BLIND, _multiplicities=m, _wires=[wires[k] for k in "abc"])      # the hooks themselves are sound
    assert proof == R.prove(wit, BLIND)["proof"]
    # moved onto the other copy of the same table row the sum closes and the proof is accepted: sound, but not the protocol's proof
    if R.rows[0] == R.rows[1] and m[0]:
        onto_copy = [m[0] - 1, 1] + m[2:]
        other, _ = pl.prove(key, wit, blinding=BLIND, _multiplicities=onto_copy)
        assert other["M"] != proof["M"]
