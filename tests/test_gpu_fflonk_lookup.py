"""eigen_zkvm_amd.fflonk_lookup end to end on the device against tests/fflonk_lookup_ref.py, over powers-of-tau files with a
KNOWN tau: with fixed blinders and with none, the device's proof equals the reference's BYTE FOR BYTE.  The circuits are plonk_ref's chain
with AND-table lookups (a duplicated table row, duplicated lookups) at n = 8 and 16 and a range check whose 256-row table alone forces
n = 256 on BN128, and n = 16 on BLS12381.  Then a circuit that selects no row, batches with random blinders, every rejection at n = 16, the
prover's refusals, and the four provers refusing each other.  Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import fflonk_lookup_ref as flref
import plonk_ref as ref

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
POWER = {"BN128": 11, "BLS12381": 7}                    # 2^(p + 1) - 1 powers: at least 8n + 8 for n = 256 and n = 16 (k + 3)
SEED = bytes(range(32))
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(14)]
ACCEPTED, REJECTED, NOT_CANONICAL = 1, 0, -1
SIZES = [("BN128", 8), ("BN128", 16), ("BN128", 256), ("BLS12381", 16)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def fl(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk_lookup")


@pytest.fixture(scope="module")
def handles(zk, tmp_path_factory):
    g16, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    d = tmp_path_factory.mktemp("fflonk_lookup")
    hs = {}
    for name, cv, power in [(cv, cv, POWER[cv]) for cv in POWER] + [("small", "BN128", 6)]:
        p = d / (name + ".ptau")
        p.write_bytes(make_test_ptau.build_ptau(zk, cv, power, TAU[cv], 5, 7))
        srs = g16.Srs(cv, p)
        hs[name] = kzg.Kzg(srs)
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
    return flref.lookup_chain({8: 0, 16: 1}[n], r)


@pytest.fixture(scope="module")
def world(zk, fl, handles):
    """per (curve, n): the circuit, its witness, the device key and the reference, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(cv, n):
        if (cv, n) not in made:
            n_vars, public, gates, table, wit = _circuit_of(cv, n)
            circuit = fl.LookupCircuit(n_vars, public, gates, table, cv)
            assert circuit.n == n
            made[(cv, n)] = (circuit, wit, fl.FflonkLookupKey(handles[cv], circuit), flref.Reference(cv, n_vars, public, gates, table, TAU[cv], points[cv]))
        return made[(cv, n)]
    get.points = points
    yield get
    for _, _, key, _ in made.values():
        key.free()


@pytest.mark.parametrize("blind", (BLIND, [0] * 14), ids=("blinded", "unblinded"))
@pytest.mark.parametrize("cv,n", SIZES)
def test_the_device_proof_is_the_reference_proof_byte_for_byte(zk, fl, handles, world, cv, n, blind):
    circuit, wit, key, R = world(cv, n)
    if n == 256:
        assert circuit.n_gates == 3 and circuit.n_table == 256                             # the table alone forces n
    assert [key.vk.c0, key.vk.c0l] == R.vk_points and (key.k1, key.k2) == R.t.k[1:] and key.vk.digest == R.vkd
    want = R.prove(wit, blind)
    proof, publics = fl.prove(key, wit, blinding=blind)
    assert publics == want["publics"]
    assert proof["values"] == want["values"]
    for name in fl.POINT_NAMES:
        assert proof[name] == want["proof"][name], name
    assert fl.proof_to_bytes(proof) == fl.proof_to_bytes(want["proof"])
    assert fl.challenges(key.vk, publics, proof) == want["challenges"]
    assert fl.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    assert fl.verify(key.vk, [publics], [proof], seed=SEED, locate=False) == (ACCEPTED, None)
    if any(blind):                                                                         # the blinders reach every commitment they should
        plain = R.prove(wit, [0] * 14)
        assert all(plain["proof"][k] != proof[k] for k in ("C1", "C2", "C3"))


def test_a_circuit_that_selects_no_row(zk, fl, handles, world):
    """qK all zero under zero blinders: m and Phi are zero -- the M part of C1, the Phi part of C2 and T3 are the zero polynomial -- and the
    proof is still the reference's"""
    cv = "BN128"
    n_vars, public, gates, table, wit = _circuit_of(cv, 16)
    gates = dict(gates, qK=[0] * len(gates["qK"]))
    key = fl.FflonkLookupKey(handles[cv], fl.LookupCircuit(n_vars, public, gates, table, cv))
    try:
        R = flref.Reference(cv, n_vars, public, gates, table, TAU[cv], world.points[cv])
        want = R.prove(wit, [0] * 14)
        proof, publics = fl.prove(key, wit, blinding=[0] * 14)
        v = dict(zip(fl.VALUE_NAMES, proof["values"]))
        assert v["M"] == v["Phi"] == v["Phiw"] == v["qK"] == 0 and v["a"] != 0
        assert fl.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
        assert proof == want["proof"]
        bad = list(wit)                                                                    # nothing is selected, so nothing is looked up
        bad[-1] = (bad[-1] + 1) % R.r
        assert fl.verify(key.vk, *[[x] for x in fl.prove(key, bad)[::-1]]) == (ACCEPTED, None)
    finally:
        key.free()


def test_keys_and_proofs_go_through_json_and_bytes(fl, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    proof, publics = fl.prove(key, wit, blinding=BLIND)
    vk = fl.vk_from_json(fl.vk_to_json(key.vk))
    assert (vk.curve, vk.log_n, vk.n_public, vk.k1, vk.k2, vk.c0, vk.c0l, vk.digest) == (cv, 4, 1, key.k1, key.k2, key.vk.c0, key.vk.c0l, key.vk.digest)
    back = fl.proof_from_json(fl.proof_to_json(proof, cv), cv)
    assert back == proof and fl.proof_from_bytes(fl.proof_to_bytes(proof), handles[cv].point_bytes) == proof
    assert fl.verify(vk, [publics], [back], kzg=handles[cv]) == (ACCEPTED, None)
    with pytest.raises(fl.ZkError, match="verify needs the Kzg handle"):
        fl.verify(vk, [publics], [back])


def test_batches_and_random_blinders(fl, world):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    made = [fl.prove(key, wit) for _ in range(3)]                                          # blinders from `secrets`
    proofs, publics = [p for p, _ in made], [x for _, x in made]
    assert fl.verify(key.vk, publics[:1], proofs[:1]) == (ACCEPTED, None)
    assert fl.verify(key.vk, publics, proofs) == (ACCEPTED, None)
    assert fl.verify(key.vk, publics, proofs, seed=SEED) == (ACCEPTED, None)
    for name in fl.POINT_NAMES:
        assert len({p[name] for p in proofs}) == 3, name                                   # every commitment moves with the blinders
    for i in range(12, 22):                                                                # and every value of a, b, c, M, Z, Phi, Zw, Phiw, T0w, T1w
        assert len({p["values"][i] for p in proofs}) == 3, i
    moved = dict(proofs[1], values=proofs[1]["values"][:17] + [(proofs[1]["values"][17] + 1) % r] + proofs[1]["values"][18:])
    other_w = dict(proofs[1], W2=proofs[0]["W2"])
    for at in range(3):
        for bad in (moved, other_w):
            batch = proofs[:at] + [bad] + proofs[at + 1:]
            assert fl.verify(key.vk, publics, batch) == (REJECTED, at), at
            assert fl.verify(key.vk, publics, batch, seed=SEED, locate=False) == (REJECTED, None), at


def test_rejections(zk, fl, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r, vk = R.r, key.vk
    proof, publics = fl.prove(key, wit, blinding=BLIND)
    assert fl.verify(vk, [publics], [proof]) == (ACCEPTED, None)
    for i in range(22):                                                                    # each of the 22 values + 1
        bad = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert fl.verify(vk, [publics], [bad]) == (REJECTED, 0), i
    other = world.points[cv](0xABCDEF)
    for name in fl.POINT_NAMES:                                                            # each of the 5 points replaced by another valid point
        assert fl.verify(vk, [publics], [dict(proof, **{name: other})]) == (REJECTED, 0), name
    assert fl.verify(vk, [[(publics[0] + 1) % r]], [proof]) == (REJECTED, 0)               # the public input + 1
    for name in ("c0", "c0l"):                                                             # each point of the key
        c0, c0l = (other if name == "c0" else vk.c0), (other if name == "c0l" else vk.c0l)
        assert fl.verify(fl.VerifyingKey(cv, vk.log_n, vk.n_public, vk.k1, vk.k2, c0, c0l, handles[cv]), [publics], [proof]) == (REJECTED, 0), name
    # the same gates over another table: another [C0L] under the same [C0], another key
    n_vars, public, gates, table, _ = _circuit_of(cv, 16)
    key2 = fl.FflonkLookupKey(handles[cv], fl.LookupCircuit(n_vars, public, gates, table + [(2, 3, 4)], cv))
    try:
        assert key2.vk.c0 == vk.c0 and key2.vk.c0l != vk.c0l
        assert fl.verify(key2.vk, [publics], [proof]) == (REJECTED, 0)
    finally:
        key2.free()
    _, wit8, key8, _ = world(cv, 8)                                                        # the other circuit size
    assert fl.verify(key8.vk, [publics], [proof]) == (REJECTED, 0)
    for i in (0, 11, 16, 21):                                                              # a value equal to r
        assert fl.verify(vk, [publics], [dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])]) == (NOT_CANONICAL, 0), i
    assert fl.verify(vk, [[r]], [proof]) == (NOT_CANONICAL, 0)
    with pytest.raises(fl.ZkError, match="a proof holds 22 values"):                       # truncated
        fl.verify(vk, [publics], [dict(proof, values=proof["values"][:21])])
    with pytest.raises(fl.ZkError, match="a proof is"):
        fl.proof_from_bytes(fl.proof_to_bytes(proof)[:-32], handles[cv].point_bytes)
    with pytest.raises(fl.ZkError, match="point C3 of the proof is 63 bytes"):
        fl.verify(vk, [publics], [dict(proof, C3=proof["C3"][:-1])])


def test_the_four_provers_refuse_each_other(fl, handles, world):
    cv = "BN128"
    plonk, fflonk, pl = [importlib.import_module("eigen_zkvm_amd." + m) for m in ("plonk", "fflonk", "plonk_lookup")]
    circuit, wit, key, R = world(cv, 16)
    proof, publics = fl.prove(key, wit, blinding=BLIND)
    n_vars, public, gates, table, _ = _circuit_of(cv, 16)
    plain = plonk.Circuit(n_vars, public, gates, cv)                                       # the same gates without their lookups
    others = [(plonk, plonk.PlonkKey(handles[cv], plain), 9, "plonk", "plonk-shplonk", 14),
              (fflonk, fflonk.FflonkKey(handles[cv], plain), 9, "fflonk", "fflonk-shplonk", 15),
              (pl, pl.LookupKey(handles[cv], circuit), 14, "plonk lookup", "plonk-shplonk-lookup", 21)]
    try:
        for mod, okey, nb, who, protocol, n_values in others:
            oproof, opublics = mod.prove(okey, wit, blinding=BLIND[:nb])
            assert opublics == publics and okey.vk.digest != key.vk.digest
            with pytest.raises(fl.ZkError, match="^fflonk lookup: (the proof holds no |a proof holds 22 values, not %d)" % n_values):
                fl.verify(key.vk, [opublics], [oproof])
            with pytest.raises(fl.ZkError, match="^%s: (the proof holds no |a proof holds %d values, not 22)" % (who, n_values)):
                mod.verify(okey.vk, [publics], [proof])
            with pytest.raises(fl.ZkError, match='fflonk lookup: not a proof of this prover on BN128 \\(protocol "%s"' % protocol):
                fl.proof_from_json(mod.proof_to_json(oproof, cv), cv)
            with pytest.raises(fl.ZkError, match='%s: not a proof of this prover on BN128 \\(protocol "fflonk-shplonk-lookup"' % who):
                mod.proof_from_json(fl.proof_to_json(proof, cv), cv)
            with pytest.raises(fl.ZkError, match='fflonk lookup: not a verification key of this prover \\(protocol "%s"\\)' % protocol):
                fl.vk_from_json(mod.vk_to_json(okey.vk))
            with pytest.raises(fl.ZkError, match='%s: not a verification key of this prover \\(protocol "fflonk-shplonk-lookup"\\)' % who):
                mod.vk_from_json(fl.vk_to_json(key.vk))
        assert others[1][1].vk.c0 == key.vk.c0                                             # [C0] is fflonk.py's, exactly
    finally:
        for _, okey, *_ in others:
            okey.free()


def test_the_prover_refuses_a_bad_witness_and_too_small_a_file(fl, handles, world):
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
    with pytest.raises(fl.ZkError, match=r"fflonk lookup: witness does not satisfy lookup at row %d \(2 rows\): \(a, b, c\) is not a row of the table" % missing[0]):
        fl.prove(key, bad, blinding=BLIND)
    # a gate failure is still named first
    both = list(bad)
    both[5] = (both[5] + 1) % r
    rows = R.gates_hold(R.wires_of(both), [both[circuit.public[0]]])
    assert rows
    with pytest.raises(fl.ZkError, match=r"fflonk lookup: witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
        fl.prove(key, both, blinding=BLIND)
    # the hook _wires skips nothing: the same row is named
    bw = R.wires_of(bad)
    with pytest.raises(fl.ZkError, match=r"does not satisfy lookup at row %d \(2 rows\)" % missing[0]):
        fl.prove(key, wit, blinding=BLIND, _wires=[bw[k] for k in "abc"])
    # multiplicities with one count moved to another row: the sum does not close
    m, _ = R.multiplicities(wires)
    j = next(i for i, c in enumerate(m) if c)
    moved = list(m)
    moved[j] -= 1
    moved[next(k for k in range(n) if R.rows[k] != R.rows[j])] += 1
    with pytest.raises(fl.ZkError, match="fflonk lookup: the lookup sum does not close"):
        fl.prove(key, wit, blinding=BLIND, _multiplicities=moved)
    proof, _ = fl.prove(key, wit, blinding=BLIND, _multiplicities=m, _wires=[wires[k] for k in "abc"])      # the hooks themselves are sound
    assert proof == R.prove(wit, BLIND)["proof"]
    # a file of power 6 holds 127 G1 powers, n = 16 needs 136: the refusal names both numbers and the power that has them
    assert handles["small"].max_coeffs == 127
    with pytest.raises(fl.ZkError, match=r"^fflonk lookup: the file holds 127 G1 powers, n = 16 rows need 8n \+ 8 = 136 \(a file of power 7 has them\)$"):
        fl.FflonkLookupKey(handles["small"], circuit)
