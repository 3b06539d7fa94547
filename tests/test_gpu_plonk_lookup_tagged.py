"""The tagged lookups of eigen_zkvm_amd.plonk_lookup end to end on the device against tests/plonk_lookup_tagged_ref.py, over
powers-of-tau files with a KNOWN tau: with fixed blinders and with none, the device's proof equals the reference's BYTE FOR BYTE.  The
circuits hold a range table and an XOR table: plonk_ref's chain with lookups into both at n = 8 and 16 (one tuple in both tables, a
duplicated row, duplicated lookups), tables that alone force n = 256, and n = 4096 on BN128; n = 16 on BLS12381.  Then batches, the
forgeries, the prover's refusal of a tuple of the other table, the codecs on the device, and fflonk_lookup's refusal.  Exact throughout."""
import importlib, pathlib, sys

import numpy as np
import pytest

import plonk_lookup_tagged_ref as tref
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
ACCEPTED, REJECTED = 1, 0
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
    d = tmp_path_factory.mktemp("plonk_lookup_tagged")
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
    """(n_vars, public, gates, tables, witness) for the n rows the tests name"""
    r = ref.R[cv]
    if n == 256:                                                                           # 128 + 64 table rows force n; three range checks, two XORs
        gates = {k: [0] * 5 for k in ref.SELECTORS}
        gates.update(a=[1, 2, 3, 4, 6], b=[0, 0, 0, 5, 4], c=[0, 0, 0, 6, 5], qK=[1, 1, 1, 2, 2])
        return 7, [1], gates, [[(v,) for v in range(128)], [(x, y, x ^ y) for x in range(8) for y in range(8)]], [0, 100, 7, 127, 5, 6, 3]
    steps, lookups = {8: (0, None), 16: (1, None), 4096: (1000, 60)}[n]
    return tref.tagged_chain(steps, r, lookups=lookups)


@pytest.fixture(scope="module")
def world(zk, pl, handles):
    """per (curve, n): the circuit, its witness, the device key, the reference and its proofs by blinding, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(cv, n):
        if (cv, n) not in made:
            n_vars, public, gates, tables, wit = _circuit_of(cv, n)
            circuit = pl.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables)
            assert circuit.n == n and circuit.tagged
            made[(cv, n)] = (circuit, wit, pl.LookupKey(handles[cv], circuit), tref.Reference(cv, n_vars, public, gates, tables, TAU[cv], points[cv]))
        return made[(cv, n)]
    get.points = points
    yield get
    for _, _, key, _ in made.values():
        key.free()


@pytest.mark.parametrize("blind", (BLIND, [0] * 14), ids=("blinded", "unblinded"))
@pytest.mark.parametrize("cv,n", SIZES)
def test_the_device_proof_is_the_reference_proof_byte_for_byte(zk, pl, handles, world, cv, n, blind):
    circuit, wit, key, R = world(cv, n)
    assert key.tagged and key.vk.tagged and len(key.vk.commitments) == 13
    assert key.vk.commitments == R.vk_points and (key.k1, key.k2) == R.t.k[1:] and key.vk.digest == R.vkd
    want = R.prove(wit, blind)
    proof, publics = pl.prove(key, wit, blinding=blind)
    assert publics == want["publics"]
    assert len(proof["values"]) == 22 and proof["values"] == want["values"]
    for name in pl.POINT_NAMES:
        assert proof[name] == want["proof"][name], name
    assert pl.proof_to_bytes(proof) == pl.proof_to_bytes(want["proof"])
    assert pl.challenges(key.vk, publics, proof) == want["challenges"]
    assert pl.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    assert pl.verify(key.vk, [publics], [proof], seed=SEED, locate=False) == (ACCEPTED, None)


def test_keys_and_proofs_go_through_the_codecs(pl, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    proof, publics = pl.prove(key, wit, blinding=BLIND)
    for ask in (None, True):
        vk = pl.vk_from_json(pl.vk_to_json(key.vk), tagged=ask)
        assert (vk.tagged, vk.curve, vk.log_n, vk.n_public, vk.k1, vk.k2, vk.commitments, vk.digest) == (True, cv, 4, 1, key.k1, key.k2, key.vk.commitments, key.vk.digest)
        assert pl.proof_from_json(pl.proof_to_json(proof, cv), cv, tagged=ask) == proof
    assert '"protocol": "plonk-shplonk-lookup-tagged"' in pl.vk_to_json(key.vk) and '"T0"' in pl.vk_to_json(key.vk)
    assert '"protocol": "plonk-shplonk-lookup-tagged"' in pl.proof_to_json(proof, cv)
    with pytest.raises(pl.ZkError, match="a verification key of the tagged protocol"):
        pl.vk_from_json(pl.vk_to_json(key.vk), tagged=False)
    with pytest.raises(pl.ZkError, match="a proof of the tagged protocol"):
        pl.proof_from_json(pl.proof_to_json(proof, cv), cv, tagged=False)
    assert pl.verify(vk, [publics], [pl.proof_from_bytes(pl.proof_to_bytes(proof), handles[cv].point_bytes, tagged=True)], kzg=handles[cv]) == (ACCEPTED, None)


def test_a_batch_of_tagged_proofs_passes_in_one_check(pl, world):
    circuit, wit, key, R = world("BN128", 16)
    made = [pl.prove(key, wit) for _ in range(3)]                                          # blinders from `secrets`
    proofs, publics = [p for p, _ in made], [x for _, x in made]
    assert pl.verify(key.vk, publics, proofs) == (ACCEPTED, None)
    assert pl.verify(key.vk, publics, proofs, seed=SEED) == (ACCEPTED, None)
    for name in pl.POINT_NAMES:
        assert len({p[name] for p in proofs}) == 3, name
    moved = dict(proofs[1], values=proofs[1]["values"][:12] + [(proofs[1]["values"][12] + 1) % R.r] + proofs[1]["values"][13:])
    for at in range(3):
        batch = proofs[:at] + [moved] + proofs[at + 1:]
        assert pl.verify(key.vk, publics, batch) == (REJECTED, at), at


def test_forgeries_are_rejected(zk, pl, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r, vk = R.r, key.vk
    proof, publics = pl.prove(key, wit, blinding=BLIND)
    assert pl.verify(vk, [publics], [proof]) == (ACCEPTED, None)
    for i in range(22):                                                                    # each opened value + 1; 12 is T0(zeta)
        bad = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert pl.verify(vk, [publics], [bad]) == (REJECTED, 0), i
    assert pl.VALUE_NAMES[:12] == pl.TAGGED_VALUE_NAMES[:12] and pl.TAGGED_VALUE_NAMES[12] == "T0"
    for tag in (0, 1, 2):                                                                  # T0(zeta) replaced by a plausible constant
        assert pl.verify(vk, [publics], [dict(proof, values=proof["values"][:12] + [tag] + proof["values"][13:])]) == (REJECTED, 0), tag
    # M from the unweighted count: the prover's own sum does not close, and the honest proof with [M] swapped for that commitment is refused
    counts, _ = R.multiplicities(R.wires_of(wit), weighted=False)
    assert counts != R.multiplicities(R.wires_of(wit))[0]
    with pytest.raises(pl.ZkError, match="plonk lookup: the lookup sum does not close"):
        pl.prove(key, wit, blinding=BLIND, _multiplicities=counts)
    zh_tau = (pow(R.tau, R.t.n, r) - 1) % r
    m_point = world.points[cv]((ref.dot(counts, R.lw_tau, r) + (BLIND[9] * R.tau + BLIND[10]) * zh_tau) % r)
    assert m_point != proof["M"] and pl.verify(vk, [publics], [dict(proof, M=m_point)]) == (REJECTED, 0)
    # a key whose table tags are swapped: the same rows, the same gates, the XOR table numbered 1
    n_vars, public, gates, tables, _ = _circuit_of(cv, 16)
    key2 = pl.LookupKey(handles[cv], pl.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables[::-1]))
    try:
        assert key2.vk.commitments[:9] == vk.commitments[:9] and key2.vk.commitments[12] != vk.commitments[12] and key2.vk.digest != vk.digest
        assert pl.verify(key2.vk, [publics], [proof]) == (REJECTED, 0)
        with pytest.raises(pl.ZkError, match=r"does not satisfy lookup at row \d+ \(\d+ rows\): \(a, b, c\) is not a row of table [12]"):
            pl.prove(key2, wit, blinding=BLIND)                                            # and the witness no longer fits it
    finally:
        key2.free()
    _, _, key8, _ = world(cv, 8)
    assert pl.verify(key8.vk, [publics], [proof]) == (REJECTED, 0)
    # the single-table prover over the concatenated table is another protocol: its proof is refused here, and this one there
    flat = [tref.pad(t) for tab in tables for t in tab]
    key1 = pl.LookupKey(handles[cv], pl.LookupCircuit(n_vars, public, dict(gates, qK=[min(q, 1) for q in gates["qK"]]), flat, cv))
    try:
        assert not key1.tagged and key1.vk.commitments[9:12] == vk.commitments[9:12] and key1.vk.digest != vk.digest
        plain, ppublics = pl.prove(key1, wit, blinding=BLIND)
        assert len(plain["values"]) == 21 and ppublics == publics
        with pytest.raises(pl.ZkError, match="a proof holds 22 values, not 21"):
            pl.verify(vk, [publics], [plain])
        with pytest.raises(pl.ZkError, match="a proof holds 21 values, not 22"):
            pl.verify(key1.vk, [publics], [proof])
        dressed = dict(plain, values=plain["values"][:12] + proof["values"][12:13] + plain["values"][12:])
        assert pl.verify(vk, [publics], [dressed]) == (REJECTED, 0)
    finally:
        key1.free()


def test_the_prover_refuses_a_tuple_of_the_other_table_by_row(pl, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r = R.r
    looked = [i for i in range(R.t.n) if R.qk[i] == 1]
    row = looked[-1]                                                                       # the range check of 1 ...
    assert (R.wires_of(wit)["a"][row], R.qk[row]) == (1, 1)
    n_vars, public, gates, tables, _ = _circuit_of(cv, 16)
    g = row - len(public)
    gates = dict(gates, b=gates["b"][:g] + [gates["a"][g]] + gates["b"][g + 1:])           # ... now holds (1, 1, 0): a row of the XOR table alone
    key2 = pl.LookupKey(handles[cv], pl.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables))
    try:
        R2 = tref.Reference(cv, n_vars, public, gates, tables, TAU[cv], world.points[cv])
        assert R2.multiplicities(R2.wires_of(wit))[1] == [row] and (2, 1, 1, 0) in R2.rows
        with pytest.raises(pl.ZkError, match=r"^plonk lookup: witness does not satisfy lookup at row %d \(1 rows\): \(a, b, c\) is not a row of table 1, the table the row's qK names$" % row):
            pl.prove(key2, wit, blinding=BLIND)
        both = list(wit)                                                                   # a gate failure is still named first
        both[5] = (both[5] + 1) % r
        rows = R2.gates_hold(R2.wires_of(both), [both[circuit.public[0]]])
        assert rows
        with pytest.raises(pl.ZkError, match=r"witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
            pl.prove(key2, both, blinding=BLIND)
    finally:
        key2.free()


def test_fflonk_with_lookups_refuses_the_circuit(pl, handles, world):
    fl = importlib.import_module("eigen_zkvm_amd.fflonk_lookup")
    circuit, _, _, _ = world("BN128", 16)
    with pytest.raises(pl.ZkError, match="^fflonk lookup: the circuit has 2 tagged tables: fflonk with lookups proves one table"):
        fl.setup(handles["BN128"], circuit)
