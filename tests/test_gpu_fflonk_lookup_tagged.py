"""eigen_zkvm_amd.fflonk_lookup_tagged end to end on the device against tests/fflonk_lookup_tagged_ref.py, over powers-of-tau
files with a KNOWN tau: with fixed blinders and with none, the device's proof equals the reference's BYTE FOR BYTE.  The circuits are
plonk_lookup_tagged_ref's chain with a range table and an XOR table that share a tuple (a duplicated table row, duplicated lookups) at n = 8
and 16, and 128 + 64 table rows that alone force n = 256, on BN128; n = 16 on BLS12381.  Then a batch in one check, every rejection at
n = 16 (each of the 23 values, Tg(xi), each point), the unweighted count, a key with the tags of its two tables swapped, the cross-table
witness refused by row and table, and a table tuple under q_K = 0 that is not counted.  Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import fflonk_lookup_tagged_ref as ftref
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
def flt(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk_lookup_tagged")


@pytest.fixture(scope="module")
def handles(zk, tmp_path_factory):
    g16, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    d = tmp_path_factory.mktemp("fflonk_lookup_tagged")
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
    """(n_vars, public, gates, tables, witness) for the n rows the tests name"""
    r = ref.R[cv]
    if n == 256:                                                                           # 128 + 64 table rows force n; three range checks, two XORs
        gates = {k: [0] * 5 for k in ref.SELECTORS}
        gates.update(a=[1, 2, 3, 4, 6], b=[0, 0, 0, 5, 4], c=[0, 0, 0, 6, 5], qK=[1, 1, 1, 2, 2])
        return 7, [1], gates, [[(v,) for v in range(128)], [(x, y, x ^ y) for x in range(8) for y in range(8)]], [0, 100, 7, 127, 5, 6, 3]
    return ftref.tagged_chain({8: 0, 16: 1}[n], r)


@pytest.fixture(scope="module")
def world(zk, flt, handles):
    """per (curve, n): the circuit, its witness, the device key and the reference, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(cv, n):
        if (cv, n) not in made:
            n_vars, public, gates, tables, wit = _circuit_of(cv, n)
            circuit = flt.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables)
            assert circuit.n == n and circuit.tagged
            made[(cv, n)] = (circuit, wit, flt.FflonkLookupTaggedKey(handles[cv], circuit), ftref.Reference(cv, n_vars, public, gates, tables, TAU[cv], points[cv]))
        return made[(cv, n)]
    get.points = points
    yield get
    for _, _, key, _ in made.values():
        key.free()


@pytest.mark.parametrize("blind", (BLIND, [0] * 14), ids=("blinded", "unblinded"))
@pytest.mark.parametrize("cv,n", SIZES)
def test_the_device_proof_is_the_reference_proof_byte_for_byte(zk, flt, handles, world, cv, n, blind):
    circuit, wit, key, R = world(cv, n)
    if n == 256:
        assert circuit.n_gates == 5 and circuit.n_table == 192                             # the tables alone force n
    assert [key.vk.c0, key.vk.c0l] == R.vk_points and (key.k1, key.k2) == R.t.k[1:] and key.vk.digest == R.vkd
    want = R.prove(wit, blind)
    proof, publics = flt.prove(key, wit, blinding=blind)
    assert publics == want["publics"]
    assert len(proof["values"]) == 23 and proof["values"] == want["values"]
    for name in flt.POINT_NAMES:
        assert proof[name] == want["proof"][name], name
    assert flt.proof_to_bytes(proof) == flt.proof_to_bytes(want["proof"])
    assert flt.challenges(key.vk, publics, proof) == want["challenges"]
    assert flt.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    assert flt.verify(key.vk, [publics], [proof], seed=SEED, locate=False) == (ACCEPTED, None)
    if any(blind):                                                                         # the blinders reach every commitment they should
        plain = R.prove(wit, [0] * 14)
        assert all(plain["proof"][k] != proof[k] for k in ("C1", "C2", "C3"))


def test_keys_and_proofs_go_through_json_and_bytes(flt, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    proof, publics = flt.prove(key, wit, blinding=BLIND)
    vk = flt.vk_from_json(flt.vk_to_json(key.vk))
    assert (vk.curve, vk.log_n, vk.n_public, vk.k1, vk.k2, vk.c0, vk.c0l, vk.digest) == (cv, 4, 1, key.k1, key.k2, key.vk.c0, key.vk.c0l, key.vk.digest)
    back = flt.proof_from_json(flt.proof_to_json(proof, cv), cv)
    assert back == proof and flt.proof_from_bytes(flt.proof_to_bytes(proof), handles[cv].point_bytes) == proof
    assert '"protocol": "fflonk-shplonk-lookup-tagged"' in flt.vk_to_json(key.vk) and '"protocol": "fflonk-shplonk-lookup-tagged"' in flt.proof_to_json(proof, cv)
    assert flt.verify(vk, [publics], [back], kzg=handles[cv]) == (ACCEPTED, None)
    with pytest.raises(flt.ZkError, match="verify needs the Kzg handle"):
        flt.verify(vk, [publics], [back])


def test_a_batch_verifies_in_one_check(flt, world):
    circuit, wit, key, R = world("BN128", 16)
    r = R.r
    made = [flt.prove(key, wit) for _ in range(3)]                                         # blinders from `secrets`
    proofs, publics = [p for p, _ in made], [x for _, x in made]
    assert flt.verify(key.vk, publics, proofs) == (ACCEPTED, None)
    assert flt.verify(key.vk, publics, proofs, seed=SEED) == (ACCEPTED, None)
    for name in flt.POINT_NAMES:
        assert len({p[name] for p in proofs}) == 3, name                                   # every commitment moves with the blinders
    for i in range(13, 23):                                                                # and every value of a, b, c, M, Z, Phi, Zw, Phiw, T0w, T1w
        assert len({p["values"][i] for p in proofs}) == 3, i
    moved = dict(proofs[1], values=proofs[1]["values"][:12] + [(proofs[1]["values"][12] + 1) % r] + proofs[1]["values"][13:])
    for at in range(3):
        batch = proofs[:at] + [moved] + proofs[at + 1:]
        assert flt.verify(key.vk, publics, batch) == (REJECTED, at), at
        assert flt.verify(key.vk, publics, batch, seed=SEED, locate=False) == (REJECTED, None), at


def test_rejections(zk, flt, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r, vk = R.r, key.vk
    proof, publics = flt.prove(key, wit, blinding=BLIND)
    assert flt.verify(vk, [publics], [proof]) == (ACCEPTED, None)
    for i in range(23):                                                                    # each of the 23 values + 1; 12 is Tg(xi)
        bad = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert flt.verify(vk, [publics], [bad]) == (REJECTED, 0), i
    assert flt.VALUE_NAMES[12] == "T0" and proof["values"][12] not in (0, 1, 2)
    for tag in (0, 1, 2):                                                                  # Tg(xi) replaced by a plausible constant
        assert flt.verify(vk, [publics], [dict(proof, values=proof["values"][:12] + [tag] + proof["values"][13:])]) == (REJECTED, 0), tag
    other = world.points[cv](0xABCDEF)
    for name in flt.POINT_NAMES:                                                           # each of the 5 points replaced by another valid point
        assert flt.verify(vk, [publics], [dict(proof, **{name: other})]) == (REJECTED, 0), name
    assert flt.verify(vk, [[(publics[0] + 1) % r]], [proof]) == (REJECTED, 0)              # the public input + 1
    for name in ("c0", "c0l"):                                                             # each point of the key
        c0, c0l = (other if name == "c0" else vk.c0), (other if name == "c0l" else vk.c0l)
        assert flt.verify(flt.VerifyingKey(cv, vk.log_n, vk.n_public, vk.k1, vk.k2, c0, c0l, handles[cv]), [publics], [proof]) == (REJECTED, 0), name
    _, _, key8, _ = world(cv, 8)                                                           # the other circuit size
    assert flt.verify(key8.vk, [publics], [proof]) == (REJECTED, 0)
    for i in (0, 12, 17, 22):                                                              # a value equal to r
        assert flt.verify(vk, [publics], [dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])]) == (NOT_CANONICAL, 0), i
    assert flt.verify(vk, [[r]], [proof]) == (NOT_CANONICAL, 0)
    with pytest.raises(flt.ZkError, match="a proof holds 23 values"):                      # truncated
        flt.verify(vk, [publics], [dict(proof, values=proof["values"][:22])])
    with pytest.raises(flt.ZkError, match="point C3 of the proof is 63 bytes"):
        flt.verify(vk, [publics], [dict(proof, C3=proof["C3"][:-1])])


def test_the_unweighted_count_and_a_key_with_swapped_tags(flt, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    proof, publics = flt.prove(key, wit, blinding=BLIND)
    # M from the unweighted count: the sum does not close
    counts, _ = R.multiplicities(R.wires_of(wit), weighted=False)
    m, _ = R.multiplicities(R.wires_of(wit))
    assert counts != m
    with pytest.raises(flt.ZkError, match="^fflonk lookup tagged: the lookup sum does not close"):
        flt.prove(key, wit, blinding=BLIND, _multiplicities=counts)
    wires = R.wires_of(wit)
    assert flt.prove(key, wit, blinding=BLIND, _multiplicities=m, _wires=[wires[k] for k in "abc"])[0] == proof       # the hooks themselves are sound
    # a key whose table tags are swapped: the same rows, the same gates, the XOR table numbered 1
    n_vars, public, gates, tables, _ = _circuit_of(cv, 16)
    key2 = flt.FflonkLookupTaggedKey(handles[cv], flt.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables[::-1]))
    try:
        assert key2.vk.c0 == key.vk.c0 and key2.vk.c0l != key.vk.c0l and key2.vk.digest != key.vk.digest
        assert flt.verify(key2.vk, [publics], [proof]) == (REJECTED, 0)
        with pytest.raises(flt.ZkError, match=r"does not satisfy lookup at row \d+ \(\d+ rows\): \(a, b, c\) is not a row of table [12]"):
            flt.prove(key2, wit, blinding=BLIND)                                           # and the witness no longer fits it
    finally:
        key2.free()
    # a file of power 6 holds 127 G1 powers, n = 16 needs 136
    with pytest.raises(flt.ZkError, match=r"^fflonk lookup tagged: the file holds 127 G1 powers, n = 16 rows need 8n \+ 8 = 136 \(a file of power 7 has them\)$"):
        flt.FflonkLookupTaggedKey(handles["small"], circuit)


def test_the_prover_refuses_a_tuple_of_the_other_table_by_row_and_table(flt, handles, world):
    cv = "BN128"
    circuit, wit, key, R = world(cv, 16)
    r = R.r
    looked = [i for i in range(R.t.n) if R.qk[i] == 1]
    row = looked[-1]                                                                       # the range check of 1 ...
    assert (R.wires_of(wit)["a"][row], R.qk[row]) == (1, 1)
    n_vars, public, gates, tables, _ = _circuit_of(cv, 16)
    g = row - len(public)
    gates = dict(gates, b=gates["b"][:g] + [gates["a"][g]] + gates["b"][g + 1:])           # ... now holds (1, 1, 0): a row of the XOR table alone
    key2 = flt.FflonkLookupTaggedKey(handles[cv], flt.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables))
    try:
        R2 = ftref.Reference(cv, n_vars, public, gates, tables, TAU[cv], world.points[cv])
        assert R2.multiplicities(R2.wires_of(wit))[1] == [row] and (2, 1, 1, 0) in R2.rows
        with pytest.raises(flt.ZkError, match=r"^fflonk lookup tagged: witness does not satisfy lookup at row %d \(1 rows\): \(a, b, c\) is not a row of table 1, the table the row's qK names$" % row):
            flt.prove(key2, wit, blinding=BLIND)
        both = list(wit)                                                                   # a gate failure is still named first
        both[5] = (both[5] + 1) % r
        rows = R2.gates_hold(R2.wires_of(both), [both[circuit.public[0]]])
        assert rows
        with pytest.raises(flt.ZkError, match=r"fflonk lookup tagged: witness does not satisfy gate %d \(%d rows\)" % (rows[0], len(rows))):
            flt.prove(key2, both, blinding=BLIND)
    finally:
        key2.free()


def test_a_table_tuple_under_qk_zero_is_not_counted(flt, handles, world):
    """the last XOR lookup's selector set to 0: its tuple is still a row of table 2, but the row is no lookup, m moves and the proof is the
    reference's for THAT circuit; any value in the row then passes"""
    cv = "BN128"
    n_vars, public, gates, tables, wit = _circuit_of(cv, 16)
    g = max(i for i, q in enumerate(gates["qK"]) if q == 2)
    gates = dict(gates, qK=gates["qK"][:g] + [0] + gates["qK"][g + 1:])
    key = flt.FflonkLookupTaggedKey(handles[cv], flt.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables))
    try:
        _, _, _, R0 = world(cv, 16)
        R = ftref.Reference(cv, n_vars, public, gates, tables, TAU[cv], world.points[cv])
        m0, m = R0.multiplicities(R0.wires_of(wit))[0], R.multiplicities(R.wires_of(wit))[0]
        assert sum(m0) - sum(m) == 2 and sum(1 for x, y in zip(m0, m) if x != y) == 1      # one row of table 2 lost one use, weight 2
        want = R.prove(wit, BLIND)
        proof, publics = flt.prove(key, wit, blinding=BLIND)
        assert proof == want["proof"] and want["m"] == m
        assert flt.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    finally:
        key.free()
