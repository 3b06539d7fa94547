"""PLONK from circom circuits end to end on the device: an R1csCircuit's key, prove() from the n_wires values of the .wtns
and from its bytes, against tests/plonk_ref.py's Reference run on the MODEL's gate table and extended witness (tests/plonk_r1cs_ref.py) over
powers-of-tau files with a known tau, as test_gpu_plonk.py builds them: with fixed blinders the device's proof is the reference's BYTE FOR
BYTE.  The circuits: the reference project's multiplier.r1cs with its witness (n = 8), mycircuit_bls12381.r1cs with the same values (n = 8),
products("BN128", 37) (n = 128), products("BLS12381", 4) (7 gates, since one of its four constraints has a = a2 and needs no auxiliary: n = 8),
products("BLS12381", 5) (n = 16) and shapes("BN128") (n = 2048, a segment of 999 terms).  Then the proof
alone and in a batch with a proof made through the gate-table route, a corrupted output wire named by its constraint, and the refusals of
a witness.  Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import plonk_r1cs_ref as model
import plonk_ref as ref
import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
POWER = {"BN128": 13, "BLS12381": 5}                    # 2^(power + 1) - 1 powers: at least 3n + 6 for n = 2048 and n = 16
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(9)]
SEED = bytes(range(32))
ACCEPTED = 1
MULT_W = [1, 11210000, 1121, 10000]
CASES = [("multiplier", "BN128", 8), ("mycircuit", "BLS12381", 8), ("products37", "BN128", 128), ("products4", "BLS12381", 8), ("products5", "BLS12381", 16),
         ("shapes", "BN128", 2048)]


def circuit_of(name, cv):
    """-> (r1cs bytes, witness, [(an output wire, its constraint)])"""
    if name == "multiplier":
        return (ROOT / "tests" / "golden" / "plonk" / "multiplier.r1cs").read_bytes(), MULT_W, [(1, 0)]
    if name == "mycircuit":
        return (ROOT / "tests" / "golden" / "groth16" / "mycircuit_bls12381.r1cs").read_bytes(), MULT_W, [(1, 0)]
    if name.startswith("products"):
        data, w, outs = cases.products(cv, int(name[8:]))
        return data, w, [(outs[-1], len(outs) - 1), (outs[0], 0)]
    data, w, long_row, cw = cases.shapes(cv)
    return data, w, [(cw, long_row)]


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
    d = tmp_path_factory.mktemp("plonk_r1cs")
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
    """per circuit: the R1csCircuit, its witness, the device key, the model and the reference over the model's table, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(name, cv):
        if name not in made:
            data, w, outs = circuit_of(name, cv)
            m = model.Compiled(data, cv)
            c = plonk.R1csCircuit(data, cv)
            made[name] = (c, w, outs, plonk.PlonkKey(handles[cv], c), m, ref.Reference(cv, m.n_vars, m.public, m.gates, TAU[cv], points[cv]))
        return made[name]
    yield get
    for c, _, _, key, _, _ in made.values():
        key.free()
        c.free()


@pytest.mark.parametrize("name,cv,n", CASES)
def test_the_proof_from_the_witness_is_the_reference_proof_of_the_models_table(zk, plonk, world, name, cv, n):
    c, w, outs, key, m, R = world(name, cv)
    assert (c.n, key.n, c.n_vars) == (n, n, m.n_vars)
    assert key.vk.commitments == R.vk_points and key.vk.digest == R.vkd
    want = R.prove(m.extend(w), BLIND)
    proof, publics = plonk.prove(key, w, blinding=BLIND)
    assert publics == want["publics"] == [w[v] for v in m.public]
    assert proof["values"] == want["values"]
    for k in plonk.POINT_NAMES:
        assert proof[k] == want["proof"][k], k
    assert plonk.proof_to_bytes(proof) == plonk.proof_to_bytes(want["proof"])
    assert plonk.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    # the same from the bytes of the .wtns
    proof2, publics2 = plonk.prove(key, cases.wtns_bytes(cv, w), blinding=BLIND)
    assert (proof2, publics2) == (proof, publics)


@pytest.mark.parametrize("name,cv", (("multiplier", "BN128"), ("products4", "BLS12381")))
def test_a_batch_with_a_proof_made_through_the_gate_table(plonk, handles, world, name, cv):
    c, w, outs, key, m, R = world(name, cv)
    key2 = plonk.PlonkKey(handles[cv], plonk.Circuit(m.n_vars, m.public, m.gates, cv))               # the model's table, through Circuit
    try:
        assert key2.vk.digest == key.vk.digest
        p1, x1 = plonk.prove(key, w)                                                                # blinders from `secrets`
        p2, x2 = plonk.prove(key2, m.extend(w))
        assert x1 == x2 and p1["A"] != p2["A"]
        for vk in (key.vk, key2.vk):
            assert plonk.verify(vk, [x1, x2], [p1, p2]) == (ACCEPTED, None)
            assert plonk.verify(vk, [x1, x2], [p1, p2], seed=SEED, locate=False) == (ACCEPTED, None)
        moved = dict(p2, values=p2["values"][:12] + [(p2["values"][12] + 1) % m.p] + p2["values"][13:])
        assert plonk.verify(key.vk, [x1, x2], [p1, moved]) == (0, 1)
    finally:
        key2.free()


def test_a_wrong_output_wire_names_its_constraint_and_a_bad_witness_is_refused_on_the_host(plonk, world):
    for name, cv in (("products37", "BN128"), ("shapes", "BN128"), ("mycircuit", "BLS12381")):
        c, w, outs, key, m, R = world(name, cv)
        for wire, con in outs:
            bad = cases.corrupt(w, wire, p=m.p)
            gates = m.failing_gates(m.extend(bad))
            assert gates and m.origin[gates[0]] == con
            text = r"witness does not satisfy gate %d \(constraint %d of the \.r1cs\) \(%d rows\)" % (gates[0], con, len(gates))
            with pytest.raises(plonk.ZkError, match=text):
                plonk.prove(key, bad, blinding=BLIND)
            with pytest.raises(plonk.ZkError, match=text):
                plonk.prove(key, cases.wtns_bytes(cv, bad), blinding=BLIND)
    c, w, outs, key, m, R = world("products37", "BN128")
    with pytest.raises(plonk.ZkError, match=r"gate 64 \(constraint 36 of the \.r1cs\)"):
        plonk.prove(key, cases.corrupt(w, outs[0][0], p=m.p), blinding=BLIND)
    with pytest.raises(plonk.ZkError, match="witness value 0 is 2: wire 0 of a circom witness is the constant 1"):
        plonk.prove(key, [2] + w[1:])
    with pytest.raises(plonk.ZkError, match="the witness has %d values, the .r1cs has %d wires" % (m.n_wires - 1, m.n_wires)):
        plonk.prove(key, w[:-1])
    with pytest.raises(plonk.ZkError, match="the witness has %d values" % m.n_vars):                 # the extended witness is not what this key takes
        plonk.prove(key, m.extend(w))
    with pytest.raises(plonk.ZkError, match="the file is not a witness over BN128"):
        plonk.prove(key, cases.wtns_bytes("BLS12381", w))
