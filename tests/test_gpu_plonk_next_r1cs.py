"""PLONK with a next-row term from circom circuits end to end on the device: a NextR1csCircuit's key, prove() from the
n_wires values of the .wtns and from its bytes, against tests/plonk_next_ref.py's Reference run on the MODEL's chain-rule table and extended
witness, over powers-of-tau files with a known tau: with fixed blinders the device's proof is the model's BYTE FOR BYTE.  The circuits:
multiplier.r1cs with its witness (n = 8, no chain at all) and shapes("BN128") (n = 1024 where plonk.py needs 2048: chains of every small
length, three on one product constraint, and a closed chain of 1001 terms).  Then a corrupted output wire named by its gate and constraint,
and the circuit of the other rule proved here as it is.  Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import plonk_next_ref as nref
import plonk_r1cs_ref as model
import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

CV = "BN128"
TAU = 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e
POWER = 11                                              # 4095 powers: at least 3n + 7 for n = 1024
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(10)]
ACCEPTED = 1
MULT_W = [1, 11210000, 1121, 10000]
CASES = [("multiplier", 8), ("shapes", 1024)]


def circuit_of(name):
    if name == "multiplier":
        return (ROOT / "tests" / "golden" / "plonk" / "multiplier.r1cs").read_bytes(), MULT_W, [(1, 0)]
    data, w, long_row, cw = cases.shapes(CV)
    return data, w, [(cw, long_row)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def pn(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_next")


@pytest.fixture(scope="module")
def handle(zk, tmp_path_factory):
    g16, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    p = tmp_path_factory.mktemp("plonk_next_r1cs") / "f.ptau"
    p.write_bytes(make_test_ptau.build_ptau(zk, CV, POWER, TAU, 5, 7))
    srs = g16.Srs(CV, p)
    h = kzg.Kzg(srs)
    srs.free()
    yield h
    h.free()


@pytest.fixture(scope="module")
def world(zk, pn, handle):
    seen = {}

    def point(k):
        if k not in seen:
            w = np.array([(k >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
            seen[k] = zk.mul_generator_fr(zk.DevArray.from_host(w), "bn254").to_host().astype("<u8").tobytes()
        return seen[k]
    made = {}

    def get(name):
        if name not in made:
            data, w, outs = circuit_of(name)
            m = nref.Compiled(data, CV)
            c = pn.NextR1csCircuit(data, CV)
            made[name] = (c, w, outs, pn.NextKey(handle, c), m, nref.Reference(CV, m.n_vars, m.public, m.gates, TAU, point))
        return made[name]
    yield get
    for c, _, _, key, _, _ in made.values():
        key.free()
        c.free()


@pytest.mark.parametrize("name,n", CASES)
def test_the_proof_from_the_witness_is_the_model_proof_of_the_models_table(zk, pn, world, name, n):
    c, w, outs, key, m, R = world(name)
    assert (c.n, key.n, c.n_vars) == (n, n, m.n_vars)
    if name == "shapes":
        old = model.Compiled(circuit_of(name)[0], CV)
        assert 1 + old.n_gates > n >= 1 + m.n_gates                                   # the table of the other rule does not fit these rows
        assert any(m.gates["qN"]) and m.gates["qN"][-1] == 0
    assert key.vk.commitments == R.vk_points and key.vk.digest == R.vkd
    want = R.prove(m.extend(w), BLIND)
    proof, publics = pn.prove(key, w, blinding=BLIND)
    assert publics == want["publics"] == [w[v] for v in m.public]
    assert proof["values"] == want["values"]
    for k in pn.POINT_NAMES:
        assert proof[k] == want["proof"][k], k
    assert pn.proof_to_bytes(proof) == pn.proof_to_bytes(want["proof"])
    assert pn.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    proof2, publics2 = pn.prove(key, cases.wtns_bytes(CV, w), blinding=BLIND)            # the same from the bytes of the .wtns
    assert (proof2, publics2) == (proof, publics)


def test_a_wrong_wire_names_its_gate_and_constraint(pn, world):
    for name in ("shapes", "multiplier"):
        c, w, outs, key, m, R = world(name)
        for wire, con in outs:
            bad = cases.corrupt(w, wire, p=m.p)
            gates = m.failing_gates(m.extend(bad))
            assert gates and m.origin[gates[0]] == con
            text = r"plonk next: witness does not satisfy gate %d \(constraint %d of the \.r1cs\) \(%d rows\)" % (gates[0], con, len(gates))
            with pytest.raises(pn.ZkError, match=text):
                pn.prove(key, bad, blinding=BLIND)
    c, w, outs, key, m, R = world("shapes")
    with pytest.raises(pn.ZkError, match="witness value 0 is 2: wire 0 of a circom witness is the constant 1"):
        pn.prove(key, [2] + w[1:])
    with pytest.raises(pn.ZkError, match="the witness has %d values, the .r1cs has %d wires" % (m.n_wires - 1, m.n_wires)):
        pn.prove(key, w[:-1])


def test_the_table_of_the_other_rule_is_proved_here_as_it_is(pn, handle):
    data, w, outs = circuit_of("multiplier")
    c = pn.R1csCircuit(data, CV)                                                       # plonk_arith's class: the rule of fan-in 2, no qN
    key = pn.NextKey(handle, c)
    try:
        proof, publics = pn.prove(key, w, blinding=BLIND)
        assert pn.verify(key.vk, [publics], [proof]) == (ACCEPTED, None) and proof["values"][8] == 0
        lib, h = importlib.import_module("eigen_zkvm_amd").lib(), c._h
        assert lib.zk_plonk_bn254_next_r1cs_qn(h, None) != 0 and "not compiled under the chain rule" in lib.zk_last_error().decode()
    finally:
        key.free()
        c.free()
