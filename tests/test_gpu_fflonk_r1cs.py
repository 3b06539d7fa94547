"""fflonk from circom circuits end to end on the device (DESIGN.md 3.23 over 3.22): an R1csCircuit's key, prove() from the n_wires values of
the .wtns and from its bytes, against tests/fflonk_ref.py's Reference run on the MODEL's gate table and extended witness
(tests/plonk_r1cs_ref.py) over powers-of-tau files with a known tau: with fixed blinders the device's proof is the reference's BYTE FOR BYTE.
The circuits: the reference project's multiplier.r1cs with its witness (n = 8), products("BN128", 37) (n = 128) and products("BLS12381", 5)
(n = 16).  Then a corrupted output wire named by its constraint and the refusals of a witness.  Exact: no tolerance anywhere."""
import importlib, pathlib, sys

import numpy as np
import pytest

import fflonk_ref as ref
import plonk_r1cs_ref as model
import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_test_ptau  # noqa: E402

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
POWER = {"BN128": 10, "BLS12381": 7}                    # 2^(power + 1) - 1 powers: at least 9n + 18 for n = 128 and n = 16
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(9)]
ACCEPTED = 1
MULT_W = [1, 11210000, 1121, 10000]
CASES = [("multiplier", "BN128", 8), ("products37", "BN128", 128), ("products5", "BLS12381", 16)]


def circuit_of(name, cv):
    """-> (r1cs bytes, witness, [(an output wire, its constraint)])"""
    if name == "multiplier":
        return (ROOT / "tests" / "golden" / "plonk" / "multiplier.r1cs").read_bytes(), MULT_W, [(1, 0)]
    data, w, outs = cases.products(cv, int(name[8:]))
    return data, w, [(outs[-1], len(outs) - 1), (outs[0], 0)]


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
    d = tmp_path_factory.mktemp("fflonk_r1cs")
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
    """per circuit: the R1csCircuit, its witness, the device key, the model and the reference over the model's table, made once"""
    made, points = {}, {cv: Points(zk, cv) for cv in POWER}

    def get(name, cv):
        if name not in made:
            data, w, outs = circuit_of(name, cv)
            m = model.Compiled(data, cv)
            c = fflonk.R1csCircuit(data, cv)
            made[name] = (c, w, outs, fflonk.FflonkKey(handles[cv], c), m, ref.Reference(cv, m.n_vars, m.public, m.gates, TAU[cv], points[cv]))
        return made[name]
    yield get
    for c, _, _, key, _, _ in made.values():
        key.free()
        c.free()


@pytest.mark.parametrize("name,cv,n", CASES)
def test_the_proof_from_the_witness_is_the_reference_proof_of_the_models_table(zk, fflonk, world, name, cv, n):
    c, w, outs, key, m, R = world(name, cv)
    assert (c.n, key.n, c.n_vars) == (n, n, m.n_vars)
    assert key.vk.c0 == R.C0 and key.vk.digest == R.vkd
    want = R.prove(m.extend(w), BLIND)
    proof, publics = fflonk.prove(key, w, blinding=BLIND)
    assert publics == want["publics"] == [w[v] for v in m.public]
    assert proof["values"] == want["values"]
    for k in fflonk.POINT_NAMES:
        assert proof[k] == want["proof"][k], k
    assert fflonk.proof_to_bytes(proof) == fflonk.proof_to_bytes(want["proof"])
    assert fflonk.verify(key.vk, [publics], [proof]) == (ACCEPTED, None)
    # the same from the bytes of the .wtns
    proof2, publics2 = fflonk.prove(key, cases.wtns_bytes(cv, w), blinding=BLIND)
    assert (proof2, publics2) == (proof, publics)


def test_a_wrong_output_wire_names_its_constraint_and_a_bad_witness_is_refused_on_the_host(fflonk, world):
    for name, cv in (("products37", "BN128"), ("multiplier", "BN128"), ("products5", "BLS12381")):
        c, w, outs, key, m, R = world(name, cv)
        for wire, con in outs:
            bad = cases.corrupt(w, wire, p=m.p)
            gates = m.failing_gates(m.extend(bad))
            assert gates and m.origin[gates[0]] == con
            text = r"witness does not satisfy gate %d \(constraint %d of the \.r1cs\) \(%d rows\)" % (gates[0], con, len(gates))
            with pytest.raises(fflonk.ZkError, match=text):
                fflonk.prove(key, bad, blinding=BLIND)
            with pytest.raises(fflonk.ZkError, match=text):
                fflonk.prove(key, cases.wtns_bytes(cv, bad), blinding=BLIND)
    c, w, outs, key, m, R = world("products37", "BN128")
    with pytest.raises(fflonk.ZkError, match="witness value 0 is 2: wire 0 of a circom witness is the constant 1"):
        fflonk.prove(key, [2] + w[1:])
    with pytest.raises(fflonk.ZkError, match="the witness has %d values, the .r1cs has %d wires" % (m.n_wires - 1, m.n_wires)):
        fflonk.prove(key, w[:-1])
    with pytest.raises(fflonk.ZkError, match="the file is not a witness over BN128"):
        fflonk.prove(key, cases.wtns_bytes("BLS12381", w))
