"""compressor12 setup on the device (csrc/c12_setup.hip through the C ABI).
Parity: gates, additions, n_bits, n_used, the .exec text and the whole .const matrix against the line-for-line restatement
of the reference (tests/c12_setup_ref.py), word for word.
Meaning: a satisfying witness goes setup -> Compressor12Exec.run -> the generated PIL compiled by tools/pilc.py ->
zk_starkinfo_generate -> a proof with the self check on, in bytecode mode (nothing is compiled); the proof must verify and
the same witness with one wire changed must not.  That checks the generated PIL, the selectors, the constants and the
wiring together without trusting the restatement.
Covered by a proof: plain gates, and plain gates + each of CMulAdd, Poseidon12, FFT4 (both types) and EvPol4."""
import importlib, json, pathlib, sys
import numpy as np
import pytest

import c12_setup_ref as REF
import c12_setup_circuits as CC

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
P = REF.P


@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)
    return importlib.import_module("eigen_zkvm_amd.compressor12")


@pytest.fixture(scope="module")
def cposeidon():
    return REF.project_cposeidon()


PARITY = {"random_50_pub1": (50, 1, (), 0), "random_300_pub12": (300, 12, (), 0), "random_120_pub13_two_L": (120, 13, (), 0),
          "forced_n_bits": (77, 3, (), 9), "one_of_each_custom_gate": (60, 3, ("CMulAdd", "Poseidon12", "FFT4_4", "FFT4_2", "EvPol4"), 0)}


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_with_the_restatement(zk, dev, cposeidon, name):
    n, pub, custom, force = PARITY[name]
    b, r = CC.random_r1cs(sorted(PARITY).index(name), n, pub, custom=custom)
    ref = REF.plonk_setup(r, cposeidon, force)
    S = dev.Compressor12Setup.from_r1cs(b, force)
    assert (S.n_bits, S.n_used, S.n_publics, S.n_const) == (ref["n_bits"], ref["n_used"], ref["n_publics"], ref["n_const"])
    assert S.gates().tolist() == [list(g) for g in ref["gates"]]
    assert (S.n_gates, S.n_adds) == (len(ref["gates"]), len(ref["adds"]))
    assert S.exec_text == REF.write_exec(ref["adds"], ref["s_map"])
    want = np.array(ref["const"], dtype=np.uint64)
    got = S.consts().to_host().reshape(1 << S.n_bits, S.n_const)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (row, column): %s" % bad[:5].tolist()
    assert np.array_equal(S.consts_host().reshape(got.shape), want)
    S.free()


def test_an_odd_gate_is_repeated(zk, dev, cposeidon):
    """three gates under one key and one under another: both rows are terminated by copying (plonk_setup.rs:346-360)"""
    mul = lambda a, b, c: ([(a, 1)], [(b, 1)], [(c, 1)])
    b = REF.write_r1cs(12, 0, 2, 9, [mul(1, 2, 3), mul(3, 4, 5), mul(5, 6, 7), ([], [], [(7, 1), (8, 2), (9, 3)])])
    ref = REF.plonk_setup(REF.read_r1cs(b), cposeidon)
    S = dev.Compressor12Setup.from_r1cs(b)
    assert S.exec_text == REF.write_exec(ref["adds"], ref["s_map"])
    assert [ref["s_map"][c][1] for c in range(12)] == [1, 2, 3, 3, 4, 5, 5, 6, 7, 5, 6, 7]      # the third gate fills the second half twice
    assert [ref["s_map"][c][2] for c in range(12)] == [7, 8, 9, 7, 8, 9, 0, 0, 0, 0, 0, 0]      # the lone sum fills its half twice, the other stays empty
    assert np.array_equal(S.consts().to_host().reshape(-1, S.n_const), np.array(ref["const"], dtype=np.uint64))


def stark_struct(n_bits):
    """tests/golden/starky_data/c12.starkStruct.json with nBits lowered"""
    steps = [{"nBits": n_bits + 1}]
    while steps[-1]["nBits"] > 5: steps.append({"nBits": max(steps[-1]["nBits"] - 4, 3)})
    return {"nBits": n_bits, "nBitsExt": n_bits + 1, "nQueries": 8, "verificationHashType": "GL", "steps": steps}


def prove(zk, dev, r1cs, witness, n_bits):
    """-> (accepted, publics): setup -> exec -> pilc -> the library's code generator -> proof with the self check on -> verify"""
    sys.path.insert(0, str(ROOT / "tools"))
    import pilc
    stark = importlib.import_module("eigen_zkvm_amd.stark")
    S = dev.Compressor12Setup.from_r1cs(r1cs, n_bits)
    ss = stark_struct(S.n_bits)
    pil = pilc.compile_pil("c12.pil", S.pil)
    assert pil["nConstants"] == S.n_const and pil["nCommitments"] == 12
    program = stark.generate_program(json.dumps(pil), json.dumps(ss))
    E = dev.Compressor12Exec(S.exec_text, len(witness))
    cm = E.run(np.array(witness, dtype=np.uint64), 1 << S.n_bits)
    setup = stark.NativeStarkSetup(S.consts_host(), program, json.dumps(ss), self_check=True, eval_mode="bytecode")
    try:
        zkin = setup.gen_json(cm)
        return setup.verify(zkin), [int(x) for x in json.loads(zkin)["publics"]]
    except zk.ZkError:
        return False, None
    finally:
        setup.free(); E.free(); S.free()


@pytest.mark.parametrize("circuit", ["plain", "cmuladd", "poseidon", "fft4", "evpol4"])
def test_a_proof_of_the_generated_pil_verifies(zk, dev, circuit):
    r1cs, w = CC.plain_circuit() if circuit == "plain" else CC.with_custom(circuit)
    ok, publics = prove(zk, dev, r1cs, w, 8)
    assert ok and publics == w[1:4]
    bad = list(w); bad[-1] = (bad[-1] + 1) % P                                  # the last wire: a sum's output / the custom gate's last output
    assert prove(zk, dev, r1cs, bad, 8)[0] is False
    bad = list(w); bad[5] = (bad[5] + 1) % P                                    # a wire several gates share: the wiring must notice
    assert prove(zk, dev, r1cs, bad, 8)[0] is False


def test_errors(zk, dev):
    new = dev.Compressor12Setup.from_r1cs
    mul = [([(1, 1)], [(2, 1)], [(3, 1)])]
    good = REF.write_r1cs(30, 0, 2, 27, mul)
    with pytest.raises(zk.ZkError, match="Invalid custom gate Rescue"):
        new(REF.write_r1cs(30, 0, 2, 27, mul, [("Rescue", [])], []))
    with pytest.raises(zk.ZkError, match="Different prime"):
        new(REF.write_r1cs(30, 0, 2, 27, mul, field_size=32, prime=21888242871839275222246405745257275088548364400416034343698204186575808495617))
    with pytest.raises(zk.ZkError, match="Different prime"):
        new(REF.write_r1cs(30, 0, 2, 27, mul, prime=P - 2))
    with pytest.raises(zk.ZkError, match="truncated file"):
        new(good[:-5])
    with pytest.raises(zk.ZkError, match="Invalid magic number"):
        new(b"r1cx" + good[4:])
    with pytest.raises(zk.ZkError, match="not a canonical field element"):
        new(REF.write_r1cs(30, 0, 2, 27, [([(1, P)], [(2, 1)], [(3, 1)])]))
    with pytest.raises(zk.ZkError, match="wire index out of range"):
        new(REF.write_r1cs(30, 0, 2, 27, [([(30, 1)], [(2, 1)], [(3, 1)])]))
    b, _ = CC.random_r1cs(0, 50, 1)
    with pytest.raises(zk.ZkError, match="force_n_bits 3 is too small"):
        new(b, 3)
    with pytest.raises(zk.ZkError, match="371 signals, not 372"):
        new(REF.write_r1cs(30, 0, 2, 27, mul, list(CC.ALL_TEMPLATES), [(1, [1] * 371)]))
