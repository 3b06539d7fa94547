"""The surface of the fflonk layer without a GPU: the header declares the new entry points and the library exports them, the package binds
them, eigen_zkvm_amd.fflonk has its functions, the command-line tool parses its three commands, what is refused before any device work comes
back with its text, and host_values / parts_of are compared with the direct evaluation of small random interleaved polynomials."""
import importlib, pathlib, random, re, sys, types

import numpy as np
import pytest

import kzg_multi_ref as mref
import kzg_ref
import plonk_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_fflonk_%s_quotients_dev" % c for c in ("bn254", "bls12_381")]


@pytest.fixture(scope="module")
def fflonk(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk")


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "d_out0" in code and "d_out1" in code and "d_out2" in code


def test_package_exports_and_binds_them(zk, fflonk):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    lib = zk.lib()                                      # dlopen + every signature: no device is touched
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == 10, name
    for name in ("FflonkKey", "setup", "prove", "verify", "host_values", "challenges", "required_powers", "vk_to_json", "vk_from_json", "vk_to_bytes", "vk_from_bytes",
                 "proof_to_json", "proof_from_json", "proof_to_bytes", "proof_from_bytes", "vk_digest", "transcript_start", "transcript_round1", "transcript_round2",
                 "transcript_values", "transcript_z", "quotients", "roots", "host_check"):
        assert callable(getattr(fflonk, name)), name
    assert zk.FflonkKey is fflonk.FflonkKey
    for fn in (fflonk.vk_digest, fflonk.transcript_start, fflonk.transcript_round1, fflonk.transcript_round2, fflonk.transcript_values, fflonk.transcript_z):
        assert "H(" in fn.__doc__, fn.__name__           # the hashed bytes are stated where the function is
    assert len(fflonk.VALUE_NAMES) == fflonk.N_VALUES == 15 and fflonk.POINT_NAMES == ("C1", "C2", "W1", "W2")


def test_cli_parses_its_three_commands():
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_fflonk")
    ap = cli.build_parser()
    a = ap.parse_args(["fflonk_setup", "-c", "BN128", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])
    assert (a.cmd, a.curve, a.ptau, a.circuit, a.r1cs, a.vk, a.no_check_srs) == ("fflonk_setup", "BN128", "f.ptau", "c.npz", None, "vk.json", False)
    a = ap.parse_args(["fflonk_setup", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "-v", "vk.json"])
    assert (a.circuit, a.r1cs) == (None, "c.r1cs")
    a = ap.parse_args(["fflonk_prove", "-c", "BLS12381", "--ptau", "f.ptau", "--circuit", "c.npz", "--witness", "w.bin", "--proof", "proof.json", "--public", "public.json",
                       "--no-check-srs"])
    assert (a.cmd, a.curve, a.witness, a.proof, a.public, a.no_check_srs) == ("fflonk_prove", "BLS12381", "w.bin", "proof.json", "public.json", True)
    a = ap.parse_args(["fflonk_prove", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--proof", "proof.json", "--public", "public.json"])
    assert (a.r1cs, a.wtns, a.witness) == ("c.r1cs", "w.wtns", None)
    a = ap.parse_args(["fflonk_verify", "-v", "vk.json", "--ptau", "f.ptau", "p1.json:x1.json", "p2.json:x2.json"])
    assert (a.cmd, a.vk, a.pairs) == ("fflonk_verify", "vk.json", ["p1.json:x1.json", "p2.json:x2.json"])
    assert cli.split_pair("p1.json:x1.json") == ("p1.json", "x1.json")
    with pytest.raises(SystemExit):
        cli.split_pair("p1.json")
    with pytest.raises(SystemExit):
        ap.parse_args(["fflonk_setup", "--ptau", "f.ptau", "-v", "vk.json"])          # the circuit is required
    with pytest.raises(SystemExit):
        ap.parse_args(["fflonk_prove", "--ptau", "f.ptau", "--circuit", "c.npz", "--r1cs", "c.r1cs", "--witness", "w.bin", "--proof", "p", "--public", "x"])
    with pytest.raises(SystemExit):
        cli.main(["fflonk_prove", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "--witness", "w.bin", "--proof", "p", "--public", "x"])   # --r1cs goes with --wtns


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_host_values_against_direct_evaluation_of_interleaved_polynomials(fflonk, cv):
    r, rng = ref.R[cv], random.Random(0x25 + len(cv))
    log_n = 4
    rt = fflonk.roots(cv, log_n, rng.randrange(1, r))
    for t, points, at in ((8, rt["S0"], rt["xi"]), (4, rt["S1"], rt["xi"]), (3, rt["S2"][:3], rt["xi"]), (3, rt["S2"][3:], rt["xiw"])):
        polys = [[rng.randrange(r) for _ in range(rng.randrange(1, 9))] for _ in range(t)]                # unequal lengths: zero-padded
        whole = mref.interleave(polys)
        parts = [kzg_ref.horner(p, at, r) for p in polys]                                                 # f_m(x^t), the same for every x of the set
        direct = [kzg_ref.horner(whole, x, r) for x in points]
        assert fflonk.host_values(cv, parts, points) == direct
        assert fflonk.parts_of(cv, direct, points) == parts                                               # and the way back
    assert fflonk.host_values(cv, [], [5]) == [0] and fflonk.host_values(cv, [7], [0, 5]) == [7, 7]


def test_refusals_before_any_device_work(zk, fflonk):
    r = ref.R["BN128"]
    n_vars, public, gates, wit = ref.chain(1, r)
    c = fflonk.Circuit(n_vars, public, gates)
    assert fflonk.required_powers(8) == 90 and fflonk.file_power(3) == 6
    small = types.SimpleNamespace(curve="BN128", max_coeffs=89)
    with pytest.raises(fflonk.ZkError, match=r"the file holds 89 G1 powers, n = 8 rows need 9n \+ 18 = 90 \(a file of power 6 has them\)"):
        fflonk.FflonkKey(small, c)
    with pytest.raises(fflonk.ZkError, match="the circuit is over BN128, the file over BLS12381"):
        fflonk.FflonkKey(types.SimpleNamespace(curve="BLS12381", max_coeffs=100), c)
    with pytest.raises(fflonk.ZkError, match="2-adicity"):
        fflonk.VerifyingKey("BN128", 27, 1, 2, 3, bytes(64))
    with pytest.raises(fflonk.ZkError, match='unknown curve "BN254"'):
        fflonk.VerifyingKey("BN254", 4, 1, 2, 3, bytes(64))
    with pytest.raises(fflonk.ZkError, match="not a verification key of this prover"):
        fflonk.vk_from_json('{"protocol": "plonk-shplonk"}')
    with pytest.raises(fflonk.ZkError, match="not a proof of this prover on BN128"):
        fflonk.proof_from_json('{"protocol": "fflonk-shplonk", "curve": "BLS12381"}', "BN128")
    with pytest.raises(fflonk.ZkError, match="a proof is 736 bytes, not 700"):
        fflonk.proof_from_bytes(bytes(700), 64)
    with pytest.raises(fflonk.ZkError, match="are no verification key"):
        fflonk.vk_from_bytes(b"BN128")
    # the verifier's refusals of a malformed proof, before any challenge is drawn
    vk = fflonk.VerifyingKey("BN128", 3, 1, 2, 3, bytes(64))
    proof = {"C1": bytes(64), "C2": bytes(64), "W1": bytes(64), "W2": bytes(64), "values": [0] * 15}
    with pytest.raises(fflonk.ZkError, match="the proof holds no C2, values"):
        fflonk.host_check(vk, [1], {"C1": bytes(64), "W1": bytes(64), "W2": bytes(64)})
    with pytest.raises(fflonk.ZkError, match="a proof holds 15 values, not 14"):
        fflonk.host_check(vk, [1], dict(proof, values=[0] * 14))
    with pytest.raises(fflonk.ZkError, match="point W1 of the proof is 63 bytes, not 64"):
        fflonk.host_check(vk, [1], dict(proof, W1=bytes(63)))
    with pytest.raises(fflonk.ZkError, match="2 public inputs, the verification key has 1"):
        fflonk.host_check(vk, [1, 2], proof)
    assert fflonk.host_check(vk, [r], proof) == (fflonk.INPUT_NOT_CANONICAL, None)
    assert fflonk.host_check(vk, [1], dict(proof, values=[0] * 14 + [r])) == (fflonk.INPUT_NOT_CANONICAL, None)
    with pytest.raises(fflonk.ZkError, match="verify needs the Kzg handle"):
        fflonk.verify(vk, [[1]], [proof])
    with pytest.raises(fflonk.ZkError, match="1 lists of public inputs for 2 proofs"):
        fflonk.verify(vk, [[1]], [proof, proof], kzg=types.SimpleNamespace(curve="BN128", point_bytes=64))
    with pytest.raises(fflonk.ZkError, match="the verification key is over BN128, the file over BLS12381"):
        fflonk.verify(vk, [[1]], [proof], kzg=types.SimpleNamespace(curve="BLS12381", point_bytes=96))
    # the prover's own: a witness of the wrong length, a value that is not below r, blinders -- before the key's device arrays are read
    key = types.SimpleNamespace(curve="BN128", n=c.n, log_n=c.log_n, circuit=c, kzg=None)
    with pytest.raises(fflonk.ZkError, match="the witness has %d values, the circuit has %d variables" % (n_vars - 1, n_vars)):
        fflonk.prove(key, wit[:-1])
    with pytest.raises(fflonk.ZkError, match="witness value 4 is not below the scalar field's modulus"):
        fflonk.prove(key, wit[:4] + [r] + wit[5:])
    with pytest.raises(fflonk.ZkError, match="blinding takes nine integers"):
        fflonk.prove(key, wit, blinding=[0] * 8)
    with pytest.raises(fflonk.ZkError, match="blinding takes nine integers"):
        fflonk.prove(key, wit, blinding=[0] * 8 + [r])
    # the quotients' wrapper and the library's refusals of a scalar and of the size, decided on the host
    with pytest.raises(fflonk.ZkError, match="the quotients take 15 columns, not 3"):
        fflonk.quotients([None] * 3, 3, 1, 2, 2, 3)
    lib = zk.lib()
    big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    ptrs = np.zeros(15, dtype=np.uint64)
    for at, name in enumerate(("beta", "gamma", "k1", "k2")):
        sc = [zk._ptr(big if j == at else one) for j in range(4)]
        assert lib.zk_fflonk_bn254_quotients_dev(zk._ptr(ptrs), 3, *sc, None, None, None, None) != 0
        assert "fflonk: %s is not below the scalar field's modulus" % name in lib.zk_last_error().decode()
    sc = [zk._ptr(one)] * 4
    assert lib.zk_fflonk_bn254_quotients_dev(zk._ptr(ptrs), 27, *sc, None, None, None, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
    assert lib.zk_fflonk_bls12_381_quotients_dev(zk._ptr(ptrs), 3, *sc, None, None, None, None) != 0 and "every output is null" in lib.zk_last_error().decode()
    assert lib.zk_fflonk_bls12_381_quotients_dev(None, 3, *sc, None, None, None, None) != 0 and "null argument" in lib.zk_last_error().decode()
