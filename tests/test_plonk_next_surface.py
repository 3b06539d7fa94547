"""The surface of the PLONK prover with a next-row term without a GPU: the header declares the entry points and the library
exports them, the package binds them, eigen_zkvm_amd.plonk_next has its functions and its docstring states the protocol, the command-line tool
parses its three commands, a circuit file round-trips with and without qN, and what is refused before any device work comes back with its
text -- a key or a proof of plonk.py here and this module's there among them."""
import importlib, json, pathlib, re, sys, types

import numpy as np
import pytest

import plonk_next_ref as nref
import plonk_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_plonk_%s_next_%s" % (c, f) for c in ("bn254", "bls12_381") for f in ("quotient_dev", "gate_check_dev", "r1cs_new", "r1cs_qn")]


@pytest.fixture(scope="module")
def pn(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_next")


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


def _circuit(r, m=3, twice=False):
    return nref.running_sums([(i + 2, 100 + i) for i in range(m)], r, twice=twice)


def test_header_declares_the_entry_points_and_states_the_rule():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    for macro, value in (("ZK_PLONK_NEXT_QUOTIENT_COLS", 16), ("ZK_PLONK_NEXT_GATE_COLS", 10), ("ZK_PLONK_QUOTIENT_COLS", 15), ("ZK_PLONK_GATE_COLS", 9)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    assert "chain(sig)" in text and "q_N = -1" in text and "CLOSED" in text
    assert not re.search(r"Not built:[^*]*\bcustom gates", text.replace("other custom gates", ""))       # struck from the lists of what is not built


def test_package_exports_and_binds_them(zk, pn):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    lib = zk.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("NextCircuit", "NextR1csCircuit", "NextKey", "setup", "prove", "verify", "vk_to_json", "vk_from_json", "proof_to_json", "proof_from_json", "vk_digest",
                 "transcript_start", "transcript_wires", "transcript_product", "transcript_quotient", "transcript_values", "transcript_z", "challenges",
                 "quotient", "gate_check", "host_check", "identity_holds", "required_powers"):
        assert callable(getattr(pn, name)), name
    assert zk.NextCircuit is pn.NextCircuit and zk.NextKey is pn.NextKey and zk.NextR1csCircuit is pn.NextR1csCircuit
    arith = importlib.import_module("eigen_zkvm_amd.plonk_arith")
    assert issubclass(pn.NextKey, arith.ArithKey) and issubclass(pn.NextCircuit, arith.Circuit) and issubclass(pn.NextR1csCircuit, arith.R1csCircuit)
    assert (pn.PROTOCOL, pn.N_VALUES, pn.N_FIXED) == ("plonk-shplonk-next", 16, 9)
    assert pn.VALUE_NAMES == arith.FIXED_NAMES + ("qN", "a", "b", "c", "t", "Z", "Zw", "cw") == nref.VALUE_NAMES
    assert pn.POINT_NAMES == ("A", "B", "C", "Z", "T", "W1", "W2")
    for text in ('"plonk-next-vk"', '"plonk-next-v1"', "q_N c(wX)", "3n + 7", "the 16 values", "b_10", "outside {zeta, zeta w}"):
        assert text in pn.__doc__, text
    text = (ROOT / "eigen-zkvm_amd" / "plonk_next.py").read_text()
    assert not re.search(r"^\s*(from\s+\.plonk\s+import|from\s+\.\s+import\s+plonk\b|import\s+\S*\.plonk\b)", text, flags=re.M)   # it stands on the layer alone


def test_required_powers():
    pn = importlib.import_module("eigen_zkvm_amd.plonk_next")
    arith = importlib.import_module("eigen_zkvm_amd.plonk_arith")
    for k in (3, 4, 10, 20):
        n = 1 << k
        assert pn.required_powers(n) == 3 * n + 7
        assert arith.smallest_power(pn.required_powers(n)) == k + 1 and (2 << (k + 2)) - 1 >= 3 * n + 7      # a file of power log n + 2 holds them
    assert arith.smallest_power(pn.required_powers(4)) == 4                           # below n = 8 one power more: n is never below 8


def test_cli_parses_its_three_commands():
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_plonk_next")
    ap = cli.build_parser()
    a = ap.parse_args(["plonk_next_setup", "-c", "BN128", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])
    assert (a.cmd, a.curve, a.ptau, a.circuit, a.r1cs, a.vk, a.no_check_srs) == ("plonk_next_setup", "BN128", "f.ptau", "c.npz", None, "vk.json", False)
    a = ap.parse_args(["plonk_next_setup", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "-v", "vk.json"])
    assert (a.r1cs, a.circuit) == ("c.r1cs", None)
    a = ap.parse_args(["plonk_next_prove", "-c", "BLS12381", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--proof", "proof.json", "--public", "public.json",
                       "--no-check-srs"])
    assert (a.cmd, a.curve, a.wtns, a.proof, a.public, a.no_check_srs) == ("plonk_next_prove", "BLS12381", "w.wtns", "proof.json", "public.json", True)
    a = ap.parse_args(["plonk_next_verify", "-v", "vk.json", "--ptau", "f.ptau", "p1.json:x1.json", "p2.json:x2.json"])
    assert (a.cmd, a.vk, a.pairs) == ("plonk_next_verify", "vk.json", ["p1.json:x1.json", "p2.json:x2.json"])
    assert cli.split_pair("p1.json:x1.json") == ("p1.json", "x1.json")
    with pytest.raises(SystemExit):
        cli.split_pair("p1.json")
    with pytest.raises(SystemExit):
        ap.parse_args(["plonk_next_setup", "--ptau", "f.ptau", "-v", "vk.json"])      # the circuit is required
    with pytest.raises(SystemExit):
        ap.parse_args(["plonk_setup", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])    # the other tool's command
    with pytest.raises(SystemExit):
        cli.main(["plonk_next_prove", "--ptau", "f.ptau", "--r1cs", "c.r1cs", "--witness", "w.bin", "--proof", "p.json", "--public", "x.json"])
    mod = importlib.import_module(cli.TOOL.module)
    assert (cli.TOOL.prefix, cli.TOOL.key, mod.CIRCUIT, mod.R1CS_CIRCUIT) == ("plonk_next", "NextKey", "NextCircuit", "NextR1csCircuit")
    assert "3n + 7 = 31 powers (a file of power 4 has them)" in cli._need("head", types.SimpleNamespace(log_n=3), 31, 4)[0] and cli._need(None, None, 31, 4) == []


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_a_circuit_file_round_trips_with_and_without_qN(pn, plonk, tmp_path, cv):
    r = ref.R[cv]
    n_vars, public, gates, wit = _circuit(r, 5, True)
    c = pn.NextCircuit(n_vars, public, gates, cv)
    t = nref.Table(cv, n_vars, public, gates)
    assert (c.n, c.n_public, c.n_gates) == (t.n, 1, len(gates["a"]))
    assert all([pn.pa.int_of(w) for w in c.sel[k]] == t.sel[k] for k in nref.SELECTORS) and all(c.wire[k].tolist() == t.wire[k] for k in "abc")
    c.save(tmp_path / "c.npz")
    with np.load(tmp_path / "c.npz") as z:
        assert z["qN"].shape == (c.n_gates, 4) and z["qN"].dtype == np.uint64
    d = pn.NextCircuit.load(tmp_path / "c.npz", cv)
    assert (d.n_vars, d.public, d.n) == (c.n_vars, c.public, c.n)
    assert all(np.array_equal(c.sel[k], d.sel[k]) for k in nref.SELECTORS) and all(np.array_equal(c.wire[k], d.wire[k]) for k in "abc")
    # without qN: plonk.Circuit's own file loads here with zeros, and is the same table
    n_vars, public, gates, wit = ref.chain(3, r)
    p = plonk.Circuit(n_vars, public, gates, cv)
    p.save(tmp_path / "p.npz")
    with np.load(tmp_path / "p.npz") as z:
        assert "qN" not in z
    e = pn.NextCircuit.load(tmp_path / "p.npz", cv)
    assert not e.sel["qN"].any() and e.sel["qN"].shape == (p.n, 4) and all(np.array_equal(p.sel[k], e.sel[k]) for k in ref.SELECTORS)
    assert not pn.NextCircuit(n_vars, public, gates, cv).gates["qN"].any()
    # the other way round the selector would be dropped: refused by name
    with pytest.raises(pn.ZkError, match="holds a next-row selector qN: it is a circuit of plonk_next.py"):
        plonk.Circuit.load(tmp_path / "c.npz", cv)
    np.savez(tmp_path / "short.npz", **{k: v for k, v in np.load(tmp_path / "c.npz").items() if k != "qO"})
    with pytest.raises(pn.ZkError, match="plonk next: .*short.npz holds no qO"):
        pn.NextCircuit.load(tmp_path / "short.npz", cv)


def test_refusals_before_any_device_work(zk, pn, plonk):
    r = ref.R["BN128"]
    n_vars, public, gates, wit = _circuit(r)
    c = pn.NextCircuit(n_vars, public, gates)
    assert (c.n, c.log_n, c.n_public, c.n_gates) == (8, 3, 1, 4)
    with pytest.raises(pn.ZkError, match="selector qN of gate 1 is not below the scalar field's modulus"):
        pn.NextCircuit(n_vars, public, dict(gates, qN=[0, r, 0, 0]))
    with pytest.raises(pn.ZkError, match="the selector and wire arrays of a circuit have one length"):
        pn.NextCircuit(n_vars, public, dict(gates, qN=[0, 0, 0]))
    with pytest.raises(pn.ZkError, match='unknown curve "BN254"'):
        pn.NextCircuit(n_vars, public, gates, "BN254")
    # a file with fewer than 3n + 7 powers: decided from the handle's count, before anything is built
    assert pn.required_powers(8) == 31
    with pytest.raises(pn.ZkError, match=r"plonk next: the file holds 30 G1 powers, n = 8 rows need 3n \+ 7 = 31 \(a file of power 4 has them\)"):
        pn.NextKey(types.SimpleNamespace(curve="BN128", max_coeffs=30), c)
    with pytest.raises(pn.ZkError, match="the circuit is over BN128, the file over BLS12381"):
        pn.NextKey(types.SimpleNamespace(curve="BLS12381", max_coeffs=100), c)
    with pytest.raises(pn.ZkError, match="plonk next: the key takes a Circuit"):
        pn.NextKey(types.SimpleNamespace(curve="BN128", max_coeffs=100), object())
    # plonk.py's key does not read qN: it refuses the circuit instead of proving another one
    with pytest.raises(pn.ZkError, match="plonk: the circuit has a next-row selector qN, which this prover does not read: prove it with plonk_next.py"):
        plonk.PlonkKey(types.SimpleNamespace(curve="BN128", max_coeffs=100), c)
    with pytest.raises(pn.ZkError, match="2-adicity"):
        pn.VerifyingKey("BN128", 27, 1, 2, 3, [bytes(64)] * 9)
    with pytest.raises(pn.ZkError, match="plonk next: a verification key holds 9 commitments, not 8"):
        pn.VerifyingKey("BN128", 3, 1, 2, 3, [bytes(64)] * 8)
    # the prover's own, before the key's device arrays are read
    key = types.SimpleNamespace(curve="BN128", n=c.n, log_n=c.log_n, circuit=c, kzg=None)
    with pytest.raises(pn.ZkError, match="plonk next: the witness has %d values, the circuit has %d variables" % (n_vars - 1, n_vars)):
        pn.prove(key, wit[:-1])
    with pytest.raises(pn.ZkError, match="witness value 2 is not below the scalar field's modulus"):
        pn.prove(key, wit[:2] + [r] + wit[3:])
    for bad in ([0] * 9, [0] * 11, [0] * 9 + [r]):
        with pytest.raises(pn.ZkError, match="plonk next: blinding takes ten integers"):
            pn.prove(key, wit, blinding=bad)
    # verify: what is decided before a handle is used
    vk = pn.VerifyingKey("BN128", 3, 1, 2, 3, [bytes(64)] * 9)
    with pytest.raises(pn.ZkError, match="plonk next: verify needs the Kzg handle"):
        pn.verify(vk, [[1]], [{}])
    with pytest.raises(pn.ZkError, match="plonk next: 2 lists of public inputs for 1 proofs"):
        pn.verify(vk, [[1], [2]], [{}], kzg=types.SimpleNamespace(curve="BN128", point_bytes=64))
    with pytest.raises(pn.ZkError, match="plonk next: the proof holds no A, B, C, Z, T, W1, W2, values"):
        pn.verify(vk, [[1]], [{}], kzg=types.SimpleNamespace(curve="BN128", point_bytes=64))
    with pytest.raises(pn.ZkError, match="plonk next: 2 public inputs, the verification key has 1"):
        pn.host_check(vk, [1, 2], dict({k: bytes(64) for k in pn.POINT_NAMES}, values=[0] * 16))
    # the library's refusals of a scalar and of a size, decided on the host
    lib = zk.lib()
    big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    ptrs = np.zeros(16, dtype=np.uint64)
    for at, name in enumerate(("alpha", "beta", "gamma", "k1", "k2")):
        sc = [zk._ptr(big if j == at else one) for j in range(5)]
        assert lib.zk_plonk_bn254_next_quotient_dev(zk._ptr(ptrs), 3, *sc, None, None) != 0
        assert "plonk next: %s is not below the scalar field's modulus" % name in lib.zk_last_error().decode()
    sc = [zk._ptr(one)] * 5
    assert lib.zk_plonk_bn254_next_quotient_dev(zk._ptr(ptrs), 27, *sc, None, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bls12_381_next_quotient_dev(zk._ptr(ptrs), 3, *sc, None, None) != 0 and "plonk next: null argument" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_next_gate_check_dev(zk._ptr(ptrs), 8, None, None, None) != 0 and "plonk next: null argument" in lib.zk_last_error().decode()


def test_the_two_provers_refuse_each_others_keys_and_proofs(pn, plonk):
    cv = "BN128"
    point = bytes(63) + b"\x00"
    mine = pn.VerifyingKey(cv, 3, 1, 2, 3, [point] * 9)
    theirs = plonk.VerifyingKey(cv, 3, 1, 2, 3, [point] * 8)
    with pytest.raises(pn.ZkError, match='^plonk next: not a verification key of this prover \\(protocol "plonk-shplonk"\\)$'):
        pn.vk_from_json(plonk.vk_to_json(theirs))
    with pytest.raises(pn.ZkError, match='^plonk: not a verification key of this prover \\(protocol "plonk-shplonk-next"\\)$'):
        plonk.vk_from_json(pn.vk_to_json(mine))
    back = pn.vk_from_json(pn.vk_to_json(mine))
    assert (back.digest, back.commitments) == (mine.digest, mine.commitments) and sorted(json.loads(pn.vk_to_json(mine))["commitments"]) == sorted(pn.NEXT_FIXED_NAMES)
    p16 = dict({k: point for k in pn.POINT_NAMES}, values=list(range(16)))
    p14 = dict(p16, values=list(range(14)))
    with pytest.raises(pn.ZkError, match='^plonk next: not a proof of this prover on BN128 \\(protocol "plonk-shplonk"'):
        pn.proof_from_json(plonk.proof_to_json(p14, cv), cv)
    with pytest.raises(pn.ZkError, match='^plonk: not a proof of this prover on BN128 \\(protocol "plonk-shplonk-next"'):
        plonk.proof_from_json(pn.proof_to_json(p16, cv), cv)
    with pytest.raises(pn.ZkError, match="not a proof of this prover on BLS12381"):
        pn.proof_from_json(pn.proof_to_json(p16, cv), "BLS12381")
    assert pn.proof_from_json(pn.proof_to_json(p16, cv), cv) == p16
    # the binary forms differ in length, and a proof of the other prover that reaches the verifier is an error, not a verdict
    with pytest.raises(pn.ZkError, match="plonk next: a proof is 960 bytes, not 896"):
        pn.proof_from_bytes(plonk.proof_to_bytes(p14), 64)
    with pytest.raises(pn.ZkError, match="plonk: a proof is 896 bytes, not 960"):
        plonk.proof_from_bytes(pn.proof_to_bytes(p16), 64)
    with pytest.raises(pn.ZkError, match="plonk next: a proof holds 16 values, not 14"):
        pn.host_check(mine, [1], p14)
    with pytest.raises(pn.ZkError, match="plonk: a proof holds 14 values, not 16"):
        plonk.host_check(theirs, [1], p16)
