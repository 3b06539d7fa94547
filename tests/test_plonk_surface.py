"""The surface of the PLONK layer without a GPU: the header declares the entry points and the library exports them, the package binds them,
eigen_zkvm_amd.plonk has its functions, the command-line tool parses its three commands, and what is refused before any device work comes
back with its text: a scalar that is not below r, a witness of the wrong length, a variable id beyond n_vars, a file with fewer than 3n + 6
powers, n above the field's 2-adicity less 2.  k_1 and k_2 are compared with their definition."""
import importlib, pathlib, re, sys, types

import numpy as np
import pytest

import plonk_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = [n % c for c in ("bn254", "bls12_381") for n in ("zk_plonk_%s_quotient_dev", "zk_plonk_%s_gate_check_dev", "zk_fr_%s_gather_dev")]


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    for macro, value in (("ZK_PLONK_QUOTIENT_COLS", 15), ("ZK_PLONK_GATE_COLS", 9)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro


def test_package_exports_and_binds_them(zk, plonk):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    lib = zk.lib()                                      # dlopen + every signature: no device is touched
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("Circuit", "PlonkKey", "setup", "prove", "verify", "vk_to_json", "vk_from_json", "proof_to_json", "proof_from_json", "vk_digest",
                 "transcript_start", "transcript_wires", "transcript_product", "transcript_quotient", "transcript_values", "transcript_z", "challenges",
                 "gather", "gather_dev", "quotient", "gate_check"):
        assert callable(getattr(plonk, name)), name
    assert zk.Circuit is plonk.Circuit and zk.PlonkKey is plonk.PlonkKey
    for fn in (plonk.vk_digest, plonk.transcript_start, plonk.transcript_wires, plonk.transcript_product, plonk.transcript_quotient, plonk.transcript_values,
               plonk.transcript_z):
        assert "H(" in fn.__doc__, fn.__name__           # the hashed bytes are stated where the function is


def test_the_layers_names_are_one_object_through_the_three_modules(zk, plonk):
    arith, fflonk = importlib.import_module("eigen_zkvm_amd.plonk_arith"), importlib.import_module("eigen_zkvm_amd.fflonk")
    for name in ("Circuit", "R1csCircuit", "ACCEPTED", "ZkError", "gather", "omega"):     # isinstance(c, R1csCircuit) decides the witness path
        assert getattr(plonk, name) is getattr(fflonk, name) is getattr(arith, name), name
    assert issubclass(plonk.PlonkKey, arith.ArithKey) and issubclass(fflonk.FflonkKey, arith.ArithKey)
    text = (ROOT / "eigen-zkvm_amd" / "fflonk.py").read_text()
    assert not re.search(r"^\s*(from\s+\.plonk\s+import|from\s+\.\s+import\s+plonk\b|import\s+\S*\.plonk\b)", text, flags=re.M)   # fflonk stands on the layer alone
    assert not any(plonk.__name__ in (getattr(v, "__module__", None), isinstance(v, types.ModuleType) and v.__name__) for v in vars(fflonk).values())


def test_cli_parses_its_three_commands():
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_plonk")
    ap = cli.build_parser()
    a = ap.parse_args(["plonk_setup", "-c", "BN128", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])
    assert (a.cmd, a.curve, a.ptau, a.circuit, a.vk, a.no_check_srs) == ("plonk_setup", "BN128", "f.ptau", "c.npz", "vk.json", False)
    a = ap.parse_args(["plonk_prove", "-c", "BLS12381", "--ptau", "f.ptau", "--circuit", "c.npz", "--witness", "w.bin", "--proof", "proof.json", "--public", "public.json",
                       "--no-check-srs"])
    assert (a.cmd, a.curve, a.witness, a.proof, a.public, a.no_check_srs) == ("plonk_prove", "BLS12381", "w.bin", "proof.json", "public.json", True)
    a = ap.parse_args(["plonk_verify", "-v", "vk.json", "--ptau", "f.ptau", "p1.json:x1.json", "p2.json:x2.json"])
    assert (a.cmd, a.vk, a.pairs) == ("plonk_verify", "vk.json", ["p1.json:x1.json", "p2.json:x2.json"])
    assert cli.split_pair("p1.json:x1.json") == ("p1.json", "x1.json")
    with pytest.raises(SystemExit):
        cli.split_pair("p1.json")
    with pytest.raises(SystemExit):
        ap.parse_args(["plonk_setup", "--ptau", "f.ptau", "-v", "vk.json"])          # the circuit is required


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
@pytest.mark.parametrize("log_n", (3, 20))
def test_k1_and_k2_are_what_their_definition_says(plonk, cv, log_n):
    r, n = ref.R[cv], 1 << log_n
    k1, k2 = plonk.coset_ks(cv, log_n)
    assert (k1, k2) == ref.ks_by_definition(cv, n)
    assert 2 <= k1 < k2 and pow(k1, n, r) != 1 and pow(k2, n, r) != 1 and pow(k2 * pow(k1, -1, r), n, r) != 1
    assert all(pow(k, n, r) == 1 for k in range(2, k1))                                # nothing smaller would do
    assert all(pow(k, n, r) == 1 or pow(k * pow(k1, -1, r), n, r) == 1 for k in range(k1 + 1, k2))
    w = plonk.omega(cv, log_n)
    assert w == ref.omega(cv, log_n) and pow(w, n, r) == 1 and pow(w, n // 2, r) == r - 1


def _gates(r, **over):
    n_vars, public, gates, wit = ref.chain(1, r)
    gates = {k: list(v) for k, v in gates.items()}
    for k, (i, v) in over.items():
        gates[k][i] = v
    return n_vars, public, gates, wit


def test_refusals_before_any_device_work(zk, plonk):
    r = ref.R["BN128"]
    n_vars, public, gates, wit = _gates(r)
    c = plonk.Circuit(n_vars, public, gates)
    assert (c.n, c.log_n, c.n_public, c.n_gates) == (8, 3, 1, 6)
    t = ref.Table("BN128", n_vars, public, gates)
    assert all([plonk.int_of(w) for w in c.sel[k]] == t.sel[k] for k in ref.SELECTORS) and all(c.wire[k].tolist() == t.wire[k] for k in "abc")
    with pytest.raises(plonk.ZkError, match="selector qM of gate 2 is not below the scalar field's modulus"):
        plonk.Circuit(*_gates(r, qM=(2, r))[:3])
    with pytest.raises(plonk.ZkError, match="wire b of gate 3 is variable %d, the circuit has %d variables" % (n_vars, n_vars)):
        plonk.Circuit(*_gates(r, b=(3, n_vars))[:3])
    with pytest.raises(plonk.ZkError, match="public input 0 is variable 99"):
        plonk.Circuit(n_vars, [99], gates)
    with pytest.raises(plonk.ZkError, match='unknown curve "BN254"'):
        plonk.Circuit(n_vars, public, gates, "BN254")
    # a file with fewer than 3n + 6 powers: decided from the handle's count, before anything is built
    assert plonk.required_powers(8) == 30
    small = types.SimpleNamespace(curve="BN128", max_coeffs=29)
    with pytest.raises(plonk.ZkError, match=r"the file holds 29 G1 powers, n = 8 rows need 3n \+ 6 = 30"):
        plonk.PlonkKey(small, c)
    with pytest.raises(plonk.ZkError, match="the circuit is over BN128, the file over BLS12381"):
        plonk.PlonkKey(types.SimpleNamespace(curve="BLS12381", max_coeffs=100), c)
    # n above the 2-adicity less 2
    for cv, s in (("BN128", 28), ("BLS12381", 32)):
        plonk.check_size(cv, s - 2)
        with pytest.raises(plonk.ZkError, match="the field's 2-adicity is %d" % s):
            plonk.check_size(cv, s - 1)
    with pytest.raises(plonk.ZkError, match="2-adicity"):
        plonk.VerifyingKey("BN128", 27, 1, 2, 3, [bytes(64)] * 8)
    # the prover's own: a witness of the wrong length, a value that is not below r -- both before the key's device arrays are read
    key = types.SimpleNamespace(curve="BN128", n=c.n, log_n=c.log_n, circuit=c, kzg=None)
    with pytest.raises(plonk.ZkError, match="the witness has %d values, the circuit has %d variables" % (n_vars - 1, n_vars)):
        plonk.prove(key, wit[:-1])
    with pytest.raises(plonk.ZkError, match="witness value 4 is not below the scalar field's modulus"):
        plonk.prove(key, wit[:4] + [r] + wit[5:])
    with pytest.raises(plonk.ZkError, match="witness value 1 is not below"):
        plonk.prove(key, b"".join(v.to_bytes(32, "little") for v in [1, r + 1] + wit[2:]))
    with pytest.raises(plonk.ZkError, match="blinding takes nine integers"):
        plonk.prove(key, wit, blinding=[0] * 8)
    # the library's refusals of a scalar, decided on the host
    lib = zk.lib()
    big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    ptrs = np.zeros(15, dtype=np.uint64)
    for at, name in enumerate(("alpha", "beta", "gamma", "k1", "k2")):
        sc = [zk._ptr(big if j == at else one) for j in range(5)]
        assert lib.zk_plonk_bn254_quotient_dev(zk._ptr(ptrs), 3, *sc, None, None) != 0
        assert "plonk: %s is not below the scalar field's modulus" % name in lib.zk_last_error().decode()
    sc = [zk._ptr(one)] * 5
    assert lib.zk_plonk_bn254_quotient_dev(zk._ptr(ptrs), 27, *sc, None, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bls12_381_quotient_dev(zk._ptr(ptrs), 3, zk._ptr(big), *sc[1:], None, None) != 0 and "null argument" in lib.zk_last_error().decode()


def test_sigma_is_the_permutation_the_reference_walks(plonk):
    r = ref.R["BN128"]
    n_vars, public, gates, wit = ref.chain(3, r)
    c = plonk.Circuit(n_vars, public, gates)
    t = ref.Table("BN128", n_vars, public, gates)
    sig = c.sigma()
    assert sorted(sig.tolist()) == list(range(3 * c.n))
    want = t.sigma_labels()
    assert [[t.label(int(sig[j * c.n + i])) for i in range(c.n)] for j in range(3)] == want


def test_a_circuit_file_round_trips(plonk, tmp_path):
    r = ref.R["BLS12381"]
    n_vars, public, gates, wit = ref.chain(3, r)
    c = plonk.Circuit(n_vars, public, gates, "BLS12381")
    c.save(tmp_path / "c.npz")
    d = plonk.Circuit.load(tmp_path / "c.npz", "BLS12381")
    assert (d.n_vars, d.public, d.n) == (c.n_vars, c.public, c.n)
    assert all(np.array_equal(c.sel[k], d.sel[k]) for k in ref.SELECTORS) and all(np.array_equal(c.wire[k], d.wire[k]) for k in "abc")
    with np.load(tmp_path / "c.npz") as z:
        assert z["qL"].shape == (c.n_gates, 4) and z["qL"].dtype == np.uint64 and z["a"].dtype == np.uint32
