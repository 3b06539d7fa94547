"""The surface of fflonk with lookups without a GPU: the header declares the entry points and the macro and the library exports them, the
package binds them, eigen_zkvm_amd.fflonk_lookup has its functions and pulls in nothing from plonk.py, the powers a file must hold and the
file power the refusal names, the command-line tool parses its three commands and refuses --r1cs with one line, and every host-side refusal
comes back with its text."""
import importlib, pathlib, re, subprocess, sys, types

import numpy as np
import pytest

import plonk_lookup_ref as lref
import plonk_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_fflonk_%s_lookup_quotients_dev" % c for c in ("bn254", "bls12_381")]


@pytest.fixture(scope="module")
def fl(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk_lookup")


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ZK_FFLONK_LOOKUP_QUOTIENT_COLS\s+21\b", code)
    flat = " ".join(text.split())
    assert "csrc/fflonk_lookup_impl.hip.h; DESIGN.md 3.25" in flat and "eigen_zkvm_amd/fflonk_lookup.py" in flat
    # the two sentences other tests pin stay as they are: they are true of plonk_lookup.py; the fflonk form is named in the new block
    assert "Not built: tables of more or fewer than three columns, several tables in one circuit, lookups under fflonk" in flat
    assert "custom gates, lookups," not in flat


def test_package_exports_and_binds_them(zk, fl):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    lib = zk.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == 13, name
    for name in ("LookupCircuit", "LookupTable", "FflonkLookupKey", "VerifyingKey", "range_table", "xor_table", "setup", "prove", "verify", "challenges", "host_check", "roots",
                 "quotients", "quotients_at", "opened_values", "values_of", "lookup_sum", "vk_to_json", "vk_from_json", "proof_to_json", "proof_from_json", "proof_to_bytes",
                 "proof_from_bytes", "vk_digest", "transcript_start", "transcript_round1", "transcript_round2", "transcript_values", "transcript_z", "required_powers", "file_power"):
        assert callable(getattr(fl, name)), name
    assert zk.FflonkLookupKey is fl.FflonkLookupKey
    pl = importlib.import_module("eigen_zkvm_amd.plonk_lookup")
    assert fl.LookupCircuit is pl.LookupCircuit and fl.FIXED == pl.FIXED and fl.CIRCUIT == pl.CIRCUIT == "LookupCircuit"
    assert (fl.PROTOCOL, fl.N_VALUES, fl.N_OPENED, len(fl.POINT_NAMES), len(fl.VALUE_NAMES), fl.QUOTIENT_COLS) == ("fflonk-shplonk-lookup", 22, 26, 5, 22, 21)
    for fn in (fl.vk_digest, fl.transcript_start, fl.transcript_round1, fl.transcript_round2, fl.transcript_values, fl.transcript_z):
        assert "H(" in fn.__doc__, fn.__name__
    assert '"fflonkl-vk"' in fl.__doc__ and '"fflonkl-v1"' in fl.__doc__
    assert "lookups under fflonk" in pl.__doc__.replace("\n", " ")                          # still true of that module, word for word


def test_it_is_a_fourth_protocol_and_pulls_in_nothing_from_plonk_py(zk, fl):
    arith = importlib.import_module("eigen_zkvm_amd.plonk_arith")
    assert issubclass(fl.FflonkLookupKey, arith.ArithKey) and fl.ZkError is arith.ZkError and not fl.FflonkLookupKey.KEEPS_COEF
    text = (ROOT / "eigen-zkvm_amd" / "fflonk_lookup.py").read_text()
    assert not re.search(r"^\s*(from\s+\.plonk\s+import|from\s+\.\s+import\s+plonk\b(?!_)|import\s+\S*\.plonk\b(?!_))", text, flags=re.M)
    assert not any("eigen_zkvm_amd.plonk" in (getattr(v, "__module__", None), isinstance(v, types.ModuleType) and v.__name__) for v in vars(fl).values())
    # a fresh interpreter that imports the module has not loaded plonk.py
    code = ("import sys; sys.path.insert(0, %r); import eigen_zkvm_amd.fflonk_lookup as m; "
            "assert 'eigen_zkvm_amd.plonk' not in sys.modules and 'eigen_zkvm_amd.plonk_lookup' in sys.modules and 'eigen_zkvm_amd.fflonk' in sys.modules; print(m.PROTOCOL)" % str(ROOT))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "fflonk-shplonk-lookup", out.stderr
    others = [importlib.import_module("eigen_zkvm_amd." + m).PROTOCOL for m in ("plonk", "fflonk", "plonk_lookup")]
    assert fl.PROTOCOL not in others and len(set(others)) == 3


def test_the_powers_a_file_must_hold(fl):
    fflonk = importlib.import_module("eigen_zkvm_amd.fflonk")
    for log_n in (3, 20):
        n = 1 << log_n
        assert fl.required_powers(n) == 8 * n + 8
        assert fl.file_power(log_n) == log_n + 3 == fflonk.file_power(log_n)
        assert (2 << (log_n + 3)) - 1 >= 8 * n + 8 > (2 << (log_n + 2)) - 1
        n0, n1, n2, n3 = fl.quotient_coeffs(n)
        assert (n0, n1, n2, n3) == (2 * n + 2, n + 2, 3 * n + 6, 2 * n + 3)
        assert 4 * max(n + 3, n0, n1) == 8 * n + 8 and 2 * max(n2, n3) == 6 * n + 12 <= 8 * n + 8 and 4 * (n + 2) <= 8 * n + 8

        circuit = object.__new__(fl.LookupCircuit)
        circuit.curve, circuit.n, circuit.log_n = "BN128", n, log_n
        with pytest.raises(fl.ZkError, match=r"^fflonk lookup: the file holds %d G1 powers, n = %d rows need 8n \+ 8 = %d \(a file of power %d has them\)$" % (8 * n + 7, n, 8 * n + 8, log_n + 3)):
            fl.FflonkLookupKey(types.SimpleNamespace(curve="BN128", max_coeffs=8 * n + 7), circuit)


def test_cli_parses_its_three_commands_and_refuses_an_r1cs(capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_fflonk_lookup")
    assert (cli.TOOL.prefix, cli.TOOL.module, cli.TOOL.key) == ("fflonk_lookup", "eigen_zkvm_amd.fflonk_lookup", "FflonkLookupKey")
    ap = cli.build_parser()
    a = ap.parse_args(["fflonk_lookup_setup", "-c", "BN128", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])
    assert (a.cmd, a.curve, a.ptau, a.circuit, a.vk, a.no_check_srs) == ("fflonk_lookup_setup", "BN128", "f.ptau", "c.npz", "vk.json", False)
    a = ap.parse_args(["fflonk_lookup_prove", "--ptau", "f.ptau", "--circuit", "c.npz", "--witness", "w.bin", "--proof", "proof.json", "--public", "public.json", "--no-check-srs"])
    assert (a.cmd, a.witness, a.proof, a.public, a.no_check_srs) == ("fflonk_lookup_prove", "w.bin", "proof.json", "public.json", True)
    a = ap.parse_args(["fflonk_lookup_verify", "-v", "vk.json", "--ptau", "f.ptau", "p1.json:x1.json", "p2.json:x2.json"])
    assert (a.cmd, a.vk, a.pairs) == ("fflonk_lookup_verify", "vk.json", ["p1.json:x1.json", "p2.json:x2.json"])
    assert cli.split_pair("p1.json:x1.json") == ("p1.json", "x1.json")
    with pytest.raises(SystemExit):
        ap.parse_args(["fflonk_lookup_setup", "--ptau", "f.ptau", "-v", "vk.json"])
    for argv in (["fflonk_lookup_setup", "--ptau", "no-such.ptau", "--r1cs", "c.r1cs", "-v", "vk.json"],
                 ["fflonk_lookup_prove", "--ptau", "no-such.ptau", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--proof", "p.json", "--public", "x.json"]):
        with pytest.raises(SystemExit) as e:                                               # before any file is opened
            cli.main(argv)
        out = capsys.readouterr().out
        assert e.value.code == 1 and out.count("\n") == 1 and "takes no --r1cs" in out and argv[0] in out and out.startswith("zkgpu_fflonk_lookup: ")
    # what setup prints about the file: n, the 8n + 8 powers and the smallest file power
    key = types.SimpleNamespace(log_n=4, n=16, circuit=types.SimpleNamespace(n_table=5, gates={"qK": np.array([[1, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]], dtype=np.uint64)}))
    assert cli._need(None, key, 136, 7) == ["fflonk_lookup_setup: n = 2^4 = 16 rows need 8n + 8 = 136 powers (a file of power 7 has them)",
                                            "fflonk_lookup_setup: a table of 5 rows, 2 of the gates look a row up"]


def test_refusals_before_any_device_work(zk, fl):
    cv = "BN128"
    r = ref.R[cv]
    n_vars, public, gates, table, wit = lref.lookup_chain(0, r)
    c = fl.LookupCircuit(n_vars, public, gates, table)
    # the key: an R1CS circuit has no lookups; a plain gate table is not enough
    fake = object.__new__(fl.R1csCircuit)
    fake._h = None
    with pytest.raises(fl.ZkError, match="^fflonk lookup: an R1csCircuit has no lookups: prove it with fflonk.py$"):
        fl.FflonkLookupKey(types.SimpleNamespace(curve=cv, max_coeffs=100), fake)
    with pytest.raises(fl.ZkError, match="the key takes a LookupCircuit"):
        fl.FflonkLookupKey(types.SimpleNamespace(curve=cv, max_coeffs=100), importlib.import_module("eigen_zkvm_amd.plonk_arith").Circuit(n_vars, public, gates))
    with pytest.raises(fl.ZkError, match="the circuit is over BN128, the file over BLS12381"):
        fl.FflonkLookupKey(types.SimpleNamespace(curve="BLS12381", max_coeffs=100), c)
    with pytest.raises(fl.ZkError, match=r"fflonk lookup: the file holds 71 G1 powers, n = 8 rows need 8n \+ 8 = 72 \(a file of power 6 has them\)"):
        fl.FflonkLookupKey(types.SimpleNamespace(curve=cv, max_coeffs=71), c)
    # the prover's own, before the key's device arrays are read
    key = types.SimpleNamespace(curve=cv, n=c.n, log_n=c.log_n, circuit=c, kzg=None)
    for bad in ([0] * 9, [0] * 13, [0] * 15, [0] * 13 + [r]):
        with pytest.raises(fl.ZkError, match="fflonk lookup: blinding takes fourteen integers"):
            fl.prove(key, wit, blinding=bad)
    with pytest.raises(fl.ZkError, match="fflonk lookup: the witness has %d values, the circuit has %d variables" % (n_vars - 1, n_vars)):
        fl.prove(key, wit[:-1])
    # keys
    pt = bytes(64)
    with pytest.raises(fl.ZkError, match="a circuit has at least 8"):
        fl.VerifyingKey(cv, 2, 1, 2, 3, pt, pt)
    with pytest.raises(fl.ZkError):
        fl.VerifyingKey(cv, 27, 1, 2, 3, pt, pt)                                             # k + 2 beyond the 2-adicity
    with pytest.raises(fl.ZkError, match="the two points of a verification key have one length"):
        fl.VerifyingKey(cv, 3, 1, 2, 3, pt, pt[:-1])
    vk = fl.VerifyingKey(cv, 3, 1, 2, 3, pt, pt)
    for other in ("plonk-shplonk", "fflonk-shplonk", "plonk-shplonk-lookup"):
        with pytest.raises(fl.ZkError, match='fflonk lookup: not a verification key of this prover \\(protocol "%s"\\)' % other):
            fl.vk_from_json('{"protocol": "%s", "curve": "BN128"}' % other)
        with pytest.raises(fl.ZkError, match='fflonk lookup: not a proof of this prover on BN128 \\(protocol "%s"' % other):
            fl.proof_from_json('{"protocol": "%s", "curve": "BN128"}' % other, cv)
    # proofs: what is missing or of the wrong length is an error, before any challenge is drawn
    proof = {"C1": pt, "C2": pt, "C3": pt, "W1": pt, "W2": pt, "values": [0] * 22}
    with pytest.raises(fl.ZkError, match="fflonk lookup: the proof holds no C3"):
        fl.host_check(vk, [1], {k: v for k, v in proof.items() if k != "C3"})
    with pytest.raises(fl.ZkError, match="fflonk lookup: a proof holds 22 values, not 15"):
        fl.host_check(vk, [1], dict(proof, values=[0] * 15))
    with pytest.raises(fl.ZkError, match="point C2 of the proof is 63 bytes, not 64"):
        fl.host_check(vk, [1], dict(proof, C2=pt[:-1]))
    with pytest.raises(fl.ZkError, match="2 public inputs, the verification key has 1"):
        fl.host_check(vk, [1, 2], proof)
    assert fl.host_check(vk, [1], dict(proof, values=[0] * 21 + [r]))[0] == fl.INPUT_NOT_CANONICAL
    assert fl.host_check(vk, [r], proof)[0] == fl.INPUT_NOT_CANONICAL
    with pytest.raises(fl.ZkError, match="a proof is %d bytes, not %d" % (5 * 64 + 22 * 32, 5 * 64 + 21 * 32)):
        fl.proof_from_bytes(bytes(5 * 64 + 21 * 32), 64)
    with pytest.raises(fl.ZkError, match="verify needs the Kzg handle"):
        fl.verify(vk, [[1]], [proof])
    # the device call's wrapper
    with pytest.raises(fl.ZkError, match="the quotients take 21 columns, not 15"):
        fl.quotients([None] * 15, 3, 1, 1, 2, 3, 1, 1)
    with pytest.raises(fl.ZkError, match="eta is not below"):
        fl.quotients([None] * 21, 3, 1, 1, 2, 3, r, 1)
    # the library's refusals, decided on the host before any device work
    lib = zk.lib()
    big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    ptrs = np.zeros(21, dtype=np.uint64)
    none = [None] * 5                                                                       # the four outputs and the stream
    for at, name in enumerate(("beta", "gamma", "k1", "k2", "eta", "delta")):                # BN254's r stands for a scalar that is not below it
        sc = [zk._ptr(big if j == at else one) for j in range(6)]
        assert lib.zk_fflonk_bn254_lookup_quotients_dev(zk._ptr(ptrs), 3, *sc, *none) != 0
        assert "fflonk lookup: %s is not below the scalar field's modulus" % name in lib.zk_last_error().decode()
    for fn in (lib.zk_fflonk_bn254_lookup_quotients_dev, lib.zk_fflonk_bls12_381_lookup_quotients_dev):
        assert fn(zk._ptr(ptrs), 3, *[zk._ptr(one)] * 6, *none) != 0 and "every output is null" in lib.zk_last_error().decode()
        assert fn(None, 3, *[zk._ptr(one)] * 6, *none) != 0 and "null argument" in lib.zk_last_error().decode()
        assert fn(zk._ptr(ptrs), 3, *[zk._ptr(one)] * 5, None, *none) != 0 and "null delta" in lib.zk_last_error().decode()
    assert lib.zk_fflonk_bn254_lookup_quotients_dev(zk._ptr(ptrs), 27, *[zk._ptr(one)] * 6, None, None, None, None, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
    assert lib.zk_fflonk_bls12_381_lookup_quotients_dev(zk._ptr(ptrs), 31, *[zk._ptr(one)] * 6, None, None, None, None, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
