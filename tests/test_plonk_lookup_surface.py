"""The surface of PLONK's lookup argument without a GPU: the header declares the entry points and the library exports them, the package binds
them, eigen_zkvm_amd.plonk_lookup has its functions and imports nothing from plonk.py or fflonk.py, the command-line tool parses its three
commands and refuses --r1cs, every host-side refusal comes back with its text, a circuit file round-trips, and the table is padded by
repeating its last row."""
import importlib, pathlib, re, sys, types

import numpy as np
import pytest

import plonk_lookup_ref as lref
import plonk_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_fr_%s_prefix_sum_dev" % c for c in ("bn254", "bls12_381")] + [
    "zk_plonk_%s_lookup_%s" % (c, f) for c in ("bn254", "bls12_381") for f in ("table_new", "table_free", "count_dev", "terms_dev", "summands_dev", "quotient_dev")]


@pytest.fixture(scope="module")
def pl(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_lookup")


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    for macro, value in (("ZK_PLONK_LOOKUP_TERMS_COLS", 6), ("ZK_PLONK_LOOKUP_QUOTIENT_COLS", 9), ("ZK_PLONK_LOOKUP_MAX_ROWS", 1 << 30)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    flat = " ".join(text.split())
    assert "Not built: tables of more or fewer than three columns, several tables in one circuit, lookups under fflonk" in flat
    assert "custom gates, lookups," not in flat                                            # the PLONK section no longer lists lookups as missing


def test_package_exports_and_binds_them(zk, pl):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    lib = zk.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("LookupCircuit", "LookupKey", "LookupTable", "range_table", "xor_table", "setup", "prove", "verify", "challenges", "identity_holds", "host_check", "vk_to_json",
                 "vk_from_json", "proof_to_json", "proof_from_json", "proof_to_bytes", "proof_from_bytes", "vk_digest", "transcript_start", "transcript_wires", "transcript_sums",
                 "transcript_quotient", "transcript_values", "transcript_z", "count", "terms", "summands", "lookup_quotient"):
        assert callable(getattr(pl, name)), name
    assert callable(importlib.import_module("eigen_zkvm_amd.frpoly").prefix_sum)
    assert zk.LookupCircuit is pl.LookupCircuit and zk.LookupKey is pl.LookupKey
    assert (pl.PROTOCOL, pl.N_VALUES, len(pl.POINT_NAMES), len(pl.FIXED), pl.MAX_TABLE_ROWS) == ("plonk-shplonk-lookup", 21, 9, 12, 1 << 30)
    for fn in (pl.vk_digest, pl.transcript_start, pl.transcript_wires, pl.transcript_sums, pl.transcript_quotient, pl.transcript_values, pl.transcript_z):
        assert "H(" in fn.__doc__, fn.__name__
    assert '"plonkl-vk"' in pl.__doc__ and '"plonkl-v1"' in pl.__doc__ and "lookups under fflonk" in pl.__doc__.replace("\n", " ")


def test_it_is_a_third_protocol_on_the_layer_alone(zk, pl):
    arith, plonk = importlib.import_module("eigen_zkvm_amd.plonk_arith"), importlib.import_module("eigen_zkvm_amd.plonk")
    assert issubclass(pl.LookupKey, arith.ArithKey) and issubclass(pl.LookupCircuit, arith.Circuit) and pl.ZkError is arith.ZkError
    text = (ROOT / "eigen-zkvm_amd" / "plonk_lookup.py").read_text()
    assert not re.search(r"^\s*(from\s+\.(plonk|fflonk)\s+import|from\s+\.\s+import\s+(plonk|fflonk)\b|import\s+\S*\.(plonk|fflonk)\b)", text, flags=re.M)
    for other in (plonk.__name__, importlib.import_module("eigen_zkvm_amd.fflonk").__name__):
        assert not any(other in (getattr(v, "__module__", None), isinstance(v, types.ModuleType) and v.__name__) for v in vars(pl).values()), other
    assert pl.PROTOCOL != plonk.PROTOCOL


def test_cli_parses_its_three_commands_and_refuses_an_r1cs(capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_plonk_lookup")
    assert (cli.TOOL.prefix, cli.TOOL.module, cli.TOOL.key) == ("plonk_lookup", "eigen_zkvm_amd.plonk_lookup", "LookupKey")
    ap = cli.build_parser()
    a = ap.parse_args(["plonk_lookup_setup", "-c", "BN128", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])
    assert (a.cmd, a.curve, a.ptau, a.circuit, a.vk, a.no_check_srs) == ("plonk_lookup_setup", "BN128", "f.ptau", "c.npz", "vk.json", False)
    a = ap.parse_args(["plonk_lookup_prove", "--ptau", "f.ptau", "--circuit", "c.npz", "--witness", "w.bin", "--proof", "proof.json", "--public", "public.json", "--no-check-srs"])
    assert (a.cmd, a.witness, a.proof, a.public, a.no_check_srs) == ("plonk_lookup_prove", "w.bin", "proof.json", "public.json", True)
    a = ap.parse_args(["plonk_lookup_verify", "-v", "vk.json", "--ptau", "f.ptau", "p1.json:x1.json", "p2.json:x2.json"])
    assert (a.cmd, a.vk, a.pairs) == ("plonk_lookup_verify", "vk.json", ["p1.json:x1.json", "p2.json:x2.json"])
    assert cli.split_pair("p1.json:x1.json") == ("p1.json", "x1.json")
    with pytest.raises(SystemExit):
        ap.parse_args(["plonk_lookup_setup", "--ptau", "f.ptau", "-v", "vk.json"])
    for argv in (["plonk_lookup_setup", "--ptau", "no-such.ptau", "--r1cs", "c.r1cs", "-v", "vk.json"],
                 ["plonk_lookup_prove", "--ptau", "no-such.ptau", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--proof", "p.json", "--public", "x.json"]):
        with pytest.raises(SystemExit) as e:                                               # before any file is opened
            cli.main(argv)
        out = capsys.readouterr().out
        assert e.value.code == 1 and out.count("\n") == 1 and "takes no --r1cs" in out and argv[0] in out


def _circuit(r, bits=1, **over):
    n_vars, public, gates, table, wit = lref.lookup_chain(0, r, bits=bits)
    gates = {k: list(v) for k, v in gates.items()}
    for k, (i, v) in over.items():
        gates[k][i] = v
    return n_vars, public, gates, table, wit


def test_refusals_before_any_device_work(zk, pl):
    r = ref.R["BN128"]
    n_vars, public, gates, table, wit = _circuit(r)
    c = pl.LookupCircuit(n_vars, public, gates, table)
    assert (c.n, c.n_public, c.n_gates, c.n_table) == (8, 1, 5, 5)
    for v in (2, r - 1):
        with pytest.raises(pl.ZkError, match="selector qK of gate 3 is not 0 or 1"):
            pl.LookupCircuit(*_circuit(r, qK=(3, v))[:4])
    with pytest.raises(pl.ZkError, match="selector qK of gate 3 is not below"):
        pl.LookupCircuit(*_circuit(r, qK=(3, r))[:4])
    with pytest.raises(pl.ZkError, match="a table has at least one row"):
        pl.LookupCircuit(n_vars, public, gates, [])
    with pytest.raises(pl.ZkError, match="a table row holds three values"):
        pl.LookupCircuit(n_vars, public, gates, [(1, 2)])
    with pytest.raises(pl.ZkError, match="table value 4 is not below"):
        pl.LookupCircuit(n_vars, public, gates, [(1, 2, 3), (1, r, 3)])
    with pytest.raises(pl.ZkError, match="carry a selector qK"):
        pl.LookupCircuit(n_vars, public, {k: v for k, v in gates.items() if k != "qK"}, table)
    with pytest.raises(pl.ZkError, match="have one length"):
        pl.LookupCircuit(n_vars, public, dict(gates, qK=gates["qK"][:-1]), table)
    # T beyond the size limit: n = 2^k must hold the table and the field must hold the coset of 4n
    for cv, limit in (("BN128", 1 << 26), ("BLS12381", 1 << 30)):
        pl.check_table_size(cv, limit)
        with pytest.raises(pl.ZkError, match="a table of %d rows does not fit n <= 2\\^%d rows on %s" % (limit + 1, limit.bit_length() - 1, cv)):
            pl.check_table_size(cv, limit + 1)

    class Huge(list):
        def __len__(self):
            return (1 << 26) + 1
    with pytest.raises(pl.ZkError, match="does not fit"):
        pl.LookupCircuit(n_vars, public, gates, Huge(table))
    # the key: an R1CS circuit has no lookups; a plain gate table is not enough; too small a file
    fake = object.__new__(pl.R1csCircuit)
    fake._h = None
    with pytest.raises(pl.ZkError, match="^plonk lookup: an R1csCircuit has no lookups: prove it with plonk.py$"):
        pl.LookupKey(types.SimpleNamespace(curve="BN128", max_coeffs=100), fake)
    with pytest.raises(pl.ZkError, match="the key takes a LookupCircuit"):
        pl.LookupKey(types.SimpleNamespace(curve="BN128", max_coeffs=100), pl.Circuit(n_vars, public, gates))
    assert pl.required_powers(8) == 30
    with pytest.raises(pl.ZkError, match=r"plonk lookup: the file holds 29 G1 powers, n = 8 rows need 3n \+ 6 = 30"):
        pl.LookupKey(types.SimpleNamespace(curve="BN128", max_coeffs=29), c)
    # the prover's own, before the key's device arrays are read
    key = types.SimpleNamespace(curve="BN128", n=c.n, log_n=c.log_n, circuit=c, kzg=None)
    for bad in ([0] * 9, [0] * 13, [0] * 15, [0] * 13 + [r]):
        with pytest.raises(pl.ZkError, match="plonk lookup: blinding takes fourteen integers"):
            pl.prove(key, wit, blinding=bad)
    with pytest.raises(pl.ZkError, match="the witness has %d values, the circuit has %d variables" % (n_vars - 1, n_vars)):
        pl.prove(key, wit[:-1])
    # the library's refusals of a scalar, decided on the host
    lib = zk.lib()
    big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    ptrs = np.zeros(9, dtype=np.uint64)
    for at, name in enumerate(("alpha", "eta", "delta")):
        sc = [zk._ptr(big if j == at else one) for j in range(3)]
        assert lib.zk_plonk_bn254_lookup_quotient_dev(zk._ptr(ptrs), 3, *sc, None, None) != 0
        assert "plonk lookup: %s is not below the scalar field's modulus" % name in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_lookup_quotient_dev(zk._ptr(ptrs), 27, *[zk._ptr(one)] * 3, None, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_lookup_terms_dev(zk._ptr(ptrs), 8, zk._ptr(one), zk._ptr(big), None, None) != 0 and "delta is not below" in lib.zk_last_error().decode()
    assert not lib.zk_plonk_bn254_lookup_table_new(None, None, None, 4, None) and "null argument" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_lookup_count_dev(None, None, None, None, None, 0, None, None, None, None) != 0 and "null table" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_lookup_table_free(None) == 0


def test_the_table_is_padded_with_its_last_row_never_with_zeros(pl):
    r = ref.R["BN128"]
    n_vars, public, gates, _, wit = _circuit(r)
    table = [(1, 1, 1), (2, 5, 7), (3, 0, 3), (4, 4, 0)]                                    # 4 rows in n = 8, none of them zero
    c = pl.LookupCircuit(n_vars, public, gates, table)
    rows = [tuple(pl.pa.int_of(c.table[j][i]) for j in range(3)) for i in range(c.n)]
    assert c.n == 8 and rows == table + [table[-1]] * 4 and (0, 0, 0) not in rows
    assert (0, 0, 0) in [tuple(pl.pa.int_of(pl.LookupCircuit(n_vars, public, gates, [(0, 0, 0), (1, 1, 1)]).table[j][i]) for j in range(3)) for i in range(8)]   # only when given
    # qK sits behind the public rows and is 0 on them and on the padding
    qk = [pl.pa.int_of(w) for w in c.sel["qK"]]
    assert qk == [0] * c.n_public + gates["qK"] + [0] * (c.n - c.n_public - c.n_gates)
    # a table that alone forces n
    big = pl.LookupCircuit(n_vars, public, gates, pl.range_table(8))
    assert (big.n, big.n_table) == (256, 256) and pl.pa.int_of(big.table[0][255]) == 255
    assert pl.LookupCircuit(n_vars, public, gates, pl.range_table(8) + [(0, 0, 1)]).n == 512
    assert pl.range_table(2) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)] and pl.xor_table(1) == [(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)] and len(pl.xor_table(4)) == 256
    # the package's padded table and selectors are the reference's
    R = lref.Reference("BN128", n_vars, public, gates, table, 5, lambda s: s.to_bytes(64, "little"))
    assert rows == R.rows and qk == R.qk


def test_a_circuit_file_round_trips(pl, tmp_path):
    r = ref.R["BLS12381"]
    n_vars, public, gates, table, wit = lref.lookup_chain(1, r)
    c = pl.LookupCircuit(n_vars, public, gates, table, "BLS12381")
    c.save(tmp_path / "c.npz")
    d = pl.LookupCircuit.load(tmp_path / "c.npz", "BLS12381")
    assert (d.n_vars, d.public, d.n, d.n_table) == (c.n_vars, c.public, c.n, c.n_table) and np.array_equal(c.table, d.table)
    assert all(np.array_equal(c.sel[k], d.sel[k]) for k in ref.SELECTORS + ("qK",)) and all(np.array_equal(c.wire[k], d.wire[k]) for k in "abc")
    with np.load(tmp_path / "c.npz") as z:
        assert z["qK"].shape == (c.n_gates, 4) and z["qK"].dtype == np.uint64 and z["table"].shape == (len(table), 3, 4) and z["table"].dtype == np.uint64
    plain = importlib.import_module("eigen_zkvm_amd.plonk_arith").Circuit(n_vars, public, gates, "BLS12381")
    plain.save(tmp_path / "plain.npz")
    with pytest.raises(pl.ZkError, match="holds no qK, table"):
        pl.LookupCircuit.load(tmp_path / "plain.npz", "BLS12381")
