"""The surface of fflonk with tagged lookups without a GPU: the header declares the entry points and the macro and the library
exports them, the package binds them, eigen_zkvm_amd.fflonk_lookup_tagged has its functions and its constants, the library's refusals that
need no device, roots and the powers a file must hold, the codecs on the model's proof, the cross-refusal of keys and proofs with all five
other protocols in both directions, an untagged circuit refused here and a tagged one still refused by fflonk_lookup.py, which now names this
module; the command-line tool parses its three commands and refuses --r1cs with one line.  The JSON round trip of a proof whose points are
real needs the device (point_to_json converts coordinates there): here the points are the point at infinity, the values the model's."""
import importlib, json, pathlib, re, sys, types

import numpy as np
import pytest

import fflonk_lookup_tagged_ref as ftref
import plonk_lookup_ref as lref
import plonk_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_fflonk_%s_lookup_tagged_quotients_dev" % c for c in ("bn254", "bls12_381")]
TAU, PB = 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, 64
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(14)]
OTHERS = (("plonk", "plonk", ("plonk-shplonk",)), ("fflonk", "fflonk", ("fflonk-shplonk",)), ("plonk_lookup", "plonk lookup", ("plonk-shplonk-lookup", "plonk-shplonk-lookup-tagged")),
          ("fflonk_lookup", "fflonk lookup", ("fflonk-shplonk-lookup",)))


@pytest.fixture(scope="module")
def flt(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk_lookup_tagged")


@pytest.fixture(scope="module")
def model():
    n_vars, public, gates, tables, wit = ftref.tagged_chain(0, ref.R["BN128"])
    R = ftref.Reference("BN128", n_vars, public, gates, tables, TAU, lambda s: s.to_bytes(PB, "little"))
    return R, R.prove(wit, BLIND)


def test_header_declares_and_the_package_binds_the_entry_points(zk, flt):
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ZK_FFLONK_LOOKUP_TAGGED_QUOTIENT_COLS\s+22\b", code)
    flat = " ".join(text.split())
    assert "csrc/fflonk_lookup_tagged_impl.hip.h; DESIGN.md 3.27" in flat and "eigen_zkvm_amd/fflonk_lookup_tagged.py" in flat
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    lib = zk.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == 13, name
    for name in ("LookupCircuit", "LookupTable", "FflonkLookupTaggedKey", "VerifyingKey", "range_table", "xor_table", "setup", "prove", "verify", "challenges", "host_check", "roots",
                 "all_points", "quotients", "quotients_at", "opened_values", "values_of", "lookup_sum", "vk_to_json", "vk_from_json", "proof_to_json", "proof_from_json",
                 "proof_to_bytes", "proof_from_bytes", "vk_digest", "transcript_start", "transcript_round1", "transcript_round2", "transcript_values", "transcript_z",
                 "required_powers", "file_power", "quotient_coeffs"):
        assert callable(getattr(flt, name)), name
    assert zk.FflonkLookupTaggedKey is flt.FflonkLookupTaggedKey


def test_the_constants_and_the_docstring(flt):
    pl, fl, arith = (importlib.import_module("eigen_zkvm_amd." + m) for m in ("plonk_lookup", "fflonk_lookup", "plonk_arith"))
    assert (flt.PROTOCOL, flt.N_VALUES, flt.N_OPENED, flt.N_FIXED, flt.N_BLINDERS, flt.QUOTIENT_COLS) == ("fflonk-shplonk-lookup-tagged", 23, 30, 13, 14, 22)
    assert flt.FIXED == pl.TAGGED_FIXED and flt.FIXED[-1] == "T0" and flt.VALUE_NAMES[:13] == flt.FIXED and len(flt.VALUE_NAMES) == 23
    assert flt.VALUE_NAMES[13:] == ("a", "b", "c", "M", "Z", "Phi", "Zw", "Phiw", "T0w", "T1w") == fl.VALUE_NAMES[12:]
    assert flt.POINT_NAMES == fl.POINT_NAMES == ("C1", "C2", "C3", "W1", "W2") and flt.CIRCUIT == "LookupCircuit" and flt.LookupCircuit is pl.LookupCircuit
    assert issubclass(flt.FflonkLookupTaggedKey, arith.ArithKey) and not flt.FflonkLookupTaggedKey.KEEPS_COEF and flt.ZkError is arith.ZkError
    # what is shared is imported, not copied
    assert flt.roots is fl.roots and flt.all_points is fl.all_points and flt.required_powers is fl.required_powers and flt.quotient_coeffs is fl.quotient_coeffs
    assert flt.transcript_round1 is fl.transcript_round1 and flt.transcript_round2 is fl.transcript_round2 and flt.transcript_z is fl.transcript_z
    assert flt.vk_digest is not fl.vk_digest and flt.transcript_start is not fl.transcript_start and flt.transcript_values is not fl.transcript_values
    doc = flt.__doc__
    assert '"fflonklt-vk"' in doc and '"fflonklt-v1"' in doc and '"fflonk-shplonk-lookup-tagged"' in doc and "DESIGN.md 3.27" in doc
    for line in ("    c1     = H(c0 || C1)                     beta, gamma, eta, delta = H(c1 || 00 / 01 / 02 / 03)",
                 "    c2     = H(c1 || C2 || C3)               s = H(c2 || ctr)"):
        assert line in doc and line in fl.__doc__                                          # byte for byte where bytes matter
    for fn in (flt.vk_digest, flt.transcript_start, flt.transcript_values):
        assert "H(" in fn.__doc__, fn.__name__
    protocols = [importlib.import_module("eigen_zkvm_amd." + m).PROTOCOL for m in ("plonk", "fflonk", "plonk_lookup", "fflonk_lookup")] + [pl.TAGGED_PROTOCOL, flt.PROTOCOL]
    assert len(set(protocols)) == 6                                                         # a sixth protocol


def test_roots_and_the_powers_a_file_must_hold(flt):
    r = ref.R["BN128"]
    for log_n in (3, 20):
        n = 1 << log_n
        assert flt.required_powers(n) == 8 * n + 8 and flt.file_power(log_n) == log_n + 3
        assert flt.quotient_coeffs(n) == (2 * n + 2, n + 2, 3 * n + 6, 2 * n + 3)
        assert flt.C0L_SLOTS * n <= flt.required_powers(n)                                  # C0L's 8n coefficients fit the file C2 needs
    rt = flt.roots("BN128", 4, 0x1234567)
    xi, model_sets = ftref.roots_of("BN128", 4, 0x1234567)
    assert rt["xi"] == xi and [rt["S0"], rt["S1"], rt["S2"], rt["S3"]] == model_sets
    assert len(rt["S0"]) == 8 and all(pow(h, 8, r) == xi for h in rt["S0"])                 # the set C0 AND C0L are opened on
    assert flt.all_points(rt) == rt["S0"] + rt["S2"] + rt["S3"]
    assert 2 * len(rt["S0"]) + len(rt["S1"]) + len(rt["S2"]) + len(rt["S3"]) == flt.N_OPENED
    with pytest.raises(flt.ZkError, match="a circuit has at least 8"):
        flt.roots("BN128", 2, 5)


def test_the_codecs_round_trip_on_the_models_proof(flt, model):
    R, res = model
    cv, proof = "BN128", res["proof"]
    data = flt.proof_to_bytes(proof)
    assert len(data) == 5 * PB + 23 * 32 and flt.proof_from_bytes(data, PB) == proof
    assert data == b"".join(proof[k] for k in flt.POINT_NAMES) + b"".join(v.to_bytes(32, "little") for v in proof["values"])
    with pytest.raises(flt.ZkError, match="fflonk lookup tagged: a proof is %d bytes, not %d" % (len(data), len(data) - 32)):
        flt.proof_from_bytes(data[:-32], PB)
    flat = dict({k: bytes(PB) for k in flt.POINT_NAMES}, values=proof["values"])           # the point at infinity needs no device to convert
    js = flt.proof_to_json(flat, cv)
    assert json.loads(js)["protocol"] == "fflonk-shplonk-lookup-tagged" and len(json.loads(js)["values"]) == 23 and flt.proof_from_json(js, cv) == flat
    with pytest.raises(flt.ZkError, match="not a proof of this prover on BLS12381"):
        flt.proof_from_json(js, "BLS12381")
    vk = flt.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], bytes(PB), bytes(PB))
    back = flt.vk_from_json(flt.vk_to_json(vk))
    assert (back.curve, back.log_n, back.n_public, back.k1, back.k2, back.c0, back.c0l, back.digest) == (cv, 3, R.t.l, R.t.k[1], R.t.k[2], vk.c0, vk.c0l, vk.digest)
    assert json.loads(flt.vk_to_json(vk))["protocol"] == "fflonk-shplonk-lookup-tagged"
    real = flt.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], *R.vk_points)
    assert real.digest == R.vkd != vk.digest
    with pytest.raises(flt.ZkError, match="a circuit has at least 8"):
        flt.VerifyingKey(cv, 2, 1, 2, 3, bytes(PB), bytes(PB))
    with pytest.raises(flt.ZkError, match="^fflonk lookup tagged: the two points of a verification key have one length"):
        flt.VerifyingKey(cv, 3, 1, 2, 3, bytes(PB), bytes(PB - 1))


def test_keys_and_proofs_are_refused_across_all_six_protocols_in_both_directions(flt, model):
    R, res = model
    cv = "BN128"
    mine = json.dumps({"protocol": flt.PROTOCOL, "curve": cv})
    for name, who, protocols in OTHERS:
        mod = importlib.import_module("eigen_zkvm_amd." + name)
        for protocol in protocols:
            theirs = json.dumps({"protocol": protocol, "curve": cv})
            with pytest.raises(flt.ZkError, match='^fflonk lookup tagged: not a verification key of this prover \\(protocol "%s"\\): %s.py proves and verifies it$' % (protocol, name)):
                flt.vk_from_json(theirs)
            with pytest.raises(flt.ZkError, match='^fflonk lookup tagged: not a proof of this prover on BN128 \\(protocol "%s"' % protocol):
                flt.proof_from_json(theirs, cv)
        with pytest.raises(flt.ZkError, match='^%s: not a verification key of this prover \\(protocol "fflonk-shplonk-lookup-tagged"\\)' % who):
            mod.vk_from_json(mine)
        with pytest.raises(flt.ZkError, match='^%s: not a proof of this prover on BN128 \\(protocol "fflonk-shplonk-lookup-tagged"' % who):
            mod.proof_from_json(mine, cv)
    with pytest.raises(flt.ZkError, match='not a verification key of this prover \\(protocol "None"\\)$'):
        flt.vk_from_json("{}")
    # the verifiers' host parts: a proof of this protocol has 23 values, no other has
    fl, pl = importlib.import_module("eigen_zkvm_amd.fflonk_lookup"), importlib.import_module("eigen_zkvm_amd.plonk_lookup")
    vk = flt.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], *R.vk_points)
    with pytest.raises(flt.ZkError, match="^fflonk lookup: a proof holds 22 values, not 23"):
        fl.host_check(fl.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], *R.vk_points), res["publics"], res["proof"])
    with pytest.raises(flt.ZkError, match="^fflonk lookup tagged: a proof holds 23 values, not 22"):
        flt.host_check(vk, res["publics"], dict(res["proof"], values=res["values"][:12] + res["values"][13:]))
    with pytest.raises(flt.ZkError, match="^fflonk lookup tagged: the proof holds no C1, C2, C3"):
        flt.host_check(vk, res["publics"], {"A": b"", "B": b"", "C": b"", "M": b"", "Z": b"", "Phi": b"", "T": b"", "W1": bytes(PB), "W2": bytes(PB), "values": [0] * 22})
    with pytest.raises(flt.ZkError, match="^plonk lookup: the proof holds no A, B, C, M, Z, Phi, T"):
        pl.host_check(pl.VerifyingKey(cv, 3, 1, 2, 3, [bytes(PB)] * 13), res["publics"], res["proof"])
    # the single-table key over the same two points has another digest, so other challenges
    assert fl.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], *R.vk_points).digest != vk.digest


def test_an_untagged_circuit_is_refused_here_and_a_tagged_one_there(flt):
    fl = importlib.import_module("eigen_zkvm_amd.fflonk_lookup")
    cv = "BN128"
    r = ref.R[cv]
    handle = types.SimpleNamespace(curve=cv, max_coeffs=1 << 20)
    n_vars, public, gates, table, wit = lref.lookup_chain(0, r)
    with pytest.raises(flt.ZkError, match=r"^fflonk lookup tagged: the circuit has one untagged table: .* fflonk_lookup.py proves a circuit of one table$"):
        flt.setup(handle, flt.LookupCircuit(n_vars, public, gates, table))
    fake = object.__new__(flt.R1csCircuit)
    fake._h = None
    with pytest.raises(flt.ZkError, match="^fflonk lookup tagged: an R1csCircuit has no lookups: prove it with fflonk.py$"):
        flt.FflonkLookupTaggedKey(handle, fake)
    with pytest.raises(flt.ZkError, match="^fflonk lookup tagged: the key takes a LookupCircuit$"):
        flt.FflonkLookupTaggedKey(handle, importlib.import_module("eigen_zkvm_amd.plonk_arith").Circuit(n_vars, public, gates))
    n_vars, public, gates, tables, wit = ftref.tagged_chain(0, r)
    c = flt.LookupCircuit(n_vars, public, gates, tables=tables)
    with pytest.raises(flt.ZkError, match=r"^fflonk lookup tagged: the file holds 71 G1 powers, n = 8 rows need 8n \+ 8 = 72 \(a file of power 6 has them\)$"):
        flt.FflonkLookupTaggedKey(types.SimpleNamespace(curve=cv, max_coeffs=71), c)
    with pytest.raises(flt.ZkError, match="the circuit is over BN128, the file over BLS12381"):
        flt.FflonkLookupTaggedKey(types.SimpleNamespace(curve="BLS12381", max_coeffs=100), c)
    # fflonk_lookup.py stays the single-table protocol: its refusal keeps its first sentence and now names this module
    with pytest.raises(flt.ZkError, match=r"^fflonk lookup: the circuit has 2 tagged tables: fflonk with lookups proves one table \(C0L interleaves four polynomials and has no slot "
                                           r"for T0\); fflonk_lookup_tagged.py proves a tagged circuit under fflonk"):
        fl.setup(handle, c)
    doc = fl.__doc__.replace("\n", " ")
    assert "setup refuses a tagged circuit" in doc.split("Not built:")[1] and "fflonk_lookup_tagged.py" in doc.split("Not built:")[1]
    # the prover's own refusals, before the key's device arrays are read
    key = types.SimpleNamespace(curve=cv, n=c.n, log_n=c.log_n, circuit=c, kzg=None)
    with pytest.raises(flt.ZkError, match="fflonk lookup tagged: blinding takes fourteen integers"):
        flt.prove(key, wit, blinding=[0] * 13)
    with pytest.raises(flt.ZkError, match="fflonk lookup tagged: the witness has %d values, the circuit has %d variables" % (n_vars - 1, n_vars)):
        flt.prove(key, wit[:-1])


def test_the_library_refuses_on_the_host_before_any_device_work(zk, flt):
    r = ref.R["BN128"]
    with pytest.raises(flt.ZkError, match="the quotients take 22 columns, not 21"):
        flt.quotients([None] * 21, 3, 1, 1, 2, 3, 1, 1)
    with pytest.raises(flt.ZkError, match="eta is not below"):
        flt.quotients([None] * 22, 3, 1, 1, 2, 3, r, 1)
    lib = zk.lib()
    big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    ptrs = np.zeros(22, dtype=np.uint64)
    none = [None] * 5                                                                       # the four outputs and the stream
    for at, name in enumerate(("beta", "gamma", "k1", "k2", "eta", "delta")):                # BN254's r stands for a scalar that is not below it
        sc = [zk._ptr(big if j == at else one) for j in range(6)]
        assert lib.zk_fflonk_bn254_lookup_tagged_quotients_dev(zk._ptr(ptrs), 3, *sc, *none) != 0
        assert "fflonk lookup tagged: %s is not below the scalar field's modulus" % name in lib.zk_last_error().decode()
    for fn in (lib.zk_fflonk_bn254_lookup_tagged_quotients_dev, lib.zk_fflonk_bls12_381_lookup_tagged_quotients_dev):
        assert fn(zk._ptr(ptrs), 3, *[zk._ptr(one)] * 6, *none) != 0 and "every output is null" in lib.zk_last_error().decode()
        assert fn(None, 3, *[zk._ptr(one)] * 6, *none) != 0 and "null argument" in lib.zk_last_error().decode()
        assert fn(zk._ptr(ptrs), 3, *[zk._ptr(one)] * 5, None, *none) != 0 and "null delta" in lib.zk_last_error().decode()
        # a null column is named before any output is looked at: the output here is an address that is never read or written
        assert fn(zk._ptr(ptrs), 3, *[zk._ptr(one)] * 6, 4096, None, None, None, None) != 0 and "fflonk lookup tagged: quotients: column 0 is null" in lib.zk_last_error().decode()
    assert lib.zk_fflonk_bn254_lookup_tagged_quotients_dev(zk._ptr(ptrs), 27, *[zk._ptr(one)] * 6, *none) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()
    assert lib.zk_fflonk_bls12_381_lookup_tagged_quotients_dev(zk._ptr(ptrs), 31, *[zk._ptr(one)] * 6, *none) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()


def test_cli_parses_its_three_commands_and_refuses_an_r1cs(capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_fflonk_lookup_tagged")
    assert (cli.TOOL.prefix, cli.TOOL.module, cli.TOOL.key) == ("fflonk_lookup_tagged", "eigen_zkvm_amd.fflonk_lookup_tagged", "FflonkLookupTaggedKey")
    ap = cli.build_parser()
    a = ap.parse_args(["fflonk_lookup_tagged_setup", "-c", "BN128", "--ptau", "f.ptau", "--circuit", "c.npz", "-v", "vk.json"])
    assert (a.cmd, a.curve, a.ptau, a.circuit, a.vk, a.no_check_srs) == ("fflonk_lookup_tagged_setup", "BN128", "f.ptau", "c.npz", "vk.json", False)
    a = ap.parse_args(["fflonk_lookup_tagged_prove", "--ptau", "f.ptau", "--circuit", "c.npz", "--witness", "w.bin", "--proof", "proof.json", "--public", "public.json", "--no-check-srs"])
    assert (a.cmd, a.witness, a.proof, a.public, a.no_check_srs) == ("fflonk_lookup_tagged_prove", "w.bin", "proof.json", "public.json", True)
    a = ap.parse_args(["fflonk_lookup_tagged_verify", "-v", "vk.json", "--ptau", "f.ptau", "p1.json:x1.json", "p2.json:x2.json"])
    assert (a.cmd, a.vk, a.pairs) == ("fflonk_lookup_tagged_verify", "vk.json", ["p1.json:x1.json", "p2.json:x2.json"])
    for argv in (["fflonk_lookup_tagged_setup", "--ptau", "no-such.ptau", "--r1cs", "c.r1cs", "-v", "vk.json"],
                 ["fflonk_lookup_tagged_prove", "--ptau", "no-such.ptau", "--r1cs", "c.r1cs", "--wtns", "w.wtns", "--proof", "p.json", "--public", "x.json"]):
        with pytest.raises(SystemExit) as e:                                               # before any file is opened
            cli.main(argv)
        out = capsys.readouterr().out
        assert e.value.code == 1 and out.count("\n") == 1 and "takes no --r1cs" in out and argv[0] in out and out.startswith("zkgpu_fflonk_lookup_tagged: ")
    c = types.SimpleNamespace(n_table=7, table_sizes=[2, 5], gates={"qK": np.array([[1, 0, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0]], dtype=np.uint64)})
    assert cli._need(None, types.SimpleNamespace(log_n=4, n=16, circuit=c), 136, 7) == [
        "fflonk_lookup_tagged_setup: n = 2^4 = 16 rows need 8n + 8 = 136 powers (a file of power 7 has them)",
        "fflonk_lookup_tagged_setup: 2 tagged tables of 2, 5 rows (7 in all), 2 of the gates look a row up"]
