"""The aggregate Groth16 check's surface without a GPU: the command line knows --batch, the header declares the new symbols and the
library exports them (the Rust shim's guard, test_ffi_drift.py, runs beside this file)."""
import ctypes, pathlib, re, sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

NEW = (["zk_groth16_verify_aggregate", "zk_groth16_verify_aggregate_dev", "zk_groth16_verify_aggregate_timing", "zk_groth16_proof_words"] +
       ["zk_pairing_product_%s%s" % (c, d) for c in ("bn254", "bls12_381") for d in ("", "_dev")] +
       ["zk_%s_%s_mul_scalars_dev" % (g, c) for c in ("bn254", "bls12_381") for g in ("g1", "g2")])


def test_cli_parser_knows_batch():
    import zkgpu_prove
    ap = zkgpu_prove.build_parser()
    a = ap.parse_args(["groth16_verify", "-c", "BLS12381", "-v", "vk.json", "--batch", "list.json"])
    assert a.batch == "list.json" and a.curve_type == "BLS12381" and a.fn is zkgpu_prove.groth16_verify
    assert ap.parse_args(["groth16_verify"]).batch is None                 # the single-proof form is what it was


def test_header_declares_and_library_exports_the_new_symbols(zk):
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "zkgpu.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(str(zk.LIB_PATH))
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n) and n in zk.EXPORTS, n
    m = re.search(r"int zk_groth16_verify_aggregate\(([^)]*)\)", txt)
    assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["vk", "proofs", "publics", "n", "seed", "verdict", "first_bad"]


def test_python_surface(zk):
    import importlib
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    assert callable(dev.Groth16VerifyingKey.verify_aggregate) and callable(dev.pairing_product) and callable(dev.mul_scalars)
