"""The ceremony's surface without a GPU: the header declares the new symbols, the library exports them, the Python layer has its calls."""
import ctypes, importlib, pathlib, re

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = ["zk_g1_bn254_mul_scalars_glv_dev", "zk_g1_bls12_381_mul_scalars_glv_dev", "zk_srs_new", "zk_srs_contribute", "zk_srs_verify", "zk_srs_transcript_count",
       "zk_groth16_key_transcript_size", "zk_groth16_params_contribute_pok", "zk_groth16_key_transcript_check"]


def test_header_declares_and_library_exports_the_new_symbols(zk):
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "zkgpu.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(str(zk.LIB_PATH))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in zk.EXPORTS, n
    # the endomorphism walk has the bit walk's prototype
    proto = lambda n: re.search(r"int %s\(([^)]*)\)" % n, txt).group(1)
    assert proto("zk_g1_bn254_mul_scalars_glv_dev") == proto("zk_g1_bn254_mul_scalars_dev")
    assert "zk_g2_bn254_mul_scalars_glv_dev" not in declared               # no G2 endomorphism here


def test_python_surface(zk):
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    for name in ("srs_new", "contribute_pok", "key_transcript_check", "srs_verify_lines", "key_transcript_lines"):
        assert callable(getattr(dev, name)), name
    assert all(callable(getattr(dev.Srs, m)) for m in ("contribute", "verify", "transcript_count"))
    assert zk.lib().zk_groth16_key_transcript_size(b"BN128", 0) == 48 and zk.lib().zk_groth16_key_transcript_size(b"BLS12381", 2) == 48 + 2 * (96 + 192)
    rep = {"file": {"findings": [{"kind": "not_powers", "section": "tauG1"}]}, "findings": [{"kind": "pok_invalid", "contribution": 2, "which": "beta"}]}
    assert dev.srs_verify_lines(rep) == ["ptau file: not_powers section=tauG1", "ptau transcript: contribution 2: no valid proof of knowledge of the beta factor"]
