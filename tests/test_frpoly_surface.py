"""The surface of the scalar-field polynomial layer without a GPU: the header declares every entry point, the package exports and binds
them, eigen_zkvm_amd.frpoly has one function per entry point, the command-line tool parses its three commands, and refusals that are
decided on the host come back as the library's text."""
import importlib, pathlib, re, sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAMES = ("prefix_product", "batch_inverse", "pointwise", "powers", "terms", "grand_product", "poly_mul", "divmod_zh", "divide_zh_coset")
ENTRY_POINTS = ["zk_frpoly_tile_elems", "zk_frpoly_span"] + ["zk_fr_%s_%s_dev" % (c, n) for c in ("bn254", "bls12_381") for n in NAMES]


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    for macro, value in (("ZK_FR_MUL", 0), ("ZK_FR_ADD", 1), ("ZK_FR_SUB", 2), ("ZK_FRPOLY_MAX_RATIO", 4096)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    assert "Not built: the prover that stands on this (gate constraints, transcript, blinding)" in " ".join(text.split())


def test_package_exports_and_binds_them(zk):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    fp = importlib.import_module("eigen_zkvm_amd.frpoly")
    for n in NAMES:
        assert callable(getattr(fp, n)), n
    assert (fp.MUL, fp.ADD, fp.SUB, fp.MAX_RATIO) == (0, 1, 2, 4096)
    lib = zk.lib()                                      # dlopen + every signature: no device is touched
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    T, S = lib.zk_frpoly_tile_elems(), lib.zk_frpoly_span()
    assert T >= 64 and T & (T - 1) == 0 and S >= 2
    assert (fp.tile_elems(), fp.span()) == (T, S)


def test_cli_parses_its_three_commands():
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_poly")
    ap = cli.build_parser()
    a = ap.parse_args(["poly_mul", "-c", "BN128", "--poly", "a.bin", "--poly", "b.bin", "-o", "c.bin"])
    assert (a.cmd, a.curve, a.poly, a.out) == ("poly_mul", "BN128", ["a.bin", "b.bin"], "c.bin")
    a = ap.parse_args(["poly_divmod_zh", "-c", "BLS12381", "--poly", "t.bin", "--log-n", "6", "-o", "q.bin", "--rem", "r.bin"])
    assert (a.cmd, a.curve, a.poly, a.log_n, a.out, a.rem) == ("poly_divmod_zh", "BLS12381", ["t.bin"], 6, "q.bin", "r.bin")
    a = ap.parse_args(["poly_divmod_zh", "-c", "BN128", "--poly", "t.bin", "--log-n", "0", "-o", "q.bin"])
    assert a.rem is None and a.log_n == 0
    a = ap.parse_args(["grand_product", "-c", "BN128", "--num", "n.bin", "--den", "d.bin", "-o", "z.bin"])
    assert (a.cmd, a.num, a.den, a.out) == ("grand_product", "n.bin", "d.bin", "z.bin")
    with pytest.raises(SystemExit):
        ap.parse_args(["poly_mul", "--poly", "a.bin", "-o", "c.bin"])          # the curve is required


def test_refusals_decided_on_the_host(zk):
    """a scalar that is not below r, an unknown operation, k outside 1 .. 16, a length beyond the 2-adicity, the ratio: each is refused
    before any device work, so no device is needed to see the text"""
    import ctypes as C
    import numpy as np
    lib = zk.lib()
    err = lambda: lib.zk_last_error().decode()
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    big = np.frombuffer(r.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    fake = None                                                                 # no vector is passed at all: every call below is refused first
    assert lib.zk_fr_bn254_powers_dev(zk._ptr(big), zk._ptr(one), 4, fake, None) != 0 and "base is not below the scalar field's modulus" in err()
    assert lib.zk_fr_bn254_powers_dev(zk._ptr(one), zk._ptr(big), 4, fake, None) != 0 and "scale is not below" in err()
    assert lib.zk_fr_bls12_381_powers_dev(zk._ptr(big), zk._ptr(one), 0, None, None) == 0        # below the other curve's modulus; n = 0 touches nothing
    ptrs = np.zeros(17, dtype=np.uint64)
    for k in (0, 17):
        assert lib.zk_fr_bn254_terms_dev(zk._ptr(ptrs), None, k, 4, zk._ptr(one), zk._ptr(one), fake, None) != 0 and "a term takes 1 to 16" in err()
    assert lib.zk_fr_bn254_terms_dev(zk._ptr(ptrs), None, 3, 4, zk._ptr(big), zk._ptr(one), fake, None) != 0 and "beta is not below" in err()
    assert lib.zk_fr_bn254_pointwise_dev(7, fake, fake, fake, 4, None) != 0 and "unknown pointwise operation" in err()
    assert lib.zk_fr_bn254_poly_mul_dev(fake, (1 << 28) + 1, fake, 1, fake, None) != 0 and "exceeds the field's 2-adicity" in err()
    assert lib.zk_fr_bn254_poly_mul_dev(fake, 0, fake, 1, fake, None) != 0 and "no coefficients" in err()
    cnt = C.c_uint64(0)
    assert lib.zk_fr_bn254_divmod_zh_dev(fake, 4097, 0, None, None, C.byref(cnt), None) != 0
    assert "ZK_FRPOLY_MAX_RATIO" in err() and "zk_kzg_bn254_divide_dev" in err()
    assert lib.zk_fr_bls12_381_divide_zh_coset_dev(fake, 3, 4, None) != 0 and "exceeds the domain" in err()
    assert lib.zk_fr_bn254_divide_zh_coset_dev(fake, 29, 4, None) != 0 and "2-adicity" in err()
    tot = np.zeros(4, dtype=np.uint64)
    assert lib.zk_fr_bn254_prefix_product_dev(None, 0, 0, None, zk._ptr(tot), None) == 0 and tot.tolist() == [1, 0, 0, 0]
