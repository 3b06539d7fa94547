"""The surface of the openings at several points without a GPU: the header declares the entry points and the proof's layout, the package
binds them with the signatures the header states, the command-line tool parses --poly / --at groups beside the one-point form, and the two
challenge functions are the hashes their docstrings state, recomputed here byte for byte."""
import ctypes as C
import hashlib, importlib, pathlib, re, sys

import pytest

import kzg_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_kzg_bn254_divide_acc_dev", "zk_kzg_bls12_381_divide_acc_dev", "zk_kzg_bn254_interleave_dev", "zk_kzg_bls12_381_interleave_dev",
                "zk_kzg_multi_begin", "zk_kzg_multi_quotient", "zk_kzg_multi_finish", "zk_kzg_multi_free", "zk_kzg_multi_verify", "zk_kzg_multi_verify_dev"]


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    assert "u64 k | k x C_i (point_bytes) | k x u64 |S_i| | P x point (32 B) | P x value (32 B) | gamma (32 B) | z (32 B) | W1 | W2" in text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "typedef struct zk_kzg_multi zk_kzg_multi_t;" in code
    assert re.search(r"#define\s+ZK_KZG_MULTI_MAX_POINTS\s+16\b", code)


def test_package_exports_and_binds_them(zk):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    assert zk.divide_acc is kzg.divide_acc and zk.interleave is kzg.interleave and kzg.MULTI_MAX_POINTS == 16
    for m in ("open_multi", "verify_multi", "multi_begin", "pack_multi"):
        assert callable(getattr(kzg.Kzg, m)), m
    for m in ("quotient", "finish", "free"):
        assert callable(getattr(kzg.MultiOpening, m)), m
    lib = zk.lib()                                      # dlopen + every signature: no device is touched
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    want = {"divide_acc_dev": (C.c_int, [vp, u64, vp, vp, vp, vp, vp]), "interleave_dev": (C.c_int, [vp, vp, u32, vp, vp])}
    for abi in ("bn254", "bls12_381"):
        for name, (res, args) in want.items():
            fn = getattr(lib, "zk_kzg_%s_%s" % (abi, name))
            assert fn.restype is res and list(fn.argtypes) == args, (abi, name)
    for name, res, args in (("zk_kzg_multi_begin", vp, [vp, vp, vp, u32, vp, vp, vp, vp]), ("zk_kzg_multi_quotient", C.c_int, [vp, vp, vp, vp]),
                            ("zk_kzg_multi_finish", C.c_int, [vp, vp, vp, vp]), ("zk_kzg_multi_free", C.c_int, [vp]),
                            ("zk_kzg_multi_verify", C.c_int, [vp, vp, u64, u64, vp, C.POINTER(C.c_int), vp]),
                            ("zk_kzg_multi_verify_dev", C.c_int, [vp, vp, u64, u64, vp, C.POINTER(C.c_int), vp, vp])):
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.zk_kzg_multi_free(None) == 0             # freeing nothing is no error


def test_cli_parses_groups_beside_the_one_point_form():
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_kzg")
    ap = cli.build_parser()
    a = ap.parse_args(["kzg_open", "--ptau", "f.ptau", "--poly", "p.bin", "--at", "1,0x10,7", "--poly", "q.bin", "--at", "9", "-o", "m.json"])
    assert (a.cmd, a.poly, a.out) == ("kzg_open", ["p.bin", "q.bin"], "m.json")
    assert cli.at_groups(a) == [[1, 16, 7], [9]]
    a = ap.parse_args(["kzg_open", "--ptau", "f.ptau", "--poly", "p.bin", "--at", "3,4", "-o", "m.json"])
    assert cli.at_groups(a) == [[3, 4]]
    a = ap.parse_args(["kzg_open", "--ptau", "f.ptau", "--poly", "p.bin", "--poly", "q.bin", "--at", "0x11", "-o", "o.json"])
    assert cli.at_groups(a) is None and a.at == "0x11"                      # every --poly, then one point: the gamma fold at one point
    a = ap.parse_args(["kzg_open", "--ptau", "f.ptau", "--poly", "p.bin", "--at", "5", "-o", "o.json"])
    assert cli.at_groups(a) is None
    for argv in (["--poly", "p.bin", "--poly", "q.bin", "--at", "1,2"], ["--poly", "p.bin", "--at", "1", "--at", "2"], ["--poly", "p.bin", "--at", "1,2", "--poly", "q.bin"]):
        with pytest.raises(SystemExit, match="one --at Z1,Z2,.. after every --poly"):
            cli.at_groups(ap.parse_args(["kzg_open", "--ptau", "f.ptau"] + argv + ["-o", "m.json"]))
    assert -2 in cli.REASONS


def test_documented_challenges():
    """challenges_of and challenge_z are the hashes their docstrings state, byte for byte"""
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    for curve, r in ref.R.items():
        cs = [bytes(range(64)), bytes(64)]
        sets, values = [[5, 6, 7], [r - 1]], [[11, 12, 13], [0]]
        le = lambda v, n=32: int(v).to_bytes(n, "little")
        msg = curve.encode("ascii") + b"kzg-multi-gamma" + le(2, 4) + cs[0] + cs[1]
        msg += le(3, 4) + le(5) + le(6) + le(7) + le(1, 4) + le(r - 1)
        msg += le(11) + le(12) + le(13) + le(0)
        gamma = int.from_bytes(hashlib.sha256(msg).digest(), "big") % r
        assert kzg.challenges_of(curve, cs, sets, values) == gamma
        W1 = bytes(reversed(range(64)))
        base = curve.encode("ascii") + b"kzg-multi-z" + le(gamma) + W1
        z0 = int.from_bytes(hashlib.sha256(base).digest(), "big") % r
        z1 = int.from_bytes(hashlib.sha256(base + b"\x01").digest(), "big") % r
        z2 = int.from_bytes(hashlib.sha256(base + b"\x02").digest(), "big") % r
        assert kzg.challenge_z(curve, gamma, W1) == z0 == kzg.challenge_z(curve, gamma, W1, avoid=[5, 6])
        assert kzg.challenge_z(curve, gamma, W1, avoid=[z0]) == z1          # z in T: the same bytes and a counter byte
        assert kzg.challenge_z(curve, gamma, W1, avoid=[z1, z0]) == z2
