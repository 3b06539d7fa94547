"""The surface of the KZG layer without a GPU: the header declares the entry points, the package exports Kzg and divide, the command-line
tool parses its three subcommands, and the reference (tests/kzg_ref.py) agrees with itself."""
import importlib, pathlib, random, re, sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_kzg_tile_elems", "zk_kzg_aggregate_span", "zk_kzg_bn254_divide_dev", "zk_kzg_bls12_381_divide_dev", "zk_kzg_bn254_lincomb_dev",
                "zk_kzg_bls12_381_lincomb_dev", "zk_kzg_new", "zk_kzg_free", "zk_kzg_info", "zk_kzg_commit_dev", "zk_kzg_commit_evals_dev", "zk_kzg_eval_dev",
                "zk_kzg_open_dev", "zk_kzg_open_many_dev", "zk_kzg_fold_commitments", "zk_kzg_verify", "zk_kzg_verify_dev"]


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "zkgpu.h").read_text()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "typedef struct zk_kzg zk_kzg_t;" in text


def test_package_exports_and_binds_them(zk):
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    assert zk.Kzg is kzg.Kzg and zk.divide is kzg.divide
    for m in ("commit", "commit_evals", "eval", "open", "open_many", "verify", "free", "fold_commitments"):
        assert callable(getattr(kzg.Kzg, m)), m
    lib = zk.lib()                                      # dlopen + every signature: no device is touched
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    T, S = lib.zk_kzg_tile_elems(), lib.zk_kzg_aggregate_span()
    assert T >= 64 and T & (T - 1) == 0 and S >= 2


def test_cli_parses_its_three_subcommands():
    sys.path.insert(0, str(ROOT / "tools"))
    cli = importlib.import_module("zkgpu_kzg")
    ap = cli.build_parser()
    a = ap.parse_args(["kzg_commit", "-c", "BN128", "--ptau", "f.ptau", "--poly", "p.bin", "--evals", "-o", "c.json"])
    assert (a.cmd, a.curve, a.ptau, a.poly, a.evals, a.out, a.no_check_srs) == ("kzg_commit", "BN128", "f.ptau", ["p.bin"], True, "c.json", False)
    a = ap.parse_args(["kzg_open", "--ptau", "f.ptau", "--poly", "p.bin", "--poly", "q.bin", "--at", "0x11", "-o", "o.json", "--no-check-srs"])
    assert (a.cmd, a.poly, a.at, a.out, a.no_check_srs, a.curve) == ("kzg_open", ["p.bin", "q.bin"], "0x11", "o.json", True, None)
    a = ap.parse_args(["kzg_verify", "--ptau", "f.ptau", "a.json", "b.json"])
    assert (a.cmd, a.openings) == ("kzg_verify", ["a.json", "b.json"])


def test_documented_gamma():
    """gamma_of is the hash the tool's text states, byte for byte"""
    import hashlib
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    import kzg_ref as ref
    cs = [bytes(range(64)), bytes(64)]
    want = int.from_bytes(hashlib.sha256(b"BN128" + cs[0] + cs[1] + (77).to_bytes(32, "little")).digest(), "big") % ref.R["BN128"]
    assert kzg.gamma_of("BN128", cs, 77) == want


def test_reference_agrees_with_itself():
    import kzg_ref as ref
    rng = random.Random(11)
    for curve, r in ref.R.items():
        for n in (0, 1, 2, 9):
            p = [rng.randrange(r) for _ in range(n)]
            for z in (0, 1, r - 1, rng.randrange(r)):
                q, y = ref.divide(p, z, r)
                assert y == ref.horner(p, z, r) and len(q) == max(n - 1, 0)
                x = rng.randrange(r)                    # p(x) = q(x) (x - z) + y at a random x
                assert (ref.horner(q, x, r) * (x - z) + y) % r == ref.horner(p, x, r)
        w = ref.root_of_unity(curve, 6)
        assert pow(w, 64, r) == 1 and pow(w, 32, r) == r - 1
        polys = [[1, 2, 3], [4], []]
        assert ref.fold_polys(polys, 10, r) == [41, 2, 3]
        assert ref.fold_values([ref.horner(p, 5, r) for p in polys], 10, r) == ref.horner(ref.fold_polys(polys, 10, r), 5, r)
