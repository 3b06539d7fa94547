"""groth16_key_check timing: python tools/key_check_time.py [points] [key] [ptau] [BN128|BLS12381 ...] [log2_constraints]

points  zk_points_check_*_dev on 2^20 device-resident points (multiples of the generator from the fixed-base kernel) per curve and
        group, in both forms: the endomorphism tests and [r]P = O bit by bit (the baseline); wall clock around the call, which
        returns after reading the eight result words back; median of 3 after one warm-up.
key     the whole check of a key of 2^k constraints (default 20; tools/groth16_bench.make_circuit, the key made on the device):
        wall clock, and the library's own split ("timing_ms" of the report under ZK_KEY_CHECK_TIMING) into parse, point checks, sums and
        pairings.  parse is all the host does before the first launch: both files read, and the circuit's three matrices built only for
        their density counts (some 150 MB of host memory at 2^20 rows).
ptau    (only when asked for) groth16_key_check --ptau on a circuit of 2^k rows (default 16, the size of profiles/r14/srs_setup.md) and a
        file of power k from tools/make_test_ptau.py (known trapdoor: timing only): wall clock of key_check_srs and its own split into
        parse, row sums, transforms, sums and pairings, next to the only alternative there was before it -- make the key again from the
        file (keygen(srs=..., check_srs=False)) and compare the bytes, which works for delta = 1 only.  One warm-up call each, then
        the median of 3."""
import importlib, json, os, pathlib, statistics, sys, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import eigen_zkvm_amd
zk = eigen_zkvm_amd; zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")
ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}


def timed(fn, reps=3):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 2)


args = sys.argv[1:]
what = [a for a in args if a in ("points", "key", "ptau")] or ["points", "key"]
curves = [a for a in args if a in ABI] or list(ABI)
logs = [int(a) for a in args if a.isdigit()]
log_n = logs[0] if logs else (16 if what == ["ptau"] else 20)
for tag in curves:
    if "points" in what:
        n = 1 << 20
        rng = np.random.default_rng(1)
        k = np.concatenate([rng.integers(0, 2**64, size=(n, 3), dtype=np.uint64), rng.integers(0, dev._FR[tag] >> 192, size=(n, 1), dtype=np.uint64)], axis=1)
        d_k = zk.DevArray.from_host(k.reshape(-1))
        for group in ("g1", "g2"):
            d_pts = zk.mul_generator_fr(d_k, ABI[tag], group=group)
            out = dict(curve=tag, group=group, n=n)
            for plain in (True, False):
                rep = dev.points_check(d_pts, tag, group, plain=plain)
                assert not any(v[0] for v in rep.values()), rep
                out["plain_ms" if plain else "endomorphism_ms"] = timed(lambda: dev.points_check(d_pts, tag, group, plain=plain))
            d_pts.free()
            print(json.dumps(out), flush=True)
        d_k.free()
    if "key" in what:
        import groth16_bench as GB
        rb, _wit, _ni, _nw = GB.make_circuit(dev._FR[tag], log_n)
        t0 = time.perf_counter(); pb, vk = dev.keygen(tag, rb); keygen_s = round(time.perf_counter() - t0, 2)
        os.environ["ZK_KEY_CHECK_TIMING"] = "1"
        rep = dev.key_check(tag, rb, pb, vk_json=vk)
        t0 = time.perf_counter(); rep = dev.key_check(tag, rb, pb, vk_json=vk); wall = round((time.perf_counter() - t0) * 1e3, 1)
        print(json.dumps(dict(curve=tag, log_constraints=log_n, key_bytes=len(pb), keygen_s=keygen_s, sections=rep["sections"], counts=rep["counts"], checked=rep["checked"],
                              wall_ms=wall, **{k + "_ms": round(v, 1) for k, v in rep["timing_ms"].items()})), flush=True)
    if "ptau" in what:
        import random, tempfile
        import groth16_bench as GB
        import make_test_ptau as MP
        rng = random.Random(16)
        rb, _wit, _ni, n_wires = GB.make_circuit(dev._FR[tag], log_n)
        with tempfile.TemporaryDirectory() as d:
            p = pathlib.Path(d) / "t.ptau"
            p.write_bytes(MP.build_ptau(zk, tag, log_n, *(rng.randrange(1, dev._FR[tag]) for _ in range(3))))
            srs = dev.Srs(tag, p)
        pb, _ = dev.keygen(tag, rb, srs=srs, check_srs=False)
        regen = timed(lambda: dev.keygen(tag, rb, srs=srs, check_srs=False)[0] == pb)
        os.environ["ZK_KEY_CHECK_TIMING"] = "1"
        reps = []
        check = timed(lambda: reps.append(dev.key_check_srs(tag, rb, pb, srs)))
        srs.free()
        assert all(not any(r["counts"].values()) and not r["skipped"] for r in reps), reps[-1]
        split = {k + "_ms": round(statistics.median(r["timing_ms"][k] for r in reps[1:]), 1) for k in reps[-1]["timing_ms"]}
        print(json.dumps(dict(curve=tag, log_rows=log_n, n_wires=n_wires, key_bytes=len(pb), checked=reps[-1]["checked"], key_check_srs_ms=check, **split,
                              regenerate_and_compare_ms=regen, regenerate_over_check=round(regen / check, 2))), flush=True)
