"""Per-proof against aggregate Groth16 verification: python tools/verify_aggregate_time.py [BN128|BLS12381 ...] [n ...]

For each curve a small circuit (tools/groth16_bench.make_circuit, 2^6 rows, 3 public inputs), its key made on the device and four
distinct proofs, tiled to n = 1, 64, 4096, 65536 proofs resident on the device.  For each n: one warm-up call and ONE timed call
of zk_groth16_verify_batch_dev (n verdicts) and of zk_groth16_verify_aggregate_dev (one verdict, operating-system weights, no
locating), host wall clock around a stream synchronisation.  A third aggregate call under ZK_VERIFY_AGG_TIMING gives the library's
own split (it synchronises after every phase, so its parts add up to a little more than the plain call): checks, scalar products,
lines and Miller loops, product, sums (weights, input sums, the two multi-scalar sums), tail ([s0]alpha, the three-pair Miller
loop, the final exponentiation, the comparison).  One JSON line per (curve, n)."""
import ctypes as C, importlib, json, os, pathlib, sys, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import eigen_zkvm_amd
zk = eigen_zkvm_amd; zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")
import groth16_bench as GB

PHASES = ("checks", "scalar_products", "lines_miller", "product", "sums", "tail")
args = sys.argv[1:]
curves = [a for a in args if a in dev._FR] or list(dev._FR)
sizes = [int(a) for a in args if a.isdigit()] or [1, 64, 4096, 65536]
lib = zk.lib()


def wall(fn):
    zk._check(lib.zk_dev_sync())
    t0 = time.perf_counter(); fn(); zk._check(lib.zk_dev_sync())
    return round((time.perf_counter() - t0) * 1e3, 3)


for tag in curves:
    rb, wit, ni, _nw = GB.make_circuit(dev._FR[tag], 6, n_pub=3)
    pb, vk_json = dev.keygen(tag, rb)
    S = dev.Groth16Setup(tag, rb, pb)
    proofs = [np.array(S.prove(wit, r=11 + k, s=23 + k)[1], np.uint64).reshape(-1) for k in range(4)]
    S.free()
    pub = wit[1:ni].reshape(-1)
    vk = dev.Groth16VerifyingKey(tag, vk_json)
    for n in sizes:
        d_pr = zk.DevArray.from_host(np.concatenate([proofs[i % 4] for i in range(n)]))
        d_pub = zk.DevArray.from_host(np.tile(pub, n))
        d_v = zk.DevArray(max(1, (n + 1) // 2))
        verdict = C.c_int(0)
        per = lambda: zk._check(lib.zk_groth16_verify_batch_dev(vk._h, d_pr.ptr, d_pub.ptr, n, d_v.ptr, None))
        agg = lambda: zk._check(lib.zk_groth16_verify_aggregate_dev(vk._h, d_pr.ptr, d_pub.ptr, n, None, C.byref(verdict), None, None))
        per(); per_ms = wall(per)
        assert np.all(d_v.to_host().view(np.int32)[:n] == dev.ACCEPTED)
        agg(); agg_ms = wall(agg)
        assert verdict.value == dev.ACCEPTED
        os.environ["ZK_VERIFY_AGG_TIMING"] = "1"
        agg()
        del os.environ["ZK_VERIFY_AGG_TIMING"]
        ms = (C.c_double * 6)()
        zk._check(lib.zk_groth16_verify_aggregate_timing(ms))
        print(json.dumps(dict(curve=tag, n=n, per_proof_ms=per_ms, aggregate_ms=agg_ms, speedup=round(per_ms / agg_ms, 2),
                              split_ms={k: round(v, 3) for k, v in zip(PHASES, ms)})), flush=True)
        for d in (d_pr, d_pub, d_v): d.free()
    vk.free()
