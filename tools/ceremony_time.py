"""The per-point scalar product, bit walk against endomorphism walk: python tools/ceremony_time.py [BN128|BLS12381 ...] [log_n ...]

For each curve and each n = 2^log_n (default 16 and 20): n distinct G1 points ([a_i]G from the fixed-base kernel) and n full-width
scalars resident on the device; one warm-up call and ONE timed call of zk_g1_<curve>_mul_scalars_dev (ecn_mul_scalars_kernel, the
bit walk) and of zk_g1_<curve>_mul_scalars_glv_dev (ecn_mul_scalars_glv_kernel), each between two HIP events on the stream the
calls run on.  A call is the walk and the shared way out (ecn_store_kernel, one inversion per 256 points), so the difference is
the walks'.  The two outputs are compared byte for byte.  One JSON line per (curve, n).

    python tools/ceremony_time.py ceremony [BN128|BLS12381 ...] [power ...]

times a whole contribution (zk_srs_contribute: file in memory -> device -> file on disk, factors from the operating system) and a
whole check (zk_srs_verify) of a new file of each power (default 16 and 20) in a temporary directory, host wall clock, one call each."""
import ctypes as C, importlib, json, pathlib, sys, tempfile, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import eigen_zkvm_amd
zk = eigen_zkvm_amd; zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")

args = sys.argv[1:]
if args[:1] == ["ceremony"]:
    curves = [a for a in args if a in dev._FR] or list(dev._FR)
    with tempfile.TemporaryDirectory() as d:
        for tag in curves:
            for power in [int(a) for a in args if a.isdigit()] or [16, 20]:
                new, out = pathlib.Path(d) / "new.ptau", pathlib.Path(d) / "out.ptau"
                dev.srs_new(tag, power, new)
                srs = dev.Srs(tag, new)
                t0 = time.perf_counter(); srs.contribute(out); t1 = time.perf_counter()
                srs.free()
                srs = dev.Srs(tag, out)
                t2 = time.perf_counter(); rep = srs.verify(); t3 = time.perf_counter()
                srs.free()
                print(json.dumps(dict(curve=tag, power=power, file_mib=round(out.stat().st_size / 2**20, 1), contribute_s=round(t1 - t0, 3), verify_s=round(t3 - t2, 3),
                                      findings=len(rep["findings"]) + len(rep["file"]["findings"]))), flush=True)
                new.unlink(); out.unlink()
    sys.exit(0)
curves = [a for a in args if a in dev._FR] or list(dev._FR)
logs = [int(a) for a in args if a.isdigit()] or [16, 20]
lib = zk.lib()
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError("hip error %d" % rc)


E0, E1 = C.c_void_p(), C.c_void_p()
hip_ok(hip.hipEventCreate(C.byref(E0))); hip_ok(hip.hipEventCreate(C.byref(E1)))


def event_ms(fn):
    zk._check(lib.zk_dev_sync())
    hip_ok(hip.hipEventRecord(E0, None)); fn(); hip_ok(hip.hipEventRecord(E1, None))
    hip_ok(hip.hipEventSynchronize(E1))
    ms = C.c_float(0)
    hip_ok(hip.hipEventElapsedTime(C.byref(ms), E0, E1))
    return round(ms.value, 3)


def fr_words(rng, r, n):
    """n scalars of full width below r, 4 x u64 each: the top word below r's, so no reduction is needed"""
    w = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    top = r >> 192
    w[:, 3] = rng.integers(top // 2, top, size=n, dtype=np.uint64)
    return w.reshape(-1)


for tag in curves:
    cv, r, pw = dev._NAME[tag], dev._FR[tag], 2 * dev._FQ_WORDS[tag]
    rng = np.random.default_rng(17)
    for log_n in logs:
        n = 1 << log_n
        d_pts = zk.mul_generator_fr(zk.DevArray.from_host(fr_words(rng, r, n)), cv, group="g1")
        d_k = zk.DevArray.from_host(fr_words(rng, r, n))
        outs, ms = {}, {}
        for name in ("mul_scalars", "mul_scalars_glv"):
            fn = getattr(lib, "zk_g1_%s_%s_dev" % (cv, name))
            outs[name] = zk.DevArray(n * pw)
            call = lambda: zk._check(fn(d_pts.ptr, n, d_k.ptr, outs[name].ptr, None))
            call(); ms[name] = event_ms(call)
        same = outs["mul_scalars"].to_host().tobytes() == outs["mul_scalars_glv"].to_host().tobytes()
        print(json.dumps(dict(curve=tag, log_n=log_n, bit_walk_ms=ms["mul_scalars"], glv_walk_ms=ms["mul_scalars_glv"],
                              speedup=round(ms["mul_scalars"] / ms["mul_scalars_glv"], 2), same_bytes=same)), flush=True)
        assert same
        for d in (d_pts, d_k, outs["mul_scalars"], outs["mul_scalars_glv"]): d.free()
