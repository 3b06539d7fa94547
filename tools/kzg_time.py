"""HIP-event times of the KZG layer: python tools/kzg_time.py [BN128|BLS12381 ...] [--steps K] [--warmup W] [--no-big]

For each curve: divide (zk_kzg_<curve>_divide_dev with q), eval (the same without q), commit and open (zk_kzg_commit_dev, zk_kzg_open_dev over
a handle) and, in the same run, the existing multi-scalar sum of the same length over the same points (zk_msm_g1_<curve>_dev) at n = 2^16,
2^20 and 2^21 - 1, the largest a file of power 20 holds; then divide alone at 2^24 (--no-big skips it).  The file is made here from a known
tau as tools/make_test_ptau.py makes it (timing only: such a file is worthless as a setup), except that nothing reads its alphaTauG1 and
betaTauG1 sections or tauG2 beyond [1], so those stay zero and the file is not checked.  Coefficients are random words below r.
Before a length is timed its results are checked once, so that no table comes from wrong results: y of divide against y of eval, q by
p(x) = q(x) (x - z) + y at a second point x (both sides by the evaluation, which never runs the fix-up that wrote q), and the opening
(commit, z, y, W) by the handle's pairing check.
W warm-up calls, then K timed ones, each between two events on the null stream with the device idle before the first: one JSON line per
(curve, n) with the median and the [min, max] of every operation in milliseconds, and divide / msm of the medians."""
import ctypes as C
import importlib, json, pathlib, statistics, sys, tempfile
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import eigen_zkvm_amd
import make_test_ptau as MP
zk = eigen_zkvm_amd; zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")
kzg = importlib.import_module("eigen_zkvm_amd.kzg")

args = sys.argv[1:]
curves = [a for a in args if a in MP.CURVES] or list(MP.CURVES)
steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 7
warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 2
POWER = 20
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
    return ms.value


def measure(fn):
    for _ in range(warmup):
        fn()
    t = sorted(event_ms(fn) for _ in range(steps))
    return {"median": round(statistics.median(t), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def fr_words(rng, r, n):
    """n values below r, 4 x u64 each: the top word below r's"""
    w = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    top = r >> 192
    w[:, 3] = rng.integers(top // 2, top, size=n, dtype=np.uint64)
    return w.reshape(-1)


def sparse_ptau(tag, tau):
    """the container of a power-20 file whose tauG1 and tauG2[0..1] are real and whose other points are zero"""
    c = MP.CURVES[tag]; r = c["r"]; n = 1 << POWER
    pw = [1]
    for _ in range(2 * n - 2):
        pw.append(pw[-1] * tau % r)
    k = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in pw), dtype="<u8").astype(np.uint64)
    g1 = zk.mul_generator_fr(zk.DevArray.from_host(k), c["abi"], group="g1").to_host().astype("<u8").tobytes()
    g2 = zk.mul_generator_fr(zk.DevArray.from_host(k[:8]), c["abi"], group="g2").to_host().astype("<u8").tobytes()
    b1, b2 = 2 * c["n8"], 4 * c["n8"]
    g1, g2 = g1[:(2 * n - 1) * b1], g2[:2 * b2]
    return MP.container(tag, POWER, {2: g1, 3: g2 + bytes((n - 2) * b2), 4: bytes(n * b1), 5: bytes(n * b1), 6: bytes(b2)}), g1


def words(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def value(d):
    return int.from_bytes(d.to_host().astype("<u8").tobytes()[:32], "little")


def check_results(tag, divide, h, d_c, n, zv, d_q, d_y, with_open):
    """one division (and opening) of n coefficients, checked as the module text says; raises on a difference"""
    r = dev._FR[tag]
    z, xv = words(zv), 0xFEDCBA9876543210FEDCBA9876543211 % r
    zk._check(divide(d_c.ptr, n, zk._ptr(z), d_q.ptr, d_y.ptr, None)); y = value(d_y)
    zk._check(divide(d_c.ptr, n, zk._ptr(z), None, d_y.ptr, None))
    if value(d_y) != y:
        raise SystemExit("kzg_time: %s n=%d: divide and eval disagree on y" % (tag, n))
    zk._check(divide(d_c.ptr, n, zk._ptr(words(xv)), None, d_y.ptr, None)); px = value(d_y)
    zk._check(divide(d_q.ptr, n - 1, zk._ptr(words(xv)), None, d_y.ptr, None)); qx = value(d_y)
    if (qx * (xv - zv) + y - px) % r:
        raise SystemExit("kzg_time: %s n=%d: q is not (p - y) / (X - z)" % (tag, n))
    if with_open:
        d_p = zk.DevArray(h.point_bytes // 8 + 1, zero=True)
        zk._check(lib.zk_kzg_commit_dev(h._h, d_c.ptr, n, d_p.ptr, None)); c = h._point(d_p)
        zk._check(lib.zk_kzg_open_dev(h._h, d_c.ptr, n, zk._ptr(z), d_y.ptr, d_p.ptr, None)); w = h._point(d_p)
        d_p.free()
        if value(d_y) != y or h.verify([(c, zv, y, w)])[0] != 1:
            raise SystemExit("kzg_time: %s n=%d: the opening does not verify" % (tag, n))


for tag in curves:
    cv, r = dev._NAME[tag], dev._FR[tag]
    rng = np.random.default_rng(18)
    zv = 0x1234567890ABCDEF1234567890ABCDEF % r
    z = words(zv)
    divide = getattr(lib, "zk_kzg_%s_divide_dev" % cv); msm = getattr(lib, "zk_msm_g1_%s_dev" % cv)
    with tempfile.TemporaryDirectory() as d:
        p = pathlib.Path(d) / "t.ptau"
        blob, g1 = sparse_ptau(tag, 0x5DEECE66D1234567 % r)
        p.write_bytes(blob); del blob
        srs = dev.Srs(tag, p)
        h = kzg.Kzg(srs)
        srs.free()
    d_bases = zk.DevArray.from_host(np.frombuffer(g1, dtype="<u8").astype(np.uint64)); del g1
    n_max = (2 << POWER) - 1
    d_c = zk.DevArray.from_host(fr_words(rng, r, n_max)); d_s = zk.DevArray.from_host(fr_words(rng, r, n_max))
    d_q = zk.DevArray(4 * n_max); d_y = zk.DevArray(4); d_out = zk.DevArray(h.point_bytes // 8 + 1); d_w = zk.DevArray(h.point_bytes // 8 + 1)
    for n in (1 << 16, 1 << 20, n_max):
        check_results(tag, divide, h, d_c, n, zv, d_q, d_y, True)
        res = {"curve": tag, "n": n, "steps": steps, "warmup": warmup, "checked": True}
        res["divide"] = measure(lambda: zk._check(divide(d_c.ptr, n, zk._ptr(z), d_q.ptr, d_y.ptr, None)))
        res["eval"] = measure(lambda: zk._check(divide(d_c.ptr, n, zk._ptr(z), None, d_y.ptr, None)))
        res["commit"] = measure(lambda: zk._check(lib.zk_kzg_commit_dev(h._h, d_c.ptr, n, d_out.ptr, None)))
        res["open"] = measure(lambda: zk._check(lib.zk_kzg_open_dev(h._h, d_c.ptr, n, zk._ptr(z), d_y.ptr, d_w.ptr, None)))
        res["msm"] = measure(lambda: zk._check(msm(d_bases.ptr, d_s.ptr, n, d_out.ptr, None)))
        res["divide_over_msm"] = round(res["divide"]["median"] / res["msm"]["median"], 4)
        print(json.dumps(res), flush=True)
    for a in (d_bases, d_c, d_s, d_q, d_out, d_w):
        a.free()
    h.free()
    if "--no-big" not in args:
        n = 1 << 24
        d_c = zk.DevArray.from_host(fr_words(rng, r, n)); d_q = zk.DevArray(4 * n)
        check_results(tag, divide, None, d_c, n, zv, d_q, d_y, False)
        res = {"curve": tag, "n": n, "steps": steps, "warmup": warmup, "checked": True}
        res["divide"] = measure(lambda: zk._check(divide(d_c.ptr, n, zk._ptr(z), d_q.ptr, d_y.ptr, None)))
        res["eval"] = measure(lambda: zk._check(divide(d_c.ptr, n, zk._ptr(z), None, d_y.ptr, None)))
        print(json.dumps(res), flush=True)
        d_c.free(); d_q.free()
    d_y.free()
