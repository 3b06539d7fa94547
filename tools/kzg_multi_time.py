"""HIP-event times of the openings at several points: python tools/kzg_multi_time.py [BN128|BLS12381 ...] [--steps K] [--warmup W]

For each curve, at n = 2^21 - 1 coefficients (the largest a file of power 20 holds), two shapes: 4 polynomials on the same 2 points {x, w x},
and 1 polynomial on 8 points.  Per shape, in the same run:
  multi     zk_kzg_multi_begin (evaluate), zk_kzg_multi_quotient, zk_kzg_multi_finish, each stage between its own pair of events
  composed  the same work from the single-point calls alone: evaluate = one zk_kzg_<curve>_divide_dev without q per (polynomial, point);
            quotient = one divide with q per (polynomial, point) into a buffer of its own, zk_kzg_<curve>_lincomb_dev over those buffers,
            zk_kzg_commit_dev of the result; finish = lincomb over the polynomials and q, zk_kzg_open_dev of the result at z.  lincomb takes the
            powers of ONE gamma, not the weights the protocol needs, so the composed numbers are stand-ins: the same launches, traffic and
            products, not a valid proof
  sum       zk_kzg_commit_dev of n coefficients, the plain sum every one of these ends in
The file is made from a known tau as tools/kzg_time.py makes it (timing only).  Before a shape is timed its proof is made once through
Kzg.open_multi and checked by Kzg.verify_multi, so no row comes from wrong results.  W warm-up rounds, then K timed ones, each operation
between two events on the null stream with the device idle before the first: one JSON line per (curve, shape) with the median and
[min, max] in milliseconds."""
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


def summary(t):
    t = sorted(t)
    return {"median": round(statistics.median(t), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def measure(fn):
    for _ in range(warmup):
        fn()
    return summary(event_ms(fn) for _ in range(steps))


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
    return MP.container(tag, POWER, {2: g1, 3: g2 + bytes((n - 2) * b2), 4: bytes(n * b1), 5: bytes(n * b1), 6: bytes(b2)})


def words(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def multi_rounds(h, polys, n, sets, gamma, z):
    """warm-up + timed rounds of the three stages over one handle each -> the three summaries"""
    k = len(polys)
    flat = [p for s in sets for p in s]
    pts = np.concatenate([words(p) for p in flat]); sizes = np.array([len(s) for s in sets], dtype=np.uint32)
    ptrs = np.array([d.ptr for d in polys], dtype=np.uint64); lens = np.array([n] * k, dtype=np.uint64)
    d_vals = zk.DevArray(4 * len(flat)); d_w = zk.DevArray(h.point_bytes // 8 + 1)
    g, zw = words(gamma), words(z)
    t = {"evaluate": [], "quotient": [], "finish": []}
    for it in range(warmup + steps):
        m = [None]

        def begin():
            m[0] = lib.zk_kzg_multi_begin(h._h, zk._ptr(ptrs), zk._ptr(lens), k, zk._ptr(pts), sizes.ctypes.data, d_vals.ptr, None)
            if not m[0]:
                raise SystemExit("kzg_multi_time: " + lib.zk_last_error().decode())
        ms = [event_ms(begin),
              event_ms(lambda: zk._check(lib.zk_kzg_multi_quotient(m[0], zk._ptr(g), d_w.ptr, None))),
              event_ms(lambda: zk._check(lib.zk_kzg_multi_finish(m[0], zk._ptr(zw), d_w.ptr, None)))]
        zk._check(lib.zk_kzg_multi_free(m[0]))
        if it >= warmup:
            for key, v in zip(t, ms):
                t[key].append(v)
    d_vals.free(); d_w.free()
    return {key: summary(v) for key, v in t.items()}


def composed(tag, h, polys, n, sets, gamma, z, bufs, d_f):
    """the single-point calls alone; bufs: one quotient buffer per (polynomial, point), d_f: the combination"""
    cv = dev._NAME[tag]
    divide = getattr(lib, "zk_kzg_%s_divide_dev" % cv); lincomb = getattr(lib, "zk_kzg_%s_lincomb_dev" % cv)
    pairs = [(d, words(p)) for d, s in zip(polys, sets) for p in s]
    d_y = zk.DevArray(4); d_w = zk.DevArray(h.point_bytes // 8 + 1)
    g, zw = words(gamma), words(z)
    q_ptrs = np.array([b.ptr for b in bufs[:len(pairs)]], dtype=np.uint64); q_lens = np.array([n - 1] * len(pairs), dtype=np.uint64)
    l_ptrs = np.array([d.ptr for d in polys] + [d_f.ptr], dtype=np.uint64); l_lens = np.array([n] * len(polys) + [n - 1], dtype=np.uint64)
    d_l = bufs[-1]

    def evaluate():
        for d, p in pairs:
            zk._check(divide(d.ptr, n, zk._ptr(p), None, d_y.ptr, None))

    def quotient():
        for (d, p), b in zip(pairs, bufs):
            zk._check(divide(d.ptr, n, zk._ptr(p), b.ptr, d_y.ptr, None))
        zk._check(lincomb(zk._ptr(q_ptrs), zk._ptr(q_lens), len(pairs), zk._ptr(g), d_f.ptr, None))
        zk._check(lib.zk_kzg_commit_dev(h._h, d_f.ptr, n - 1, d_w.ptr, None))

    def finish():
        zk._check(lincomb(zk._ptr(l_ptrs), zk._ptr(l_lens), len(polys) + 1, zk._ptr(g), d_l.ptr, None))
        zk._check(lib.zk_kzg_open_dev(h._h, d_l.ptr, n, zk._ptr(zw), d_y.ptr, d_w.ptr, None))
    out = {"evaluate": measure(evaluate), "quotient": measure(quotient), "finish": measure(finish)}
    d_y.free(); d_w.free()
    return out


for tag in curves:
    r = dev._FR[tag]
    rng = np.random.default_rng(19)
    with tempfile.TemporaryDirectory() as d:
        p = pathlib.Path(d) / "t.ptau"
        p.write_bytes(sparse_ptau(tag, 0x5DEECE66D1234567 % r))
        srs = dev.Srs(tag, p)
        h = kzg.Kzg(srs)
        srs.free()
    n = (2 << POWER) - 1
    polys = [zk.DevArray.from_host(fr_words(rng, r, n)) for _ in range(4)]
    bufs = [zk.DevArray(4 * n) for _ in range(9)]                           # up to 8 quotients, and the combination that is opened
    d_f = zk.DevArray(4 * n); d_out = zk.DevArray(h.point_bytes // 8 + 1)
    x = 0x1234567890ABCDEF1234567890ABCDEF % r
    w = pow(7, (r - 1) >> 3, r)                                             # a primitive 8th root of unity
    gamma, z = 0xFEDCBA9876543210FEDCBA9876543211 % r, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % r
    sum_ms = measure(lambda: zk._check(lib.zk_kzg_commit_dev(h._h, polys[0].ptr, n, d_out.ptr, None)))
    for name, ps, sets in (("4 polynomials x 2 points", polys, [[x, x * w % r]] * 4), ("1 polynomial x 8 points", polys[:1], [[x * pow(w, j, r) % r for j in range(8)]])):
        cs = [h.commit(d) for d in ps]
        values, W1, W2, g, zz = h.open_multi(ps, sets, commitments=cs, gamma=gamma, z=z)
        if h.verify_multi([(cs, sets, values, g, zz, W1, W2)])[0] != 1:
            raise SystemExit("kzg_multi_time: %s, %s: the proof does not verify" % (tag, name))
        res = {"curve": tag, "shape": name, "n": n, "steps": steps, "warmup": warmup, "checked": True, "sum": sum_ms}
        res["multi"] = multi_rounds(h, ps, n, sets, gamma, z)
        res["composed"] = composed(tag, h, ps, n, sets, gamma, z, bufs, d_f)
        for part in ("multi", "composed"):
            res[part]["total"] = round(sum(res[part][s]["median"] for s in ("evaluate", "quotient", "finish")), 3)
        res["multi_over_composed"] = round(res["multi"]["total"] / res["composed"]["total"], 4)
        print(json.dumps(res), flush=True)
    for a in polys + bufs + [d_f, d_out]:
        a.free()
    h.free()
