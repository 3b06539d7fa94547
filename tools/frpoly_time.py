"""HIP-event times of the scalar-field polynomial layer: python tools/frpoly_time.py CURVE LOG_N [--steps K] [--warmup W]

For one curve (BN128 | BLS12381) and n = 2^LOG_N elements: the prefix product (exclusive, with the vector written), the batch inverse, the
grand product, poly_mul of two polynomials of n coefficients (2n - 1 out), divide_zh_coset over n values with N = n / 2, and in the same run
zk_kzg_<curve>_divide_dev over n coefficients -- the existing scan of the same structure, the one figure these can be read against.
Elements are random Montgomery words below r.  Before an operation is timed its result is checked once against tests/frpoly_ref.py, in
plain Python integers: the running product's total and every 4099th product by the reference's own loop over all n elements; every 4099th
inverse by pow(x, -1, r) and the zero count; the grand product of a vector against its rotation by one (z_i = x_0 / x_i at every 4099th
row, and it must close); the product by a(x) b(x) = c(x) at a random x with the reference's Horner evaluation; every 4099th coset factor from
its definition; y of the division by the same Horner evaluation.
W warm-up calls, then K timed ones, each between two events on the null stream with the device idle before the first: one JSON line with
the median and the [min, max] of every operation in milliseconds."""
import ctypes as C
import importlib, json, pathlib, statistics, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import eigen_zkvm_amd
import frpoly_ref as ref
zk = eigen_zkvm_amd; zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")
fp = importlib.import_module("eigen_zkvm_amd.frpoly")

args = sys.argv[1:]
tag, log_n = args[0], int(args[1])
steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 7
warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 2
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
    """n non-zero values below r, 4 x u64 each: the top word below r's"""
    w = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    top = r >> 192
    w[:, 3] = rng.integers(top // 2, top, size=n, dtype=np.uint64)
    return w.reshape(-1)


def fail(what):
    raise SystemExit("frpoly_time: %s n=2^%d: %s" % (tag, log_n, what))


def elems(d, idx):
    """the field elements at the indices idx of a device vector of Montgomery words"""
    w = d.to_host().reshape(-1, 4)[idx]
    return [x * RINV % r for x in ref.words_ints(w)]


r, cv = dev._FR[tag], dev._NAME[tag]
RINV = pow(1 << 256, -1, r)
n = 1 << log_n
rng = np.random.default_rng(21)
wa, wb = fr_words(rng, r, n), fr_words(rng, r, n)
a = [x * RINV % r for x in ref.words_ints(wa)]                      # the elements the words stand for
b = [x * RINV % r for x in ref.words_ints(wb)]
idx = list(range(0, n, 4099)) + [n - 1]
d_a, d_b = zk.DevArray.from_host(wa), zk.DevArray.from_host(wb)
d_o = zk.DevArray(4 * n); d_c = zk.DevArray(4 * (2 * n - 1)); d_y = zk.DevArray(4)
res = {"curve": tag, "n": n, "steps": steps, "warmup": warmup, "checked": True, "batch_inverse_design": "one inversion per tile"}

# ---- prefix product
want, total = ref.prefix_products(a, r)
_, got_total = fp.prefix_product(d_a, tag, out=d_o)
if got_total != total or elems(d_o, idx) != [want[i] for i in idx]:
    fail("the prefix product differs from the reference")
del want
tot = np.zeros(4, np.uint64)
f = getattr(lib, "zk_fr_%s_prefix_product_dev" % cv)
res["prefix_product"] = measure(lambda: zk._check(f(d_a.ptr, n, 0, d_o.ptr, zk._ptr(tot), None)))
res["prefix_total_only"] = measure(lambda: zk._check(f(d_a.ptr, n, 0, None, zk._ptr(tot), None)))

# ---- batch inverse
_, nz, first = fp.batch_inverse(d_a, tag, out=d_o)
if (nz, first) != (0, None) or elems(d_o, idx) != ref.inverses([a[i] for i in idx], r)[0]:
    fail("the batch inverse differs from the reference")
f = getattr(lib, "zk_fr_%s_batch_inverse_dev" % cv)
c0, c1 = C.c_uint64(0), C.c_uint64(0)
res["batch_inverse"] = measure(lambda: zk._check(f(d_a.ptr, n, d_o.ptr, C.byref(c0), C.byref(c1), None)))

# ---- grand product: a against its rotation by one, z_i = a_0 / a_i
d_rot = zk.DevArray.from_host(np.concatenate([wa[4:], wa[:4]]))
_, last = fp.grand_product(d_a, d_rot, tag, out=d_o)
inv_s = ref.inverses([a[i] for i in idx], r)[0]
if last != 1 or elems(d_o, idx) != [a[0] * v % r for v in inv_s]:
    fail("the grand product differs from the reference")
f = getattr(lib, "zk_fr_%s_grand_product_dev" % cv)
res["grand_product"] = measure(lambda: zk._check(f(d_a.ptr, d_rot.ptr, n, d_o.ptr, zk._ptr(tot), None)))
d_rot.free()

# ---- poly_mul, n x n coefficients
f = getattr(lib, "zk_fr_%s_poly_mul_dev" % cv)
zk._check(f(d_a.ptr, n, d_b.ptr, n, d_c.ptr, None))
x = 0xFEDCBA9876543210FEDCBA9876543211 % r
cw = ref.words_ints(d_c.to_host())                                  # the words spell c_i R: Horner is linear, so R comes out at the end
if ref.poly_eval(cw, x, r) * RINV % r != ref.poly_eval(a, x, r) * ref.poly_eval(b, x, r) % r:
    fail("poly_mul: c(x) is not a(x) b(x)")
del cw
res["poly_mul"] = measure(lambda: zk._check(f(d_a.ptr, n, d_b.ptr, n, d_c.ptr, None)))
res["poly_mul_out"] = 2 * n - 1

# ---- divide_zh_coset, m = n, N = n / 2
zk._check(lib.zk_dev_upload(d_o.ptr, zk._ptr(wa), n * 32))
fp.divide_zh_coset(d_o, log_n, log_n - 1, tag)
w_m, g = ref.root_of_unity(tag, log_n), pow(7, n // 2, r)
if elems(d_o, idx) != [a[i] * pow((g * pow(w_m, i * (n // 2), r) - 1) % r, -1, r) % r for i in idx]:
    fail("divide_zh_coset differs from the definition")
f = getattr(lib, "zk_fr_%s_divide_zh_coset_dev" % cv)
res["divide_zh_coset"] = measure(lambda: zk._check(f(d_o.ptr, log_n, log_n - 1, None)))

# ---- the existing division by X - z over the same coefficients
zv = 0x1234567890ABCDEF1234567890ABCDEF % r
z = np.frombuffer(zv.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
f = getattr(lib, "zk_kzg_%s_divide_dev" % cv)
zk._check(f(d_a.ptr, n, zk._ptr(z), d_o.ptr, d_y.ptr, None))
if int.from_bytes(d_y.to_host().astype("<u8").tobytes()[:32], "little") != ref.poly_eval(a, zv, r):
    fail("kzg divide: y is not p(z)")
res["kzg_divide"] = measure(lambda: zk._check(f(d_a.ptr, n, zk._ptr(z), d_o.ptr, d_y.ptr, None)))
print(json.dumps(res), flush=True)
for d in (d_a, d_b, d_o, d_c, d_y):
    d.free()
