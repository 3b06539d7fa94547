// Test hooks for the field operations that have no entry point of their own: the NTT passes' twiddle product (gl::mul_tw, gl::mul_tw_nc)
// applied to operand pairs from the host, and the shift twiddle gl::mul_pow2<E> for every exponent (tests/test_gpu_ntt_lean.py); the
// passes' multiply-add forms gl::add_m, gl::sub_m, gl::mad_eps_m beside gl::sub and gl::add_nc (tests/test_gpu_ntt_issue_slots.py); every
// paired forms of the passes' sums, differences, products and shifts on two slots of operands (tests/test_gpu_ntt_pairs.py); every
// other primitive of gl.hip.h, the carry-free accumulators of acc6.hip.h and the matrix-pipe product of gl_mfma.hip.h on operands from
// the host (tests/test_gpu_field_ops.py).  Not part of include/zkgpu.h; the tests bind them by name.  Every probe writes what the
// primitive returned, unreduced.
#include "zk_internal.h"
#include "ntt_reg.hip.h"
#include "acc6.hip.h"
#include "gl_mfma.hip.h"
#include "poseidon_gl_constants.h"

namespace zk {
namespace {

__device__ __forceinline__ u64 canon(u64 v) { return v >= GL_P ? v - GL_P : v; }

// out[0][i] = mul_tw(a, b); out[1][i] = mul_tw_nc(a, b), canonicalised once; out[2][i] = mul_tw(mul_tw_nc(a, b), mul_tw_nc(b, b)):
// non-canonical products as the operands of a further product
__global__ void twmul_probe_kernel(const u64* __restrict__ a, const u64* __restrict__ b, u64* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 x = a[i], w = b[i];
    out[i] = gl::mul_tw(x, w);
    const u64 nc = gl::mul_tw_nc(x, w);
    out[n + i] = canon(nc);
    out[2 * n + i] = gl::mul_tw(nc, gl::mul_tw_nc(w, w));
}

// out[E][i] = x[i] * 2^E for every 0 <= E < 96 (canonical x)
__global__ void pow2_probe_kernel(const u64* __restrict__ x, u64* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 v = x[i];
    static_for<0, 96>([&](auto EI) { constexpr int E = decltype(EI)::value; out[(u64)E * n + i] = gl::mul_pow2<E>(v); });
}

// One row of n results per primitive, in this order (tests/test_gpu_field_ops.py names the rows the same way).  add, sub and neg are
// defined on canonical operands: they get a mod p, b mod p.  add_nc's second operand must be canonical: b mod p.  Everything else takes
// the words as they come.
constexpr int SCALAR_ROWS = 17;
__global__ void scalar_probe_kernel(const u64* __restrict__ pa, const u64* __restrict__ pb, const u64* __restrict__ pc, u64* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 a = pa[i], b = pb[i], c = pc[i], ca = canon(a), cb = canon(b);
    u64* __restrict__ o = out + i;
    o[0 * n] = gl::add(ca, cb);
    o[1 * n] = gl::sub(ca, cb);
    o[2 * n] = gl::neg(ca);
    o[3 * n] = gl::mul(a, b);
    o[4 * n] = gl::mul_add(a, b, c);
    o[5 * n] = gl::sqr(a);
    o[6 * n] = gl::inv(a);
    o[7 * n] = gl::pow(a, b);
    o[8 * n] = gl::reduce128(a, b);                                  // a + 2^64 b
    o[9 * n] = gl::mul_nc(a, b);
    o[10 * n] = gl::sqr_nc(a);
    o[11 * n] = gl::mul_add_nc(a, b, c);
    o[12 * n] = gl::add_nc(a, cb);
    o[13 * n] = gl::add_word(a, (u32)b);                             // a + (u32)b mod 2^64: an addition of words, not of field elements
    o[14 * n] = gl::mad_eps_nc((u32)b, a);                           // a + (u32)b (2^32 - 1)
    const u64 x2 = gl::sqr_nc(a), x3 = gl::mul_nc(x2, a), x6 = gl::sqr_nc(x3);
    o[15 * n] = gl::mul_nc(x6, a);                                   // pow7 of poseidon.hip: a^7
    o[16 * n] = gl::mul_add_nc(gl::mul_nc(a, b), gl::sqr_nc(c), gl::add_nc(gl::mul_nc(a, c), cb));   // a b c^2 + a c + b
}

// The NTT passes' own forms (gl::add_m, gl::sub_m, gl::mad_eps_m) beside the ones they stand in for, and a non-canonical sum as the
// operand of a twiddle product.  Rows of n: add_m(a mod p, b mod p), sub_m(same), sub(same), add_nc(a, b mod p) as returned,
// mul_tw(add_nc(a, b mod p), w), mad_eps_m((u32)w, a) = a + (u32)w (2^32 - 1) mod p, mul_tw(a, w)   (tests/test_gpu_ntt_issue_slots.py)
constexpr int NTT_ARITH_ROWS = 7;
__global__ void ntt_arith_probe_kernel(const u64* __restrict__ pa, const u64* __restrict__ pb, const u64* __restrict__ pw, u64* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 a = pa[i], w = pw[i], ca = canon(a), cb = canon(pb[i]);
    u64* __restrict__ o = out + i;
    o[0 * n] = gl::add_m(ca, cb);
    o[1 * n] = gl::sub_m(ca, cb);
    o[2 * n] = gl::sub(ca, cb);
    const u64 s = gl::add_nc(a, cb);
    o[3 * n] = s;
    o[4 * n] = gl::mul_tw(s, w);
    o[5 * n] = gl::mad_eps_m((u32)w, a);
    o[6 * n] = gl::mul_tw(a, w);
}

// The paired forms of the NTT passes (gl::bfly_m, gl::bfly2_m, gl::sub2_m, gl::mul_tw2, gl::mul_tw2_nc, gl::mul_tw2_m_nc, gl::mad_eps2_m,
// gl::mul_pow2_2) on two slots of operands, (p0, q0) and (p1, q1), as returned.  The sums, differences and shifts get the operands
// mod p.  Rows of n: 0-1 bfly_m of slot 0 (sum, difference); 2-5 bfly2_m (sum, difference of slot 0, then of slot 1); 6-7 sub2_m;
// 8-9 mul_tw2; 10-11 mul_tw2_nc; 12-13 mul_tw2_m_nc; 14-15 mad_eps2_m((u32)q, p); then for every E < 96 the rows 16 + 4 E ... + 3:
// mul_pow2_2<E, E>(p0, p1) and mul_pow2_2<E, 95 - E>(p0, p1)   (tests/test_gpu_ntt_pairs.py)
constexpr int NTT_PAIR_ROWS = 16 + 4 * 96;
__global__ void ntt_pair_probe_kernel(const u64* __restrict__ pp0, const u64* __restrict__ pq0, const u64* __restrict__ pp1, const u64* __restrict__ pq1,
                                      u64* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 p0 = pp0[i], q0 = pq0[i], p1 = pp1[i], q1 = pq1[i], a = canon(p0), b = canon(q0), c = canon(p1), d = canon(q1);
    u64* __restrict__ o = out + i;
    gl::bfly_m(a, b, o[0 * n], o[1 * n]);
    gl::bfly2_m(a, b, c, d, o[2 * n], o[3 * n], o[4 * n], o[5 * n]);
    gl::sub2_m(a, b, c, d, o[6 * n], o[7 * n]);
    gl::mul_tw2(p0, q0, p1, q1, o[8 * n], o[9 * n]);
    gl::mul_tw2_nc(p0, q0, p1, q1, o[10 * n], o[11 * n]);
    gl::mul_tw2_m_nc(p0, q0, p1, q1, o[12 * n], o[13 * n]);
    gl::mad_eps2_m((u32)q0, p0, (u32)q1, p1, o[14 * n], o[15 * n]);
    static_for<0, 96>([&](auto EI) {
        constexpr int E = decltype(EI)::value;
        gl::mul_pow2_2<E, E>(a, c, o[(u64)(16 + 4 * E) * n], o[(u64)(17 + 4 * E) * n]);
        gl::mul_pow2_2<E, 95 - E>(a, c, o[(u64)(18 + 4 * E) * n], o[(u64)(19 + 4 * E) * n]);
    });
}

// rows of 3 n words: f3_add(x, y), f3_sub(x, y), f3_mul(x, y), f3_muls(x, s), f3_inv(x); x, y canonical, s any u64
__global__ void f3_probe_kernel(const u64* __restrict__ px, const u64* __restrict__ py, const u64* __restrict__ ps, u64* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const gl::f3 x{{px[3 * i], px[3 * i + 1], px[3 * i + 2]}}, y{{py[3 * i], py[3 * i + 1], py[3 * i + 2]}};
    const gl::f3 r[5] = {gl::f3_add(x, y), gl::f3_sub(x, y), gl::f3_mul(x, y), gl::f3_muls(x, ps[i]), gl::f3_inv(x)};
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[(u64)k * 3 * n + 3 * i + j] = r[k].v[j];
}

// out[lane] = acc_finish of start[lane] (acc_word; acc_zero without a start) + sum_j c[lane][j] x[lane][j], j < n <= 512.
// c: split constants, two words each (acc_split)
__global__ void acc6_probe_kernel(const u64* __restrict__ c, const u64* __restrict__ x, const u64* __restrict__ start, u64* __restrict__ out, u64 lanes, u32 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lanes) return;
    Acc6 A;
    if (start) acc_word(A, start[i]); else acc_zero(A);
#pragma unroll 4
    for (u32 j = 0; j < n; ++j) {
        const u64 w = x[i * n + j];
        acc_mac(A, c + 2 * (i * n + j), (u32)w, (u32)(w >> 32));
    }
    out[i] = acc_finish(A);
}

// Whole waves, one 12-word vector per lane: out[v][o] = product<3>, out[n_vec + v][o] = product_add<3> with the lane's own addends
// (product folds its byte columns with pmfma::recombine, product_add with pmfma::recombine_add)
template <int N_IN>
__global__ __launch_bounds__(256) void mfma_probe_kernel(const u64* __restrict__ tab, const u64* __restrict__ x, const u64* __restrict__ ad, u64* __restrict__ out, u64 n_vec) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // n_vec is a multiple of the block: every lane of every wave is here
    u64 st[12], a[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) { st[j] = x[12 * v + j]; a[j] = ad[12 * v + j]; }
    pmfma::BOps B;
    pmfma::make_b<N_IN>(B, [&](int j) { return st[j]; });
    pmfma::product<3>(B, tab, [&](int o, u64 r) { out[12 * v + o] = r; });
    pmfma::product_add<3>(B, tab, [&](int o) { return a[o]; }, [&](int o, u64 r) { out[12 * (n_vec + v) + o] = r; });
}

}  // namespace
}  // namespace zk

// a, b: n host words each (any u64); out: 3 n host words
extern "C" int zk_gl_twmul_probe(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(a && b && out && n > 0 && n <= ((size_t)1 << 24), "zk_gl_twmul_probe: bad arguments");
        DevBuf da, db, dout;
        da.reserve(n * 8); db.reserve(n * 8); dout.reserve(3 * n * 8);
        ZK_HIP(hipMemcpy(da.p, a, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(db.p, b, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(twmul_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, da.u(), db.u(), dout.u(), (u64)n);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, 3 * n * 8, hipMemcpyDeviceToHost));
    });
}

// x: n canonical host words; out: 96 n host words, row E = x * 2^E
extern "C" int zk_gl_pow2_probe(const uint64_t* x, uint64_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(x && out && n > 0 && n <= ((size_t)1 << 20), "zk_gl_pow2_probe: bad arguments");
        DevBuf dx, dout;
        dx.reserve(n * 8); dout.reserve(96 * n * 8);
        ZK_HIP(hipMemcpy(dx.p, x, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(pow2_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dx.u(), dout.u(), (u64)n);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, 96 * n * 8, hipMemcpyDeviceToHost));
    });
}

// a, b, c: n host words each (any u64); out: 17 n host words, one row per primitive (scalar_probe_kernel)
extern "C" int zk_gl_scalar_probe(const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(a && b && c && out && n > 0 && n <= ((size_t)1 << 20), "zk_gl_scalar_probe: bad arguments");
        DevBuf da, db, dc, dout;
        da.reserve(n * 8); db.reserve(n * 8); dc.reserve(n * 8); dout.reserve(SCALAR_ROWS * n * 8);
        ZK_HIP(hipMemcpy(da.p, a, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(db.p, b, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(dc.p, c, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(scalar_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, da.u(), db.u(), dc.u(), dout.u(), (u64)n);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, SCALAR_ROWS * n * 8, hipMemcpyDeviceToHost));
    });
}

// a, b, w: n host words each (any u64); out: 7 n host words, one row per form (ntt_arith_probe_kernel)
extern "C" int zk_gl_ntt_arith_probe(const uint64_t* a, const uint64_t* b, const uint64_t* w, uint64_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(a && b && w && out && n > 0 && n <= ((size_t)1 << 20), "zk_gl_ntt_arith_probe: bad arguments");
        DevBuf da, db, dw, dout;
        da.reserve(n * 8); db.reserve(n * 8); dw.reserve(n * 8); dout.reserve(NTT_ARITH_ROWS * n * 8);
        ZK_HIP(hipMemcpy(da.p, a, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(db.p, b, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(dw.p, w, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ntt_arith_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, da.u(), db.u(), dw.u(), dout.u(), (u64)n);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, NTT_ARITH_ROWS * n * 8, hipMemcpyDeviceToHost));
    });
}

// p0, q0, p1, q1: n host words each (any u64); out: (16 + 4 * 96) n host words, one row per result (ntt_pair_probe_kernel)
extern "C" int zk_gl_ntt_pair_probe(const uint64_t* p0, const uint64_t* q0, const uint64_t* p1, const uint64_t* q1, uint64_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(p0 && q0 && p1 && q1 && out && n > 0 && n <= ((size_t)1 << 16), "zk_gl_ntt_pair_probe: bad arguments");
        DevBuf d0, d1, d2, d3, dout;
        d0.reserve(n * 8); d1.reserve(n * 8); d2.reserve(n * 8); d3.reserve(n * 8); dout.reserve(NTT_PAIR_ROWS * n * 8);
        ZK_HIP(hipMemcpy(d0.p, p0, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(d1.p, q0, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(d2.p, p1, n * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(d3.p, q1, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ntt_pair_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d0.u(), d1.u(), d2.u(), d3.u(), dout.u(), (u64)n);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, NTT_PAIR_ROWS * n * 8, hipMemcpyDeviceToHost));
    });
}

// x, y: 3 n canonical host words; s: n host words (any u64); out: 5 rows of 3 n host words (f3_probe_kernel)
extern "C" int zk_gl_f3_probe(const uint64_t* x, const uint64_t* y, const uint64_t* s, uint64_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(x && y && s && out && n > 0 && n <= ((size_t)1 << 20), "zk_gl_f3_probe: bad arguments");
        DevBuf dx, dy, ds, dout;
        dx.reserve(n * 24); dy.reserve(n * 24); ds.reserve(n * 8); dout.reserve(15 * n * 8);
        ZK_HIP(hipMemcpy(dx.p, x, n * 24, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(dy.p, y, n * 24, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(ds.p, s, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(f3_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dx.u(), dy.u(), ds.u(), dout.u(), (u64)n);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, 15 * n * 8, hipMemcpyDeviceToHost));
    });
}

// consts: lanes * n canonical host words, split here as production splits them (acc_split); words: lanes * n host words (any u64);
// start: lanes host words (any u64) or null; out: lanes host words
extern "C" int zk_gl_acc6_probe(const uint64_t* consts, const uint64_t* words, const uint64_t* start, uint64_t* out, size_t lanes, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(consts && words && out && lanes > 0 && n > 0 && n <= 512 && lanes * n <= ((size_t)1 << 22), "zk_gl_acc6_probe: bad arguments");
        std::vector<u64> split(2 * lanes * n);
        for (size_t i = 0; i < lanes * n; ++i) {
            ZK_REQUIRE(consts[i] < GL_P, "zk_gl_acc6_probe: a constant is not canonical");
            acc_split(consts[i], &split[2 * i]);
        }
        DevBuf dc, dx, ds, dout;
        dc.reserve(lanes * n * 16); dx.reserve(lanes * n * 8); dout.reserve(lanes * 8);
        ZK_HIP(hipMemcpy(dc.p, split.data(), lanes * n * 16, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(dx.p, words, lanes * n * 8, hipMemcpyHostToDevice));
        if (start) { ds.reserve(lanes * 8); ZK_HIP(hipMemcpy(ds.p, start, lanes * 8, hipMemcpyHostToDevice)); }
        hipLaunchKernelGGL(acc6_probe_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, nullptr, (const u64*)dc.u(), (const u64*)dx.u(),
                           (const u64*)(start ? ds.u() : nullptr), dout.u(), (u64)lanes, (u32)n);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, lanes * 8, hipMemcpyDeviceToHost));
    });
}

// coef: n_out * n_in canonical host words, row-major; n_in 11 or 12, n_out <= 12; addend: n_out canonical host words or null (the
// table's own addend); x, lane_add: 12 n_vec host words (any u64; of x the first n_in words of a vector are read); n_vec a multiple
// of 256.  out: 2 * 12 n_vec host words: product<3>, then product_add<3> with lane_add.  Fails if the table does not build or check_tables objects.
extern "C" int zk_gl_mfma_probe(const uint64_t* coef, int n_out, int n_in, const uint64_t* addend, const uint64_t* x, const uint64_t* lane_add,
                                uint64_t* out, size_t n_vec) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(coef && x && lane_add && out && (n_in == 11 || n_in == 12) && n_out >= 1 && n_out <= 12 && n_vec > 0 && n_vec % 256 == 0 && n_vec <= ((size_t)1 << 20),
                   "zk_gl_mfma_probe: bad arguments");
        std::vector<u64> tab(pmfma::TAB_WORDS);
        ZK_REQUIRE(pmfma::build_tables((const u64*)coef, n_out, n_in, (const u64*)addend, tab.data()), "zk_gl_mfma_probe: a digit column exceeds its bound");
        const std::string why = pmfma::check_tables((const u64*)coef, n_out, n_in, (const u64*)addend, tab.data());
        ZK_REQUIRE(why.empty(), "zk_gl_mfma_probe: " + why);
        DevBuf dt, dx, da, dout;
        dt.reserve(tab.size() * 8); dx.reserve(n_vec * 96); da.reserve(n_vec * 96); dout.reserve(2 * n_vec * 96);
        ZK_HIP(hipMemcpy(dt.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(dx.p, x, n_vec * 96, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(da.p, lane_add, n_vec * 96, hipMemcpyHostToDevice));
        const dim3 grid((unsigned)(n_vec / 256));
        if (n_in == 12) hipLaunchKernelGGL(mfma_probe_kernel<12>, grid, dim3(256), 0, nullptr, (const u64*)dt.u(), (const u64*)dx.u(), (const u64*)da.u(), dout.u(), (u64)n_vec);
        else hipLaunchKernelGGL(mfma_probe_kernel<11>, grid, dim3(256), 0, nullptr, (const u64*)dt.u(), (const u64*)dx.u(), (const u64*)da.u(), dout.u(), (u64)n_vec);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpy(out, dout.p, 2 * n_vec * 96, hipMemcpyDeviceToHost));
    });
}

// Host only, no device: whether a coefficient set builds (0) or build_tables refuses it / check_tables objects (-1, zk_last_error says which)
extern "C" int zk_gl_mfma_tables_probe(const uint64_t* coef, int n_out, int n_in, const uint64_t* addend) {
    using namespace zk;
    try {
        ZK_REQUIRE(coef && n_in >= 1 && n_in <= 12 && n_out >= 1 && n_out <= 12, "zk_gl_mfma_tables_probe: bad arguments");
        std::vector<u64> tab(pmfma::TAB_WORDS);
        ZK_REQUIRE(pmfma::build_tables((const u64*)coef, n_out, n_in, (const u64*)addend, tab.data()), "a digit column exceeds its bound");
        const std::string why = pmfma::check_tables((const u64*)coef, n_out, n_in, (const u64*)addend, tab.data());
        ZK_REQUIRE(why.empty(), why);
        return 0;
    } catch (const std::exception& e) { set_error(e.what()); return -1; }
}

// Host only: the pre-sparse matrix P of the permutation as poseidon.hip's full-width product takes it, out[12 o + j] = P[j][o]
extern "C" int zk_gl_poseidon_matrix_probe(uint64_t out[144]) {
    if (!out) return -1;
    for (int o = 0; o < 12; ++o)
        for (int j = 0; j < 12; ++j) out[12 * o + j] = ZK_POSEIDON_P[12 * j + o];
    return 0;
}
