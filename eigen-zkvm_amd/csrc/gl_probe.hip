// Test hooks for the field operations that have no entry point of their own: the NTT passes' twiddle product (gl::mul_tw, gl::mul_tw_nc)
// applied to operand pairs from the host, and the shift twiddle gl::mul_pow2<E> for every exponent.  Not part of include/zkgpu.h;
// tests/test_gpu_ntt_lean.py binds them by name.
#include "zk_internal.h"
#include "ntt_reg.hip.h"

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
