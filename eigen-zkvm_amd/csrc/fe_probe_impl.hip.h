// Body of fe_probe.hip: included once per field inside a namespace that provides fe29_impl.hip.h's parameters and has included
// fe29_impl.hip.h.  One kernel per primitive family; operands and results are raw internal limbs (NR u32 per element, whatever lazy
// representative the host chose), element-major: element i reads in[i * in_words ...] and writes out[i * out_words ...].
// FE_PROBE_NO_WIDE: the field has too many limbs for fe_wide_* (fe29_impl.hip.h) and gets no such rows.  No include guard on purpose.
constexpr int PB = 64;
enum { F_LIN = 0, F_MUL, F_MUL2, F_ACC, F_WIDE, F_PRED, F_INV, F_STD, F_COUNT };

__device__ __forceinline__ fe ld_fe(const u32* __restrict__ p) {
    fe a;
#pragma unroll
    for (int k = 0; k < NR; ++k) a.l[k] = p[k];
    return a;
}
__device__ __forceinline__ void st_fe(u32* __restrict__ p, const fe& a) {
#pragma unroll
    for (int k = 0; k < NR; ++k) p[k] = a.l[k];
}

// (a, b) -> fe_add(a, b), fe_dbl(a), fe_sub<2>(a, b), fe_sub<4>(a, b), fe_sub<8>(a, b)
__global__ __launch_bounds__(PB) void lin_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const fe a = ld_fe(in + i * 2 * NR), b = ld_fe(in + i * 2 * NR + NR);
    u32* o = out + i * 5 * NR;
    st_fe(o, fe_add(a, b)); st_fe(o + NR, fe_dbl(a)); st_fe(o + 2 * NR, fe_sub<2>(a, b)); st_fe(o + 3 * NR, fe_sub<4>(a, b)); st_fe(o + 4 * NR, fe_sub<8>(a, b));
}
// (a, b) -> fe_mul(a, b), the dedicated fe_sqr(a), fe_mul(a, a)
__global__ __launch_bounds__(PB) void mul_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const fe a = ld_fe(in + i * 2 * NR), b = ld_fe(in + i * 2 * NR + NR);
    u32* o = out + i * 3 * NR;
    st_fe(o, fe_mul(a, b)); st_fe(o + NR, fe_sqr(a)); st_fe(o + 2 * NR, fe_mul(a, a));
}
// (a, b, c, d) -> fe_mul2(a, b, c, d)
__global__ __launch_bounds__(PB) void mul2_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const u32* p = in + i * 4 * NR;
    st_fe(out + i * NR, fe_mul2(ld_fe(p), ld_fe(p + NR), ld_fe(p + 2 * NR), ld_fe(p + 3 * NR)));
}
// (a, b, c) -> fe_mul_acc(a, b, c)
__global__ __launch_bounds__(PB) void acc_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const u32* p = in + i * 3 * NR;
    st_fe(out + i * NR, fe_mul_acc(ld_fe(p), ld_fe(p + NR), ld_fe(p + 2 * NR)));
}
#ifndef FE_PROBE_NO_WIDE
// (a_0, b_0, ..., a_5, b_5) -> row m - 1 = fe_wide_reduce of the first m pairs, m = 1 .. FE_WIDE_MAX
__global__ __launch_bounds__(PB) void wide_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const u32* p = in + i * 2 * FE_WIDE_MAX * NR;
    fe_wide acc; fe_wide_zero(acc);
#pragma unroll
    for (int m = 0; m < FE_WIDE_MAX; ++m) {
        fe_wide_mac(acc, ld_fe(p + 2 * m * NR), ld_fe(p + (2 * m + 1) * NR));
        fe_wide w = acc;                                   // fe_wide_reduce consumes its argument
        st_fe(out + (i * FE_WIDE_MAX + m) * NR, fe_wide_reduce(w));
    }
}
#endif
// a -> fe_is_zero_m(a) (one word), fe_canon(a)
__global__ __launch_bounds__(PB) void pred_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const fe a = ld_fe(in + i * NR);
    out[i * (NR + 1)] = fe_is_zero_m(a) ? 1u : 0u;
    st_fe(out + i * (NR + 1) + 1, fe_canon(a));
}
// a -> fe_inv(a)
__global__ __launch_bounds__(PB) void inv_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    st_fe(out + i * NR, fe_inv(ld_fe(in + i * NR)));
}
// (w: NL external words, a) -> fe_from_std(w) (NR limbs), fe_to_std(a), fe_to_std(fe_from_std(w)) (NL words each)
__global__ __launch_bounds__(PB) void std_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const u32* p = in + i * (NL + NR);
    u32 w[NL], v[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) w[k] = p[k];
    const fe x = fe_from_std(w);
    u32* o = out + i * (NR + 2 * NL);
    st_fe(o, x);
    fe_to_std(ld_fe(p + NL), v);
#pragma unroll
    for (int k = 0; k < NL; ++k) o[NR + k] = v[k];
    fe_to_std(x, v);
#pragma unroll
    for (int k = 0; k < NL; ++k) o[NR + NL + k] = v[k];
}

inline void run(int fam, const u32* in, u32* out, size_t n) {
    static const int IN_W[F_COUNT] = {2 * NR, 2 * NR, 4 * NR, 3 * NR, 2 * FE_WIDE_MAX * NR, NR, NR, NL + NR};
    static const int OUT_W[F_COUNT] = {5 * NR, 3 * NR, NR, NR, FE_WIDE_MAX * NR, NR + 1, NR, NR + 2 * NL};
    ZK_REQUIRE(fam >= 0 && fam < F_COUNT, "zk_fe29_probe: no such family");
    DevBuf din, dout;
    din.reserve(n * IN_W[fam] * 4); dout.reserve(n * OUT_W[fam] * 4);
    ZK_HIP(hipMemcpy(din.p, in, n * IN_W[fam] * 4, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((n + PB - 1) / PB)), block(PB);
    const u32* i = (const u32*)din.p; u32* o = (u32*)dout.p;
    switch (fam) {
        case F_LIN: hipLaunchKernelGGL(lin_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case F_MUL: hipLaunchKernelGGL(mul_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case F_MUL2: hipLaunchKernelGGL(mul2_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case F_ACC: hipLaunchKernelGGL(acc_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
#ifndef FE_PROBE_NO_WIDE
        case F_WIDE: hipLaunchKernelGGL(wide_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
#else
        case F_WIDE: throw Error("zk_fe29_probe: fe_wide_* is not defined for this field (too many limbs for its 64-bit columns)");
#endif
        case F_PRED: hipLaunchKernelGGL(pred_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case F_INV: hipLaunchKernelGGL(inv_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        default: hipLaunchKernelGGL(std_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpy(out, dout.p, n * OUT_W[fam] * 4, hipMemcpyDeviceToHost));
}
// host only: NL, NR, QINV29, then NR words each of Q29, ONE29, CIN29, COUT29, RRP29, Q2_29, Q4_29, Q8_29, fe_qm2_limb
inline void consts(u32* out) {
    out[0] = NL; out[1] = NR; out[2] = QINV29;
    for (int k = 0; k < NR; ++k) {
        u32* o = out + 3 + k;
        o[0] = Q29(k); o[NR] = ONE29(k); o[2 * NR] = CIN29(k); o[3 * NR] = COUT29(k); o[4 * NR] = RRP29(k);
        o[5 * NR] = Q2_29(k); o[6 * NR] = Q4_29(k); o[7 * NR] = Q8_29(k); o[8 * NR] = fe_qm2_limb(k);
    }
}
