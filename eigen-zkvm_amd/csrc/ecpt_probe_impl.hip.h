// Body of ecpt_probe.hip: included once per (curve, group) inside a namespace that has included ecpt_impl.hip.h.  One kernel per
// primitive (code size: see msm.hip), the point formulas stay the out-of-line functions ecpt_impl.hip.h makes them.  A coordinate is
// CW_INT raw internal limbs (Fq2: c0 then c1), a point X, Y, ZZ, ZZZ, an affine point x, y; element-major like fe_probe_impl.hip.h.
// No include guard on purpose.
constexpr int PB = 64, PW = 4 * CW_INT, AW = 2 * CW_INT;
enum { E_CFMUL = 0, E_CFSQR, E_CFINV, E_RENORM, E_DBL_AFF, E_DBL, E_MADD, E_ADD, E_NEG, E_TO_STD, E_DBL4, E_ADD4, E_COUNT };

__device__ __forceinline__ xyzz ld_pt(const u32* __restrict__ p) {
    xyzz r;
    r.X = cf_load_int(p); r.Y = cf_load_int(p + CW_INT); r.ZZ = cf_load_int(p + 2 * CW_INT); r.ZZZ = cf_load_int(p + 3 * CW_INT);
    return r;
}
__device__ __forceinline__ void st_pt(u32* __restrict__ p, const xyzz& r) {
    cf_store_int(r.X, p); cf_store_int(r.Y, p + CW_INT); cf_store_int(r.ZZ, p + 2 * CW_INT); cf_store_int(r.ZZZ, p + 3 * CW_INT);
}
__device__ __forceinline__ aff ld_aff(const u32* __restrict__ p) {
    aff a;
    a.x = cf_load_int(p); a.y = cf_load_int(p + CW_INT);
    return a;
}

__global__ __launch_bounds__(PB) void cfmul_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    cf_store_int(cf_mul(cf_load_int(in + i * 2 * CW_INT), cf_load_int(in + i * 2 * CW_INT + CW_INT)), out + i * CW_INT);
}
__global__ __launch_bounds__(PB) void cfsqr_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    cf_store_int(cf_sqr(cf_load_int(in + i * CW_INT)), out + i * CW_INT);
}
__global__ __launch_bounds__(PB) void cfinv_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    cf_store_int(cf_inv(cf_load_int(in + i * CW_INT)), out + i * CW_INT);
}
#ifdef MSM_G2
__global__ __launch_bounds__(PB) void renorm_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // one Fq element
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    fe a;
#pragma unroll
    for (int k = 0; k < NR; ++k) a.l[k] = in[i * NR + k];
    const fe r = fe_renorm(a);
#pragma unroll
    for (int k = 0; k < NR; ++k) out[i * NR + k] = r.l[k];
}
#endif
__global__ __launch_bounds__(PB) void dbl_aff_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    st_pt(out + i * PW, pt_dbl_aff(ld_aff(in + i * AW)));
}
__global__ __launch_bounds__(PB) void dbl_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    st_pt(out + i * PW, pt_dbl(ld_pt(in + i * PW)));
}
__global__ __launch_bounds__(PB) void madd_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // (point, affine point)
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    st_pt(out + i * PW, pt_madd(ld_pt(in + i * (PW + AW)), ld_aff(in + i * (PW + AW) + PW)));
}
__global__ __launch_bounds__(PB) void add_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    st_pt(out + i * PW, pt_add(ld_pt(in + i * 2 * PW), ld_pt(in + i * 2 * PW + PW)));
}
__global__ __launch_bounds__(PB) void neg_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    st_pt(out + i * PW, pt_neg(ld_pt(in + i * PW)));
}
__global__ __launch_bounds__(PB) void to_std_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // a finite point -> x, y (external words)
    const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    pt_to_std(ld_pt(in + i * PW), out + i * 2 * CW_STD, out + i * 2 * CW_STD + CW_STD);
}
// The four lanes of a quad work on element t / 4 with identical arguments; lane 0's result goes out, then one word: 1 when every
// word of the result is the same in the four lanes
__device__ __forceinline__ void quad_out(u32* __restrict__ o, const xyzz& r) {
    u32 w[PW];
    st_pt(w, r);
    u32 diff = 0;
#pragma unroll
    for (int k = 0; k < PW; ++k) diff |= w[k] ^ quad_word(w[k], 0);
    diff = quad_word(diff, 0) | quad_word(diff, 1) | quad_word(diff, 2) | quad_word(diff, 3);
    if ((threadIdx.x & 3) == 0) {
#pragma unroll
        for (int k = 0; k < PW; ++k) o[k] = w[k];
        o[PW] = diff == 0 ? 1u : 0u;
    }
}
__global__ __launch_bounds__(PB) void dbl4_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = ((u64)blockIdx.x * PB + threadIdx.x) >> 2;
    if (i >= n) return;                                        // a whole quad leaves or stays
    quad_out(out + i * (PW + 1), pt_dbl4(ld_pt(in + i * PW)));
}
__global__ __launch_bounds__(PB) void add4_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = ((u64)blockIdx.x * PB + threadIdx.x) >> 2;
    if (i >= n) return;
    quad_out(out + i * (PW + 1), pt_add4(ld_pt(in + i * 2 * PW), ld_pt(in + i * 2 * PW + PW)));
}

inline void run(int fam, const u32* in, u32* out, size_t n) {
    static const int IN_W[E_COUNT] = {2 * CW_INT, CW_INT, CW_INT, NR, AW, PW, PW + AW, 2 * PW, PW, PW, PW, 2 * PW};
    static const int OUT_W[E_COUNT] = {CW_INT, CW_INT, CW_INT, NR, PW, PW, PW, PW, PW, 2 * CW_STD, PW + 1, PW + 1};
    ZK_REQUIRE(fam >= 0 && fam < E_COUNT, "zk_ecpt_probe: no such family");
    DevBuf din, dout;
    din.reserve(n * IN_W[fam] * 4); dout.reserve(n * OUT_W[fam] * 4);
    ZK_HIP(hipMemcpy(din.p, in, n * IN_W[fam] * 4, hipMemcpyHostToDevice));
    const size_t lanes = fam == E_DBL4 || fam == E_ADD4 ? 4 * n : n;
    const dim3 grid((unsigned)((lanes + PB - 1) / PB)), block(PB);
    const u32* i = (const u32*)din.p; u32* o = (u32*)dout.p;
    switch (fam) {
        case E_CFMUL: hipLaunchKernelGGL(cfmul_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_CFSQR: hipLaunchKernelGGL(cfsqr_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_CFINV: hipLaunchKernelGGL(cfinv_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
#ifdef MSM_G2
        case E_RENORM: hipLaunchKernelGGL(renorm_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
#else
        case E_RENORM: throw Error("zk_ecpt_probe: fe_renorm belongs to the Fq2 coordinate field (G2)");
#endif
        case E_DBL_AFF: hipLaunchKernelGGL(dbl_aff_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_DBL: hipLaunchKernelGGL(dbl_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_MADD: hipLaunchKernelGGL(madd_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_ADD: hipLaunchKernelGGL(add_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_NEG: hipLaunchKernelGGL(neg_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_TO_STD: hipLaunchKernelGGL(to_std_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        case E_DBL4: hipLaunchKernelGGL(dbl4_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
        default: hipLaunchKernelGGL(add4_kernel, grid, block, 0, nullptr, i, o, (u64)n); break;
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpy(out, dout.p, n * OUT_W[fam] * 4, hipMemcpyDeviceToHost));
}
