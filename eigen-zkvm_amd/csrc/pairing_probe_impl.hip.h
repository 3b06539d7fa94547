// Body of pairing_probe.hip: included once per curve inside a namespace that has included ecpt_impl.hip.h and pairing_impl.hip.h with
// MSM_G2.  One kernel per family; the line steps and the Fq12 primitives stay the functions pairing_impl.hip.h makes them.  An Fq2 value
// is W = CW_INT raw internal limbs (c0 then c1), an Fq12 value six of them (the coefficients of w^0 .. w^5), element-major like
// ecpt_probe_impl.hip.h.  The Fq12 kernels run as miller_kernel and final_exp_kernel do: workgroups of 64 lanes, eight groups of eight,
// an idle group shadows the last element and stores nothing, and every group of a workgroup meets every barrier.
// No include guard on purpose.
constexpr int TB = 64, W = CW_INT, W12 = 6 * CW_INT;
enum { T_CF = 0, T_XI, T_LINE_DBL, T_LINE_ADD, T_LINES, T_F12_MUL, T_F12_TAB, T_F12_LINE, T_F12_CYC, T_F12_MAPS, T_CANON, T_FINAL_EXP, T_COUNT };

__global__ __launch_bounds__(TB) void cf_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // (a, b) -> a b, a^2, 1 / a
    const u64 i = (u64)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const cf a = cf_load_int(in + i * 2 * W), b = cf_load_int(in + i * 2 * W + W);
    cf_store_int(cf_mul(a, b), out + i * 3 * W);
    cf_store_int(cf_sqr(a), out + i * 3 * W + W);
    cf_store_int(cf_inv(a), out + i * 3 * W + 2 * W);
}
__global__ __launch_bounds__(TB) void xi_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // a -> xi a, cf_red(a), -a
    const u64 i = (u64)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const cf a = cf_load_int(in + i * W);
    cf_store_int(cf_mul_xi(a), out + i * 3 * W);
    cf_store_int(cf_red(a), out + i * 3 * W + W);
    cf_store_int(cf_neg(a), out + i * 3 * W + 2 * W);
}
__device__ __forceinline__ void st_jac(u32* __restrict__ p, const jac& T) { cf_store_int(T.X, p); cf_store_int(T.Y, p + W); cf_store_int(T.Z, p + 2 * W); }
__device__ __forceinline__ jac ld_jac(const u32* __restrict__ p) { jac T; T.X = cf_load_int(p); T.Y = cf_load_int(p + W); T.Z = cf_load_int(p + 2 * W); return T; }
__global__ __launch_bounds__(TB) void line_dbl_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // T -> T', (cY, cX, c0)
    const u64 i = (u64)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    jac T = ld_jac(in + i * 3 * W);
    line_dbl(T, out + i * 6 * W + 3 * W);
    st_jac(out + i * 6 * W, T);
}
__global__ __launch_bounds__(TB) void line_add_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // T, x2, y2 -> T', (cY, cX, c0)
    const u64 i = (u64)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    jac T = ld_jac(in + i * 5 * W);
    line_add(T, cf_load_int(in + i * 5 * W + 3 * W), cf_load_int(in + i * 5 * W + 4 * W), out + i * 6 * W + 3 * W);
    st_jac(out + i * 6 * W, T);
}

// the element of this lane's group (the last one for an idle group) and whether the group stores
__device__ __forceinline__ u64 f12_item(u64 n, bool& have) {
    u64 i = (u64)blockIdx.x * PR_GROUPS + threadIdx.x / PR_GROUP;
    have = i < n;
    return have ? i : n - 1;
}
__global__ __launch_bounds__(TB) void f12_mul_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    const f12ctx c = f12_ctx(sh_all);
    bool have;
    const u64 i = f12_item(n, have);
    const cf r = f12_mul(c, cf_load_int(in + i * 2 * W12 + c.k * W), cf_load_int(in + i * 2 * W12 + W12 + c.k * W));
    if (have && c.live) cf_store_int(r, out + i * W12 + c.k * W);
}
__global__ __launch_bounds__(TB) void f12_tab_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // a, then the table entry (g, xi g)
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    const f12ctx c = f12_ctx(sh_all);
    bool have;
    const u64 i = f12_item(n, have);
    const cf r = f12_mul_tab(c, cf_load_int(in + i * 3 * W12 + c.k * W), in + i * 3 * W12 + W12);
    if (have && c.live) cf_store_int(r, out + i * W12 + c.k * W);
}
__global__ __launch_bounds__(TB) void f12_line_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // f, v0, v1, v2
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    const f12ctx c = f12_ctx(sh_all);
    bool have;
    const u64 i = f12_item(n, have);
    const u32* e = in + i * (W12 + 3 * W);
    const cf r = f12_mul_line(c, cf_load_int(e + c.k * W), cf_load_int(e + W12), cf_load_int(e + W12 + W), cf_load_int(e + W12 + 2 * W));
    if (have && c.live) cf_store_int(r, out + i * W12 + c.k * W);
}
__global__ __launch_bounds__(TB) void f12_cyc_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    const f12ctx c = f12_ctx(sh_all);
    bool have;
    const u64 i = f12_item(n, have);
    const cf r = f12_cyc_sqr(c, cf_load_int(in + i * W12 + c.k * W));
    if (have && c.live) cf_store_int(r, out + i * W12 + c.k * W);
}
__global__ __launch_bounds__(TB) void f12_maps_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // a -> conj6(a), frob2(a)
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    const f12ctx c = f12_ctx(sh_all);
    bool have;
    const u64 i = f12_item(n, have);
    const cf a = cf_load_int(in + i * W12 + c.k * W);
    const cf r0 = f12_conj6(c, a), r1 = f12_frob2(c, a);
    if (have && c.live) { cf_store_int(r0, out + i * 2 * W12 + c.k * W); cf_store_int(r1, out + i * 2 * W12 + W12 + c.k * W); }
}
__global__ __launch_bounds__(TB) void canon_probe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {   // one Fq -> NL canonical words
    const u64 i = (u64)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    fe a;
#pragma unroll
    for (int k = 0; k < NR; ++k) a.l[k] = in[i * NR + k];
    u32 w[NL];
    fe_to_canon_words(a, w);
#pragma unroll
    for (int k = 0; k < NL; ++k) out[i * NL + k] = w[k];
}

inline void run(int fam, const u32* in, u32* out, size_t n) {
    constexpr int LINES_W = PR_STEPS * PR_LINE_WORDS, GT_W = 12 * NL;
    static const int IN_W[T_COUNT] = {2 * W, W, 3 * W, 5 * W, 2 * CW_STD, 2 * W12, 3 * W12, W12 + 3 * W, W12, W12, NR, W12};
    static const int OUT_W[T_COUNT] = {3 * W, 3 * W, 6 * W, 6 * W, LINES_W + 1, W12, W12, W12, W12, 2 * W12, NL, 2 * GT_W};
    ZK_REQUIRE(fam >= 0 && fam < T_COUNT, "zk_pairing_probe: no such family");
    DevBuf din, dout, dtmp;
    din.reserve(n * IN_W[fam] * 4); dout.reserve(n * OUT_W[fam] * 4);
    ZK_HIP(hipMemcpy(din.p, in, n * IN_W[fam] * 4, hipMemcpyHostToDevice));
    const dim3 lanes((unsigned)((n + TB - 1) / TB)), groups((unsigned)((n + PR_GROUPS - 1) / PR_GROUPS)), block(TB);
    const u32* i = (const u32*)din.p; u32* o = (u32*)dout.p;
    switch (fam) {
        case T_CF: hipLaunchKernelGGL(cf_probe_kernel, lanes, block, 0, nullptr, i, o, (u64)n); break;
        case T_XI: hipLaunchKernelGGL(xi_probe_kernel, lanes, block, 0, nullptr, i, o, (u64)n); break;
        case T_LINE_DBL: hipLaunchKernelGGL(line_dbl_probe_kernel, lanes, block, 0, nullptr, i, o, (u64)n); break;
        case T_LINE_ADD: hipLaunchKernelGGL(line_add_probe_kernel, lanes, block, 0, nullptr, i, o, (u64)n); break;
        case T_LINES: g2_lines_dev(i, 2 * CW_STD, n, o, o + n * LINES_W, nullptr); break;                   // the tables, then the infinity words
        case T_F12_MUL: hipLaunchKernelGGL(f12_mul_probe_kernel, groups, block, 0, nullptr, i, o, (u64)n); break;
        case T_F12_TAB: hipLaunchKernelGGL(f12_tab_probe_kernel, groups, block, 0, nullptr, i, o, (u64)n); break;
        case T_F12_LINE: hipLaunchKernelGGL(f12_line_probe_kernel, groups, block, 0, nullptr, i, o, (u64)n); break;
        case T_F12_CYC: hipLaunchKernelGGL(f12_cyc_probe_kernel, groups, block, 0, nullptr, i, o, (u64)n); break;
        case T_F12_MAPS: hipLaunchKernelGGL(f12_maps_probe_kernel, groups, block, 0, nullptr, i, o, (u64)n); break;
        case T_CANON: hipLaunchKernelGGL(canon_probe_kernel, lanes, block, 0, nullptr, i, o, (u64)n); break;
        default:                                                                                             // with the exponentiation, then without
            dtmp.reserve(final_exp_tab_bytes(n));
            final_exp_dev(i, n, dtmp.p, o, 1, nullptr);
            final_exp_dev(i, n, dtmp.p, o + n * GT_W, 0, nullptr);
            break;
    }
    ZK_HIP(hipGetLastError());
    if (fam == T_LINES || fam == T_FINAL_EXP) {                                                              // two blocks on the device -> element-major
        const size_t a = fam == T_LINES ? LINES_W : GT_W, b = OUT_W[fam] - a;
        std::vector<u32> h(n * OUT_W[fam]);
        ZK_HIP(hipMemcpy(h.data(), dout.p, h.size() * 4, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < n; ++e) {
            for (size_t k = 0; k < a; ++k) out[e * (a + b) + k] = h[e * a + k];
            for (size_t k = 0; k < b; ++k) out[e * (a + b) + a + k] = h[n * a + e * b + k];
        }
        return;
    }
    ZK_HIP(hipMemcpy(out, dout.p, n * OUT_W[fam] * 4, hipMemcpyDeviceToHost));
}
