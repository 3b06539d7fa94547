// Test hooks for the matrix-pipe form of the scalar-field Poseidon (fr_mfma.hip.h): included by frhash.hip and frhash_bls12381.hip after
// frhash_impl.hip.h, inside the field's namespace, so that the kernels below see the tables load_constants loaded (g_prm, the mf_* tables)
// and the host probe the tables mf_build builds.  mf_dense, mf_sparse and poseidon_fr_reg are applied once to states from the host and what
// they return is written back as raw internal limbs (NR u32 per word, element-major: state i reads in[(i * t + j) * NR ...] and writes the
// same place of out), so that the test decides the exact representative (tests/test_gpu_fr_mfma.py, tests/fr_mfma_model.py).  Blocks of
// 256 threads (both device functions want the whole block), LDS laid out as the production kernels lay it out, idle lanes of the last
// block shadow the last state.  Not part of include/zkgpu.h; the tests bind zk_<field>_mf_probe and zk_<field>_mf_emulate_probe by name.
// No include guard on purpose.
namespace {
enum { MFP_DENSE = 0, MFP_SPARSE, MFP_PERM, MFP_COUNT };

template <int T>
__device__ __forceinline__ void mfp_load(fe (&st)[T], const u32* __restrict__ p) {
    fh_static_for<0, T>([&](auto J) {
        constexpr int j = decltype(J)::value;
#pragma unroll
        for (int k = 0; k < NR; ++k) st[j].l[k] = p[j * NR + k];
    });
}
template <int T>
__device__ __forceinline__ void mfp_store(const fe (&st)[T], u32* __restrict__ p) {
    fh_static_for<0, T>([&](auto J) {
        constexpr int j = decltype(J)::value;
#pragma unroll
        for (int k = 0; k < NR; ++k) p[j * NR + k] = st[j].l[k];
    });
}
// one dense layer: the matrix and the addends poseidon_fr_reg gives mf_dense for `layer` (P for layer 3, M otherwise)
template <int T>
__global__ __launch_bounds__(256) void mfp_dense_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n, u32 layer) {
    __shared__ __attribute__((aligned(16))) u32 lds[REG_LDS_WORDS<T>];
    mf_v4i* const abuf = (mf_v4i*)(lds + REG_ABUF_AT<T>);
    const u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x, i = i0 < n ? i0 : n - 1;
    fe st[T];
    mfp_load<T>(st, in + i * T * NR);
    const mf_v4i* mat = (const mf_v4i*)(layer == 3 ? g_prm[T - 2].mf_p : g_prm[T - 2].mf_m);
    mf_dense<T>(st, mat, g_prm[T - 2].mf_k + (size_t)layer * T * 8, abuf);
    if (i0 < n) mfp_store<T>(st, out + i * T * NR);
}
// the first n_rp sparse rounds
template <int T>
__global__ __launch_bounds__(256) void mfp_sparse_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n, u32 n_rp) {
    __shared__ __attribute__((aligned(16))) u32 lds[REG_LDS_WORDS<T>];
    mf_v4i* const abuf = (mf_v4i*)(lds + REG_ABUF_AT<T>);
    const u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x, i = i0 < n ? i0 : n - 1;
    fe st[T];
    mfp_load<T>(st, in + i * T * NR);
    mf_sparse<T>(st, (const mf_v4i*)g_prm[T - 2].mf_s, (const mf_v4i*)g_prm[T - 2].mf_i, abuf, n_rp);
    if (i0 < n) mfp_store<T>(st, out + i * T * NR);
}
// the whole permutation, under the register budget of bn128_leaf_reg_kernel<T - 1>
template <int T>
__global__ __launch_bounds__(256, T - 1 <= ZK_LB3 ? 3 : T - 1 <= ZK_LB2 ? 2 : 1) void mfp_perm_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    __shared__ __attribute__((aligned(16))) u32 lds[REG_LDS_WORDS<T>];
    const fe* tab = reg_tables_to_lds<T>(lds);
    const u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x, i = i0 < n ? i0 : n - 1;
    fe st[T];
    mfp_load<T>(st, in + i * T * NR);
    poseidon_fr_reg<T>(st, tab);
    if (i0 < n) mfp_store<T>(st, out + i * T * NR);
}
template <int T>
void mfp_launch(int kind, u32 arg, const u32* in, u32* out, u64 n) {
    if constexpr (REG_MF<T>) {                                               // (the A/B knob ZK_FR_MFMA_FROM may leave a t without tables: refused by the caller)
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        if (kind == MFP_DENSE) hipLaunchKernelGGL(mfp_dense_kernel<T>, grid, block, 0, nullptr, in, out, n, arg);
        else if (kind == MFP_SPARSE) hipLaunchKernelGGL(mfp_sparse_kernel<T>, grid, block, 0, nullptr, in, out, n, arg);
        else hipLaunchKernelGGL(mfp_perm_kernel<T>, grid, block, 0, nullptr, in, out, n);
    }
}

// the host's tables of one t, built once per constants file
struct MfpHost { std::string path; MfHost mf[16]; bool have[16] = {}; };
MfpHost g_mfp_host;
std::mutex g_mfp_mu;
}  // namespace

// kind: MFP_DENSE (arg = layer 0..7), MFP_SPARSE (arg = rounds, 1..fh_nrp(t)), MFP_PERM (arg unused).  in / out: n states of t words of NR limbs.
void FH_FN(mf_probe)(int kind, int t, int arg, const u32* in, u32* out, size_t n) {
    const std::string me = "zk_" FH_NAME "_mf_probe: ";
    ZK_REQUIRE(in && out, me + "null buffer");
    ZK_REQUIRE(n > 0 && n <= ((size_t)1 << 16), me + "n must be 1 .. 65536");
    ZK_REQUIRE(kind >= 0 && kind < MFP_COUNT, me + "no such probe");
    ZK_REQUIRE(t >= (ZK_FR_MFMA_FROM > 3 ? ZK_FR_MFMA_FROM : 3) && t <= 17, me + "t must be 3 .. 17 (the matrix-pipe kernels)");
    if (kind == MFP_DENSE) ZK_REQUIRE(arg >= 0 && arg < 8, me + "layer must be 0 .. 7");
    if (kind == MFP_SPARSE) ZK_REQUIRE(arg >= 1 && (u32)arg <= fh_nrp(t), me + "rounds must be 1 .. the sparse rounds of t");
    require_tables();
    const size_t bytes = n * (size_t)t * NR * 4;
    DevBuf din, dout;
    din.reserve(bytes); dout.reserve(bytes);
    ZK_HIP(hipMemcpy(din.p, in, bytes, hipMemcpyHostToDevice));
    const u32* i = (const u32*)din.p; u32* o = (u32*)dout.p;
#define ZK_MFP(N) case N: mfp_launch<N>(kind, (u32)arg, i, o, (u64)n); break;
    switch (t) {
        ZK_MFP(3) ZK_MFP(4) ZK_MFP(5) ZK_MFP(6) ZK_MFP(7) ZK_MFP(8) ZK_MFP(9) ZK_MFP(10)
        ZK_MFP(11) ZK_MFP(12) ZK_MFP(13) ZK_MFP(14) ZK_MFP(15) ZK_MFP(16) ZK_MFP(17)
    }
#undef ZK_MFP
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
}

// Host only, no device: what mf_emulate / mf_emulate_gen compute from the tables mf_build builds from the constants file.
// which: 0..7 = that dense layer (its matrix, its addends), 8 + r = sparse round r (word 0 of a state stands for x_0^5, as in
// mf_selfcheck_sparse).  x: n states of t words of eight 32-bit words (any integers < 2^256); out: per state and output word eleven
// words -- the 320-bit result, then the ok flag (every digit column and biased word inside the range the device code assumes).
void FH_FN(mf_emulate_probe)(const char* path, int t, int which, const u32* x, size_t n, u32* out) {
    const std::string me = "zk_" FH_NAME "_mf_emulate_probe: ";
    ZK_REQUIRE(path && x && out, me + "null argument");
    ZK_REQUIRE(n > 0 && n <= ((size_t)1 << 16), me + "n must be 1 .. 65536");
    ZK_REQUIRE(t >= (ZK_FR_MFMA_FROM > 3 ? ZK_FR_MFMA_FROM : 3) && t <= 17, me + "t must be 3 .. 17 (the matrix-pipe kernels)");
    ZK_REQUIRE(which >= 0 && (u32)which < 8 + fh_nrp(t), me + "no such layer or sparse round");
    std::lock_guard<std::mutex> lk(g_mfp_mu);
    MfpHost& G = g_mfp_host;
    if (G.path != path) { for (int k = 0; k < 16; ++k) { G.have[k] = false; G.mf[k] = MfHost(); } G.path = path; }
    if (!G.have[t - 2]) {
        std::vector<unsigned char> canon; TabOff off[16];
        read_constants(path, canon, off);
        const TabOff& o = off[t - 2];
        G.mf[t - 2] = mf_build(canon.data(), o.c, o.m, o.p, o.s, t, NRP[t - 2]);
        G.have[t - 2] = true;
    }
    const MfHost& H = G.mf[t - 2];
    std::vector<MfInt> xs(t);
    for (size_t i = 0; i < n; ++i) {
        for (int j = 0; j < t; ++j) {
            xs[j] = mf_zero();
            for (int w = 0; w < 8; ++w) xs[j].w[w >> 1] |= (u64)x[(i * t + j) * 8 + w] << (32 * (w & 1));
        }
        for (int o = 0; o < t; ++o) {
            bool ok = true;
            MfInt R;
            if (which < 8) {
                R = mf_emulate(H.frag.data() + (which == 3 ? H.fb : 0), &H.K[((size_t)which * t + o) * 8], t, o, xs.data(), ok);
            } else {
                const unsigned char* blk = H.sp.data() + mf_sparse_round_bytes(t) * (size_t)(which - 8);
                const u64* K = reinterpret_cast<const u64*>(blk + (size_t)(2 * t - 1) * 1024);
                if (o == 0) {
                    std::vector<const signed char*> f(t);
                    for (int j = 0; j < t; ++j) f[j] = (const signed char*)blk + (size_t)j * 1024;
                    R = mf_emulate_gen(f.data(), t, K, xs.data(), MF_SP_SHIFT, ok);
                } else {
                    const signed char* f[2] = {(const signed char*)blk + (size_t)(t + o - 1) * 1024, (const signed char*)H.sp.data() + H.sb};
                    const MfInt xx[2] = {xs[0], xs[o]};
                    R = mf_emulate_gen(f, 2, K + 8 * o, xx, MF_SP_SHIFT, ok);
                }
            }
            u32* dst = out + (i * t + o) * 11;
            for (int w = 0; w < 10; ++w) dst[w] = (u32)(R.w[w >> 1] >> (32 * (w & 1)));
            dst[10] = ok ? 1u : 0u;
        }
    }
}

#define ZK_MFP_CAT_(a, b) a##b
#define ZK_MFP_CAT(a, b) ZK_MFP_CAT_(a, b)
extern "C" int ZK_MFP_CAT(zk_, FH_FN(mf_probe))(int kind, int t, int arg, const uint32_t* in, uint32_t* out, size_t n) {
    return guard([&] { FH_FN(mf_probe)(kind, t, arg, in, out, n); });
}
extern "C" int ZK_MFP_CAT(zk_, FH_FN(mf_emulate_probe))(const char* path, int t, int which, const uint32_t* x, size_t n, uint32_t* out) {   // host arithmetic only: no CallScope, no device
    try { FH_FN(mf_emulate_probe)(path, t, which, x, n, out); return 0; }
    catch (const std::exception& e) { set_error(e.what()); }
    return -1;
}
#undef ZK_MFP_CAT
#undef ZK_MFP_CAT_
