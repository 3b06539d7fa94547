// Fixed-base multiplication by full-width scalars, P_i = [k_i] G for the group's generator G: what key generation
// (groth16_keygen_impl.hip.h; bellman's generate_parameters, groth16/src/groth16.rs:77-86) spends its time in.
// Included at the end of msm_impl.hip.h, once per curve and group, and uses that file's field, point formulas and
// internal affine layout (load_aff, PTW).  No include guard on purpose.
//
// Window table: entry [t * 256 + j] = [j 2^(8 t)] G for the 32 byte-wide windows of a 255-bit scalar (j = 0 is
// unused).  A scalar is then the sum of at most 32 table entries -- 32 mixed additions, no doubling -- and digit t
// is simply byte t of the little-endian scalar.  8 bits keep the table at 8 192 entries of PTW words: 640 KB
// (BN254 G1) to 1.75 MB (BLS12-381 G2), inside one XCD's 4 MB L2 next to the streamed scalars and results, so the
// random gathers never go to HBM; 16-bit windows would halve the additions with a table of 1 M entries per window
// pair (80-224 MB), which no cache level holds.  The table is built once per device by a bit-serial kernel (one lane
// per entry, its own inversion: 8 192 lanes, once) and kept as an owned constant (DevConst).
//
// Affine results need 1 / ZZZ per point.  A field inversion is a chain of ~1.5 log2 q products (fe_inv) -- more than
// the 32 additions in front of it for G1 -- so the 256 lanes of a workgroup share ONE: a product tree over their ZZZ
// (norms for Fq2) in LDS, one lane inverts the root, and the way back down hands every leaf its own inverse
// (Montgomery's trick in tree form: 3 products per lane and level instead of an inversion per lane).  While that lane
// inverts, the other three waves of the group wait at the barrier and their SIMDs run other workgroups.
constexpr int FB_W = 8, FB_NWIN = 32, FB_ENTRIES = FB_NWIN << FB_W;
static_assert(FB_W * FB_NWIN >= 255, "windows cover the scalar");

__global__ __launch_bounds__(64) void fb_table_kernel(u32* __restrict__ table) {   // FB_ENTRIES lanes
    const u32 e = blockIdx.x * 64 + threadIdx.x, t = e >> FB_W, j = e & ((1u << FB_W) - 1);
    u32* o = table + (u64)e * PTW;
    for (int k = 0; k < PTW; ++k) o[k] = 0;
    if (j == 0) return;
    u32 gx[CW_STD], gy[CW_STD];
    for (int k = 0; k < CW_STD; ++k) { gx[k] = GEN_X(k); gy[k] = GEN_Y(k); }
    aff g; g.x = cf_from_std(gx); g.y = cf_from_std(gy);
    xyzz acc = pt_inf();
    const int low = FB_W * (int)t;
    for (int b = low + FB_W - 1; b >= 0; --b) {                   // [j 2^low] G, bit by bit; never infinity (r is prime)
        acc = pt_dbl(acc);
        if (b >= low && ((j >> (b - low)) & 1)) acc = pt_madd(acc, g);
    }
    const cf izzz = cf_inv(acc.ZZZ), s = cf_mul(acc.ZZ, izzz), izz = cf_sqr(s);
    cf_store_int(cf_mul(acc.X, izz), o); cf_store_int(cf_mul(acc.Y, izzz), o + CW_INT);
}

// the value the workgroup inverts for a finite point: ZZZ, or its norm over Fq2 (1 / z = conj(z) / norm(z))
__device__ __forceinline__ fe fb_leaf(const xyzz& p) {
#ifndef MSM_G2
    return p.ZZZ;
#else
    return fe_mul(fe_add(fe_sqr(p.ZZZ.c0), fe_sqr(p.ZZZ.c1)), fe_one());
#endif
}
// x = X / ZZ, y = Y / ZZZ in the external layout from 1 / leaf; 1 / ZZ = (ZZ / ZZZ)^2 because ZZ^3 = ZZZ^2
// (a real function: inlined, the BLS12-381 G1 kernel passes the code size msm.hip warns about)
__device__ __noinline__ void fb_store_affine(const xyzz& p, const fe& inv_leaf, u32* __restrict__ o) {
#ifndef MSM_G2
    const cf izzz = inv_leaf;
#else
    cf izzz; izzz.c0 = fe_mul(p.ZZZ.c0, inv_leaf); izzz.c1 = fe_mul(fe_sub<2>(fe_zero(), p.ZZZ.c1), inv_leaf);
#endif
    const cf s = cf_mul(p.ZZ, izzz), izz = cf_sqr(s);
    u32 x[CW_STD], y[CW_STD];
    cf_to_std(cf_mul(p.X, izz), x); cf_to_std(cf_mul(p.Y, izzz), y);
    for (int k = 0; k < CW_STD; ++k) { o[k] = x[k]; o[CW_STD + k] = y[k]; }
}

constexpr int FB_BLOCK = 256;
__global__ __launch_bounds__(FB_BLOCK) void fb_mul_kernel(const u32* __restrict__ table, const u64* __restrict__ k, u64 n, u32* __restrict__ out) {
    __shared__ fe node[2 * FB_BLOCK];                              // heap order: node[p] = node[2p] node[2p + 1], leaves at FB_BLOCK + lane
    const u32 l = threadIdx.x;
    const u64 i = (u64)blockIdx.x * FB_BLOCK + l;
    const bool live = i < n;
    xyzz acc = pt_inf();
    if (live) {
        const unsigned char* d = (const unsigned char*)(k + 4 * i);   // digit t = byte t
        // the next window's entry is requested before the current addition starts (the table sits in L2)
        aff cur = load_aff(table, d[0]);
        for (int t = 0; t < FB_NWIN; ++t) {
            const u32 dt = d[t];
            aff nxt = cur;
            if (t + 1 < FB_NWIN) nxt = load_aff(table, ((u32)(t + 1) << FB_W) + d[t + 1]);
            if (dt) acc = pt_madd(acc, cur);                        // k < r: the partial sum never meets +-entry, pt_madd covers it anyway
            cur = nxt;
        }
    }
    const bool finite = live && !pt_is_inf(acc);
    node[FB_BLOCK + l] = finite ? fb_leaf(acc) : fe_one();
    for (u32 s = FB_BLOCK / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (l < s) node[s + l] = fe_mul(node[2 * (s + l)], node[2 * (s + l) + 1]);
    }
    __syncthreads();
    if (l == 0) node[1] = fe_inv(node[1]);
    for (u32 s = 1; s < (u32)FB_BLOCK; s <<= 1) {
        __syncthreads();
        if (l < s) {
            const u32 p = s + l;
            const fe ip = node[p], a = node[2 * p], b = node[2 * p + 1];
            node[2 * p] = fe_mul(ip, b); node[2 * p + 1] = fe_mul(ip, a);
        }
    }
    __syncthreads();
    if (!live) return;
    u32* o = out + i * (2 * CW_STD);
    if (!finite) { for (int j = 0; j < 2 * CW_STD; ++j) o[j] = 0; return; }   // k = 0: the all-zero encoding of g1_mul_generator_kernel
    const fe inv_leaf = node[FB_BLOCK + l];
    fb_store_affine(acc, inv_leaf, o);
}

// Built on a stream of its own, so the caller's stream sees neither the launch nor the wait.  The first call on a device allocates and
// synchronises: it must not be made while a stream is capturing; every later call only looks the table up.
static const u32* fb_table() {
    static std::mutex mu;
    static auto& tables = *new std::map<int, DevConst>();          // per device, never destroyed (DevConst, zk_internal.h)
    int dev = 0; ZK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = tables.find(dev);
    if (it != tables.end()) return (const u32*)it->second.p;
    DevConst t((size_t)FB_ENTRIES * PTW * 4);
    hipStream_t st = nullptr;
    ZK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipLaunchKernelGGL(fb_table_kernel, dim3(FB_ENTRIES / 64), dim3(64), 0, st, (u32*)t.p);
    const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    ZK_HIP(launched); ZK_HIP(done);
    return (const u32*)tables.emplace(dev, std::move(t)).first->second.p;
}
// d_k: n x 4 u64 canonical little-endian scalars < r; d_bases: n affine points, Montgomery, the layout of g1_mul_generator_dev
void mul_generator_fr_dev(const u64* d_k, uint64_t n, void* d_bases, hipStream_t st) {
    if (n == 0) return;
    ZK_REQUIRE(n < (1ull << 32) * FB_BLOCK, "mul_generator: n out of range");
    const u32* table = fb_table();
    hipLaunchKernelGGL(fb_mul_kernel, dim3((unsigned)((n + FB_BLOCK - 1) / FB_BLOCK)), dim3(FB_BLOCK), 0, st, table, d_k, n, (u32*)d_bases);
    ZK_HIP(hipGetLastError());
}
