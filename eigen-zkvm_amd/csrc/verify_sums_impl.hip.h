// The scalar side of the aggregate Groth16 check (pairing.hip groth16_verify_aggregate_dev): from the weights rho_i (n x 8 canonical words,
// 128 bits each) and the public inputs (n x n_pub x 8 canonical words) the n_pub + 1 scalars
//     s_0 = sum_i rho_i mod r,    s_j = sum_i rho_i pub_ij mod r,
// and in the same pass the number of inputs that are not below r.  Included by groth16.hip inside each scalar field's namespace, behind
// fe29_impl.hip.h.  No include guard on purpose.
//
// Arithmetic: pub R' (one product with R'^2) times the PLAIN integer rho is pub rho R' / R' = pub rho, a plain residue below 2r -- one
// Montgomery product per term and no conversion on the way out.  Sums are kept canonical term by term (an addition and a conditional
// subtraction next to a product of 2 x 81 multiply-adds).
// Order: column j is blockIdx.y.  A launch of B = min(ceil(n / VS_BLOCK), VS_MAX_BLOCKS) blocks per column: lane t of block b adds the rows
// b VS_BLOCK + t, + B VS_BLOCK, ... in rising order, the block's lanes meet as a tree in LDS, and vs_final_kernel adds the B partial sums
// of a column in rising order.  Nothing is atomic; n alone fixes the order.
constexpr int VS_BLOCK = 256, VS_MAX_BLOCKS = 64;
constexpr int VS_PART = NR + 1;                         // a partial sum: NR canonical limbs and the count of inputs >= r

// 8 canonical words -> the 29-bit limbs of the same integer (below 2^256 < 11 r), and whether it is below r
__device__ __forceinline__ fe vs_split(const u32* __restrict__ w, bool& below_r) {
    fe x;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int bit = LB * k, wi = bit >> 5, s = bit & 31;
        u32 v = wi < NL ? w[wi] >> s : 0;
        if (s > 32 - LB && wi + 1 < NL) v |= w[wi + 1] << (32 - s);
        x.l[k] = v & LMASK;
    }
    bool lt = false, decided = false;
#pragma unroll
    for (int k = NR - 1; k >= 0; --k) {
        const bool ne = x.l[k] != Q29(k);
        if (!decided && ne) lt = x.l[k] < Q29(k);
        decided = decided || ne;
    }
    below_r = lt;
    return x;
}
__device__ __forceinline__ fe vs_add(const fe& a, const fe& b) { return fe_canon(fe_add(a, b)); }   // canonical operands, canonical sum
__global__ __launch_bounds__(VS_BLOCK) void vs_partial_kernel(const u32* __restrict__ rho, const u32* __restrict__ pub, u64 n, u32 n_pub,
                                                              u32* __restrict__ part) {
    __shared__ fe sh[VS_BLOCK];
    __shared__ u32 shbad[VS_BLOCK];
    const u32 j = blockIdx.y, t = threadIdx.x;
    fe acc = fe_zero();
    u32 bad = 0;
    fe rr2;
#pragma unroll
    for (int k = 0; k < NR; ++k) rr2.l[k] = RRP29(k);
    for (u64 i = (u64)blockIdx.x * VS_BLOCK + t; i < n; i += (u64)gridDim.x * VS_BLOCK) {
        bool ok;
        const fe w = vs_split(rho + i * 8, ok);         // 128 bits: below r as it stands
        if (j == 0) { acc = vs_add(acc, w); continue; }
        const fe x = vs_split(pub + (i * n_pub + (j - 1)) * 8, ok);
        if (!ok) { ++bad; continue; }                   // the batch is refused; the sums are not read
        acc = vs_add(acc, fe_canon(fe_mul(fe_mul(x, rr2), w)));
    }
    sh[t] = acc; shbad[t] = bad;
    for (u32 s = VS_BLOCK / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (t < s) { sh[t] = vs_add(sh[t], sh[t + s]); shbad[t] += shbad[t + s]; }
    }
    if (t == 0) {
        u32* o = part + ((u64)j * gridDim.x + blockIdx.x) * VS_PART;
        for (int k = 0; k < NR; ++k) o[k] = sh[0].l[k];
        o[NR] = shbad[0];
    }
}
// out: n_cols = n_pub + 1 scalars of 8 canonical words, then n_cols words: per column the number of inputs >= r (saturating)
__global__ __launch_bounds__(64) void vs_final_kernel(const u32* __restrict__ part, u32 blocks, u32 n_cols, u32* __restrict__ out) {
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    if (j >= n_cols) return;
    fe acc = fe_zero();
    u32 bad = 0;
    for (u32 b = 0; b < blocks; ++b) {
        const u32* p = part + ((u64)j * blocks + b) * VS_PART;
        fe x;
        for (int k = 0; k < NR; ++k) x.l[k] = p[k];
        acc = vs_add(acc, x);
        const u32 sum = bad + p[NR];
        bad = sum < bad ? ~0u : sum;
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const int bit = 32 * w, k = bit / LB, s = bit % LB;
        u32 v = acc.l[k] >> s;
        if (k + 1 < NR) v |= acc.l[k + 1] << (LB - s);
        if (k + 2 < NR && 2 * LB - s < 32) v |= acc.l[k + 2] << (2 * LB - s);
        out[j * 8 + w] = v;
    }
    out[n_cols * 8 + j] = bad;
}
size_t verify_sums_bytes(u32 n_pub) { return (size_t)(n_pub + 1) * 9 * 4; }
void verify_sums_dev(const void* d_rho, const void* d_pub, uint64_t n, uint32_t n_pub, void* d_out, hipStream_t st) {
    ZK_REQUIRE(n >= 1 && n < (1ull << 32) && n_pub < 65535, "groth16 verify: batch or input count out of range");
    const u32 blocks = (u32)std::min<u64>((n + VS_BLOCK - 1) / VS_BLOCK, VS_MAX_BLOCKS), n_cols = n_pub + 1;
    DevBuf part; part.reserve((size_t)n_cols * blocks * VS_PART * 4);
    hipLaunchKernelGGL(vs_partial_kernel, dim3(blocks, n_cols), dim3(VS_BLOCK), 0, st, (const u32*)d_rho, (const u32*)d_pub, n, n_pub, (u32*)part.p);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(vs_final_kernel, dim3((n_cols + 63) / 64), dim3(64), 0, st, (const u32*)part.p, blocks, n_cols, (u32*)d_out);
    ZK_HIP(hipGetLastError());
}
