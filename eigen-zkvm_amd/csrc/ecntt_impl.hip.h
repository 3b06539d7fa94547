// Transforms, column sums and scalar products whose elements are curve points: what a Groth16 key costs when it is made from a
// powers-of-tau file instead of a trapdoor (groth16.hip keygen_from_srs).  Nothing can be computed on scalars and multiplied into the
// generator there, so the work of groth16_keygen_impl.hip.h happens in the group.  Included once per (curve, group) by ecntt.hip inside
// a namespace that has included ecpt_impl.hip.h; no include guard on purpose.
//
// Layouts.  Outside: affine (x, y), Montgomery, little-endian limbs, all zero = infinity (the layout of the sums).  Between kernels:
// a work buffer of XYZZ points as raw internal limbs (EW words each), so a point is converted once on the way in and once on the way
// out -- the way out shares one inversion per workgroup by the product tree of fb_mul_kernel (fixedbase_impl.hip.h).
//
// Transform: radix 2, decimation in time -- the load permutes by bit reversal, log n stage launches follow, one lane per butterfly
// (a, b) -> (a + [w]b, a - [w]b).  [w]b is a double-and-add over the bits of w (canonical words from a table the host fills):
// about 254 doublings and 127 additions of ~2 700 instructions each, next to which the 4 x EW words a butterfly moves are nothing, so
// lanes are laid out for the arithmetic and not for the memory: butterfly t of stage s has twiddle index t / groups, which is the
// same for all 64 lanes of a wave while the stage has 64 groups or more.  There the index is made wave-uniform (readfirstlane): the
// scalar's words come through scalar loads and the branch on each bit is a scalar branch -- one recoding for the wave.  In the last
// six stages the lanes of a wave hold different twiddles and the additions run under EXEC masks.  Twiddle 1 (index 0: every butterfly
// of the first stage, one per group after that) skips the product altogether.
// The point formulas are called through two real functions, so a kernel holds one copy of each (code size: see msm.hip).
// pt_add is complete -- equal operands go to the doubling, opposite ones to infinity -- which a constant column of a file needs.
constexpr int EW = 4 * CW_INT, AW = 2 * CW_STD;
#if !defined(MSM_G2) && (defined(GLV_CURVE_BN254) || defined(GLV_CURVE_BLS12_381))
#define ECN_GLV 1
#include "glv_split.hip.h"
#endif

__device__ __forceinline__ xyzz ecn_ld(const u32* __restrict__ p) {
    xyzz r;
    r.X = cf_load_int(p); r.Y = cf_load_int(p + CW_INT); r.ZZ = cf_load_int(p + 2 * CW_INT); r.ZZZ = cf_load_int(p + 3 * CW_INT);
    return r;
}
__device__ __forceinline__ void ecn_st(u32* __restrict__ p, const xyzz& r) {
    cf_store_int(r.X, p); cf_store_int(r.Y, p + CW_INT); cf_store_int(r.ZZ, p + 2 * CW_INT); cf_store_int(r.ZZZ, p + 3 * CW_INT);
}
__device__ __forceinline__ xyzz ecn_load_ext(const u32* __restrict__ p) {
    u32 w[AW], any = 0;
#pragma unroll
    for (int k = 0; k < AW; ++k) { w[k] = p[k]; any |= w[k]; }
    if (!any) return pt_inf();
    xyzz r;
    r.X = cf_from_std(w); r.Y = cf_from_std(w + CW_STD); r.ZZ = cf_one(); r.ZZZ = cf_one();
    return r;
}
__device__ __noinline__ xyzz ecn_add(const xyzz& p, const xyzz& q) { return pt_add(p, q); }
__device__ __noinline__ xyzz ecn_dbl(const xyzz& p) { return pt_dbl(p); }
// [k]b for k of 8 canonical words in memory, k < r; k = 0 or b = infinity gives infinity
__device__ __forceinline__ xyzz ecn_mul(const xyzz& b, const u32* __restrict__ k) {
    int top = -1;
    for (int w = 7; w >= 0 && top < 0; --w)
        if (k[w]) top = 32 * w + 31 - __clz((int)k[w]);
    if (top < 0 || pt_is_inf(b)) return pt_inf();
    xyzz acc = b;
    for (int bit = top - 1; bit >= 0; --bit) {
        acc = ecn_dbl(acc);
        if ((k[bit >> 5] >> (bit & 31)) & 1) acc = ecn_add(acc, b);
    }
    return acc;
}

__global__ __launch_bounds__(64) void ecn_load_kernel(const u32* __restrict__ pts, u32 logn, u32* __restrict__ work) {
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    if (i >> logn) return;
    const u32 j = logn ? __brev(i) >> (32 - logn) : 0u;
    ecn_st(work + (u64)j * EW, ecn_load_ext(pts + (u64)i * AW));
}
// stage s of logn: halves of 2^s, groups = 2^(logn - 1 - s); tw[k] = w_n^k for k < n / 2, 8 canonical words each
__global__ __launch_bounds__(64) void ecn_stage_kernel(u32* __restrict__ work, const u32* __restrict__ tw, u32 logn, u32 s) {
    const u32 t = blockIdx.x * 64u + threadIdx.x;
    if (t >> (logn - 1)) return;
    const u32 lg = logn - 1 - s;                                    // log2 of the number of groups
    u32 j = t >> lg;
    const u32 g = t & ((1u << lg) - 1);
    if (lg >= 6) j = (u32)__builtin_amdgcn_readfirstlane((int)j);  // the wave's 64 butterflies share the twiddle
    u32* p0 = work + (((u64)g << (s + 1)) + j) * EW;
    u32* p1 = p0 + ((u64)EW << s);
    const xyzz a = ecn_ld(p0);
    xyzz b = ecn_ld(p1);
    if (j) b = ecn_mul(b, tw + ((u64)j << lg) * 8);
    ecn_st(p0, ecn_add(a, b));
    ecn_st(p1, ecn_add(a, pt_neg(b)));
}
// work[i] = [k] work[i], one scalar for all (the 1 / n of the inverse transform)
__global__ __launch_bounds__(64) void ecn_scale_kernel(u32* __restrict__ work, u64 n, const u32* __restrict__ k) {
    const u64 i = blockIdx.x * 64ull + threadIdx.x;
    if (i >= n) return;
    ecn_st(work + i * EW, ecn_mul(ecn_ld(work + i * EW), k));
}
// work[i] = [k] pts[i]: every lane walks the same bits
__global__ __launch_bounds__(64) void ecn_mul_scalar_kernel(const u32* __restrict__ pts, u64 n, const u32* __restrict__ k, u32* __restrict__ work) {
    const u64 i = blockIdx.x * 64ull + threadIdx.x;
    if (i >= n) return;
    ecn_st(work + i * EW, ecn_mul(ecn_load_ext(pts + i * AW), k));
}
// work[i] = [k_i] pts[i]: one scalar per point (8 canonical words each), points `stride` words apart.  Every lane starts at the top set
// bit of its own scalar, so the wave walks as many bits as its longest scalar has: 128-bit scalars cost half of full-width ones.
__global__ __launch_bounds__(64) void ecn_mul_scalars_kernel(const u32* __restrict__ pts, u64 stride, u64 n, const u32* __restrict__ k, u32* __restrict__ work) {
    const u64 i = blockIdx.x * 64ull + threadIdx.x;
    if (i >= n) return;
    ecn_st(work + i * EW, ecn_mul(ecn_load_ext(pts + i * stride), k + i * 8));
}
#ifdef ECN_GLV
// work[i] = [k_i] pts[i] through the curve's endomorphism (G1 only; the points must lie in the subgroup of order r, where phi = [lambda]).
// k = s1 |k1| + s2 |k2| lambda with both halves below 2^128 (glv_split), so [k]P = [|k1|]P1 + [|k2|]P2 with P1 = s1 P and
// P2 = s2 phi(P) = (beta x, s2 y): one joint (Straus) walk over the two halves from the higher top bit down -- a doubling per step and
// the addition of P1, P2 or P1 + P2 as the two bits say.  The addend is picked by masks from named values (a branch per table entry would
// make a wave run up to three additions per step; an array indexed by the digit would live in scratch), and the one addition of a step is
// skipped by the lanes whose digit is 00.  The halves are kept as two 128-bit shift registers, top bit first, for the same reason.
// Point operations a wave executes per product, counted from the code below: 1 addition for P1 + P2, then per step 1 doubling and 1
// addition, and the steps are as many as the longest half of the wave has bits: at most 128 doublings + 129 additions (with 64 lanes a
// step in which every digit is 00 does not happen: 4^-64).  The bit walk of ecn_mul_scalars_kernel executes 253 doublings and, under
// divergence, 253 additions for scalars of full width.  The affine answers are the same bytes: the way out is ecn_store_kernel's.
__device__ __forceinline__ cf ecn_pick(u32 m1, u32 m2, u32 m3, const cf& a1, const cf& a2, const cf& a3) {
    cf r;
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = (a1.l[i] & m1) | (a2.l[i] & m2) | (a3.l[i] & m3);
    return r;
}
__global__ __launch_bounds__(64) void ecn_mul_scalars_glv_kernel(const u32* __restrict__ pts, u64 stride, u64 n, const u32* __restrict__ k, u32* __restrict__ work) {
    const u64 i = blockIdx.x * 64ull + threadIdx.x;
    if (i >= n) return;
    const xyzz b = ecn_load_ext(pts + i * stride);
    u32 kk[8], k1[8], k2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kk[j] = k[i * 8 + j];
    bool n1, n2;
    glv_split(kk, k1, k2, n1, n2);
    unsigned __int128 h1 = ((unsigned __int128)(((u64)k1[3] << 32) | k1[2]) << 64) | (((u64)k1[1] << 32) | k1[0]);
    unsigned __int128 h2 = ((unsigned __int128)(((u64)k2[3] << 32) | k2[2]) << 64) | (((u64)k2[1] << 32) | k2[0]);
    const u64 hi = (u64)((h1 | h2) >> 64), lo = (u64)(h1 | h2);
    if (!(hi | lo) || pt_is_inf(b)) { ecn_st(work + i * EW, pt_inf()); return; }
    const int steps = hi ? 128 - __clzll((long long)hi) : 64 - __clzll((long long)lo);
    h1 <<= 128 - steps; h2 <<= 128 - steps;                            // the top bit of the longer half at bit 127
    // the table: P1 = (x, y1), P2 = (beta x, y2), both with ZZ = ZZZ = 1, and P3 = P1 + P2
    const cf ny = cf_sub<4>(cf_zero(), b.Y), one = cf_one();
    xyzz p1 = b, p2 = b;
    if (n1) p1.Y = ny;
    if (n2) p2.Y = ny;
    p2.X = cf_mul(b.X, glv_beta());
    const xyzz p3 = ecn_add(p1, p2);
    xyzz acc = pt_inf();
    for (int s = 0; s < steps; ++s) {
        acc = ecn_dbl(acc);                                             // infinity returns at once
        const u32 d = (u32)(h1 >> 127) | ((u32)(h2 >> 127) << 1);
        h1 <<= 1; h2 <<= 1;
        if (d) {
            u32 m1 = d == 1 ? ~0u : 0u, m2 = d == 2 ? ~0u : 0u, m3 = d == 3 ? ~0u : 0u;
            asm volatile("" : "+v"(m1), "+v"(m2), "+v"(m3));            // masks, not `?:` between structures (ecpt_impl.hip.h pick_fe)
            xyzz q;
            q.X = ecn_pick(m1, m2, m3, p1.X, p2.X, p3.X); q.Y = ecn_pick(m1, m2, m3, p1.Y, p2.Y, p3.Y);
            q.ZZ = ecn_pick(m1, m2, m3, one, one, p3.ZZ); q.ZZZ = ecn_pick(m1, m2, m3, one, one, p3.ZZZ);
            acc = ecn_add(acc, q);
        }
    }
    ecn_st(work + i * EW, acc);
}
#endif
// work[i] = a[i] - b[i]
__global__ __launch_bounds__(64) void ecn_diff_kernel(const u32* __restrict__ a, const u32* __restrict__ b, u64 n, u32* __restrict__ work) {
    const u64 i = blockIdx.x * 64ull + threadIdx.x;
    if (i >= n) return;
    ecn_st(work + i * EW, ecn_add(ecn_load_ext(a + i * AW), pt_neg(ecn_load_ext(b + i * AW))));
}

// Column sums in the group: work[j] = sum over the sets q and the terms k of column j of coef[k] * base_q[rows[k]].  One wave per wire, as
// kg_wire_sums_kernel has it (ONE can sit in every row, most wires in two or three): lane l takes the terms l, l + 64, ... of each set in
// turn, then the 64 partial sums meet in a fixed order -- no atomics.  A coefficient of 1 or r - 1 (nearly all of a circom circuit's)
// costs an addition; any other one a full product.
struct EcnSums { EcCsc s[3]; int n_sets; u32 rm1[8]; };
__device__ __forceinline__ xyzz ecn_shfl_down(const xyzz& p, int d) {
    u32 w[EW];
    ecn_st(w, p);
#pragma unroll
    for (int k = 0; k < EW; ++k) w[k] = __shfl_down(w[k], d, 64);
    return ecn_ld(w);
}
__global__ __launch_bounds__(64) void ecn_column_sums_kernel(const EcnSums S, u32 n_wires, u32* __restrict__ work) {
    const u32 j = blockIdx.x, lane = threadIdx.x;
    if (j >= n_wires) return;
    xyzz acc = pt_inf();
    for (int q = 0; q < S.n_sets; ++q) {
        const EcCsc& M = S.s[q];
        for (u64 k = M.ptr[j] + lane; k < M.ptr[j + 1]; k += 64) {
            xyzz b = ecn_load_ext(M.base + (u64)M.rows[k] * AW);
            const u32* c = M.coef + k * 8;
            u32 not_one = c[0] ^ 1u, not_m1 = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) { if (i) not_one |= c[i]; not_m1 |= c[i] ^ S.rm1[i]; }
            if (!not_m1) b = pt_neg(b);
            else if (not_one) b = ecn_mul(b, c);
            acc = ecn_add(acc, b);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) acc = ecn_add(acc, ecn_shfl_down(acc, d));   // lanes >= d add what nobody reads
    if (lane == 0) ecn_st(work + (u64)j * EW, acc);
}

// ---- the way out: one inversion per workgroup (the tree of fb_mul_kernel) --------------------------------------------------------------
__device__ __forceinline__ fe ecn_leaf(const xyzz& p) {            // ZZZ, or its norm over Fq2
#ifndef MSM_G2
    return p.ZZZ;
#else
    return fe_mul(fe_add(fe_sqr(p.ZZZ.c0), fe_sqr(p.ZZZ.c1)), fe_one());
#endif
}
__device__ __noinline__ void ecn_store_affine(const xyzz& p, const fe& inv_leaf, u32* __restrict__ o) {
#ifndef MSM_G2
    const cf izzz = inv_leaf;
#else
    cf izzz; izzz.c0 = fe_mul(p.ZZZ.c0, inv_leaf); izzz.c1 = fe_mul(fe_sub<2>(fe_zero(), p.ZZZ.c1), inv_leaf);
#endif
    const cf s = cf_mul(p.ZZ, izzz), izz = cf_sqr(s);              // 1 / ZZ = (ZZ / ZZZ)^2
    u32 x[CW_STD], y[CW_STD];
    cf_to_std(cf_mul(p.X, izz), x); cf_to_std(cf_mul(p.Y, izzz), y);
    for (int k = 0; k < CW_STD; ++k) { o[k] = x[k]; o[CW_STD + k] = y[k]; }
}
constexpr int ECN_BLOCK = 256;
__global__ __launch_bounds__(ECN_BLOCK) void ecn_store_kernel(const u32* __restrict__ work, u64 n, u32* __restrict__ out) {
    __shared__ fe node[2 * ECN_BLOCK];                              // heap order, leaves at ECN_BLOCK + lane
    const u32 l = threadIdx.x;
    const u64 i = (u64)blockIdx.x * ECN_BLOCK + l;
    const bool live = i < n;
    xyzz acc = pt_inf();
    if (live) acc = ecn_ld(work + i * EW);
    const bool finite = live && !pt_is_inf(acc);
    node[ECN_BLOCK + l] = finite ? ecn_leaf(acc) : fe_one();
    for (u32 s = ECN_BLOCK / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (l < s) node[s + l] = fe_mul(node[2 * (s + l)], node[2 * (s + l) + 1]);
    }
    __syncthreads();
    if (l == 0) node[1] = fe_inv(node[1]);
    for (u32 s = 1; s < (u32)ECN_BLOCK; s <<= 1) {
        __syncthreads();
        if (l < s) {
            const u32 p = s + l;
            const fe ip = node[p], a = node[2 * p], b = node[2 * p + 1];
            node[2 * p] = fe_mul(ip, b); node[2 * p + 1] = fe_mul(ip, a);
        }
    }
    __syncthreads();
    if (!live) return;
    u32* o = out + i * AW;
    if (!finite) { for (int k = 0; k < AW; ++k) o[k] = 0; return; }
    const fe inv_leaf = node[ECN_BLOCK + l];
    ecn_store_affine(acc, inv_leaf, o);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
static unsigned ecn_blocks(u64 n, unsigned per) {
    ZK_REQUIRE(n < (1ull << 31) * per, "group transform: too many points");
    return (unsigned)((n + per - 1) / per);
}
static void ecn_store(const DevBuf& work, u64 n, void* d_out, hipStream_t st) {
    hipLaunchKernelGGL(ecn_store_kernel, dim3(ecn_blocks(n, ECN_BLOCK)), dim3(ECN_BLOCK), 0, st, (const u32*)work.p, n, (u32*)d_out);
    ZK_HIP(hipGetLastError());
}
// d_points: 2^logn points, in place.  d_tw: 2^(logn - 1) twiddles; d_scale: one scalar for the way out, or null
void ntt_run(void* d_points, int logn, const u32* d_tw, const u32* d_scale, hipStream_t st) {
    const u64 n = 1ull << logn;
    DevBuf work; work.reserve(n * EW * 4);
    hipLaunchKernelGGL(ecn_load_kernel, dim3(ecn_blocks(n, 64)), dim3(64), 0, st, (const u32*)d_points, (u32)logn, (u32*)work.p);
    ZK_HIP(hipGetLastError());
    for (int s = 0; s < logn; ++s) {
        hipLaunchKernelGGL(ecn_stage_kernel, dim3(ecn_blocks(n / 2, 64)), dim3(64), 0, st, (u32*)work.p, d_tw, (u32)logn, (u32)s);
        ZK_HIP(hipGetLastError());
    }
    if (d_scale) {
        hipLaunchKernelGGL(ecn_scale_kernel, dim3(ecn_blocks(n, 64)), dim3(64), 0, st, (u32*)work.p, n, d_scale);
        ZK_HIP(hipGetLastError());
    }
    ecn_store(work, n, d_points, st);
}
void mul_scalar_run(const void* d_pts, u64 n, const u32* d_k, void* d_out, hipStream_t st) {
    if (n == 0) return;
    DevBuf work; work.reserve(n * EW * 4);
    hipLaunchKernelGGL(ecn_mul_scalar_kernel, dim3(ecn_blocks(n, 64)), dim3(64), 0, st, (const u32*)d_pts, n, d_k, (u32*)work.p);
    ZK_HIP(hipGetLastError());
    ecn_store(work, n, d_out, st);
}
void mul_scalars_run(const void* d_pts, u64 stride_words, u64 n, const u32* d_k, void* d_out, hipStream_t st) {
    if (n == 0) return;
    DevBuf work; work.reserve(n * EW * 4);
    hipLaunchKernelGGL(ecn_mul_scalars_kernel, dim3(ecn_blocks(n, 64)), dim3(64), 0, st, (const u32*)d_pts, stride_words, n, d_k, (u32*)work.p);
    ZK_HIP(hipGetLastError());
    ecn_store(work, n, d_out, st);
}
#ifdef ECN_GLV
void mul_scalars_glv_run(const void* d_pts, u64 stride_words, u64 n, const u32* d_k, void* d_out, hipStream_t st) {
    if (n == 0) return;
    DevBuf work; work.reserve(n * EW * 4);
    hipLaunchKernelGGL(ecn_mul_scalars_glv_kernel, dim3(ecn_blocks(n, 64)), dim3(64), 0, st, (const u32*)d_pts, stride_words, n, d_k, (u32*)work.p);
    ZK_HIP(hipGetLastError());
    ecn_store(work, n, d_out, st);
}
#undef ECN_GLV
#else
constexpr auto mul_scalars_glv_run = nullptr;                       // no endomorphism in this group
#endif
void diff_run(const void* d_a, const void* d_b, u64 n, void* d_out, hipStream_t st) {
    if (n == 0) return;
    DevBuf work; work.reserve(n * EW * 4);
    hipLaunchKernelGGL(ecn_diff_kernel, dim3(ecn_blocks(n, 64)), dim3(64), 0, st, (const u32*)d_a, (const u32*)d_b, n, (u32*)work.p);
    ZK_HIP(hipGetLastError());
    ecn_store(work, n, d_out, st);
}
void column_sums_run(const EcCsc* sets, int n_sets, const u32* r, u32 n_wires, void* d_out, hipStream_t st) {
    if (n_wires == 0) return;
    ZK_REQUIRE(n_sets >= 1 && n_sets <= 3, "column sums: one to three matrices");
    EcnSums S;
    for (int q = 0; q < n_sets; ++q) S.s[q] = sets[q];
    for (int q = n_sets; q < 3; ++q) S.s[q] = sets[0];
    S.n_sets = n_sets;
    for (int i = 0; i < 8; ++i) S.rm1[i] = r[i];
    S.rm1[0] -= 1;                                                  // r is odd
    DevBuf work; work.reserve((u64)n_wires * EW * 4);
    hipLaunchKernelGGL(ecn_column_sums_kernel, dim3(n_wires), dim3(64), 0, st, S, n_wires, (u32*)work.p);
    ZK_HIP(hipGetLastError());
    ecn_store(work, n_wires, d_out, st);
}
