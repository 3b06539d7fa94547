// The device side of the PLONK prover over the scalar field on gfx950, generic over the field: the numerator of the quotient
// on the coset as ONE kernel, the row-by-row check of the gate equation, and a gather.  The protocol itself (rounds, transcript, files) is
// eigen_zkvm_amd/plonk.py.  Included by groth16.hip after frpoly_impl.hip.h, in the same namespace: it uses that file's word helpers
// (fp_load_words, fp_split, fp_pack, fp_put_plain), its constants (fp_const_rr2 / _cin / _cout) and its host checks.  No include guard on purpose.
//
// A vector is n x 8 u32 Montgomery words (R = 2^256), element-major, as every zk_fr_<curve>_*_dev leaves it; the words of an input may be any
// integer below 2^256 (< 6r), every output word vector is the canonical representative.
//
// Forms.  R' = 2^261 is the internal radix (fe29_impl.hip.h), fe_mul(x, y) = x y / R'.
//   plain     P(v) = fp_split(words) = the integer the words are, = v R mod r, < 6r          -- no product to make it
//   internal  I(v) = v R'.  fe_mul(I(u), P(v)) = u v R: a product of an internal and a plain value IS plain
// so a, b, c are brought to internal form once (three products, shared by the gate part and both permutation products), every selector, Z,
// Z(wX) and L_1 stay plain, sums of plain values are plain, and the bracket comes out plain: one reduction on the way out (fp_put_plain).
//
// zk_plonk_<curve>_quotient_dev, per lane (pk_quotient_kernel); "=" is the value, "<" the bound against fe29_impl.hip.h's A B <= 68:
//   A, B, C    = I(a), I(b), I(c) by fe_from_std                                     P < 6r times CIN < r: 6.                 < 2r each
//   AB         = fe_mul(A, B) = I(a b)                                               2 x 2 = 4                                < 2r
//   Bx         = fe_mul(P(X), BI) = I(beta X), BI = beta R'^2 / R (< 2r)             6 x 2 = 12                               < 2r
//                beta X is made ONCE; k_1 beta X and k_2 beta X are k_j additions of it when k_j <= PK_SMALL_K (= 3: < 6r), else one more
//                product each by I(k_j) (2 x 2 = 4, < 2r)
//   f_1 .. f_3 = A + Bx + G, B + k_1 Bx + G, C + k_2 Bx + G, G = I(gamma) canonical  (< r)                                    < 5r, < 9r, < 9r
//   P1         = ((f_1 f_2) f_3) P(Z): 5 x 9 = 45 -> < 2r; 2 x 9 = 18 -> < 2r; 2 x 6 = 12 -> plain                            < 2r
//   s_j        = fe_mul(P(S_sigma_j), BI) = I(beta S_sigma_j): 12                                                             < 2r
//   g_j        = A + s_1 + G, B + s_2 + G, C + s_3 + G                                                                        < 5r each
//   P2         = ((g_1 g_2) g_3) P(Z(wX)): 25, 10, 12 -> plain                                                                < 2r
//   D          = P1 - P2 + 2r  (fe_sub<2>, P2 < 2r)                                                                           < 4r
//   u          = fe_mul(P(L_1), A2) = I(alpha^2 L_1), A2 = alpha^2 R'^2 / R (< 2r): 12                                        < 2r
//   zm1        = P(Z) - P(1) + 2r  (fe_sub<2>, P(1) = R mod r < r)                                                            < 8r
//   W          = A P(q_L) + B P(q_R) + C P(q_O) + AB P(q_M) + D AI + u zm1 with ONE reduction (fe_wide_mac, 6 pairs = FE_WIDE_MAX),
//                AI = I(alpha) canonical (< r): 4 x (2 x 6) + 4 x 1 + 2 x 8 = 68                                              < 2r, plain
//   out        = W + P(q_C) + P(PI): < 14r, times R' mod r (< r) in fp_put_plain: 14                                          canonical
// (6r is 2^256 against BN254's r; the true factor is 5.3 there and 2.3 for BLS12-381, so the 68 of W is 61 and 30 in fact.)
// Products: 3 + 1 + 1 + 3 + 3 + 3 + 1 = 15, six multiply-accumulates with one reduction, one on the way out; 2 more when a k_j is large.
// pk_gate_kernel is the first four pairs of W plus q_C + PI over the rows of H (48, then < 14r renormalised and compared with 0 and r).
constexpr int PK_NCOL = 15, PK_GATE_NCOL = 9;
constexpr u32 PK_SMALL_K = 3;
enum { PK_A, PK_B, PK_C, PK_Z, PK_QL, PK_QR, PK_QO, PK_QM, PK_QC, PK_S1, PK_S2, PK_S3, PK_PI, PK_L1, PK_X };   // the order of d_cols
enum { PG_A, PG_B, PG_C, PG_QL, PG_QR, PG_QO, PG_QM, PG_QC, PG_PI };                                          // the order of the gate check's

struct PkCols { const u32* c[PK_NCOL]; };
struct PkConsts { fe BI, G, AI, A2, K1, K2; u32 k1_small, k2_small; };      // k_j when it is <= PK_SMALL_K, else 0

__device__ __forceinline__ fe pk_plain(const u32* v, u64 i) {
    u32 w[NL];
    fp_load_words(v, i, w);
    return fp_split(w);
}
__device__ __forceinline__ fe pk_internal(const u32* v, u64 i) {
    u32 w[NL];
    fp_load_words(v, i, w);
    return fe_from_std(w);
}
// alpha, beta, gamma, k_1, k_2: 8 canonical words each -> the constants of the kernel
__global__ void pk_setup_kernel(const FpWords alpha, const FpWords beta, const FpWords gamma, const FpWords k1, const FpWords k2, PkConsts* __restrict__ pc) {
    if (threadIdx.x || blockIdx.x) return;
    const fe a = fe_mul(fp_split(alpha.w), fp_const_rr2());                    // I(alpha), < 2r
    pc->AI = fe_canon(a);
    pc->A2 = fe_mul(fe_mul(a, a), fp_const_cin());
    pc->BI = fe_mul(fe_mul(fp_split(beta.w), fp_const_rr2()), fp_const_cin());
    pc->G = fe_canon(fe_mul(fp_split(gamma.w), fp_const_rr2()));
    pc->K1 = fe_mul(fp_split(k1.w), fp_const_rr2());
    pc->K2 = fe_mul(fp_split(k2.w), fp_const_rr2());
    u32 hi1 = 0, hi2 = 0;
    for (int j = 1; j < NL; ++j) { hi1 |= k1.w[j]; hi2 |= k2.w[j]; }
    pc->k1_small = (!hi1 && k1.w[0] <= PK_SMALL_K) ? k1.w[0] : 0;
    pc->k2_small = (!hi2 && k2.w[0] <= PK_SMALL_K) ? k2.w[0] : 0;
}
// k x for k in 1 .. PK_SMALL_K by additions (k is the same for every lane), or x I(k) / R'
__device__ __forceinline__ fe pk_times_k(const fe& x, u32 k_small, const fe& KI) {
    if (k_small == 0) return fe_mul(x, KI);
    fe r = x;
    for (u32 j = 1; j < k_small; ++j) r = fe_add(r, x);
    return r;
}
// the first four pairs of W: A P(q_L) + B P(q_R) + C P(q_O) + (A B) P(q_M), unreduced
template <int QL, int QR, int QO, int QM, class Cols>
__device__ __forceinline__ void pk_gate_macs(fe_wide& acc, const Cols& cs, u64 i, const fe& A, const fe& B, const fe& C) {
    fe_wide_mac(acc, A, pk_plain(cs.c[QL], i));
    fe_wide_mac(acc, B, pk_plain(cs.c[QR], i));
    fe_wide_mac(acc, C, pk_plain(cs.c[QO], i));
    fe_wide_mac(acc, fe_mul(A, B), pk_plain(cs.c[QM], i));
}

// out_i = the bracket of round 3 at point i of the coset 7 H_m, m = 4n; Z(wX) is element (i + 4) mod m.  One lane per element.
__global__ __launch_bounds__(FP_BLOCK) void pk_quotient_kernel(const PkCols cs, const PkConsts* __restrict__ pc, u32* __restrict__ out, u64 m) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u64 iw = (i + 4) & (m - 1);
    const fe A = pk_internal(cs.c[PK_A], i), B = pk_internal(cs.c[PK_B], i), C = pk_internal(cs.c[PK_C], i);
    const fe G = pc->G, BI = pc->BI;
    const fe Zp = pk_plain(cs.c[PK_Z], i);
    fe D;
    {
        const fe Bx = fe_mul(pk_plain(cs.c[PK_X], i), BI);
        const fe f1 = fe_add(fe_add(A, Bx), G);
        const fe f2 = fe_add(fe_add(B, pk_times_k(Bx, pc->k1_small, pc->K1)), G);
        const fe f3 = fe_add(fe_add(C, pk_times_k(Bx, pc->k2_small, pc->K2)), G);
        const fe P1 = fe_mul(fe_mul(fe_mul(f1, f2), f3), Zp);
        const fe g1 = fe_add(fe_add(A, fe_mul(pk_plain(cs.c[PK_S1], i), BI)), G);
        const fe g2 = fe_add(fe_add(B, fe_mul(pk_plain(cs.c[PK_S2], i), BI)), G);
        const fe g3 = fe_add(fe_add(C, fe_mul(pk_plain(cs.c[PK_S3], i), BI)), G);
        const fe P2 = fe_mul(fe_mul(fe_mul(g1, g2), g3), pk_plain(cs.c[PK_Z], iw));
        D = fe_sub<2>(P1, P2);
    }
    fe_wide acc;
    fe_wide_zero(acc);
    pk_gate_macs<PK_QL, PK_QR, PK_QO, PK_QM>(acc, cs, i, A, B, C);
    fe_wide_mac(acc, D, pc->AI);
    fe_wide_mac(acc, fe_mul(pk_plain(cs.c[PK_L1], i), pc->A2), fe_sub<2>(Zp, fp_const_cout()));
    const fe W = fe_wide_reduce(acc);
    fp_put_plain(out, i, fe_add(fe_add(W, pk_plain(cs.c[PK_QC], i)), pk_plain(cs.c[PK_PI], i)));
}

struct PkGateCols { const u32* c[PK_GATE_NCOL]; };
// row i of H: q_L a + q_R b + q_O c + q_M a b + q_C + PI = 0?  stat[0] += the rows that fail, stat[1] = min(stat[1], the first of them): the
// lanes count in LDS, one atomic add and one atomic min per workgroup that has a failure (as fp_inverse_kernel reports zeros)
__global__ __launch_bounds__(FP_BLOCK) void pk_gate_kernel(const PkGateCols cs, u64 n, unsigned long long* __restrict__ stat) {
    __shared__ unsigned long long zs[2];
    const int t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * FP_BLOCK + t;
    if (t == 0) { zs[0] = 0; zs[1] = ~0ull; }
    __syncthreads();
    if (i < n) {
        const fe A = pk_internal(cs.c[PG_A], i), B = pk_internal(cs.c[PG_B], i), C = pk_internal(cs.c[PG_C], i);
        fe_wide acc;
        fe_wide_zero(acc);
        pk_gate_macs<PG_QL, PG_QR, PG_QO, PG_QM>(acc, cs, i, A, B, C);
        const fe W = fe_wide_reduce(acc);
        const fe s = fe_renorm(fe_add(fe_add(W, pk_plain(cs.c[PG_QC], i)), pk_plain(cs.c[PG_PI], i)));
        if (!fe_is_zero_m(s)) {
            atomicAdd(&zs[0], 1ull);
            atomicMin(&zs[1], (unsigned long long)i);
        }
    }
    __syncthreads();
    if (t == 0 && zs[0]) {
        atomicAdd(&stat[0], zs[0]);
        atomicMin(&stat[1], zs[1]);
    }
}
// out_i = src[idx_i]; an index that is not below n_src reads nothing, leaves zero and is counted as the gate check counts
__global__ __launch_bounds__(FP_BLOCK) void pk_gather_kernel(const u32* __restrict__ src, u64 n_src, const u32* __restrict__ idx, u64 n, u32* __restrict__ out,
                                                            unsigned long long* __restrict__ stat) {
    __shared__ unsigned long long zs[2];
    const int t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * FP_BLOCK + t;
    if (t == 0) { zs[0] = 0; zs[1] = ~0ull; }
    __syncthreads();
    if (i < n) {
        const u64 j = idx[i];
        u32 w[NL] = {};
        if (j < n_src) fp_load_words(src, j, w);
        else {
            atomicAdd(&zs[0], 1ull);
            atomicMin(&zs[1], (unsigned long long)i);
        }
        fp_store_words(out, i, w);
    }
    __syncthreads();
    if (t == 0 && zs[0]) {
        atomicAdd(&stat[0], zs[0]);
        atomicMin(&stat[1], zs[1]);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// who: the caller's prefix, "plonk" or "fflonk", and further down its call as well ("plonk: quotient")
static FpWords pk_scalar(const std::string& who, const u64* v, const char* what) {
    ZK_REQUIRE(v, who + ": null " + what);
    ZK_REQUIRE(fp_curve().fr_canonical((const u32*)v), who + ": " + what + " is not below the scalar field's modulus");
    FpWords w;
    std::memcpy(w.w, v, 32);
    return w;
}
// the PK_NCOL columns of d_cols, every one there and aligned
static PkCols pk_columns(const std::string& who, const u64* const* d_cols) {
    PkCols cs{};
    for (int c = 0; c < PK_NCOL; ++c) {
        cs.c[c] = (const u32*)d_cols[c];
        ZK_REQUIRE(cs.c[c], who + ": column " + std::to_string(c) + " is null");
        fp_aligned({cs.c[c]});
    }
    return cs;
}
// two vectors of m elements do not overlap
static bool pk_apart(const void* a, const void* b, u64 m) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + m * 32 <= y || y + m * 32 <= x;
}
void FRN_FN(pk_quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, u64* d_out, hipStream_t st) {
    const FpWords a = pk_scalar("plonk", alpha, "alpha"), b = pk_scalar("plonk", beta, "beta"), g = pk_scalar("plonk", gamma, "gamma"), w1 = pk_scalar("plonk", k1, "k1"), w2 = pk_scalar("plonk", k2, "k2");
    if (log_n + 2 > (u32)FRN_S) throw std::runtime_error("plonk: the coset of 2^" + std::to_string(log_n + 2) + " points for n = 2^" + std::to_string(log_n) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(d_cols && d_out, "plonk: null argument");
    const u64 m = 4ull << log_n;
    const PkCols cs = pk_columns("plonk: quotient", d_cols);
    for (int c = 0; c < PK_NCOL; ++c) ZK_REQUIRE(pk_apart(d_out, cs.c[c], m), "plonk: quotient: the output overlaps column " + std::to_string(c));
    fp_aligned({d_out});
    DevBuf pc;
    pc.reserve(sizeof(PkConsts));
    hipLaunchKernelGGL(pk_setup_kernel, dim3(1), dim3(64), 0, st, a, b, g, w1, w2, (PkConsts*)pc.p);
    hipLaunchKernelGGL(pk_quotient_kernel, dim3(fp_blocks(m)), dim3(FP_BLOCK), 0, st, cs, (const PkConsts*)pc.p, (u32*)d_out, m);
    ZK_HIP(hipGetLastError());
}
void FRN_FN(pk_gate_check_dev)(const u64* const* d_cols, u64 n, u64* n_bad, u64* first_bad, hipStream_t st) {
    ZK_REQUIRE(d_cols && n_bad && first_bad, "plonk: null argument");
    fp_limit(n);
    u64 stat[2] = {0, ~0ull};
    if (n) {
        PkGateCols cs{};
        for (int c = 0; c < PK_GATE_NCOL; ++c) {
            cs.c[c] = (const u32*)d_cols[c];
            ZK_REQUIRE(cs.c[c], "plonk: gate check: column " + std::to_string(c) + " is null");
            fp_aligned({cs.c[c]});
        }
        DevBuf ds;
        ds.reserve(16);
        h2d_sync(ds.p, stat, 16);
        hipLaunchKernelGGL(pk_gate_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, cs, n, (unsigned long long*)ds.p);
        ZK_HIP(hipGetLastError());
        d2h_sync(stat, ds.p, 16);
    }
    *n_bad = stat[0];
    *first_bad = stat[1];
}
void FRN_FN(pk_gather_dev)(const u64* d_src, u64 n_src, const u32* d_idx, u64 n, u64* d_out, hipStream_t st) {
    ZK_REQUIRE((d_src || n_src == 0) && ((d_idx && d_out) || n == 0), "plonk: null argument");
    fp_limit(n); fp_limit(n_src);
    if (!n) return;
    fp_aligned({d_src, d_out});
    ZK_REQUIRE((uintptr_t)d_idx % 4 == 0, "plonk: gather: the indices must be 4-byte aligned");
    const uintptr_t s = (uintptr_t)d_src, o = (uintptr_t)d_out;
    ZK_REQUIRE(!n_src || o + n * 32 <= s || s + n_src * 32 <= o, "plonk: gather: the output overlaps the source");
    u64 stat[2] = {0, ~0ull};
    DevBuf ds;
    ds.reserve(16);
    h2d_sync(ds.p, stat, 16);
    hipLaunchKernelGGL(pk_gather_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, (const u32*)d_src, n_src, d_idx, n, (u32*)d_out, (unsigned long long*)ds.p);
    ZK_HIP(hipGetLastError());
    d2h_sync(stat, ds.p, 16);
    ZK_REQUIRE(stat[0] == 0, "plonk: gather: " + std::to_string(stat[0]) + " indices are not below the source's " + std::to_string(n_src) + " elements, the first at position " +
                                 std::to_string(stat[1]));
}
