// Polynomial arithmetic over the scalar field on gfx950, generic over the field: running products as a tiled scan, batch
// inversion, pointwise work, powers, the terms of a grand product, products by transform and quotients by X^N - 1.  No protocol.
// Included by groth16.hip after frntt_impl.hip.h, inside a namespace that has fr29_consts.hip.h, fe29_impl.hip.h and fr_rows_impl.hip.h and
// defines FRP_CURVE (the namespace's CurveId): poly_mul runs frn_transform_batch on the limb-major buffers the transforms own, so the
// pointwise step between the transforms never leaves that layout.  No include guard on purpose.
//
// A vector is n x 8 u32 Montgomery words (R = 2^256), element-major, as zk_fr_<curve>_ntt_dev and zk_kzg_<curve>_divide_dev leave it; the
// words of an input may be any integer below 2^256 (< 6r), every output word vector is the canonical representative.
//
// The running product is the scan of kzg_impl.hip.h with the field product as the operation:
//   1. fp_tile_prod_kernel   A_b = prod of the tile's T elements: a lane's 8 in registers, the lanes' products by a tree in LDS
//   2. fp_combine_kernel     one workgroup walks the aggregates FP_S at a time from the bottom, carrying the product across the steps; it leaves
//                            carry_b = prod_{b' < b} A_b' per tile and the total.  The total alone stops here
//   3. fp_fixup_kernel       per tile again: the prefixes of a lane's 8 elements in registers, the lanes' totals by a scan in LDS with the tile's
//                            carry folded into lane 0, then every element fixed up by (what comes in from below)
// fp_inverse_kernel is Montgomery's trick with ONE inversion per tile: the same two levels (registers, LDS), a prefix and a suffix scan of the
// lanes' totals, the inverse of the tile's total by its last wave, and the way back down.  No device-wide phase, so no scratch beside the counters.
// Value bounds (fe29_impl.hip.h: A B <= 68 for a product of a < A r, b < B r): every scanned value is a product, < 2r, and meets only
// products or loaded elements < 2r (4).  The words of an element taken as the plain integer they are (fp_split) are < 6r; such a value meets
// a factor < 2r (12), sums of two or three of them (< 12r, < 14r with the bias 8r of a difference, < 10r for a term of fp_terms_kernel) meet
// a factor < 2r (28 at most).  fe_to_std takes < 68r against R mod r < r.
constexpr int FP_E = 8, FP_BLOCK = 256, FP_T = FP_E * FP_BLOCK, FP_S = 512;
static_assert((u64)FP_T == FRPOLY_TILE && (u64)FP_S == FRPOLY_SPAN && FP_S == 2 * FP_BLOCK, "frpoly: tile constants");

struct FpWords { u32 w[NL]; };
struct FpPow { fe chain[40]; fe scale; };                            // base^(2^b), b < 40; the factor of every power
struct FpTerms { fe beta, gammaR, fix; };                            // beta R' ; gamma R ; R'^k / R^(k-1): all as plain limbs
struct FpCols { const u32* col[16]; const u32* lab[16]; };

template <int B, int E, class F>
__device__ __forceinline__ void fp_static_for(F&& f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); fp_static_for<B + 1, E>(f); }
}
__device__ __forceinline__ void fp_load_words(const u32* p, u64 i, u32 (&w)[NL]) {                 // element i of 8 words, 16-byte aligned
    const uint4* q = (const uint4*)p + 2 * i;
    const uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void fp_store_words(u32* p, u64 i, const u32 (&w)[NL]) {
    uint4* q = (uint4*)p + 2 * i;
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// 8 words of a plain integer below 2^256 -> its 29-bit limbs
__device__ __forceinline__ fe fp_split(const u32 (&w)[NL]) {
    fe x;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int bit = LB * k, wi = bit >> 5, s = bit & 31;
        u32 v = wi < NL ? w[wi] >> s : 0;
        if (s > 32 - LB && wi + 1 < NL) v |= w[wi + 1] << (32 - s);
        x.l[k] = v & LMASK;
    }
    return x;
}
// the limbs of a canonical value -> 8 words
__device__ __forceinline__ void fp_pack(const fe& x, u32 (&w)[NL]) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int bit = 32 * j, k = bit / LB, s = bit % LB;
        u32 v = x.l[k] >> s;
        if (k + 1 < NR) v |= x.l[k + 1] << (LB - s);
        if (k + 2 < NR && 2 * LB - s < 32) v |= x.l[k + 2] << (2 * LB - s);
        w[j] = v;
    }
}
__device__ __forceinline__ fe fp_const_rr2() { fe c; for (int k = 0; k < NR; ++k) c.l[k] = RRP29(k); return c; }
__device__ __forceinline__ fe fp_const_cin() { fe c; for (int k = 0; k < NR; ++k) c.l[k] = CIN29(k); return c; }
__device__ __forceinline__ fe fp_const_cout() { fe c; for (int k = 0; k < NR; ++k) c.l[k] = COUT29(k); return c; }
// element i in internal form (< 2r); `one` beyond n
__device__ __forceinline__ fe fp_elem(const u32* v, u64 n, u64 i) {
    if (i >= n) return fe_one();
    u32 w[NL];
    fp_load_words(v, i, w);
    return fe_from_std(w);
}
__device__ __forceinline__ void fp_put(u32* v, u64 i, const fe& x) {                               // internal form, < 68r -> canonical Montgomery words
    u32 w[NL];
    fe_to_std(x, w);
    fp_store_words(v, i, w);
}
__device__ __forceinline__ void fp_put_plain(u32* v, u64 i, const fe& x) {                         // x R as a plain integer, < 68r -> canonical words
    u32 w[NL];
    fp_pack(fe_canon(fe_renorm(x)), w);
    fp_store_words(v, i, w);
}
__device__ __forceinline__ fe fp_fe_load(const u32* __restrict__ p, u64 i) {                       // element-major internal form, 9 words
    fe r;
#pragma unroll
    for (int l = 0; l < NR; ++l) r.l[l] = p[i * NR + l];
    return r;
}
__device__ __forceinline__ void fp_fe_store(u32* __restrict__ p, u64 i, const fe& v) {
#pragma unroll
    for (int l = 0; l < NR; ++l) p[i * NR + l] = v.l[l];
}
// a^(r - 2), fe_inv's loop inlined: as a call (which fe_inv becomes in a unit with this many callers) it costs fp_inverse_kernel a stack frame
__device__ __forceinline__ fe fp_inv(const fe& a) {
    fe r = fe_one();
    for (int i = NR - 1; i >= 0; --i) {
        const u32 w = fe_qm2_limb(i);
        for (int b = LB - 1; b >= 0; --b) {
            r = fe_sqr(r);
            if ((w >> b) & 1) r = fe_mul(r, a);
        }
    }
    return r;
}
// inclusive scan of sh[0 .. FP_BLOCK) under the field product, in place; every lane of the workgroup calls it
__device__ __forceinline__ void fp_scan_up(fe* sh, int t) {
    for (int s = 0; s < 8; ++s) {
        const int d = 1 << s;
        const bool has = t >= d;
        fe x = fe_one();
        if (has) x = sh[t - d];
        __syncthreads();
        if (has) sh[t] = fe_mul(x, sh[t]);
        __syncthreads();
    }
}

// ---- 1. running products ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FP_BLOCK) void fp_tile_prod_kernel(const u32* __restrict__ in, u64 n, u32* __restrict__ agg) {
    __shared__ fe sh[FP_BLOCK];
    const int t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * FP_T + (u64)t * FP_E;
    fe part = fe_one();
    if (base < n) {
        part = fp_elem(in, n, base);
        fp_static_for<1, FP_E>([&](auto K) { part = fe_mul(part, fp_elem(in, n, base + decltype(K)::value)); });
    }
    sh[t] = part;
    for (int s = FP_BLOCK / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (t < s) sh[t] = fe_mul(sh[t], sh[t + s]);
    }
    if (t == 0) fp_fe_store(agg, blockIdx.x, sh[0]);
}
// one workgroup over the m aggregates, FP_S at a time: carry_b = prod_{b' < b} A_b' (when carry is not null) and the total as 8 canonical
// words (plain, not Montgomery).  A lane owns two neighbours; the lanes' pairs are scanned in LDS.
__global__ __launch_bounds__(FP_BLOCK) void fp_combine_kernel(const u32* __restrict__ agg, u64 m, u32* __restrict__ carry, u32* __restrict__ total) {
    __shared__ fe sh[FP_BLOCK];
    const int t = threadIdx.x;
    fe carry_in = fe_one();
    const u64 steps = (m + FP_S - 1) / FP_S;
    for (u64 st = 0; st < steps; ++st) {
        const u64 i0 = st * FP_S + 2 * (u64)t;
        const fe a0 = i0 < m ? fp_fe_load(agg, i0) : fe_one(), a1 = i0 + 1 < m ? fp_fe_load(agg, i0 + 1) : fe_one();
        fe v = fe_mul(a0, a1);
        if (t == 0) v = fe_mul(carry_in, v);
        sh[t] = v;
        __syncthreads();
        fp_scan_up(sh, t);
        const fe below = t == 0 ? carry_in : sh[t - 1];                 // the product of everything before aggregate i0
        if (carry) {
            if (i0 < m) fp_fe_store(carry, i0, below);
            if (i0 + 1 < m) fp_fe_store(carry, i0 + 1, fe_mul(below, a0));
        }
        carry_in = sh[FP_BLOCK - 1];
        __syncthreads();
    }
    if (t == 0) fe_store_canon(carry_in, total);
}
// out_i = prod_{j < i} in_j (exclusive) or prod_{j <= i} in_j.  A lane reads its 8 elements before it writes them and no other lane touches
// them: out may be in (neither is __restrict__).
__global__ __launch_bounds__(FP_BLOCK) void fp_fixup_kernel(const u32* in, u64 n, const u32* __restrict__ carry, int inclusive, u32* out) {
    __shared__ fe sh[FP_BLOCK];
    const int t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * FP_T + (u64)t * FP_E;
    fe loc[FP_E];                                                       // prefixes of the lane's own run
    loc[0] = fp_elem(in, n, base);
    fp_static_for<1, FP_E>([&](auto K) { constexpr int k = decltype(K)::value; loc[k] = fe_mul(loc[k - 1], fp_elem(in, n, base + k)); });
    fe v = loc[FP_E - 1];
    if (t == 0) v = fe_mul(fp_fe_load(carry, blockIdx.x), v);
    sh[t] = v;
    __syncthreads();
    fp_scan_up(sh, t);
    const fe below = t == 0 ? fp_fe_load(carry, blockIdx.x) : sh[t - 1];
    fp_static_for<0, FP_E>([&](auto K) {
        constexpr int k = decltype(K)::value;
        if (base + k < n) {
            if (inclusive) fp_put(out, base + k, fe_mul(below, loc[k]));
            else if constexpr (k == 0) fp_put(out, base, below);
            else fp_put(out, base + k, fe_mul(below, loc[k - 1]));
        }
    });
}

// ---- 2. batch inversion: one inversion per tile -----------------------------------------------------------------------------------------
// out_i = 1 / in_i; a zero stays zero and enters the products as 1.  stat[0] += zeros met, stat[1] = min(stat[1], first zero's index).
// With L_t the product of lane t's run: 1 / L_t = (1 / tile total) (prod of the lanes below) (prod of the lanes above), then down the run.
__global__ __launch_bounds__(FP_BLOCK) void fp_inverse_kernel(const u32* in, u64 n, u32* out, unsigned long long* __restrict__ stat) {
    __shared__ fe sh[2 * FP_BLOCK + 1];                                 // prefixes | suffixes | 1 / total
    __shared__ unsigned long long zs[2];
    fe* up = sh;
    fe* dn = sh + FP_BLOCK;
    const int t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * FP_T + (u64)t * FP_E;
    if (t == 0) { zs[0] = 0; zs[1] = ~0ull; }
    fe loc[FP_E];                                                       // prefixes of the lane's own run, zeros taken as 1
    u32 zero = 0;
    fp_static_for<0, FP_E>([&](auto K) {
        constexpr int k = decltype(K)::value;
        fe x = fp_elem(in, n, base + k);
        if (fe_is_zero_m(x)) { zero |= 1u << k; x = fe_one(); }
        if constexpr (k == 0) loc[0] = x; else loc[k] = fe_mul(loc[k - 1], x);
    });
    up[t] = loc[FP_E - 1];
    dn[t] = loc[FP_E - 1];
    __syncthreads();
    if (zero) {
        atomicAdd(&zs[0], (unsigned long long)__popc(zero));
        atomicMin(&zs[1], (unsigned long long)(base + (u64)(__ffs(zero) - 1)));
    }
    for (int s = 0; s < 8; ++s) {                                       // both scans in the same steps
        const int d = 1 << s;
        const bool hu = t >= d, hd = t + d < FP_BLOCK;
        fe a = fe_one(), b = fe_one();
        if (hu) a = up[t - d];
        if (hd) b = dn[t + d];
        __syncthreads();
        if (hu) up[t] = fe_mul(a, up[t]);
        if (hd) dn[t] = fe_mul(dn[t], b);
        __syncthreads();
    }
    if (t >= FP_BLOCK - 64) {                                           // the last wave as a whole: no lane of it would do anything else meanwhile
        const fe ti = fp_inv(up[FP_BLOCK - 1]);
        if (t == FP_BLOCK - 1) sh[2 * FP_BLOCK] = ti;
    }
    __syncthreads();
    fe inv = sh[2 * FP_BLOCK];                                          // 1 / L_t after the two products
    if (t > 0) inv = fe_mul(inv, up[t - 1]);
    if (t + 1 < FP_BLOCK) inv = fe_mul(inv, dn[t + 1]);
    // down the run: the element is read again (the lane's registers hold the prefixes), before its place is written
    fp_static_for<0, FP_E>([&](auto K) {
        constexpr int k = FP_E - 1 - decltype(K)::value;
        const bool z = (zero >> k) & 1;
        fe x = fe_one();
        if (k > 0 && !z) x = fp_elem(in, n, base + k);
        if (base + k < n) {
            fe o = inv;
            if constexpr (k > 0) o = fe_mul(inv, loc[k - 1]);
            fp_put(out, base + k, z ? fe_zero() : o);
        }
        if constexpr (k > 0) inv = fe_mul(inv, x);
    });
    if (t == 0 && zs[0]) {
        atomicAdd(&stat[0], zs[0]);
        atomicMin(&stat[1], zs[1]);
    }
}

// ---- 3. pointwise work --------------------------------------------------------------------------------------------------------------------
// op: ZK_FR_MUL, ZK_FR_ADD, ZK_FR_SUB.  The words a R are taken as the plain integer they are; a product takes the other operand in internal
// form, which keeps the factor R, sums and differences need no conversion at all: one reduction on the way out.
__global__ __launch_bounds__(FP_BLOCK) void fp_pointwise_kernel(int op, const u32* a, const u32* b, u32* out, u64 n) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 wa[NL], wb[NL];
    fp_load_words(a, i, wa); fp_load_words(b, i, wb);
    const fe x = fp_split(wa);
    if (op == ZK_FR_MUL) {
        fp_pack(fe_canon(fe_mul(x, fe_from_std(wb))), wa);
        fp_store_words(out, i, wa);
    } else if (op == ZK_FR_ADD) fp_put_plain(out, i, fe_add(x, fp_split(wb)));
    else fp_put_plain(out, i, fe_sub<8>(x, fp_split(wb)));
}
// v_i <- v_i tab[i mod c], c a power of two
__global__ __launch_bounds__(FP_BLOCK) void fp_scale_cyclic_kernel(u32* v, u64 n, const u32* __restrict__ tab, u64 c) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 wa[NL], wb[NL];
    fp_load_words(v, i, wa); fp_load_words(tab, i & (c - 1), wb);
    fp_pack(fe_canon(fe_mul(fp_split(wa), fe_from_std(wb))), wa);
    fp_store_words(v, i, wa);
}
// base, scale: 8 canonical words each -> the square chain and the factor in internal form
__global__ void fp_pow_setup_kernel(const FpWords base, const FpWords scale, FpPow* __restrict__ pc) {
    if (threadIdx.x || blockIdx.x) return;
    fe x = fe_mul(fp_split(base.w), fp_const_rr2());
    for (int b = 0; b < 40; ++b) { pc->chain[b] = x; x = fe_sqr(x); }
    pc->scale = fe_mul(fp_split(scale.w), fp_const_rr2());
}
// out_i = scale base^i (- 1 with minus_one): frn_pow_table_kernel's form in the element-major layout
__global__ __launch_bounds__(FP_BLOCK) void fp_powers_kernel(const FpPow* __restrict__ pc, int minus_one, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    fe acc = pc->scale;
    for (int b = 0; (i >> b) != 0; ++b)
        if ((i >> b) & 1) acc = fe_mul(acc, pc->chain[b]);
    if (minus_one) acc = fe_sub<2>(acc, fe_one());
    fp_put(out, i, acc);
}
// beta, gamma: 8 canonical words each; k columns
__global__ void fp_terms_setup_kernel(const FpWords beta, const FpWords gamma, u32 k, FpTerms* __restrict__ tc) {
    if (threadIdx.x || blockIdx.x) return;
    tc->beta = fe_mul(fp_split(beta.w), fp_const_rr2());                                   // beta R' as plain limbs
    tc->gammaR = fe_mul(fe_mul(fp_split(gamma.w), fp_const_rr2()), fp_const_cout());       // gamma R' R / R'
    fe f = fe_one();                                                                       // R'
    for (u32 c = 1; c < k; ++c) f = fe_mul(f, fp_const_cin());                             // x (R'^2 / R) / R'
    tc->fix = f;
}
// out_i = prod_c (col_c[i] + beta lab_c[i] + gamma).  A term is built as the plain integer v R (< 10r) and multiplied into the running value,
// which picks up R / R' each time; the running value starts at R'^k / R^(k-1), so that k products leave (prod v) R: one product per column,
// one more where a label takes beta.
__global__ __launch_bounds__(FP_BLOCK) void fp_terms_kernel(const FpCols cs, u32 k, int with_labels, const FpTerms* __restrict__ tc, u32* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const fe beta = tc->beta, gammaR = tc->gammaR;
    fe acc = tc->fix;
    for (u32 c = 0; c < k; ++c) {
        u32 w[NL];
        fp_load_words(cs.col[c], i, w);
        fe v = fe_add(fp_split(w), gammaR);
        if (with_labels) {
            fp_load_words(cs.lab[c], i, w);
            v = fe_add(v, fe_mul(fp_split(w), beta));
        }
        acc = fe_mul(acc, v);
    }
    u32 w[NL];
    fp_pack(fe_canon(acc), w);
    fp_store_words(out, i, w);
}

// ---- 5. products and quotients by X^N - 1 -------------------------------------------------------------------------------------------------
// limb-major a <- a b: stored values are < 16r, one operand is renormalised first; the product is < 2r, the next transform's input contract
__global__ __launch_bounds__(FP_BLOCK) void fp_soa_mul_kernel(u32* __restrict__ a, const u32* __restrict__ b, u64 n) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    soa_store(a, n, i, fe_mul(soa_load(a, n, i), fe_renorm(soa_load(b, n, i))));
}
// p = q (X^N - 1) + rem: lane j owns the residue class j mod N and walks it from the top, adding: q_i = sum_{k >= 1} p_(i + kN), rem_j the whole
// class.  Sums stay plain integers (v R); every stored value is reduced once.  count += the non-zero remainder coefficients.
__global__ __launch_bounds__(FP_BLOCK) void fp_divmod_zh_kernel(const u32* __restrict__ p, u64 n_p, u64 N, u32* __restrict__ q, u32* __restrict__ rem,
                                                               unsigned long long* __restrict__ count) {
    const u64 j = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= N) return;
    fe acc = fe_zero();                                                 // canonical between the steps
    u32 w[NL];
    if (j < n_p) {
        for (u64 k = (n_p - 1 - j) / N; k >= 1; --k) {
            fp_load_words(p, j + k * N, w);
            acc = fe_canon(fe_renorm(fe_add(acc, fp_split(w))));
            if (q) { fp_pack(acc, w); fp_store_words(q, j + (k - 1) * N, w); }
        }
        fp_load_words(p, j, w);
        acc = fe_canon(fe_renorm(fe_add(acc, fp_split(w))));
    }
    u32 any = 0;
#pragma unroll
    for (int l = 0; l < NR; ++l) any |= acc.l[l];
    if (rem) { fp_pack(acc, w); fp_store_words(rem, j, w); }
    if (any) atomicAdd(count, 1ull);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
static inline unsigned fp_blocks(u64 n) { return (unsigned)((n + FP_BLOCK - 1) / FP_BLOCK); }
static const Curve& fp_curve() { return curve(FRP_CURVE); }
static FpWords fp_scalar(const u64* v, const char* what) {
    ZK_REQUIRE(v, std::string("frpoly: null ") + what);
    ZK_REQUIRE(fp_curve().fr_canonical((const u32*)v), std::string("frpoly: ") + what + " is not below the scalar field's modulus");
    FpWords w;
    std::memcpy(w.w, v, 32);
    return w;
}
static void fp_aligned(std::initializer_list<const void*> ps) {
    for (const void* p : ps) ZK_REQUIRE((uintptr_t)p % 16 == 0, "frpoly: vectors must be 16-byte aligned");
}
static void fp_limit(u64 n) { ZK_REQUIRE(n < (1ull << 40), "frpoly: more than 2^40 elements"); }

void FRN_FN(fp_prefix_product_dev)(const u64* d_in, u64 n, bool inclusive, u64* d_out, u64* total_out, hipStream_t st) {
    ZK_REQUIRE(total_out && (d_in || n == 0), "frpoly: null argument");
    fp_limit(n);
    if (n == 0) { total_out[0] = 1; total_out[1] = total_out[2] = total_out[3] = 0; return; }
    fp_aligned({d_in, d_out});
    const u64 tiles = (n + FP_T - 1) / FP_T;
    DevBuf agg, carry, tot;
    agg.reserve(tiles * NR * 4); tot.reserve(32);
    if (d_out) carry.reserve(tiles * NR * 4);
    hipLaunchKernelGGL(fp_tile_prod_kernel, dim3((unsigned)tiles), dim3(FP_BLOCK), 0, st, (const u32*)d_in, n, (u32*)agg.p);
    hipLaunchKernelGGL(fp_combine_kernel, dim3(1), dim3(FP_BLOCK), 0, st, (const u32*)agg.p, tiles, (u32*)carry.p, (u32*)tot.p);
    if (d_out)
        hipLaunchKernelGGL(fp_fixup_kernel, dim3((unsigned)tiles), dim3(FP_BLOCK), 0, st, (const u32*)d_in, n, (const u32*)carry.p, inclusive ? 1 : 0, (u32*)d_out);
    ZK_HIP(hipGetLastError());
    d2h_sync(total_out, tot.p, 32);
}

void FRN_FN(fp_batch_inverse_dev)(const u64* d_in, u64 n, u64* d_out, u64* n_zero, u64* first_zero, hipStream_t st) {
    ZK_REQUIRE((d_in && d_out) || n == 0, "frpoly: null argument");
    fp_limit(n);
    u64 stat[2] = {0, ~0ull};
    if (n) {
        fp_aligned({d_in, d_out});
        DevBuf ds;
        ds.reserve(16);
        h2d_sync(ds.p, stat, 16);
        hipLaunchKernelGGL(fp_inverse_kernel, dim3((unsigned)((n + FP_T - 1) / FP_T)), dim3(FP_BLOCK), 0, st, (const u32*)d_in, n, (u32*)d_out, (unsigned long long*)ds.p);
        ZK_HIP(hipGetLastError());
        if (n_zero || first_zero) d2h_sync(stat, ds.p, 16);
    }
    if (n_zero) *n_zero = stat[0];
    if (first_zero) *first_zero = stat[1];
}

void FRN_FN(fp_pointwise_dev)(int op, const u64* d_a, const u64* d_b, u64* d_out, u64 n, hipStream_t st) {
    ZK_REQUIRE(op == ZK_FR_MUL || op == ZK_FR_ADD || op == ZK_FR_SUB, "frpoly: unknown pointwise operation " + std::to_string(op) + " (ZK_FR_MUL | ZK_FR_ADD | ZK_FR_SUB)");
    ZK_REQUIRE((d_a && d_b && d_out) || n == 0, "frpoly: null argument");
    fp_limit(n);
    if (!n) return;
    fp_aligned({d_a, d_b, d_out});
    hipLaunchKernelGGL(fp_pointwise_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, op, (const u32*)d_a, (const u32*)d_b, (u32*)d_out, n);
    ZK_HIP(hipGetLastError());
}

static void fp_powers(const FpWords& base, const FpWords& scale, bool minus_one, u64 n, u64* d_out, hipStream_t st) {
    DevBuf pc;
    pc.reserve(sizeof(FpPow));
    hipLaunchKernelGGL(fp_pow_setup_kernel, dim3(1), dim3(64), 0, st, base, scale, (FpPow*)pc.p);
    hipLaunchKernelGGL(fp_powers_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, (const FpPow*)pc.p, minus_one ? 1 : 0, (u32*)d_out, n);
    ZK_HIP(hipGetLastError());
}
void FRN_FN(fp_powers_dev)(const u64* base, const u64* scale, u64 n, u64* d_out, hipStream_t st) {
    const FpWords b = fp_scalar(base, "base"), s = fp_scalar(scale, "scale");
    ZK_REQUIRE(d_out || n == 0, "frpoly: null argument");
    fp_limit(n);
    if (!n) return;
    fp_aligned({d_out});
    fp_powers(b, s, false, n, d_out, st);
}

void FRN_FN(fp_terms_dev)(const u64* const* d_cols, const u64* const* d_labels, u32 k, u64 n, const u64* beta, const u64* gamma, u64* d_out, hipStream_t st) {
    ZK_REQUIRE(k >= 1 && k <= 16, "frpoly: " + std::to_string(k) + " columns, a term takes 1 to 16");
    const FpWords b = fp_scalar(beta, "beta"), g = fp_scalar(gamma, "gamma");
    ZK_REQUIRE(d_cols && (d_out || n == 0), "frpoly: null argument");
    fp_limit(n);
    FpCols cs{};
    for (u32 c = 0; c < k; ++c) {
        cs.col[c] = (const u32*)d_cols[c];
        cs.lab[c] = d_labels ? (const u32*)d_labels[c] : nullptr;
        ZK_REQUIRE(n == 0 || (cs.col[c] && (!d_labels || cs.lab[c])), "frpoly: null column");
        fp_aligned({cs.col[c], cs.lab[c]});
    }
    if (!n) return;
    fp_aligned({d_out});
    DevBuf tc;
    tc.reserve(sizeof(FpTerms));
    hipLaunchKernelGGL(fp_terms_setup_kernel, dim3(1), dim3(64), 0, st, b, g, k, (FpTerms*)tc.p);
    hipLaunchKernelGGL(fp_terms_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, cs, k, d_labels ? 1 : 0, (const FpTerms*)tc.p, (u32*)d_out, n);
    ZK_HIP(hipGetLastError());
}

// z_0 = 1, z_(i+1) = z_i num_i / den_i: the inverses, the ratios, their exclusive running product
void FRN_FN(fp_grand_product_dev)(const u64* d_num, const u64* d_den, u64 n, u64* d_z, u64* last_out, hipStream_t st) {
    ZK_REQUIRE(last_out && ((d_num && d_den && d_z) || n == 0), "frpoly: null argument");
    fp_limit(n);
    DevBuf t;
    if (n) t.reserve(n * 32);
    u64 n_zero = 0, first = 0;
    FRN_FN(fp_batch_inverse_dev)(d_den, n, (u64*)t.p, &n_zero, &first, st);
    ZK_REQUIRE(n_zero == 0, "frpoly: grand product: the denominator of row " + std::to_string(first) + " is zero (" + std::to_string(n_zero) + " zero denominators in all)");
    FRN_FN(fp_pointwise_dev)(ZK_FR_MUL, d_num, (const u64*)t.p, (u64*)t.p, n, st);
    FRN_FN(fp_prefix_product_dev)((const u64*)t.p, n, false, d_z, last_out, st);
}

void FRN_FN(fp_poly_mul_dev)(const u64* d_a, u64 na, const u64* d_b, u64 nb, u64* d_out, hipStream_t st) {
    ZK_REQUIRE(na >= 1 && nb >= 1, "frpoly: poly_mul: an operand has no coefficients");
    fp_limit(na); fp_limit(nb);
    const u64 n_out = na + nb - 1;
    int logn = 0;
    while ((1ull << logn) < n_out) ++logn;
    if (logn > FRN_S) throw std::runtime_error("fr ntt: domain of 2^" + std::to_string(logn) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(d_a && d_b && d_out, "frpoly: null argument");
    ZK_REQUIRE(d_out != d_a && d_out != d_b, "frpoly: poly_mul: the output must not be an operand");
    fp_aligned({d_a, d_b, d_out});
    const FrDomain& D = frn_domain(logn, st);
    const u64 n = 1ull << logn;
    DevBuf buf[4];
    for (auto& x : buf) x.reserve(n * NR * 4);
    hipLaunchKernelGGL(frn_from_std_kernel, dim3(frn_blocks(n)), dim3(256), 0, st, (const u32*)d_a, (u32*)buf[0].p, n, na);
    hipLaunchKernelGGL(frn_from_std_kernel, dim3(frn_blocks(n)), dim3(256), 0, st, (const u32*)d_b, (u32*)buf[1].p, n, nb);
    u32* v[2] = {(u32*)buf[0].p, (u32*)buf[1].p};
    u32* s[2] = {(u32*)buf[2].p, (u32*)buf[3].p};
    if (frn_transform_batch(D, v, s, 2, false, nullptr, nullptr, n, st)) for (int i = 0; i < 2; ++i) std::swap(v[i], s[i]);
    hipLaunchKernelGGL(fp_soa_mul_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, v[0], (const u32*)v[1], n);
    ZK_HIP(hipGetLastError());
    const u32* res = frn_transform(D, v[0], s[0], true, nullptr, (const u32*)D.minv(), 1, st);
    hipLaunchKernelGGL(frn_to_std_kernel, dim3(frn_blocks(n_out)), dim3(256), 0, st, res, (u32*)d_out, n, n_out);
    ZK_HIP(hipGetLastError());
}

void FRN_FN(fp_divmod_zh_dev)(const u64* d_p, u64 n_p, u32 log_n, u64* d_q, u64* d_rem, u64* rem_nonzero, hipStream_t st) {
    ZK_REQUIRE(log_n <= 32, "frpoly: divmod_zh: log_n is " + std::to_string(log_n) + ", at most 32");
    fp_limit(n_p);
    const u64 N = 1ull << log_n, ratio = (n_p + N - 1) / N;
    ZK_REQUIRE(ratio <= ZK_FRPOLY_MAX_RATIO, "frpoly: divmod_zh: " + std::to_string(n_p) + " coefficients over X^" + std::to_string(N) + " - 1 is a chain of " + std::to_string(ratio) +
                                                 " additions per lane, more than ZK_FRPOLY_MAX_RATIO (" + std::to_string(ZK_FRPOLY_MAX_RATIO) + "); for a linear divisor use zk_kzg_" +
                                                 fp_curve().abi_name + "_divide_dev");
    ZK_REQUIRE(d_p || n_p == 0, "frpoly: null argument");
    ZK_REQUIRE(!d_q || n_p <= N || (d_q != d_p), "frpoly: divmod_zh: the quotient must not overwrite the dividend");
    fp_aligned({d_p, d_q, d_rem});
    u64 count = 0;
    DevBuf dc;
    dc.reserve(8);
    h2d_sync(dc.p, &count, 8);
    hipLaunchKernelGGL(fp_divmod_zh_kernel, dim3(fp_blocks(N)), dim3(FP_BLOCK), 0, st, (const u32*)d_p, n_p, N, (u32*)d_q, (u32*)d_rem, (unsigned long long*)dc.p);
    ZK_HIP(hipGetLastError());
    if (rem_nonzero) d2h_sync(rem_nonzero, dc.p, 8);
}

// d_evals_i <- d_evals_i / (7^N w_m^(iN) - 1): the m / N distinct factors from the powers of w_m^N, one batch inversion, one pointwise pass
void FRN_FN(fp_divide_zh_coset_dev)(u64* d_evals, u32 log_m, u32 log_n, hipStream_t st) {
    if (log_m > (u32)FRN_S) throw std::runtime_error("fr ntt: domain of 2^" + std::to_string(log_m) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(log_n <= log_m, "frpoly: divide_zh_coset: N = 2^" + std::to_string(log_n) + " exceeds the domain of 2^" + std::to_string(log_m));
    ZK_REQUIRE(d_evals, "frpoly: null argument");
    fp_aligned({d_evals});
    const FrHost F(fp_curve());
    const u64 m = 1ull << log_m, c = 1ull << (log_m - log_n);
    u64 w[4], g[4], t[4];
    const u64 seven[4] = {7, 0, 0, 0}, e[4] = {1ull << log_n, 0, 0, 0};
    F.omega((int)(log_m - log_n), t); F.from_mont(t, w);               // w_m^N, the root of order m / N
    F.to_mont(seven, t); F.pow(t, e, t); F.from_mont(t, g);            // 7^N
    FpWords base, scale;
    std::memcpy(base.w, w, 32); std::memcpy(scale.w, g, 32);
    DevBuf tab;
    tab.reserve(c * 32);
    fp_powers(base, scale, true, c, (u64*)tab.p, st);
    FRN_FN(fp_batch_inverse_dev)((const u64*)tab.p, c, (u64*)tab.p, nullptr, nullptr, st);
    hipLaunchKernelGGL(fp_scale_cyclic_kernel, dim3(fp_blocks(m)), dim3(FP_BLOCK), 0, st, (u32*)d_evals, m, (const u32*)tab.p, c);
    ZK_HIP(hipGetLastError());
}
