// The polynomial side of a KZG opening on gfx950, generic over the scalar field: y = p(z) and q = (p - y) / (X - z) as ONE tiled scan, the
// linear combination of polynomials that folds many openings at one point, and the scalars of the batched verification.  Included by
// kzg.hip inside a namespace that has already pulled in fr29_consts.hip.h, fe29_impl.hip.h and fr_rows_impl.hip.h.  No include guard on
// purpose.  DESIGN.md 3.18 has the algebra and the reasons for the tile.
//
// With h_j = sum_{i >= j} c_i z^(i - j): h_j = c_j + z h_(j+1), y = h_0 and q_j = h_(j+1).  Coefficient i is the affine map x -> c_i + z x,
// a run [a, b) composes to x -> V + z^(b - a) x with V = sum_{a <= i < b} c_i z^(i - a), and every h_j is a suffix composition applied to 0.
// All runs that meet in one scan step have the same length, so only V travels and the factor z^len is one value per step, read from the
// table.  Nothing divides by z: z = 0 is an ordinary point.
//   1. kz_tile_sum_kernel   A_b = sum_k c_(bT+k) z^k per tile of T coefficients: products against the table z^0 .. z^(T-1), four to a
//                           reduction (fe_wide), and a tree of additions -- no dependent chain
//   2. kz_combine_kernel    the same scan one level up, over the aggregates at the point z^T: one workgroup walks them from the top, KZ_SPAN at a
//                           time, carrying h across the steps; it leaves carry_b = h_((b+1)T) per tile and y.  Evaluation stops here
//                           (carry of the last tile is h past the end, zero: the host zeroes the buffer, the kernel need not meet that entry)
//   3. kz_fixup_kernel      per tile again: the suffixes of a lane's 8 coefficients in registers (Horner), the lanes' suffixes by a scan in LDS with
//                           the tile's carry folded into the last lane, then every element fixed up by z^k . (what comes in from above);
//                           kz_fixup_acc_kernel is the same body adding w q to a running sum (openings at several points)
//      kz_interleave_kernel stands apart: the permutation that combines k polynomials into one, sum_i f_i(X^k) X^i
// Value bounds (fe29_impl.hip.h: A B <= 68 for a product of a < A r, b < B r): loaded coefficients, table entries and products are < 2r;
// Horner suffixes < 4r; a scanned value grows by 2r per step from < 6r to < 22r, and meets only factors < 2r (44).
constexpr int KZ_E = 8, KZ_BLOCK = 256, KZ_LOGT = 11, KZ_T = KZ_E * KZ_BLOCK, KZ_S = 512;
static_assert(KZ_T == (1 << KZ_LOGT) && (u64)KZ_T == KZG_TILE && (u64)KZ_S == KZG_SPAN && KZ_S == 2 * KZ_BLOCK, "kzg: tile constants");

struct KzWords { u32 w[NL]; };
struct KzConsts { fe pw[KZ_LOGT + 1]; };             // z^(2^b); pw[0] = z, pw[KZ_LOGT] = z^T

template <int B, int E, class F>
__device__ __forceinline__ void kz_static_for(F&& f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); kz_static_for<B + 1, E>(f); }
}
// 8 words of a plain integer below 2^256 -> its 29-bit limbs, and whether it is below r
__device__ __forceinline__ fe kz_split(const u32 (&w)[NL], bool& below_r) {
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
// the limbs of a canonical value -> 8 words
__device__ __forceinline__ void kz_pack(const fe& x, u32 (&w)[NL]) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int bit = 32 * j, k = bit / LB, s = bit % LB;
        u32 v = x.l[k] >> s;
        if (k + 1 < NR) v |= x.l[k + 1] << (LB - s);
        if (k + 2 < NR && 2 * LB - s < 32) v |= x.l[k + 2] << (2 * LB - s);
        w[j] = v;
    }
}
__device__ __forceinline__ fe kz_rr2() {
    fe c;
#pragma unroll
    for (int k = 0; k < NR; ++k) c.l[k] = RRP29(k);
    return c;
}
__device__ __forceinline__ void kz_load_words(const u32* __restrict__ p, u64 i, u32 (&w)[NL]) {   // element i of 8 words, 16-byte aligned
    const uint4* q = (const uint4*)p + 2 * i;
    const uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void kz_store_words(u32* __restrict__ p, u64 i, const u32 (&w)[NL]) {
    uint4* q = (uint4*)p + 2 * i;
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// coefficient i (Montgomery words), zero beyond n: internal form, < 2r
__device__ __forceinline__ fe kz_coeff(const u32* __restrict__ c, u64 n, u64 i) {
    if (i >= n) return fe_zero();
    u32 w[NL];
    kz_load_words(c, i, w);
    return fe_from_std(w);
}
__device__ __forceinline__ fe kz_fe_load(const u32* __restrict__ p, u64 i) {                      // element-major internal form, 9 words
    fe r;
#pragma unroll
    for (int l = 0; l < NR; ++l) r.l[l] = p[i * NR + l];
    return r;
}
__device__ __forceinline__ void kz_fe_store(u32* __restrict__ p, u64 i, const fe& v) {
#pragma unroll
    for (int l = 0; l < NR; ++l) p[i * NR + l] = v.l[l];
}
// The table: z^e for e = t KZ_E + k sits at [(k NR + limb) KZ_BLOCK + t], so that lane t's k-th factor is one coalesced load per limb
__device__ __forceinline__ fe kz_tab(const u32* __restrict__ tab, int k, int t) {
    fe r;
#pragma unroll
    for (int l = 0; l < NR; ++l) r.l[l] = tab[(k * NR + l) * KZ_BLOCK + t];
    return r;
}
__device__ __forceinline__ fe kz_add_canon(const fe& a, const fe& b) { return fe_canon(fe_add(a, b)); }   // canonical operands, canonical sum

__global__ void kz_setup_kernel(const KzWords z, KzConsts* __restrict__ kc) {
    if (threadIdx.x || blockIdx.x) return;
    bool ok;
    fe x = fe_mul(kz_split(z.w, ok), kz_rr2());
    for (int b = 0; b <= KZ_LOGT; ++b) { kc->pw[b] = x; x = fe_sqr(x); }
}
__global__ __launch_bounds__(KZ_BLOCK) void kz_table_kernel(const KzConsts* __restrict__ kc, u32* __restrict__ tab) {
    const int e = blockIdx.x * KZ_BLOCK + threadIdx.x;                 // KZ_T lanes in all
    fe acc = fe_one();
    for (int b = 0; b < KZ_LOGT; ++b)
        if ((e >> b) & 1) acc = fe_mul(acc, kc->pw[b]);
    const int k = e % KZ_E, t = e / KZ_E;
#pragma unroll
    for (int l = 0; l < NR; ++l) tab[(k * NR + l) * KZ_BLOCK + t] = acc.l[l];
}

// 1. A_b = sum_{k < T} c_(bT + k) z^k, canonical, element-major internal form
__global__ __launch_bounds__(KZ_BLOCK) void kz_tile_sum_kernel(const u32* __restrict__ c, u64 n, const u32* __restrict__ tab, u32* __restrict__ agg) {
    __shared__ fe sh[KZ_BLOCK];
    const int t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * KZ_T + (u64)t * KZ_E;
    fe part = fe_zero();
    if (base < n) {
        fe_wide w;
        fe_wide_zero(w);
        kz_static_for<0, 4>([&](auto K) { constexpr int k = decltype(K)::value; fe_wide_mac(w, kz_coeff(c, n, base + k), kz_tab(tab, k, t)); });
        part = fe_canon(fe_wide_reduce(w));
        fe_wide_zero(w);
        kz_static_for<4, 8>([&](auto K) { constexpr int k = decltype(K)::value; fe_wide_mac(w, kz_coeff(c, n, base + k), kz_tab(tab, k, t)); });
        part = kz_add_canon(part, fe_canon(fe_wide_reduce(w)));
    }
    sh[t] = part;
    for (int s = KZ_BLOCK / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (t < s) sh[t] = kz_add_canon(sh[t], sh[t + s]);
    }
    if (t == 0) kz_fe_store(agg, blockIdx.x, sh[0]);
}

// 2. one workgroup over the m aggregates at Z = z^T, KZ_S at a time from the top: carry_b = sum_{b' > b} A_b' Z^(b' - b - 1) (when carry is not
// null) and y = sum_b A_b Z^b as 8 canonical words.  A lane owns two neighbours; the lanes' pairs are scanned in LDS.
__global__ __launch_bounds__(KZ_BLOCK) void kz_combine_kernel(const u32* __restrict__ agg, u64 m, const KzConsts* __restrict__ kc, u32* __restrict__ carry,
                                                              u32* __restrict__ y_out) {
    __shared__ fe sh[KZ_BLOCK];
    __shared__ fe shm[9];                                              // Z^(2^i)
    const int t = threadIdx.x;
    if (t == 0) {
        fe x = kc->pw[KZ_LOGT];
        for (int i = 0; i < 9; ++i) { shm[i] = x; x = fe_sqr(x); }
    }
    __syncthreads();
    const fe Z = shm[0];
    fe carry_in = fe_zero();                                           // h at the end of the step's span, < 2r
    const long long steps = (long long)((m + KZ_S - 1) / KZ_S);
    for (long long st = steps - 1; st >= 0; --st) {
        const u64 i0 = (u64)st * KZ_S + 2 * (u64)t;
        const fe a0 = i0 < m ? kz_fe_load(agg, i0) : fe_zero(), a1 = i0 + 1 < m ? kz_fe_load(agg, i0 + 1) : fe_zero();
        fe v = fe_add(a0, fe_mul(Z, a1));                              // < 3r
        if (t == KZ_BLOCK - 1) v = fe_add(v, fe_mul(shm[1], carry_in)); // < 5r
        sh[t] = v;
        __syncthreads();
        for (int s = 0; s < 8; ++s) {                                  // lanes 2^s apart are 2^(s+1) aggregates apart
            const int d = 1 << s;
            const bool has = t + d < KZ_BLOCK;
            fe x = fe_zero();
            if (has) x = sh[t + d];
            __syncthreads();
            if (has) sh[t] = fe_add(sh[t], fe_mul(shm[s + 1], x));     // < 5r + 16r
            __syncthreads();
        }
        const fe inc = t == KZ_BLOCK - 1 ? carry_in : sh[t + 1 < KZ_BLOCK ? t + 1 : t];
        const fe h1 = fe_add(a1, fe_mul(Z, inc));                      // h at i0 + 1
        const fe h0 = fe_add(a0, fe_mul(Z, h1));                       // h at i0
        if (carry) {
            if (i0 < m) kz_fe_store(carry, i0, h1);
            if (i0 >= 1 && i0 - 1 < m) kz_fe_store(carry, i0 - 1, h0);
        }
        if (st == 0 && t == 0) fe_store_canon(h0, y_out);
        carry_in = fe_renorm(sh[0]);
        __syncthreads();
    }
}

// 3. q_j = h_(j+1) for the tile's elements, as one body for three ways of leaving them:
//   KZ_Q_MONT   Montgomery words, as the coefficients are
//   KZ_Q_CANON  8 canonical words (the scalars of the sums)
//   KZ_Q_ACC    out_j = acc_j + w h_(j+1), Montgomery words in and out: the quotient by a vanishing polynomial is a weighted sum of quotients
//               by X - s, and this mode adds one of them to the running sum.  Element j is read and written by the one lane that
//               owns h_(j+1), so acc and out may be the same buffer (neither is __restrict__ in kz_fixup_acc_kernel).  Bounds: h < 6r meets
//               w < 2r (12 <= 68), the product is < 2r; acc's words are any integer below 2^256 < 6r against CIN < r, so acc is < 2r on load;
//               the sum < 4r meets COUT < r in fe_to_std, which leaves the canonical value.
enum { KZ_Q_MONT = 0, KZ_Q_CANON = 1, KZ_Q_ACC = 2 };
template <int MODE>
__device__ __forceinline__ void kz_fixup_body(const u32* c, u64 n, const u32* tab, const KzConsts* kc, const u32* carry, u32* q, const u32* acc, const fe* wt) {
    __shared__ fe sh[KZ_BLOCK];
    const int t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * KZ_T + (u64)t * KZ_E;
    const fe z = kc->pw[0];
    fe loc[KZ_E];                                                      // suffixes of the lane's own run, < 4r
    loc[KZ_E - 1] = kz_coeff(c, n, base + KZ_E - 1);
    kz_static_for<1, KZ_E>([&](auto K) {
        constexpr int k = KZ_E - 1 - decltype(K)::value;
        loc[k] = fe_add(kz_coeff(c, n, base + k), fe_mul(z, loc[k + 1]));
    });
    const fe cb = kz_fe_load(carry, blockIdx.x);                       // h at the end of the tile, < 3r
    const fe zE = kz_tab(tab, 0, 1);
    fe v = loc[0];
    if (t == KZ_BLOCK - 1) v = fe_add(v, fe_mul(zE, cb));              // < 6r
    sh[t] = v;
    __syncthreads();
    for (int s = 0; s < 8; ++s) {
        const int d = 1 << s;
        const bool has = t + d < KZ_BLOCK;
        fe x = fe_zero();
        if (has) x = sh[t + d];
        __syncthreads();
        if (has) sh[t] = fe_add(sh[t], fe_mul(kz_tab(tab, 0, d), x));  // z^(KZ_E d); < 6r + 16r
        __syncthreads();
    }
    const fe inc = t == KZ_BLOCK - 1 ? cb : sh[t + 1 < KZ_BLOCK ? t + 1 : t];   // h at the end of the lane's run
    kz_static_for<0, KZ_E>([&](auto K) {
        constexpr int k = decltype(K)::value;
        const u64 i = base + k;                                        // h_i is q_(i-1)
        if (i >= 1 && i < n) {
            const fe h = fe_add(loc[k], fe_mul(k == 0 ? zE : kz_tab(tab, KZ_E - k, 0), inc));
            u32 w[NL];
            if constexpr (MODE == KZ_Q_ACC) {
                kz_load_words(acc, i - 1, w);
                fe_to_std(fe_add(fe_from_std(w), fe_mul(*wt, h)), w);
            } else if constexpr (MODE == KZ_Q_CANON) fe_store_canon(h, w);
            else fe_to_std(h, w);
            kz_store_words(q, i - 1, w);
        }
    });
}
template <bool CANON>
__global__ __launch_bounds__(KZ_BLOCK) void kz_fixup_kernel(const u32* __restrict__ c, u64 n, const u32* __restrict__ tab, const KzConsts* __restrict__ kc,
                                                            const u32* __restrict__ carry, u32* __restrict__ q) {
    kz_fixup_body<CANON ? KZ_Q_CANON : KZ_Q_MONT>(c, n, tab, kc, carry, q, nullptr, nullptr);
}
__global__ __launch_bounds__(KZ_BLOCK) void kz_fixup_acc_kernel(const u32* __restrict__ c, u64 n, const u32* __restrict__ tab, const KzConsts* __restrict__ kc,
                                                                const u32* __restrict__ carry, const fe* __restrict__ wt, const u32* acc, u32* out) {
    kz_fixup_body<KZ_Q_ACC>(c, n, tab, kc, carry, out, acc, wt);
}
// the weight of an accumulating division, 8 canonical words -> internal form, < 2r
__global__ void kz_weight_kernel(const KzWords w, fe* __restrict__ wt) {
    if (threadIdx.x || blockIdx.x) return;
    bool ok;
    *wt = fe_mul(kz_split(w.w, ok), kz_rr2());
}

// Sum_i f_i(X^k) X^i, the combination of fflonk: out[j k + i] = f_i[j] for j < n_max, zero where f_i is shorter.  A permutation of 32-byte
// elements; one lane per OUTPUT element, so a wave's stores are 2 KiB in a row and its loads are k strided streams that the neighbouring
// waves complete.  The block's first element is divided by k once (uniform); a lane then divides a value below k + KZ_BLOCK.
__global__ __launch_bounds__(KZ_BLOCK) void kz_interleave_kernel(const u64* const* __restrict__ polys, const u64* __restrict__ lens, u32 k, u64 total,
                                                                 u32* __restrict__ out) {
    const u64 e0 = (u64)blockIdx.x * KZ_BLOCK, e = e0 + threadIdx.x;
    if (e >= total) return;
    const u32 off = (u32)(e0 % k) + threadIdx.x;
    const u64 j = e0 / k + off / k;
    const u32 i = off % k;
    u32 w[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) w[l] = 0;
    if (j < lens[i]) kz_load_words((const u32*)polys[i], j, w);
    kz_store_words(out, e, w);
}

// out_j = sum_i gamma^i p_i[j], Montgomery words in and out.  The words of x R are taken as the plain integer they are (< 2^256 < 6r) and
// multiplied by gamma in internal form, which keeps the factor R: no conversion on the way in, one canonicalisation on the way out.
__global__ __launch_bounds__(KZ_BLOCK) void kz_lincomb_kernel(const u64* const* __restrict__ polys, const u64* __restrict__ lens, u32 k, u64 n_max,
                                                              const KzConsts* __restrict__ kc, u32* __restrict__ out) {
    const u64 j = (u64)blockIdx.x * KZ_BLOCK + threadIdx.x;
    if (j >= n_max) return;
    const fe g = kc->pw[0];
    fe acc = fe_zero();
    for (u32 i = k; i-- > 0;) {
        acc = fe_mul(acc, g);                                          // < 8r x 2r
        if (j < lens[i]) {
            u32 w[NL];
            bool ok;
            kz_load_words((const u32*)polys[i], j, w);
            acc = fe_add(acc, kz_split(w, ok));                        // < 2r + 6r
        }
    }
    u32 w[NL];
    kz_pack(fe_canon(fe_renorm(acc)), w);
    kz_store_words(out, j, w);
}

// the scalars of the batched check: rz_j = rho_j z_j mod r and y_j packed, 8 canonical words each; flag_j = z_j is not below r
__global__ __launch_bounds__(KZ_BLOCK) void kz_weights_kernel(const u32* __restrict__ open, u64 stride, u64 z_off, u64 m, const u32* __restrict__ rho,
                                                              u32* __restrict__ rz, u32* __restrict__ y, u32* __restrict__ flag) {
    const u64 j = (u64)blockIdx.x * KZ_BLOCK + threadIdx.x;
    if (j >= m) return;
    u32 zw[NL], rw[NL], w[NL];
    for (int i = 0; i < NL; ++i) { zw[i] = open[j * stride + z_off + i]; rw[i] = rho[j * NL + i]; y[j * NL + i] = open[j * stride + z_off + NL + i]; }
    bool z_ok, r_ok;
    const fe zs = kz_split(zw, z_ok), rs = kz_split(rw, r_ok);
    kz_pack(fe_canon(fe_mul(fe_mul(zs, kz_rr2()), rs)), w);            // z R' times the plain rho: z rho, below 2r
    for (int i = 0; i < NL; ++i) rz[j * NL + i] = z_ok ? w[i] : 0u;
    flag[j] = z_ok ? 0u : 1u;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static inline unsigned kz_blocks(u64 n) { return (unsigned)((n + KZ_BLOCK - 1) / KZ_BLOCK); }
static KzWords kz_words(const u32* v) { KzWords w; for (int i = 0; i < NL; ++i) w.w[i] = v[i]; return w; }

// The square chain of z and the table z^0 .. z^(T-1), in one block of table_bytes(): what every division and evaluation at the same z shares
constexpr size_t KZ_TAB_OFF = (sizeof(KzConsts) + 255) / 256 * 256;
size_t table_bytes() { return KZ_TAB_OFF + (size_t)KZ_T * NR * 4; }
void table_dev(const u32* z, void* d_table, hipStream_t st) {
    hipLaunchKernelGGL(kz_setup_kernel, dim3(1), dim3(64), 0, st, kz_words(z), (KzConsts*)d_table);
    hipLaunchKernelGGL(kz_table_kernel, dim3(KZ_T / KZ_BLOCK), dim3(KZ_BLOCK), 0, st, (const KzConsts*)d_table, (u32*)((uint8_t*)d_table + KZ_TAB_OFF));
    ZK_HIP(hipGetLastError());
}
// The three phases.  mode: one of KZ_Q_*; d_q null: evaluation alone.  KZ_Q_ACC: d_q[j] = d_acc[j] + w h_(j+1) with w 8 canonical words on the host
static void kz_divide(const u64* d_coeffs, u64 n, const u32* z, const void* d_table, u64* d_q, int mode, const u64* d_acc, const u32* w, u32* d_y, hipStream_t st) {
    ZK_REQUIRE(n < (1ull << 40), "kzg: more than 2^40 coefficients");
    if (n == 0) { ZK_HIP(hipMemsetAsync(d_y, 0, 4 * NL, st)); return; }
    ZK_REQUIRE(((uintptr_t)d_coeffs | (uintptr_t)d_q | (uintptr_t)d_acc) % 16 == 0, "kzg: coefficient vectors must be 16-byte aligned");
    const u64 tiles = (n + KZ_T - 1) / KZ_T;
    const bool want_q = d_q && n > 1;
    DevBuf own, agg, carry, wt;
    if (!d_table) { own.reserve(table_bytes()); table_dev(z, own.p, st); d_table = own.p; }
    const KzConsts* kc = (const KzConsts*)d_table;
    const u32* tab = (const u32*)((const uint8_t*)d_table + KZ_TAB_OFF);
    agg.reserve(tiles * NR * 4);
    hipLaunchKernelGGL(kz_tile_sum_kernel, dim3((unsigned)tiles), dim3(KZ_BLOCK), 0, st, (const u32*)d_coeffs, n, tab, (u32*)agg.p);
    if (want_q) {
        // carry_(tiles-1) is h past the end, zero, and the one entry kz_combine_kernel may leave unwritten (when tiles is a multiple of KZ_S no lane of a
        // higher step has it as its lower neighbour); the pool hands out recycled blocks, so the zeros are written here
        carry.reserve(tiles * NR * 4);
        ZK_HIP(hipMemsetAsync(carry.p, 0, tiles * NR * 4, st));
    }
    hipLaunchKernelGGL(kz_combine_kernel, dim3(1), dim3(KZ_BLOCK), 0, st, (const u32*)agg.p, tiles, kc, want_q ? (u32*)carry.p : (u32*)nullptr, d_y);
    if (want_q) {
        if (mode == KZ_Q_ACC) {
            wt.reserve(sizeof(fe));
            hipLaunchKernelGGL(kz_weight_kernel, dim3(1), dim3(64), 0, st, kz_words(w), (fe*)wt.p);
            hipLaunchKernelGGL(kz_fixup_acc_kernel, dim3((unsigned)tiles), dim3(KZ_BLOCK), 0, st, (const u32*)d_coeffs, n, tab, kc, (const u32*)carry.p, (const fe*)wt.p,
                               (const u32*)d_acc, (u32*)d_q);
        } else if (mode == KZ_Q_CANON)
            hipLaunchKernelGGL(kz_fixup_kernel<true>, dim3((unsigned)tiles), dim3(KZ_BLOCK), 0, st, (const u32*)d_coeffs, n, tab, kc, (const u32*)carry.p, (u32*)d_q);
        else hipLaunchKernelGGL(kz_fixup_kernel<false>, dim3((unsigned)tiles), dim3(KZ_BLOCK), 0, st, (const u32*)d_coeffs, n, tab, kc, (const u32*)carry.p, (u32*)d_q);
    }
    ZK_HIP(hipGetLastError());
}
// d_table: table_dev's block for this z, or null to build one for this call
void divide_dev(const u64* d_coeffs, u64 n, const u32* z, const void* d_table, u64* d_q, bool q_canon, u32* d_y, hipStream_t st) {
    kz_divide(d_coeffs, n, z, d_table, d_q, q_canon ? KZ_Q_CANON : KZ_Q_MONT, nullptr, nullptr, d_y, st);
}
// d_out[j] = d_acc[j] + w q_j for j < n - 1 (Montgomery words; d_out may be d_acc) and y = p(z): phases 1 and 2 as divide_dev runs them
void divide_acc_dev(const u64* d_coeffs, u64 n, const u32* z, const void* d_table, const u32* w, const u64* d_acc, u64* d_out, u32* d_y, hipStream_t st) {
    kz_divide(d_coeffs, n, z, d_table, d_out, KZ_Q_ACC, d_acc, w, d_y, st);
}
// d_out[j k + i] = p_i[j] for j < n_max; d_polys, d_lens: k device pointers / lengths, on the device
void interleave_dev(const u64* const* d_polys, const u64* d_lens, u32 k, u64 n_max, u64* d_out, hipStream_t st) {
    if (n_max == 0) return;
    hipLaunchKernelGGL(kz_interleave_kernel, dim3(kz_blocks(n_max * k)), dim3(KZ_BLOCK), 0, st, d_polys, d_lens, k, n_max * k, (u32*)d_out);
    ZK_HIP(hipGetLastError());
}

void lincomb_dev(const u64* const* d_polys, const u64* d_lens, u32 k, u64 n_max, const u32* gamma, u64* d_out, hipStream_t st) {
    if (n_max == 0) return;
    DevBuf kc;
    kc.reserve(sizeof(KzConsts));
    hipLaunchKernelGGL(kz_setup_kernel, dim3(1), dim3(64), 0, st, kz_words(gamma), (KzConsts*)kc.p);
    hipLaunchKernelGGL(kz_lincomb_kernel, dim3(kz_blocks(n_max)), dim3(KZ_BLOCK), 0, st, d_polys, d_lens, k, n_max, (const KzConsts*)kc.p, (u32*)d_out);
    ZK_HIP(hipGetLastError());
}

void weights_dev(const u32* d_open, u64 stride, u64 z_off, u64 m, const u32* d_rho, u32* d_rz, u32* d_y, u32* d_flag, hipStream_t st) {
    if (m == 0) return;
    hipLaunchKernelGGL(kz_weights_kernel, dim3(kz_blocks(m)), dim3(KZ_BLOCK), 0, st, d_open, stride, z_off, m, d_rho, d_rz, d_y, d_flag);
    ZK_HIP(hipGetLastError());
}
