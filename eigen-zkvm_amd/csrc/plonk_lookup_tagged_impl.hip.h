// The device side of PLONK's TAGGED lookup argument over the scalar field on gfx950, generic over the field: several tables in
// one circuit, a row bound to its table by a fourth column.  Table row j is (T0_j, t1_j, t2_j, t3_j) with T0_j = k in 1 .. PLT_MAX_TAG the
// number of its table; a gate row with q_K = k != 0 claims that (a, b, c) is a row of table k, and q_K is both the row's tag and its weight.
// Included by groth16.hip after plonk_lookup_impl.hip.h, in the same namespace: it uses that file's pl_canon_words and PL_EMPTY / PL_ROUNDS,
// frpoly_impl.hip.h's word helpers and host checks and plonk_impl.hip.h's pk_plain / pk_scalar / pk_apart.  The three-column kernels of
// plonk_lookup_impl.hip.h are not touched: these are kernels of their own, so that the register counts of those cannot move.  The summand
// (pl_summands_kernel) and the running sum (fps_*) are the three-column argument's, reused as they are.  No include guard on purpose.
//
// Forms and the bound A B <= 68 as in plonk_lookup_impl.hip.h.  What one more column changes:
//  the constants (plt_setup_kernel): E1, E2, DP, A3 as there, and
//   E3 = I(eta^3) = fe_mul(E2, E1): 2 x 2 = 4                                                                                  < 2r
//  lookup_tagged_terms, per lane (plt_term)
//   out = P(x) + fe_mul(P(y), E1) + fe_mul(P(z), E2) + fe_mul(P(w), E3) + DP: products 6 x 2 = 12 each;
//         the sum 6r + 2r + 2r + 2r + r                                                                                        < 13r, fp_put_plain: 13
//  lookup_tagged_quotient, per lane (plt_quotient_kernel)
//   Fp = P(delta + f), Tp = P(delta + t)  as lookup_tagged_terms                                                               < 13r each
//   X1 = fe_mul(Fp, A3) = I(alpha^3 (delta + f)): 13 x 2 = 26                                                                  < 2r
//   TA = fe_mul(Tp, A3) = I(alpha^3 (delta + t)): 26                                                                           < 2r
//   TI = fe_mul(Tp, CIN) = I(delta + t): 13 x 1                                                                                < 2r
//   X2, D, NQ, W and out as in pl_quotient_kernel: 4; < 14r; <= 8r; 2 x 14 + 2 x 8 + 2 x 6 = 56; 8                             canonical
//  Products per lane: 6 + 4 + three multiply-accumulates with one reduction + one on the way out (the three-column term: 4 + 4 + ...).
//  the tag as an integer (plt_keys_kernel)
//   fe_mul(P(T0), 2^5) = T0 R 2^5 / R' = T0 (R' / R = 2^(29 NR - 256) = 2^5): 6 x 1, then fe_canon                             the integer, < r
//  the multiplicities (plt_counts_out_kernel)
//   m_j = T0_j cnt_j as an INTEGER: T0_j <= 65535 < 2^16 and cnt_j <= n <= ZK_PLONK_LOOKUP_MAX_ROWS = 2^30, so the product is below 2^46 and
//   fits the two low 29-bit limbs (58 bits: limb 0 takes 29 bits, limb 1 the 17 left); times R'^2 / R' = I(.) (1 x 1), then fe_to_std.
//
// The hash table is plonk_lookup_impl.hip.h's with a key of 32 words: the CANONICAL Montgomery representatives of T0, t1, t2, t3 in that
// order (8 whole uint4s), the same FNV-1a over the 32 words, the same slots, walk, atomicCAS and atomicMin.  The same (t1, t2, t3) under two
// tags are two keys.  The count forms a row's key from (q_K, a, b, c): a tuple that sits in another table than the one q_K names is a miss.
constexpr int PLT_KEY = 4 * NL;                    // words of a tagged key
constexpr u32 PLT_MAX_TAG = 65535;                 // ZK_PLONK_LOOKUP_MAX_TABLES
constexpr int PLT_TERMS_NCOL = 8, PLT_QUOT_NCOL = 10;
enum { PLTQ_A, PLTQ_B, PLTQ_C, PLTQ_QK, PLTQ_T1, PLTQ_T2, PLTQ_T3, PLTQ_T0, PLTQ_M, PLTQ_PHI };    // the order of lookup_tagged_quotient's d_cols
static_assert(PLT_KEY % 4 == 0 && NR * LB - 32 * NL == 5, "plonk lookup: a tagged key is whole uint4s; R' / R = 2^5");

struct PltConsts { fe E1, E2, E3, DP, A3; };
struct PltTermCols { const u32* c[PLT_TERMS_NCOL]; };
struct PltQuotCols { const u32* c[PLT_QUOT_NCOL]; };

// ---- 1. the hash table and the count --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 plt_hash(const u32 (&key)[PLT_KEY]) {
    u32 h = 0x811c9dc5u;
#pragma unroll
    for (int j = 0; j < PLT_KEY; ++j) h = (h ^ key[j]) * 0x01000193u;
    return h ^ (h >> 16);
}
__device__ __forceinline__ bool plt_same(const u32 (&key)[PLT_KEY], const u32* __restrict__ keys, u32 row) {
    const uint4* q = (const uint4*)(keys + (u64)row * PLT_KEY);
    u32 d = 0;
#pragma unroll
    for (int j = 0; j < PLT_KEY / 4; ++j) {
        const uint4 x = q[j];
        d |= (x.x ^ key[4 * j]) | (x.y ^ key[4 * j + 1]) | (x.z ^ key[4 * j + 2]) | (x.w ^ key[4 * j + 3]);
    }
    return d == 0;
}
// keys[j] = the key of table row j, tags[j] = T0_j as an integer (0 where it is none of 1 .. PLT_MAX_TAG: counted in stat[0], the smallest
// such row in stat[1])
__global__ __launch_bounds__(FP_BLOCK) void plt_keys_kernel(const u32* __restrict__ t0, const u32* __restrict__ t1, const u32* __restrict__ t2, const u32* __restrict__ t3, u64 T,
                                                           u32* __restrict__ keys, u32* __restrict__ tags, unsigned long long* __restrict__ stat) {
    const u64 j = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= T) return;
    u32 key[PLT_KEY];
    pl_canon_words(t0, j, key); pl_canon_words(t1, j, key + NL); pl_canon_words(t2, j, key + 2 * NL); pl_canon_words(t3, j, key + 3 * NL);
    uint4* q = (uint4*)(keys + j * PLT_KEY);
#pragma unroll
    for (int k = 0; k < PLT_KEY / 4; ++k) q[k] = make_uint4(key[4 * k], key[4 * k + 1], key[4 * k + 2], key[4 * k + 3]);
    fe c = fe_zero();
    c.l[0] = 1u << (NR * LB - 32 * NL);
    const fe v = fe_canon(fe_mul(pk_plain(t0, j), c));
    u32 high = v.l[1] >> (32 - LB);
#pragma unroll
    for (int k = 2; k < NR; ++k) high |= v.l[k];
    const u32 tag = v.l[0] | (v.l[1] << LB);
    const bool ok = high == 0 && tag >= 1 && tag <= PLT_MAX_TAG;
    tags[j] = ok ? tag : 0;
    if (!ok) {
        atomicAdd(&stat[0], 1ull);
        atomicMin(&stat[1], (unsigned long long)j);
    }
}
// row j into the slots (all PL_EMPTY before the launch): pl_insert_kernel over the wider key
__global__ __launch_bounds__(FP_BLOCK) void plt_insert_kernel(const u32* __restrict__ keys, u64 T, u32* slots, u32 mask) {
    const u64 j = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= T) return;
    u32 key[PLT_KEY];
    const uint4* q = (const uint4*)(keys + j * PLT_KEY);
#pragma unroll
    for (int k = 0; k < PLT_KEY / 4; ++k) { const uint4 x = q[k]; key[4 * k] = x.x; key[4 * k + 1] = x.y; key[4 * k + 2] = x.z; key[4 * k + 3] = x.w; }
    u32 h = plt_hash(key) & mask;
    for (u32 step = 0; step <= mask; ++step) {
        const u32 cur = atomicCAS(&slots[h], PL_EMPTY, (u32)j);
        if (cur == PL_EMPTY) return;
        if (plt_same(key, keys, cur)) { atomicMin(&slots[h], (u32)j); return; }
        h = (h + 1) & mask;
    }
}
// one lane per row of H, as pl_count_kernel: a selected row (q_K != 0) looks (q_K, a, b, c) up and adds 1 to its table row's counter.  The
// counters are COUNTS: the weight T0 is applied by plt_counts_out_kernel.  Every lane on one counter holds the same key, so the same tag, and
// the popcount of the wave's combining is the count whatever the tag.  A tuple found only under another tag is a miss.
__global__ __launch_bounds__(FP_BLOCK) void plt_count_kernel(const u32* __restrict__ keys, const u32* __restrict__ slots, u32 mask, const u32* __restrict__ a, const u32* __restrict__ b,
                                                            const u32* __restrict__ c, const u32* __restrict__ qk, u64 n, u32* __restrict__ cnt,
                                                            unsigned long long* __restrict__ stat) {
    __shared__ unsigned long long zs[2];
    const int t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * FP_BLOCK + t;
    if (t == 0) { zs[0] = 0; zs[1] = ~0ull; }
    __syncthreads();
    u32 target = PL_EMPTY;
    if (i < n && !fe_is_zero_m(fe_renorm(pk_plain(qk, i)))) {
        u32 key[PLT_KEY];
        pl_canon_words(qk, i, key); pl_canon_words(a, i, key + NL); pl_canon_words(b, i, key + 2 * NL); pl_canon_words(c, i, key + 3 * NL);
        u32 h = plt_hash(key) & mask;
        for (u32 step = 0; step <= mask; ++step) {
            const u32 row = slots[h];
            if (row == PL_EMPTY) break;
            if (plt_same(key, keys, row)) { target = row; break; }
            h = (h + 1) & mask;
        }
        if (target == PL_EMPTY) {
            atomicAdd(&zs[0], 1ull);
            atomicMin(&zs[1], (unsigned long long)i);
        }
    }
    for (int round = 0; round < PL_ROUNDS; ++round) {                   // every lane of the wave walks these together
        const unsigned long long left = __ballot(target != PL_EMPTY);
        if (!left) break;
        const int leader = __ffsll(left) - 1;
        const u32 lt = __shfl(target, leader, 64);
        const unsigned long long same = __ballot(target == lt);
        if ((t & 63) == leader) atomicAdd(&cnt[lt], (u32)__popcll(same));
        if (target == lt) target = PL_EMPTY;
    }
    if (target != PL_EMPTY) atomicAdd(&cnt[target], 1u);
    __syncthreads();
    if (t == 0 && zs[0]) {
        atomicAdd(&stat[0], zs[0]);
        atomicMin(&stat[1], zs[1]);
    }
}
// m_i = T0_i cnt[i] for i < T, 0 from T on, as Montgomery words.  The product is an integer below 2^46 (T0 < 2^16, cnt <= n <= 2^30): 29 bits
// in limb 0, at most 17 in limb 1; times R'^2 / R' = I(.), then fe_to_std
__global__ __launch_bounds__(FP_BLOCK) void plt_counts_out_kernel(const u32* __restrict__ cnt, const u32* __restrict__ tags, u64 T, u64 n, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 v = i < T ? (u64)tags[i] * cnt[i] : 0;
    fe x = fe_zero();
    x.l[0] = (u32)v & LMASK; x.l[1] = (u32)(v >> LB);
    fp_put(out, i, fe_mul(x, fp_const_rr2()));
}

// ---- 2. the denominators and the quotient's term --------------------------------------------------------------------------------------------
__global__ void plt_setup_kernel(const FpWords eta, const FpWords delta, const FpWords alpha, PltConsts* __restrict__ pc) {
    if (threadIdx.x || blockIdx.x) return;
    const fe e = fe_mul(fp_split(eta.w), fp_const_rr2());
    const fe e2 = fe_mul(e, e);
    pc->E1 = e;
    pc->E2 = e2;
    pc->E3 = fe_mul(e2, e);
    pc->DP = fe_canon(fe_mul(fe_mul(fp_split(delta.w), fp_const_rr2()), fp_const_cout()));
    const fe a = fe_mul(fp_split(alpha.w), fp_const_rr2());
    pc->A3 = fe_mul(fe_mul(fe_mul(a, a), a), fp_const_cin());
}
// P(delta + x + eta y + eta^2 z + eta^3 w) < 13r
__device__ __forceinline__ fe plt_term(const u32* x, const u32* y, const u32* z, const u32* w, u64 i, const PltConsts* __restrict__ pc) {
    return fe_add(fe_add(fe_add(pk_plain(x, i), fe_mul(pk_plain(y, i), pc->E1)), fe_add(fe_mul(pk_plain(z, i), pc->E2), pc->DP)), fe_mul(pk_plain(w, i), pc->E3));
}
// out_i = delta + f_i, out_(n+i) = delta + t_i: 2n lanes.  The columns: a, b, c, q_K, then t1, t2, t3, T0
__global__ __launch_bounds__(FP_BLOCK) void plt_terms_kernel(const PltTermCols cs, const PltConsts* __restrict__ pc, u64 n, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= 2 * n) return;
    const int g = i < n ? 0 : 4;
    const u64 k = i < n ? i : i - n;
    fp_put_plain(out, i, plt_term(cs.c[g], cs.c[g + 1], cs.c[g + 2], cs.c[g + 3], k, pc));
}
// acc_i += alpha^3 L_i at point i of the coset 7 H_m, m = 4n, as pl_quotient_kernel with the four-column terms
__global__ __launch_bounds__(FP_BLOCK) void plt_quotient_kernel(const PltQuotCols cs, const PltConsts* __restrict__ pc, u32* acc_io, u64 m) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u64 iw = (i + 4) & (m - 1);
    const fe A3 = pc->A3;
    const fe Tp = plt_term(cs.c[PLTQ_T1], cs.c[PLTQ_T2], cs.c[PLTQ_T3], cs.c[PLTQ_T0], i, pc);
    const fe X1 = fe_mul(plt_term(cs.c[PLTQ_A], cs.c[PLTQ_B], cs.c[PLTQ_C], cs.c[PLTQ_QK], i, pc), A3);
    const fe X2 = fe_mul(X1, fe_mul(Tp, fp_const_cin()));
    fe_wide acc;
    fe_wide_zero(acc);
    fe_wide_mac(acc, X2, fe_sub<8>(pk_plain(cs.c[PLTQ_PHI], iw), pk_plain(cs.c[PLTQ_PHI], i)));
    fe_wide_mac(acc, fe_mul(Tp, A3), fe_sub<8>(fe_zero(), pk_plain(cs.c[PLTQ_QK], i)));
    fe_wide_mac(acc, X1, pk_plain(cs.c[PLTQ_M], i));
    const fe W = fe_wide_reduce(acc);
    fp_put_plain(acc_io, i, fe_add(W, pk_plain(acc_io, i)));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
PlonkLookupTable* FRN_FN(plt_table_new)(const u64* d_t0, const u64* d_t1, const u64* d_t2, const u64* d_t3, u64 T, hipStream_t st) {
    ZK_REQUIRE(d_t0 && d_t1 && d_t2 && d_t3, "plonk lookup: null argument");
    ZK_REQUIRE(T >= 1, "plonk lookup: a table has at least one row");
    ZK_REQUIRE(T <= ZK_PLONK_LOOKUP_MAX_ROWS, "plonk lookup: a table of " + std::to_string(T) + " rows, at most ZK_PLONK_LOOKUP_MAX_ROWS (" + std::to_string(ZK_PLONK_LOOKUP_MAX_ROWS) + ")");
    fp_aligned({d_t0, d_t1, d_t2, d_t3});
    std::unique_ptr<PlonkLookupTable> h(new PlonkLookupTable);
    h->curve = &fp_curve();
    h->tagged = true;
    h->n_rows = T;
    h->n_slots = 2;
    while (h->n_slots < 2 * T) h->n_slots <<= 1;
    h->d_keys.reserve(T * PLT_KEY * 4);
    h->d_tags.reserve(T * 4);
    h->d_slots.reserve(h->n_slots * 4);
    u64 stat[2] = {0, ~0ull};
    DevBuf ds;
    ds.reserve(16);
    h2d_sync(ds.p, stat, 16);
    ZK_HIP(hipMemsetAsync(h->d_slots.p, 0xff, h->n_slots * 4, st));
    hipLaunchKernelGGL(plt_keys_kernel, dim3(fp_blocks(T)), dim3(FP_BLOCK), 0, st, (const u32*)d_t0, (const u32*)d_t1, (const u32*)d_t2, (const u32*)d_t3, T, (u32*)h->d_keys.p,
                       (u32*)h->d_tags.p, (unsigned long long*)ds.p);
    hipLaunchKernelGGL(plt_insert_kernel, dim3(fp_blocks(T)), dim3(FP_BLOCK), 0, st, (const u32*)h->d_keys.p, T, (u32*)h->d_slots.p, (u32)(h->n_slots - 1));
    ZK_HIP(hipGetLastError());
    d2h_sync(stat, ds.p, 16);
    ZK_REQUIRE(stat[0] == 0, "plonk lookup: the tag of table row " + std::to_string(stat[1]) + " is not in 1 .. " + std::to_string(PLT_MAX_TAG) + " (" + std::to_string(stat[0]) + " such rows)");
    return h.release();
}

void FRN_FN(plt_count_dev)(const PlonkLookupTable& h, const u64* d_a, const u64* d_b, const u64* d_c, const u64* d_qk, u64 n, u64* d_m_out, u64* n_bad, u64* first_bad, hipStream_t st) {
    ZK_REQUIRE(n_bad && first_bad && ((d_a && d_b && d_c && d_qk && d_m_out) || n == 0), "plonk lookup: null argument");
    ZK_REQUIRE(h.tagged, "plonk lookup: tagged count: the table has no tags");
    fp_limit(n);
    ZK_REQUIRE(n == 0 || h.n_rows <= n, "plonk lookup: count: the table has " + std::to_string(h.n_rows) + " rows, the multiplicities only " + std::to_string(n));
    u64 stat[2] = {0, ~0ull};
    if (n) {
        fp_aligned({d_a, d_b, d_c, d_qk, d_m_out});
        DevBuf ds, cnt;
        ds.reserve(16);
        cnt.reserve(h.n_rows * 4);
        h2d_sync(ds.p, stat, 16);
        ZK_HIP(hipMemsetAsync(cnt.p, 0, h.n_rows * 4, st));
        hipLaunchKernelGGL(plt_count_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, (const u32*)h.d_keys.p, (const u32*)h.d_slots.p, (u32)(h.n_slots - 1), (const u32*)d_a, (const u32*)d_b,
                           (const u32*)d_c, (const u32*)d_qk, n, (u32*)cnt.p, (unsigned long long*)ds.p);
        hipLaunchKernelGGL(plt_counts_out_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, (const u32*)cnt.p, (const u32*)h.d_tags.p, h.n_rows, n, (u32*)d_m_out);
        ZK_HIP(hipGetLastError());
        d2h_sync(stat, ds.p, 16);
    }
    *n_bad = stat[0];
    *first_bad = stat[1];
}

static const PltConsts* plt_consts(DevBuf& pc, const FpWords& eta, const FpWords& delta, const FpWords& alpha, hipStream_t st) {
    pc.reserve(sizeof(PltConsts));
    hipLaunchKernelGGL(plt_setup_kernel, dim3(1), dim3(64), 0, st, eta, delta, alpha, (PltConsts*)pc.p);
    return (const PltConsts*)pc.p;
}
void FRN_FN(plt_terms_dev)(const u64* const* d_cols, u64 n, const u64* eta, const u64* delta, u64* d_out, hipStream_t st) {
    const FpWords e = pk_scalar("plonk lookup", eta, "eta"), d = pk_scalar("plonk lookup", delta, "delta");
    ZK_REQUIRE(d_cols && (d_out || n == 0), "plonk lookup: null argument");
    fp_limit(n);
    if (!n) return;
    PltTermCols cs{};
    for (int c = 0; c < PLT_TERMS_NCOL; ++c) {
        cs.c[c] = (const u32*)d_cols[c];
        ZK_REQUIRE(cs.c[c], "plonk lookup: tagged terms: column " + std::to_string(c) + " is null");
        fp_aligned({cs.c[c]});
        ZK_REQUIRE(pk_apart(d_out, cs.c[c], n) && pk_apart(d_out + 4 * n, cs.c[c], n), "plonk lookup: tagged terms: the output overlaps column " + std::to_string(c));
    }
    fp_aligned({d_out});
    DevBuf pc;
    const PltConsts* k = plt_consts(pc, e, d, FpWords{}, st);
    hipLaunchKernelGGL(plt_terms_kernel, dim3(fp_blocks(2 * n)), dim3(FP_BLOCK), 0, st, cs, k, n, (u32*)d_out);
    ZK_HIP(hipGetLastError());
}
void FRN_FN(plt_quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* eta, const u64* delta, u64* d_acc, hipStream_t st) {
    const FpWords a = pk_scalar("plonk lookup", alpha, "alpha"), e = pk_scalar("plonk lookup", eta, "eta"), d = pk_scalar("plonk lookup", delta, "delta");
    if (log_n + 2 > (u32)FRN_S) throw std::runtime_error("plonk lookup: the coset of 2^" + std::to_string(log_n + 2) + " points for n = 2^" + std::to_string(log_n) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(d_cols && d_acc, "plonk lookup: null argument");
    const u64 m = 4ull << log_n;
    PltQuotCols cs{};
    for (int c = 0; c < PLT_QUOT_NCOL; ++c) {
        cs.c[c] = (const u32*)d_cols[c];
        ZK_REQUIRE(cs.c[c], "plonk lookup: tagged quotient: column " + std::to_string(c) + " is null");
        fp_aligned({cs.c[c]});
        ZK_REQUIRE(pk_apart(d_acc, cs.c[c], m), "plonk lookup: tagged quotient: the accumulator overlaps column " + std::to_string(c));
    }
    fp_aligned({d_acc});
    DevBuf pc;
    const PltConsts* k = plt_consts(pc, e, d, a, st);
    hipLaunchKernelGGL(plt_quotient_kernel, dim3(fp_blocks(m)), dim3(FP_BLOCK), 0, st, cs, k, (u32*)d_acc, m);
    ZK_HIP(hipGetLastError());
}
