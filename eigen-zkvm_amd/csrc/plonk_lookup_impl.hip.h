// The device side of PLONK's lookup argument over the scalar field on gfx950, generic over the field: the log-derivative
// argument of eigen_zkvm_amd/plonk_lookup.py.  A running SUM beside frpoly_impl.hip.h's running product, a hash table over the table's rows
// and the count of how often each is used, the two denominators of a row, the summand of the sum, and the term alpha^3 L the quotient gains.
// Included by groth16.hip after plonk_impl.hip.h, in the same namespace: it uses frpoly_impl.hip.h's word helpers and host checks and
// plonk_impl.hip.h's pk_plain / pk_internal / pk_scalar / pk_apart.  No include guard on purpose.  Several tables in one circuit, bound by a
// tag column, are plonk_lookup_tagged_impl.hip.h: kernels of its own over four-column keys; the summand and the running sum
// of this file serve both.
//
// A vector is n x 8 u32 Montgomery words (R = 2^256), element-major; the words of an input may be any integer below 2^256 (< 6r), every
// output word vector is the canonical representative.  Forms as in plonk_impl.hip.h: plain P(v) = fp_split(words) = v R mod r as the integer
// the words are (< 6r), internal I(v) = v R' (R' = 2^261); fe_mul(I(u), P(v)) = P(u v).
//
// Value bounds, against fe29_impl.hip.h's A B <= 68 (a product of a < A r and b < B r; a sum of products under ONE reduction: sum A_i B_i):
//  the running sum (fps_*): every value is PLAIN, and canonical between the steps
//   a lane's run          p_0 + .. + p_7, p_k = P(in_k) < 6r                                                                   < 48r
//   its total             fe_canon(fe_renorm(.)): 48 x 1 (R' mod r < r) = 48                                                   < r
//   a step of a tree      fe_canon(x + y), x, y < r                                                                            < r
//   an element out        below + loc_k: r + 48r, then fp_put_plain: 49                                                        canonical
//   the total             fe_mul(sum, CIN) = I(sum) (1 x 1), then fe_store_canon                                               canonical
//  the constants of terms / quotient (pl_setup_kernel)
//   E1 = I(eta) = fe_mul(P'(eta), RR2), P' the canonical integer: 1 x 1                                                        < 2r
//   E2 = I(eta^2) = fe_mul(E1, E1): 4                                                                                          < 2r
//   DP = P(delta) = fe_canon(fe_mul(I(delta), COUT)): 2 x 1                                                                    < r
//   A3 = alpha^3 R'^2 / R = fe_mul(I(alpha^3), CIN), I(alpha^3) by two products of values < 2r (4, 4), then 2 x 1              < 2r
//  lookup_terms, per lane
//   out = P(x) + fe_mul(P(y), E1) + fe_mul(P(z), E2) + DP: products 6 x 2 = 12 each; the sum 6r + 2r + 2r + r                  < 11r, fp_put_plain: 11
//  lookup_summands, per lane
//   W = I(inv_i) P(q_K) + I(inv_(n+i)) (8r - P(m)) with ONE reduction; I(.) by fe_from_std (6 x 1) < 2r, 8r - P(m) <= 8r
//       (fe_sub<8> of zero): 2 x 6 + 2 x 8 = 28                                                                               < 2r, plain
//  lookup_quotient, per lane (pl_quotient_kernel)
//   Fp = P(delta + f), Tp = P(delta + t)  as lookup_terms                                                                      < 11r each
//   X1 = fe_mul(Fp, A3) = I(alpha^3 (delta + f)): 11 x 2 = 22                                                                  < 2r
//   TA = fe_mul(Tp, A3) = I(alpha^3 (delta + t)): 22                                                                           < 2r
//   TI = fe_mul(Tp, CIN) = I(delta + t): 11 x 1                                                                                < 2r
//   X2 = fe_mul(X1, TI) = I(alpha^3 (delta + f)(delta + t)): 4                                                                 < 2r
//   D  = P(Phi(wX)) - P(Phi) + 8r  (fe_sub<8>, P(Phi) < 6r <= 8r)                                                              < 14r
//   NQ = 8r - P(q_K)  (fe_sub<8> of zero)                                                                                      <= 8r
//   W  = X2 D + TA NQ + X1 P(M) with ONE reduction (3 pairs <= FE_WIDE_MAX): 2 x 14 + 2 x 8 + 2 x 6 = 56                       < 2r, plain
//   out = W + P(acc): 2r + 6r, fp_put_plain: 8                                                                                 canonical
//  (6r is 2^256 against BN254's r; the true factor is 5.3 there and 2.3 for BLS12-381.)
//  Products per lane: 4 + 4 + three multiply-accumulates with one reduction + one on the way out.
//
// The hash table.  A key is the 24 words of the CANONICAL Montgomery representatives of a row's three elements (so v and v + r are one key);
// its hash is FNV-1a over those words (h = 0x811c9dc5; h = (h ^ word) * 0x01000193 for the 24 words in order), then h ^= h >> 16, and the
// slot is h & (slots - 1).  slots is the smallest power of two >= 2T; a slot holds a row index or PL_EMPTY; collisions walk to the next slot
// and wrap.  pl_insert_kernel claims an empty slot by atomicCAS; where the slot's row has the same key, atomicMin leaves the smaller row, so
// a key sits in ONE slot and that slot ends on the smallest row of the key whatever the order of arrival.  The table is read only after
// the launch that built it: the kernel boundary is the only synchronisation.
constexpr u32 PL_EMPTY = 0xffffffffu;
constexpr int PL_KEY = 3 * NL, PL_ROUNDS = 4;      // words of a key; rounds of combining in a wave before the lanes left add on their own
constexpr int PL_TERMS_NCOL = 6, PL_QUOT_NCOL = 9;
enum { PLQ_A, PLQ_B, PLQ_C, PLQ_QK, PLQ_T1, PLQ_T2, PLQ_T3, PLQ_M, PLQ_PHI };    // the order of lookup_quotient's d_cols

struct PlConsts { fe E1, E2, DP, A3; };
struct PlTermCols { const u32* c[PL_TERMS_NCOL]; };
struct PlQuotCols { const u32* c[PL_QUOT_NCOL]; };

// ---- 1. the running sum: fp_tile_prod / fp_combine / fp_fixup under addition ---------------------------------------------------------------
__device__ __forceinline__ fe fps_elem(const u32* v, u64 n, u64 i) {              // P(in_i); zero beyond n
    if (i >= n) return fe_zero();
    return pk_plain(v, i);
}
__device__ __forceinline__ fe fps_add(const fe& a, const fe& b) { return fe_canon(fe_add(a, b)); }   // a, b < r -> < r
// inclusive scan of sh[0 .. FP_BLOCK) under addition, in place; every lane of the workgroup calls it
__device__ __forceinline__ void fps_scan_up(fe* sh, int t) {
    for (int s = 0; s < 8; ++s) {
        const int d = 1 << s;
        const bool has = t >= d;
        fe x = fe_zero();
        if (has) x = sh[t - d];
        __syncthreads();
        if (has) sh[t] = fps_add(x, sh[t]);
        __syncthreads();
    }
}
__global__ __launch_bounds__(FP_BLOCK) void fps_tile_sum_kernel(const u32* __restrict__ in, u64 n, u32* __restrict__ agg) {
    __shared__ fe sh[FP_BLOCK];
    const int t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * FP_T + (u64)t * FP_E;
    fe part = fe_zero();
    if (base < n) {
        part = fps_elem(in, n, base);
        fp_static_for<1, FP_E>([&](auto K) { part = fe_add(part, fps_elem(in, n, base + decltype(K)::value)); });
        part = fe_canon(fe_renorm(part));
    }
    sh[t] = part;
    for (int s = FP_BLOCK / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (t < s) sh[t] = fps_add(sh[t], sh[t + s]);
    }
    if (t == 0) fp_fe_store(agg, blockIdx.x, sh[0]);
}
// one workgroup over the m aggregates, FP_S at a time: carry_b = sum_{b' < b} A_b' (when carry is not null) and the total as 8 canonical
// words (the integer, not Montgomery)
__global__ __launch_bounds__(FP_BLOCK) void fps_combine_kernel(const u32* __restrict__ agg, u64 m, u32* __restrict__ carry, u32* __restrict__ total) {
    __shared__ fe sh[FP_BLOCK];
    const int t = threadIdx.x;
    fe carry_in = fe_zero();
    const u64 steps = (m + FP_S - 1) / FP_S;
    for (u64 st = 0; st < steps; ++st) {
        const u64 i0 = st * FP_S + 2 * (u64)t;
        const fe a0 = i0 < m ? fp_fe_load(agg, i0) : fe_zero(), a1 = i0 + 1 < m ? fp_fe_load(agg, i0 + 1) : fe_zero();
        fe v = fps_add(a0, a1);
        if (t == 0) v = fps_add(carry_in, v);
        sh[t] = v;
        __syncthreads();
        fps_scan_up(sh, t);
        const fe below = t == 0 ? carry_in : sh[t - 1];                 // the sum of everything before aggregate i0
        if (carry) {
            if (i0 < m) fp_fe_store(carry, i0, below);
            if (i0 + 1 < m) fp_fe_store(carry, i0 + 1, fps_add(below, a0));
        }
        carry_in = sh[FP_BLOCK - 1];
        __syncthreads();
    }
    if (t == 0) fe_store_canon(fe_mul(carry_in, fp_const_cin()), total);
}
// out_i = sum_{j < i} in_j (exclusive) or sum_{j <= i} in_j.  A lane reads its 8 elements before it writes them and no other lane touches
// them: out may be in (neither is __restrict__).
__global__ __launch_bounds__(FP_BLOCK) void fps_fixup_kernel(const u32* in, u64 n, const u32* __restrict__ carry, int inclusive, u32* out) {
    __shared__ fe sh[FP_BLOCK];
    const int t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * FP_T + (u64)t * FP_E;
    fe loc[FP_E];                                                       // prefixes of the lane's own run, < 48r
    loc[0] = fps_elem(in, n, base);
    fp_static_for<1, FP_E>([&](auto K) { constexpr int k = decltype(K)::value; loc[k] = fe_add(loc[k - 1], fps_elem(in, n, base + k)); });
    fe v = fe_canon(fe_renorm(loc[FP_E - 1]));
    if (t == 0) v = fps_add(fp_fe_load(carry, blockIdx.x), v);
    sh[t] = v;
    __syncthreads();
    fps_scan_up(sh, t);
    const fe below = t == 0 ? fp_fe_load(carry, blockIdx.x) : sh[t - 1];
    fp_static_for<0, FP_E>([&](auto K) {
        constexpr int k = decltype(K)::value;
        if (base + k < n) {
            if (inclusive) fp_put_plain(out, base + k, fe_add(below, loc[k]));
            else if constexpr (k == 0) fp_put_plain(out, base, below);
            else fp_put_plain(out, base + k, fe_add(below, loc[k - 1]));
        }
    });
}

// ---- 2. the hash table and the count ------------------------------------------------------------------------------------------------------
// the canonical Montgomery words of element i
__device__ __forceinline__ void pl_canon_words(const u32* v, u64 i, u32* w8) {
    u32 w[NL];
    fp_pack(fe_canon(fe_renorm(pk_plain(v, i))), w);
#pragma unroll
    for (int j = 0; j < NL; ++j) w8[j] = w[j];
}
__device__ __forceinline__ u32 pl_hash(const u32 (&key)[PL_KEY]) {
    u32 h = 0x811c9dc5u;
#pragma unroll
    for (int j = 0; j < PL_KEY; ++j) h = (h ^ key[j]) * 0x01000193u;
    return h ^ (h >> 16);
}
__device__ __forceinline__ bool pl_same(const u32 (&key)[PL_KEY], const u32* __restrict__ keys, u32 row) {
    const uint4* q = (const uint4*)(keys + (u64)row * PL_KEY);
    u32 d = 0;
#pragma unroll
    for (int j = 0; j < PL_KEY / 4; ++j) {
        const uint4 x = q[j];
        d |= (x.x ^ key[4 * j]) | (x.y ^ key[4 * j + 1]) | (x.z ^ key[4 * j + 2]) | (x.w ^ key[4 * j + 3]);
    }
    return d == 0;
}
// keys[j] = the key of table row j
__global__ __launch_bounds__(FP_BLOCK) void pl_keys_kernel(const u32* __restrict__ t1, const u32* __restrict__ t2, const u32* __restrict__ t3, u64 T, u32* __restrict__ keys) {
    const u64 j = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= T) return;
    u32 key[PL_KEY];
    pl_canon_words(t1, j, key); pl_canon_words(t2, j, key + NL); pl_canon_words(t3, j, key + 2 * NL);
    uint4* q = (uint4*)(keys + j * PL_KEY);
#pragma unroll
    for (int k = 0; k < PL_KEY / 4; ++k) q[k] = make_uint4(key[4 * k], key[4 * k + 1], key[4 * k + 2], key[4 * k + 3]);
}
// row j into the slots (all PL_EMPTY before the launch).  At most T of the slots >= 2T slots are ever taken, so a walk ends within `slots` steps.
__global__ __launch_bounds__(FP_BLOCK) void pl_insert_kernel(const u32* __restrict__ keys, u64 T, u32* slots, u32 mask) {
    const u64 j = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= T) return;
    u32 key[PL_KEY];
    const uint4* q = (const uint4*)(keys + j * PL_KEY);
#pragma unroll
    for (int k = 0; k < PL_KEY / 4; ++k) { const uint4 x = q[k]; key[4 * k] = x.x; key[4 * k + 1] = x.y; key[4 * k + 2] = x.z; key[4 * k + 3] = x.w; }
    u32 h = pl_hash(key) & mask;
    for (u32 step = 0; step <= mask; ++step) {
        const u32 cur = atomicCAS(&slots[h], PL_EMPTY, (u32)j);
        if (cur == PL_EMPTY) return;
        if (pl_same(key, keys, cur)) { atomicMin(&slots[h], (u32)j); return; }
        h = (h + 1) & mask;
    }
}
// one lane per row of H: a selected row (q_K != 0) looks its tuple up and adds 1 to its table row's counter; the lanes of a wave that hit
// the same counter are combined first (PL_ROUNDS rounds: the lowest lane left names its counter and adds for every lane on it; the lanes
// still left after that add on their own), so a range check, whose rows crowd on few counters, costs a wave one atomic and spread lookups
// at most PL_ROUNDS rounds more than their own.  A miss is counted as pk_gate_kernel counts failures.
__global__ __launch_bounds__(FP_BLOCK) void pl_count_kernel(const u32* __restrict__ keys, const u32* __restrict__ slots, u32 mask, const u32* __restrict__ a, const u32* __restrict__ b,
                                                           const u32* __restrict__ c, const u32* __restrict__ qk, u64 n, u32* __restrict__ cnt,
                                                           unsigned long long* __restrict__ stat) {
    __shared__ unsigned long long zs[2];
    const int t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * FP_BLOCK + t;
    if (t == 0) { zs[0] = 0; zs[1] = ~0ull; }
    __syncthreads();
    u32 target = PL_EMPTY;
    if (i < n && !fe_is_zero_m(fe_renorm(pk_plain(qk, i)))) {
        u32 key[PL_KEY];
        pl_canon_words(a, i, key); pl_canon_words(b, i, key + NL); pl_canon_words(c, i, key + 2 * NL);
        u32 h = pl_hash(key) & mask;
        for (u32 step = 0; step <= mask; ++step) {
            const u32 row = slots[h];
            if (row == PL_EMPTY) break;
            if (pl_same(key, keys, row)) { target = row; break; }
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
// m_i = cnt[i] for i < T, 0 from T on, as Montgomery words: the integer times R'^2 / R' = I(.), then fe_to_std
__global__ __launch_bounds__(FP_BLOCK) void pl_counts_out_kernel(const u32* __restrict__ cnt, u64 T, u64 n, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 v = i < T ? cnt[i] : 0;
    fe x = fe_zero();
    x.l[0] = v & LMASK; x.l[1] = v >> LB;
    fp_put(out, i, fe_mul(x, fp_const_rr2()));
}

// ---- 3. the denominators, the summand, the quotient's term ----------------------------------------------------------------------------------
// eta, delta, alpha: 8 canonical words each -> the constants of the kernels below
__global__ void pl_setup_kernel(const FpWords eta, const FpWords delta, const FpWords alpha, PlConsts* __restrict__ pc) {
    if (threadIdx.x || blockIdx.x) return;
    const fe e = fe_mul(fp_split(eta.w), fp_const_rr2());
    pc->E1 = e;
    pc->E2 = fe_mul(e, e);
    pc->DP = fe_canon(fe_mul(fe_mul(fp_split(delta.w), fp_const_rr2()), fp_const_cout()));
    const fe a = fe_mul(fp_split(alpha.w), fp_const_rr2());
    pc->A3 = fe_mul(fe_mul(fe_mul(a, a), a), fp_const_cin());
}
// P(delta + x + eta y + eta^2 z) < 11r
__device__ __forceinline__ fe pl_term(const u32* x, const u32* y, const u32* z, u64 i, const PlConsts* __restrict__ pc) {
    return fe_add(fe_add(pk_plain(x, i), fe_mul(pk_plain(y, i), pc->E1)), fe_add(fe_mul(pk_plain(z, i), pc->E2), pc->DP));
}
// out_i = delta + f_i, out_(n+i) = delta + t_i: 2n lanes
__global__ __launch_bounds__(FP_BLOCK) void pl_terms_kernel(const PlTermCols cs, const PlConsts* __restrict__ pc, u64 n, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= 2 * n) return;
    const int g = i < n ? 0 : 3;
    const u64 k = i < n ? i : i - n;
    fp_put_plain(out, i, pl_term(cs.c[g], cs.c[g + 1], cs.c[g + 2], k, pc));
}
// out_i = q_K,i inv_i - m_i inv_(n+i)
__global__ __launch_bounds__(FP_BLOCK) void pl_summands_kernel(const u32* __restrict__ inv, const u32* __restrict__ qk, const u32* __restrict__ m, u64 n, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    fe_wide acc;
    fe_wide_zero(acc);
    fe_wide_mac(acc, pk_internal(inv, i), pk_plain(qk, i));
    fe_wide_mac(acc, pk_internal(inv, n + i), fe_sub<8>(fe_zero(), pk_plain(m, i)));
    fp_put_plain(out, i, fe_wide_reduce(acc));
}
// acc_i += alpha^3 L_i at point i of the coset 7 H_m, m = 4n; Phi(wX) is element (i + 4) mod m.  One lane per element.
__global__ __launch_bounds__(FP_BLOCK) void pl_quotient_kernel(const PlQuotCols cs, const PlConsts* __restrict__ pc, u32* acc_io, u64 m) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u64 iw = (i + 4) & (m - 1);
    const fe A3 = pc->A3;
    const fe Tp = pl_term(cs.c[PLQ_T1], cs.c[PLQ_T2], cs.c[PLQ_T3], i, pc);
    const fe X1 = fe_mul(pl_term(cs.c[PLQ_A], cs.c[PLQ_B], cs.c[PLQ_C], i, pc), A3);
    const fe X2 = fe_mul(X1, fe_mul(Tp, fp_const_cin()));
    fe_wide acc;
    fe_wide_zero(acc);
    fe_wide_mac(acc, X2, fe_sub<8>(pk_plain(cs.c[PLQ_PHI], iw), pk_plain(cs.c[PLQ_PHI], i)));
    fe_wide_mac(acc, fe_mul(Tp, A3), fe_sub<8>(fe_zero(), pk_plain(cs.c[PLQ_QK], i)));
    fe_wide_mac(acc, X1, pk_plain(cs.c[PLQ_M], i));
    const fe W = fe_wide_reduce(acc);
    fp_put_plain(acc_io, i, fe_add(W, pk_plain(acc_io, i)));
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
void FRN_FN(fp_prefix_sum_dev)(const u64* d_in, u64 n, bool inclusive, u64* d_out, u64* total_out, hipStream_t st) {
    ZK_REQUIRE(total_out && (d_in || n == 0), "frpoly: null argument");
    fp_limit(n);
    if (n == 0) { total_out[0] = total_out[1] = total_out[2] = total_out[3] = 0; return; }
    fp_aligned({d_in, d_out});
    const u64 tiles = (n + FP_T - 1) / FP_T;
    DevBuf agg, carry, tot;
    agg.reserve(tiles * NR * 4); tot.reserve(32);
    if (d_out) carry.reserve(tiles * NR * 4);
    hipLaunchKernelGGL(fps_tile_sum_kernel, dim3((unsigned)tiles), dim3(FP_BLOCK), 0, st, (const u32*)d_in, n, (u32*)agg.p);
    hipLaunchKernelGGL(fps_combine_kernel, dim3(1), dim3(FP_BLOCK), 0, st, (const u32*)agg.p, tiles, (u32*)carry.p, (u32*)tot.p);
    if (d_out)
        hipLaunchKernelGGL(fps_fixup_kernel, dim3((unsigned)tiles), dim3(FP_BLOCK), 0, st, (const u32*)d_in, n, (const u32*)carry.p, inclusive ? 1 : 0, (u32*)d_out);
    ZK_HIP(hipGetLastError());
    d2h_sync(total_out, tot.p, 32);
}

PlonkLookupTable* FRN_FN(pl_table_new)(const u64* d_t1, const u64* d_t2, const u64* d_t3, u64 T, hipStream_t st) {
    ZK_REQUIRE(d_t1 && d_t2 && d_t3, "plonk lookup: null argument");
    ZK_REQUIRE(T >= 1, "plonk lookup: a table has at least one row");
    ZK_REQUIRE(T <= ZK_PLONK_LOOKUP_MAX_ROWS, "plonk lookup: a table of " + std::to_string(T) + " rows, at most ZK_PLONK_LOOKUP_MAX_ROWS (" + std::to_string(ZK_PLONK_LOOKUP_MAX_ROWS) + ")");
    fp_aligned({d_t1, d_t2, d_t3});
    std::unique_ptr<PlonkLookupTable> h(new PlonkLookupTable);
    h->curve = &fp_curve();
    h->n_rows = T;
    h->n_slots = 2;
    while (h->n_slots < 2 * T) h->n_slots <<= 1;
    h->d_keys.reserve(T * PL_KEY * 4);
    h->d_slots.reserve(h->n_slots * 4);
    ZK_HIP(hipMemsetAsync(h->d_slots.p, 0xff, h->n_slots * 4, st));
    hipLaunchKernelGGL(pl_keys_kernel, dim3(fp_blocks(T)), dim3(FP_BLOCK), 0, st, (const u32*)d_t1, (const u32*)d_t2, (const u32*)d_t3, T, (u32*)h->d_keys.p);
    hipLaunchKernelGGL(pl_insert_kernel, dim3(fp_blocks(T)), dim3(FP_BLOCK), 0, st, (const u32*)h->d_keys.p, T, (u32*)h->d_slots.p, (u32)(h->n_slots - 1));
    ZK_HIP(hipGetLastError());
    return h.release();
}

void FRN_FN(pl_count_dev)(const PlonkLookupTable& h, const u64* d_a, const u64* d_b, const u64* d_c, const u64* d_qk, u64 n, u64* d_m_out, u64* n_bad, u64* first_bad, hipStream_t st) {
    ZK_REQUIRE(n_bad && first_bad && ((d_a && d_b && d_c && d_qk && d_m_out) || n == 0), "plonk lookup: null argument");
    ZK_REQUIRE(!h.tagged, "plonk lookup: count: the table is a tagged one (zk_plonk_<curve>_lookup_tagged_count_dev counts over it)");
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
        hipLaunchKernelGGL(pl_count_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, (const u32*)h.d_keys.p, (const u32*)h.d_slots.p, (u32)(h.n_slots - 1), (const u32*)d_a, (const u32*)d_b,
                           (const u32*)d_c, (const u32*)d_qk, n, (u32*)cnt.p, (unsigned long long*)ds.p);
        hipLaunchKernelGGL(pl_counts_out_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, (const u32*)cnt.p, h.n_rows, n, (u32*)d_m_out);
        ZK_HIP(hipGetLastError());
        d2h_sync(stat, ds.p, 16);
    }
    *n_bad = stat[0];
    *first_bad = stat[1];
}

static const PlConsts* pl_consts(DevBuf& pc, const FpWords& eta, const FpWords& delta, const FpWords& alpha, hipStream_t st) {
    pc.reserve(sizeof(PlConsts));
    hipLaunchKernelGGL(pl_setup_kernel, dim3(1), dim3(64), 0, st, eta, delta, alpha, (PlConsts*)pc.p);
    return (const PlConsts*)pc.p;
}
void FRN_FN(pl_terms_dev)(const u64* const* d_cols, u64 n, const u64* eta, const u64* delta, u64* d_out, hipStream_t st) {
    const FpWords e = pk_scalar("plonk lookup", eta, "eta"), d = pk_scalar("plonk lookup", delta, "delta");
    ZK_REQUIRE(d_cols && (d_out || n == 0), "plonk lookup: null argument");
    fp_limit(n);
    if (!n) return;
    PlTermCols cs{};
    for (int c = 0; c < PL_TERMS_NCOL; ++c) {
        cs.c[c] = (const u32*)d_cols[c];
        ZK_REQUIRE(cs.c[c], "plonk lookup: terms: column " + std::to_string(c) + " is null");
        fp_aligned({cs.c[c]});
        ZK_REQUIRE(pk_apart(d_out, cs.c[c], n) && pk_apart(d_out + 4 * n, cs.c[c], n), "plonk lookup: terms: the output overlaps column " + std::to_string(c));
    }
    fp_aligned({d_out});
    DevBuf pc;
    const PlConsts* k = pl_consts(pc, e, d, FpWords{}, st);
    hipLaunchKernelGGL(pl_terms_kernel, dim3(fp_blocks(2 * n)), dim3(FP_BLOCK), 0, st, cs, k, n, (u32*)d_out);
    ZK_HIP(hipGetLastError());
}
void FRN_FN(pl_summands_dev)(const u64* d_inv, const u64* d_qk, const u64* d_m, u64 n, u64* d_out, hipStream_t st) {
    ZK_REQUIRE((d_inv && d_qk && d_m && d_out) || n == 0, "plonk lookup: null argument");
    fp_limit(n);
    if (!n) return;
    fp_aligned({d_inv, d_qk, d_m, d_out});
    ZK_REQUIRE(pk_apart(d_out, d_inv, n) && pk_apart(d_out, d_inv + 4 * n, n) && pk_apart(d_out, d_qk, n) && pk_apart(d_out, d_m, n), "plonk lookup: summands: the output overlaps an input");
    hipLaunchKernelGGL(pl_summands_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, (const u32*)d_inv, (const u32*)d_qk, (const u32*)d_m, n, (u32*)d_out);
    ZK_HIP(hipGetLastError());
}
void FRN_FN(pl_quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* eta, const u64* delta, u64* d_acc, hipStream_t st) {
    const FpWords a = pk_scalar("plonk lookup", alpha, "alpha"), e = pk_scalar("plonk lookup", eta, "eta"), d = pk_scalar("plonk lookup", delta, "delta");
    if (log_n + 2 > (u32)FRN_S) throw std::runtime_error("plonk lookup: the coset of 2^" + std::to_string(log_n + 2) + " points for n = 2^" + std::to_string(log_n) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(d_cols && d_acc, "plonk lookup: null argument");
    const u64 m = 4ull << log_n;
    PlQuotCols cs{};
    for (int c = 0; c < PL_QUOT_NCOL; ++c) {
        cs.c[c] = (const u32*)d_cols[c];
        ZK_REQUIRE(cs.c[c], "plonk lookup: quotient: column " + std::to_string(c) + " is null");
        fp_aligned({cs.c[c]});
        ZK_REQUIRE(pk_apart(d_acc, cs.c[c], m), "plonk lookup: quotient: the accumulator overlaps column " + std::to_string(c));
    }
    fp_aligned({d_acc});
    DevBuf pc;
    const PlConsts* k = pl_consts(pc, e, d, a, st);
    hipLaunchKernelGGL(pl_quotient_kernel, dim3(fp_blocks(m)), dim3(FP_BLOCK), 0, st, cs, k, (u32*)d_acc, m);
    ZK_HIP(hipGetLastError());
}
