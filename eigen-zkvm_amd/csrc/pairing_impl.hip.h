// Curve-generic body of the pairing and of Groth16 verification (see pairing.hip): included twice per curve after
// ecpt_impl.hip.h -- once without MSM_G2 (the G1 side: curve and subgroup checks, the public-input sum) and once with it
// (the twist: checks, line tables; Fq12: Miller loop, final exponentiation).  tools/pairing_constants.py carries the same
// algorithm on Python integers (`Model`) and emits the constants (pairing_consts.hip.h).  No include guard on purpose.
//
// Verdicts (include/zkgpu.h): 1 accepted, 0 the equation fails, < 0 malformed input; a status array starts at 1 and every
// check lowers it to its code.

__device__ __forceinline__ bool pr_zero(const fe& x) { return fe_is_zero_m(fe_mul(x, fe_one())); }   // x = 0 mod q, any lazily reduced x
__device__ __forceinline__ fe pr_const(const unsigned* p) {
    fe r;
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = p[i];
    return r;
}
__device__ __forceinline__ bool pr_all_zero(const u32* w, int n) {
    u32 z = 0;
    for (int i = 0; i < n; ++i) z |= w[i];
    return z == 0;
}
__device__ __forceinline__ u32 pr_r_bit(int b) { return (PAIR_R[b >> 5] >> (b & 31)) & 1; }
__device__ __forceinline__ void pr_lower(int* status, int code) { if (*status > code) *status = code; }

#ifndef MSM_G2
// ---- G1 ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ aff g1_load(const u32* w) { aff a; a.x = cf_from_std(w); a.y = cf_from_std(w + CW_STD); return a; }
__device__ bool g1_on_curve(const aff& a) {
    const fe rhs = fe_add(fe_mul(fe_sqr(a.x), a.x), pr_const(PAIR_G1_B));
    return pr_zero(fe_sub<4>(fe_sqr(a.y), rhs));
}
__device__ xyzz g1_mul_bits(const aff& a, const u32* k /* 8 words */) {
    xyzz t = pt_inf();
    for (int b = 255; b >= 0; --b) {
        t = pt_dbl(t);
        if ((k[b >> 5] >> (b & 31)) & 1) t = pt_madd(t, a);
    }
    return t;
}
// points[i * stride ...]: on the curve and, where G1 is a proper subgroup (BLS12-381), of order r; the all-zero encoding is infinity
__global__ __launch_bounds__(64) void g1_check_kernel(const u32* __restrict__ pts, u64 stride, u64 n, int* __restrict__ status, u64 status_stride) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32* w = pts + i * stride;
    if (pr_all_zero(w, 2 * CW_STD)) return;
    const aff a = g1_load(w);
    if (!g1_on_curve(a)) { pr_lower(status + i * status_stride, -3); return; }
    if (!PAIR_BN) {
        u32 k[8];
        for (int j = 0; j < 8; ++j) k[j] = PAIR_R[j];
        if (!pt_is_inf(g1_mul_bits(a, k))) pr_lower(status + i * status_stride, -4);
    }
}
// acc_i = IC_0 + sum_j x_ij IC_j (zero inputs skipped); an input >= r lowers the status
__global__ __launch_bounds__(64) void g16_acc_kernel(const u32* __restrict__ ic, u32 n_pub, const u32* __restrict__ pub, u64 n,
                                                     u32* __restrict__ acc_out, int* __restrict__ status) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    xyzz acc = pt_inf();
    if (!pr_all_zero(ic, 2 * CW_STD)) acc = pt_madd(acc, g1_load(ic));
    for (u32 j = 0; j < n_pub; ++j) {
        u32 k[8];
        for (int t = 0; t < 8; ++t) k[t] = pub[(i * n_pub + j) * 8 + t];
        bool lt = false;                                   // k < r, from the top word down
        for (int t = 7; t >= 0; --t) { if (k[t] != PAIR_R[t]) { lt = k[t] < PAIR_R[t]; break; } }
        if (!lt) { pr_lower(status + i, -1); continue; }
        const u32* w = ic + (u64)(j + 1) * 2 * CW_STD;
        if (pr_all_zero(k, 8) || pr_all_zero(w, 2 * CW_STD)) continue;
        acc = pt_add(acc, g1_mul_bits(g1_load(w), k));
    }
    u32* o = acc_out + i * 2 * CW_STD;
    if (pt_is_inf(acc)) { for (int t = 0; t < 2 * CW_STD; ++t) o[t] = 0; return; }
    u32 x[CW_STD], y[CW_STD];
    pt_to_std(acc, x, y);
    for (int t = 0; t < CW_STD; ++t) { o[t] = x[t]; o[CW_STD + t] = y[t]; }
}
void g1_check_dev(const void* pts, u64 stride_words, u64 n, int* status, u64 status_stride, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(g1_check_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const u32*)pts, stride_words, n, status, status_stride);
    ZK_HIP(hipGetLastError());
}
void g16_acc_dev(const void* ic, u32 n_pub, const void* pub, u64 n, void* acc, int* status, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(g16_acc_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const u32*)ic, n_pub, (const u32*)pub, n, (u32*)acc, status);
    ZK_HIP(hipGetLastError());
}
#else
// ---- the twist ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ cf cf_red(const cf& a) { cf r; r.c0 = fe_renorm(a.c0); r.c1 = fe_renorm(a.c1); return r; }   // components < 2q
__device__ __forceinline__ cf cf_neg(const cf& a) { return cf_sub<2>(cf_zero(), a); }                                    // a <= 2q
__device__ __forceinline__ cf cf_scale(const cf& a, const fe& s) { cf r; r.c0 = fe_mul(a.c0, s); r.c1 = fe_mul(a.c1, s); return r; }
__device__ __forceinline__ cf cf_const(const unsigned* p) { cf r; r.c0 = pr_const(p); r.c1 = pr_const(p + NR); return r; }
__device__ __forceinline__ bool cf_zero_any(const cf& a) { return pr_zero(a.c0) && pr_zero(a.c1); }
// xi a, xi = PAIR_XI0 + u: (XI0 a0 - a1) + (XI0 a1 + a0) u.  a < 4q.  XI0 = 1: components < 8q; XI0 = 9: brought back below 2q.
__device__ __forceinline__ cf cf_mul_xi(const cf& a) {
    cf r;
    if (PAIR_XI0 == 1) { r.c0 = fe_sub<4>(a.c0, a.c1); r.c1 = fe_add(a.c0, a.c1); return r; }
    const cf a8 = cf_dbl(cf_dbl(cf_dbl(a))), a9 = cf_add(a8, a);                        // < 36q
    r.c0 = fe_renorm(fe_sub<4>(a9.c0, a.c1)); r.c1 = fe_renorm(fe_add(a9.c1, a.c0));    // < 40q before
    return r;
}
__device__ __forceinline__ aff g2_load(const u32* w) { aff a; a.x = cf_from_std(w); a.y = cf_from_std(w + CW_STD); return a; }
__global__ __launch_bounds__(64) void g2_check_kernel(const u32* __restrict__ pts, u64 stride, u64 n, int* __restrict__ status, u64 status_stride) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32* w = pts + i * stride;
    if (pr_all_zero(w, 2 * CW_STD)) return;
    const aff a = g2_load(w);
    const cf rhs = cf_add(cf_mul(cf_sqr(a.x), a.x), cf_const(PAIR_TWIST_B));
    if (!cf_zero_any(cf_sub<4>(cf_sqr(a.y), rhs))) { pr_lower(status + i * status_stride, -3); return; }
    xyzz t = pt_inf();                                                                   // [r]Q = O, plainly
    for (int b = 255; b >= 0; --b) {
        t = pt_dbl(t);
        if (pr_r_bit(b)) t = pt_madd(t, a);
    }
    if (!pt_is_inf(t)) pr_lower(status + i * status_stride, -4);
}

// Line tables.  One lane walks T = [..]Q in Jacobian coordinates (X < 2q, Y < 2q, Z < 4q) through the loop count and stores, per step, the
// three Fq2 coefficients (cY, cX, c0) of the line scaled by a factor in Fq2 (which the final exponentiation removes): the value at
// P = (xP, yP) is cY yP + cX xP w + c0 w^3 on the D-type twist and c0 + cX xP w^2 + cY yP w^3 on the M-type one.
constexpr int pr_popcount(unsigned long long v) { int c = 0; while (v) { c += (int)(v & 1); v >>= 1; } return c; }
constexpr int PR_STEPS = (PAIR_LOOP_BITS - 1) + (pr_popcount(PAIR_LOOP_LO) + pr_popcount(PAIR_LOOP_HI) - 1) + (PAIR_BN ? 2 : 0);
__device__ __forceinline__ bool pr_loop_bit(int b) { return b < 64 ? (PAIR_LOOP_LO >> b) & 1 : (PAIR_LOOP_HI >> (b - 64)) & 1; }
constexpr int PR_LINE_WORDS = 3 * CW_INT;
struct jac { cf X, Y, Z; };
__device__ __noinline__ void line_dbl(jac& T, u32* __restrict__ out) {
    const cf A = cf_sqr(T.X), B = cf_sqr(T.Y), ZZ = cf_sqr(T.Z);
    const cf S = cf_dbl(cf_dbl(cf_mul(T.X, B)));                                        // 4 X Y^2 < 8q
    const cf M = cf_add(cf_dbl(A), A);                                                  // 3 X^2 < 6q
    const cf X3 = cf_red(cf_sub<8>(cf_sub<8>(cf_sqr(M), S), S));
    const cf Z3 = cf_dbl(cf_mul(T.Y, T.Z));                                             // < 4q
    const cf B4 = cf_dbl(cf_dbl(cf_sqr(B)));                                            // 4 Y^4 < 8q
    const cf Y3 = cf_red(cf_sub<8>(cf_sub<8>(cf_mul(cf_sub<2>(S, X3), M), B4), B4));    // (S - X3 < 10q) M - 8 Y^4
    cf_store_int(cf_mul(Z3, ZZ), out);                                                  // cY = Z3 Z^2
    cf_store_int(cf_neg(cf_mul(M, ZZ)), out + CW_INT);                                  // cX = -3 X^2 Z^2
    cf_store_int(cf_sub<4>(cf_mul(M, T.X), cf_dbl(B)), out + 2 * CW_INT);               // c0 = 3 X^3 - 2 Y^2 < 6q
    T.X = X3; T.Y = Y3; T.Z = Z3;
}
__device__ __noinline__ void line_add(jac& T, const cf& x2, const cf& y2, u32* __restrict__ out) {
    const cf ZZ = cf_sqr(T.Z), ZZZ = cf_mul(T.Z, ZZ);
    const cf H = cf_sub<2>(cf_mul(x2, ZZ), T.X), Rr = cf_sub<2>(cf_mul(y2, ZZZ), T.Y);  // < 4q
    const cf HH = cf_sqr(H), HHH = cf_mul(H, HH), V = cf_mul(T.X, HH);
    const cf X3 = cf_red(cf_sub<4>(cf_sub<2>(cf_sqr(Rr), HHH), cf_dbl(V)));
    const cf Z3 = cf_mul(T.Z, H);
    const cf Y3 = cf_red(cf_sub<2>(cf_mul(cf_sub<2>(V, X3), Rr), cf_mul(T.Y, HHH)));
    cf_store_int(Z3, out);                                                              // cY = Z3
    cf_store_int(cf_sub<4>(cf_zero(), Rr), out + CW_INT);                               // cX = -R
    cf_store_int(cf_sub<2>(cf_mul(Rr, x2), cf_mul(y2, Z3)), out + 2 * CW_INT);          // c0 = R x2 - y2 Z3
    T.X = X3; T.Y = Y3; T.Z = Z3;
}
__global__ __launch_bounds__(64) void g2_lines_kernel(const u32* __restrict__ pts, u64 stride, u64 n, u32* __restrict__ lines, u32* __restrict__ inf) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32* w = pts + i * stride;
    inf[i] = pr_all_zero(w, 2 * CW_STD) ? 1u : 0u;
    const aff q = g2_load(w);
    jac T; T.X = q.x; T.Y = q.y; T.Z = cf_one();
    u32* out = lines + i * (u64)(PR_STEPS * PR_LINE_WORDS);
    int step = 0;
    for (int b = PAIR_LOOP_BITS - 2; b >= 0; --b) {
        line_dbl(T, out + (step++) * PR_LINE_WORDS);
        if (pr_loop_bit(b)) line_add(T, q.x, q.y, out + (step++) * PR_LINE_WORDS);
    }
    if (PAIR_BN) {                                                                      // pi(Q), then -pi^2(Q)
        cf cx = q.x, cy = q.y;
        cx.c1 = fe_sub<2>(fe_zero(), cx.c1); cy.c1 = fe_sub<2>(fe_zero(), cy.c1);
        line_add(T, cf_mul(cx, cf_const(PAIR_GAMMA1[2])), cf_mul(cy, cf_const(PAIR_GAMMA1[3])), out + (step++) * PR_LINE_WORDS);
        line_add(T, cf_scale(q.x, pr_const(PAIR_GAMMA2[2])), cf_neg(cf_scale(q.y, pr_const(PAIR_GAMMA2[3]))), out + (step++) * PR_LINE_WORDS);
    }
}

// ---- Fq12 = Fq2[w]/(w^6 - xi) on groups of eight lanes: lane k < 6 of a group owns the coefficient of w^k (lanes 6 and 7 idle along as
// copies of lane 0 and store nothing).  Operands cross the group through LDS: every lane publishes its coefficient -- and xi times it,
// for the terms that wrap past w^5 -- and then forms its own coefficient of the product as a sum of Fq2 products.  One workgroup is one
// wave (64 lanes, eight groups), so the barriers are cheap; all control flow around them is uniform (the exponents are constants).
constexpr int PR_GROUP = 8, PR_GROUPS = 64 / PR_GROUP;
constexpr int PR_SLOT = 6 * CW_INT;                    // one Fq12 in words
constexpr int PR_SH_WORDS = 4 * PR_SLOT;               // per group: A, xi A, B, xi B
struct f12ctx { u32* sh; int k; bool live; };          // sh: the group's LDS; k: the coefficient this lane computes; live: it also stores
__device__ __forceinline__ void f12_put(const f12ctx& c, int slot, const cf& v) { if (c.live) cf_store_int(v, c.sh + slot * PR_SLOT + c.k * CW_INT); }
__device__ __forceinline__ cf f12_get(const u32* base, int i) { return cf_load_int(base + i * CW_INT); }
// coefficient k of a b: sum_{i <= k} a_i b_{k-i} + sum_{i > k} a_i (xi b)_{k-i+6}; A, B, BX: six coefficients each (LDS or global)
__device__ __noinline__ cf f12_dot(const u32* A, const u32* B, const u32* BX, int k) {
    cf acc = cf_zero();
    for (int i = 0; i < 6; ++i) {
        const int j = k - i;
        const cf b = j < 0 ? f12_get(BX, j + 6) : f12_get(B, j);
        acc = cf_add(acc, cf_mul(b, f12_get(A, i)));                                     // b < 8q first, a <= 2q (2q itself: a coefficient f12_conj6 negated)
    }
    return cf_red(acc);                                                                  // < 12q -> < 2q
}
__device__ __forceinline__ cf f12_mul(const f12ctx& c, const cf& a, const cf& b) {
    __syncthreads();
    f12_put(c, 0, a); f12_put(c, 2, b); f12_put(c, 3, cf_mul_xi(b));
    __syncthreads();
    return f12_dot(c.sh, c.sh + 2 * PR_SLOT, c.sh + 3 * PR_SLOT, c.k);
}
// a times a table entry in global memory: tab = six coefficients, then xi times them
__device__ __forceinline__ cf f12_mul_tab(const f12ctx& c, const cf& a, const u32* tab) {
    __syncthreads();
    f12_put(c, 0, a);
    __syncthreads();
    return f12_dot(c.sh, tab, tab + PR_SLOT, c.k);
}
// f times a line with the Fq2 values v0, v1, v2 at w^0, w^P1, w^3 (P1 = 1 D-type, 2 M-type)
__device__ __noinline__ cf f12_mul_line(const f12ctx& c, const cf& f, const cf& v0, const cf& v1, const cf& v2) {
    constexpr int P1 = PAIR_DTYPE ? 1 : 2;
    __syncthreads();
    f12_put(c, 0, f); f12_put(c, 1, cf_mul_xi(f));
    __syncthreads();
    const u32 *A = c.sh, *AX = c.sh + PR_SLOT;
    const int j1 = c.k - P1, j2 = c.k - 3;
    cf acc = cf_mul(v0, f12_get(A, c.k));
    acc = cf_add(acc, cf_mul(j1 < 0 ? f12_get(AX, j1 + 6) : f12_get(A, j1), v1));
    acc = cf_add(acc, cf_mul(j2 < 0 ? f12_get(AX, j2 + 6) : f12_get(A, j2), v2));
    return cf_red(acc);
}
// Granger-Scott squaring in the cyclotomic subgroup (see Model.cyc_sqr): the pairs (a_k, a_{k+3}) are elements of Fq4 = Fq2[w^3]
__device__ __noinline__ cf f12_cyc_sqr(const f12ctx& c, const cf& a) {
    __syncthreads();
    f12_put(c, 0, a); f12_put(c, 1, cf_mul_xi(a));
    __syncthreads();
    const bool lo = c.k < 3;
    const int pk = lo ? c.k + 3 : c.k - 3;
    const cf p = f12_get(c.sh, pk), xp = f12_get(c.sh + PR_SLOT, pk);
    const cf X = lo ? a : p, Y = lo ? xp : a;
    const cf t = cf_add(cf_mul(X, a), cf_mul(Y, p));                                     // k < 3: a^2 + xi p^2; else 2 a p.  < 4q
    __syncthreads();
    f12_put(c, 0, t); f12_put(c, 1, cf_mul_xi(t));
    __syncthreads();
    const int src = c.k == 0 ? 0 : c.k == 1 ? 5 : c.k == 2 ? 1 : c.k == 3 ? 3 : c.k == 4 ? 2 : 4;
    const cf s = f12_get(c.k == 1 ? c.sh + PR_SLOT : c.sh, src);                          // < 8q
    const cf s3 = cf_add(cf_dbl(s), s), a2 = cf_dbl(a);                                  // < 24q, < 4q
    return cf_red((c.k & 1) ? cf_add(s3, a2) : cf_sub<4>(s3, a2));
}
__device__ __forceinline__ cf f12_conj6(const f12ctx& c, const cf& a) { return (c.k & 1) ? cf_neg(a) : a; }   // odd k: 2q - a, up to 2q itself
__device__ __forceinline__ cf f12_frob2(const f12ctx& c, const cf& a) { return cf_scale(a, pr_const(PAIR_GAMMA2[c.k])); }
__device__ __forceinline__ cf f12_one(const f12ctx& c) { return c.k == 0 ? cf_one() : cf_zero(); }
__device__ __forceinline__ f12ctx f12_ctx(u32* sh_all) {
    const int l = threadIdx.x % PR_GROUP;
    f12ctx c; c.sh = sh_all + (threadIdx.x / PR_GROUP) * PR_SH_WORDS; c.live = l < 6; c.k = c.live ? l : 0;
    return c;
}

// Product of up to three Miller loops per item with one shared squaring per step.  Pair p of item i: the G1 point g1[p] + i g1_stride
// (external layout), the line table lines[p] + i lines_stride and its infinity flag (strides 0: one table for all items).
__global__ __launch_bounds__(64) void miller_kernel(MillerArgs ar, u64 n, u32* __restrict__ f_out) {
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    const f12ctx c = f12_ctx(sh_all);
    u64 i = (u64)blockIdx.x * PR_GROUPS + threadIdx.x / PR_GROUP;
    const bool have = i < n;
    if (!have) i = n - 1;                                                                // (idle groups recompute the last item; they store nothing)
    fe xp[3], yp[3]; bool skip[3]; const u32* ln[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        skip[p] = true; xp[p] = fe_zero(); yp[p] = fe_zero(); ln[p] = nullptr;
        if (p < ar.np) {
            const u32* w = ar.g1[p] + i * ar.g1_stride[p];
            u32 t0[NL], t1[NL];
            u32 z = 0;
            for (int j = 0; j < NL; ++j) { t0[j] = w[j]; t1[j] = w[NL + j]; z |= t0[j] | t1[j]; }
            xp[p] = fe_from_std(t0); yp[p] = fe_from_std(t1);
            skip[p] = z == 0 || ar.inf[p][i * ar.inf_stride[p]] != 0;
            ln[p] = ar.lines[p] + i * ar.lines_stride[p];
        }
    }
    cf f = f12_one(c);
    int step = 0;
    auto lines_in = [&](int s) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if (p >= ar.np) continue;                                                    // uniform
            const u32* l = ln[p] + (u64)s * PR_LINE_WORDS;
            cf vy = cf_scale(cf_load_int(l), yp[p]), vx = cf_scale(cf_load_int(l + CW_INT), xp[p]), v0 = cf_load_int(l + 2 * CW_INT);
            if (skip[p]) { vy = cf_zero(); vx = cf_zero(); v0 = cf_zero(); if (PAIR_DTYPE) vy = cf_one(); else v0 = cf_one(); }
            f = PAIR_DTYPE ? f12_mul_line(c, f, vy, vx, v0) : f12_mul_line(c, f, v0, vx, vy);
        }
    };
    for (int b = PAIR_LOOP_BITS - 2; b >= 0; --b) {
        f = f12_mul(c, f, f);
        lines_in(step++);
        if (pr_loop_bit(b)) lines_in(step++);
    }
    if (PAIR_BN) { lines_in(step++); lines_in(step++); }
    if (!PAIR_BN) f = f12_conj6(c, f);                                                   // the curve parameter is negative
    if (have && c.live) cf_store_int(f, f_out + (i * 6 + c.k) * CW_INT);
}

// canonical little-endian words of an internal value
__device__ __forceinline__ void fe_to_canon_words(const fe& a, u32* w) {
    fe one = fe_zero(); one.l[0] = 1;
    const fe x = fe_canon(fe_mul(a, one));
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int bit = 32 * j, k = bit / LB, s = bit % LB;
        u32 v = x.l[k] >> s;
        if (k + 1 < NR) v |= x.l[k + 1] << (LB - s);
        if (k + 2 < NR && 2 * LB - s < 32) v |= x.l[k + 2] << (2 * LB - s);
        w[j] = v;
    }
}
// f^((q^12 - 1)/r): easy part by conjugation, one inversion and the q^2 map; hard part (q^4 - q^2 + 1)/r in a fixed 4-bit window over
// cyclotomic squarings.  tab: 16 x 2 x 6 Fq2 per item in global memory (g^d and xi g^d).  gt_out: 12 canonical Fq per item.
constexpr int PR_TAB_WORDS = 16 * 2 * PR_SLOT;
__global__ __launch_bounds__(64) void final_exp_kernel(const u32* __restrict__ f_in, u64 n, u32* tab_all, u32* __restrict__ gt_out, int do_exp) {
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    const f12ctx c = f12_ctx(sh_all);
    u64 i = (u64)blockIdx.x * PR_GROUPS + threadIdx.x / PR_GROUP;
    const bool have = i < n;
    if (!have) i = n - 1;
    const cf f = cf_load_int(f_in + (i * 6 + c.k) * CW_INT);
    cf r = f;
    if (do_exp) {
        u32* tab = tab_all + i * (u64)PR_TAB_WORDS;
        // f^-1 = fbar A B / (N A B): fbar the conjugate over Fq6, N = f fbar in Fq6, A = N^(q^2), B = N^(q^4); N A B is the norm to Fq2
        const cf fbar = f12_conj6(c, f);
        const cf nn = f12_mul(c, f, fbar);
        const cf a = f12_frob2(c, nn);
        const cf ab = f12_mul(c, a, f12_frob2(c, a));
        const cf t = f12_mul(c, nn, ab);
        __syncthreads();
        f12_put(c, 0, t);
        __syncthreads();
        const cf ti = cf_inv(f12_get(c.sh, 0));
        const cf finv = cf_mul(f12_mul(c, fbar, ab), ti);
        cf g = f12_mul(c, fbar, finv);                                                   // f^(q^6 - 1)
        g = f12_mul(c, f12_frob2(c, g), g);                                              // ^(q^2 + 1)
        cf cur = g;
        for (int d = 1; d < 16; ++d) {
            if (have && c.live) {
                cf_store_int(cur, tab + (d * 2) * PR_SLOT + c.k * CW_INT);
                cf_store_int(cf_mul_xi(cur), tab + (d * 2 + 1) * PR_SLOT + c.k * CW_INT);
            }
            if (d < 15) cur = f12_mul(c, cur, g);
        }
        __syncthreads();
        const u32 d0 = PAIR_HARD[0] & 15;
        r = cf_load_int(tab + (d0 * 2) * PR_SLOT + c.k * CW_INT);
        for (int e = 1; e < PAIR_HARD_DIGITS; ++e) {
            const u32 d = (PAIR_HARD[e >> 3] >> (4 * (e & 7))) & 15;
            for (int s = 0; s < 4; ++s) r = f12_cyc_sqr(c, r);
            if (d) r = f12_mul_tab(c, r, tab + (d * 2) * PR_SLOT);
        }
    }
    if (have && c.live) {
        u32* o = gt_out + (i * 6 + c.k) * 2 * NL;
        fe_to_canon_words(r.c0, o); fe_to_canon_words(r.c1, o + NL);
    }
}
// Product of n Fq12 values in the layout miller_kernel writes.  A launch of B blocks has 8 B groups; group g multiplies the items g, g + 8 B,
// g + 16 B, ... (an idle group holds one), the eight groups of the block then meet through LDS as a tree (4, 2, 1: group j takes in group
// j + s) and group 0 stores the block's product.  B = ceil(n / PR_PROD_BLOCK) capped at PR_PROD_MAX_BLOCKS; more than one block means a
// second launch of one block over the B partial products.  The order is fixed by n alone and nothing is atomic: the same input gives the
// same limbs.  All control flow around the barriers of f12_mul is uniform in the block (the trip count depends on n and gridDim only).
constexpr int PR_PROD_SHARE = 8;                               // items a group takes before the launch opens another block
constexpr int PR_PROD_BLOCK = PR_GROUPS * PR_PROD_SHARE;       // items per block at that point
constexpr int PR_PROD_MAX_BLOCKS = 1024;
__global__ __launch_bounds__(64) void f12_prod_kernel(const u32* __restrict__ f_in, u64 n, u32* __restrict__ f_out) {
    __shared__ u32 sh_all[PR_GROUPS * PR_SH_WORDS];
    __shared__ u32 meet[PR_GROUPS * PR_SLOT];
    const f12ctx c = f12_ctx(sh_all);
    const u32 grp = threadIdx.x / PR_GROUP;
    const u64 tg = (u64)gridDim.x * PR_GROUPS, gg = (u64)blockIdx.x * PR_GROUPS + grp;
    cf acc = gg < n ? cf_load_int(f_in + (gg * 6 + c.k) * CW_INT) : f12_one(c);
    for (u64 base = tg; base < n; base += tg) {
        const u64 i = base + gg;
        const cf b = i < n ? cf_load_int(f_in + (i * 6 + c.k) * CW_INT) : f12_one(c);
        acc = f12_mul(c, acc, b);
    }
    for (u32 s = PR_GROUPS / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (c.live) cf_store_int(acc, meet + grp * PR_SLOT + c.k * CW_INT);
        __syncthreads();
        const cf b = grp < s ? cf_load_int(meet + (grp + s) * PR_SLOT + c.k * CW_INT) : f12_one(c);
        acc = f12_mul(c, acc, b);
    }
    if (grp == 0 && c.live) cf_store_int(acc, f_out + ((u64)blockIdx.x * 6 + c.k) * CW_INT);
}
__global__ __launch_bounds__(64) void g16_verdict_kernel(const u32* __restrict__ gt, const u32* __restrict__ want, u64 n, const int* __restrict__ status, int* __restrict__ verdict) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 d = 0;
    for (int j = 0; j < 12 * NL; ++j) d |= gt[i * 12 * NL + j] ^ want[j];
    verdict[i] = status[i] < 1 ? status[i] : (d == 0 ? 1 : 0);
}

void g2_check_dev(const void* pts, u64 stride_words, u64 n, int* status, u64 status_stride, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(g2_check_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const u32*)pts, stride_words, n, status, status_stride);
    ZK_HIP(hipGetLastError());
}
size_t g2_lines_bytes(u64 n) { return n * (size_t)(PR_STEPS * PR_LINE_WORDS) * 4; }
void g2_lines_dev(const void* pts, u64 stride_words, u64 n, void* lines, void* inf, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(g2_lines_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const u32*)pts, stride_words, n, (u32*)lines, (u32*)inf);
    ZK_HIP(hipGetLastError());
}
size_t f12_bytes(u64 n) { return n * (size_t)PR_SLOT * 4; }
size_t final_exp_tab_bytes(u64 n) { return n * (size_t)PR_TAB_WORDS * 4; }
void miller_dev(const MillerArgs& ar, u64 n, void* f_out, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(miller_kernel, dim3((unsigned)((n + PR_GROUPS - 1) / PR_GROUPS)), dim3(64), 0, st, ar, n, (u32*)f_out);
    ZK_HIP(hipGetLastError());
}
void final_exp_dev(const void* f_in, u64 n, void* tab, void* gt_out, int do_exp, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(final_exp_kernel, dim3((unsigned)((n + PR_GROUPS - 1) / PR_GROUPS)), dim3(64), 0, st, (const u32*)f_in, n, (u32*)tab, (u32*)gt_out, do_exp);
    ZK_HIP(hipGetLastError());
}
// f_out: one value; scratch: f12_prod_scratch_bytes(n) for the partial products of a two-level run (unused below PR_PROD_BLOCK + 1 items).
// f_out and scratch must not overlap f_in.
size_t f12_prod_scratch_bytes(u64 n) {
    const u64 b = (n + PR_PROD_BLOCK - 1) / PR_PROD_BLOCK;
    return (size_t)(b < PR_PROD_MAX_BLOCKS ? b : PR_PROD_MAX_BLOCKS) * PR_SLOT * 4;
}
void f12_prod_dev(const void* f_in, u64 n, void* scratch, void* f_out, hipStream_t st) {
    ZK_REQUIRE(n >= 1, "pairing product: nothing to multiply");
    u64 blocks = (n + PR_PROD_BLOCK - 1) / PR_PROD_BLOCK;
    if (blocks > PR_PROD_MAX_BLOCKS) blocks = PR_PROD_MAX_BLOCKS;
    hipLaunchKernelGGL(f12_prod_kernel, dim3((unsigned)blocks), dim3(64), 0, st, (const u32*)f_in, n, (u32*)(blocks > 1 ? scratch : f_out));
    ZK_HIP(hipGetLastError());
    if (blocks > 1) {
        hipLaunchKernelGGL(f12_prod_kernel, dim3(1), dim3(64), 0, st, (const u32*)scratch, blocks, (u32*)f_out);
        ZK_HIP(hipGetLastError());
    }
}
void g16_verdict_dev(const void* gt, const void* want, u64 n, const int* status, int* verdict, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(g16_verdict_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const u32*)gt, (const u32*)want, n, status, verdict);
    ZK_HIP(hipGetLastError());
}
#endif
