// Point checks at the scale of a proving key (groth16_key_check, zk_points_check_*): included per curve and group right behind
// pairing_impl.hip.h, whose loaders, curve equations and constants it uses.  No include guard on purpose.
//
// One lane per affine point, the first class that applies (KC_* below), and per launch the exact number of points and the smallest
// index of every class: a ballot per class, and only a wave that saw the class adds its popcount and lowers the index (two atomics on
// 2 x KC_CLASSES words; a clean section issues none).  No per-point status reaches the host.
//
// Subgroup membership with plain = 0 -- tests that are equivalent to [r]P = O on the WHOLE curve, not only on random points:
//   BN254 G1        none: the cofactor is 1, every point of the curve has order r.
//   BLS12-381 G1    phi(P) = [-x^2]P with phi(a, b) = (beta a, b), beta = PAIR_GAMMA2[2] (a primitive cube root of unity of Fq; of the two
//                   it is the one whose phi acts on G1 as -x^2).  Sound everywhere: phi^2 + phi + 1 = 0 on this j = 0 curve, so
//                   phi(P) = [-x^2]P gives [x^4 - x^2 + 1]P = [r]P = O (M. Scott, "A note on group membership tests for G1, G2 and GT on BLS
//                   pairing-friendly curves", ePrint 2021/1130, section 3).  128 scalar bits as two runs of 64.
//   BLS12-381 G2    psi(Q) = [x]Q (Scott 2021, section 4: psi^2 - t psi + q = 0 on the twist gives [h1 r]Q = O, and gcd(h1, h2) = 1).  64 bits.
//   BN254 G2        [x + 1]Q + psi([x]Q) + psi^2([x]Q) = psi^3([2x]Q) (Y. El Housni, A. Guillevic, T. Piellard, "Co-factor clearing and
//                   subgroup membership testing on pairing-friendly curves", AFRICACRYPT 2022, ePrint 2022/352, section 4.3, proven for this
//                   curve's cofactor).  63 bits.
// psi = twist o Frobenius o untwist.  On the D-type twist (BN254) psi(a, b) = (conj(a) g2, conj(b) g3) with g_k = PAIR_GAMMA1[k] =
// xi^(k (q - 1)/6); on the M-type twist (BLS12-381) the factors are their inverses, which the table also holds: 1/g2 = conj(g2) PAIR_GAMMA2[4]
// (g2 conj(g2) = PAIR_GAMMA2[2], a cube root of unity) and 1/g3 = -conj(g3) (g3 conj(g3) = PAIR_GAMMA2[3] = -1).
// With plain = 1 the same kernel runs [r]P = O bit by bit (BN254 G1 included): the comparator of the tests and of the timing.
//
// Input: the layout of the multi-scalar sums (Montgomery words), or with canon = 1 canonical integers as a key file holds them; either way
// a coordinate whose words are >= q is coordinate_range (pairing_ce refuses it even unchecked).

enum { KC_INFINITY = 0, KC_RANGE = 1, KC_CURVE = 2, KC_SUBGROUP = 3, KC_CLASSES = 4 };
constexpr unsigned long long KC_X = PAIR_BN ? 0x44e992b44a6909f1ull : PAIR_LOOP_LO;   // |x| of the curve family's parameter
static_assert(!PAIR_BN || 6 * KC_X + 2 == PAIR_LOOP_LO, "BN254: the loop count is 6x + 2");

// words -> 29-bit limbs of the integer they spell, and whether it is below q
__device__ __forceinline__ fe kc_split(const u32* w, bool& below_q) {
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
    below_q = lt;
    return x;
}
__device__ __forceinline__ fe kc_load_fe(const u32* w, int canon, bool& below_q) {
    const fe x = kc_split(w, below_q);
    fe c;
#pragma unroll
    for (int i = 0; i < NR; ++i) c.l[i] = canon ? RRP29(i) : CIN29(i);
    return fe_mul(x, c);                                    // x R'^2 / R' or (x R) (R'^2 / R) / R': the internal form either way
}
__device__ __forceinline__ u32 kc_x_bit(int b) { return (u32)(KC_X >> b) & 1u; }

#ifndef MSM_G2
__device__ __forceinline__ int kc_classify(const u32* __restrict__ w, int plain, int canon) {
    if (pr_all_zero(w, 2 * CW_STD)) return KC_INFINITY;
    bool okx, oky;
    aff a; a.x = kc_load_fe(w, canon, okx); a.y = kc_load_fe(w + NL, canon, oky);
    if (!okx || !oky) return KC_RANGE;
    if (!g1_on_curve(a)) return KC_CURVE;
    if (plain) {
        u32 k[8];
        for (int j = 0; j < 8; ++j) k[j] = PAIR_R[j];
        return pt_is_inf(g1_mul_bits(a, k)) ? -1 : KC_SUBGROUP;
    }
    if (PAIR_BN) return -1;
    xyzz t = pt_inf();                                      // [|x|]P
    for (int b = 63; b >= 0; --b) { t = pt_dbl(t); if (kc_x_bit(b)) t = pt_madd(t, a); }
    xyzz u = pt_inf();                                      // [x^2]P = [|x|]([|x|]P)
    for (int b = 63; b >= 0; --b) { u = pt_dbl(u); if (kc_x_bit(b)) u = pt_add(u, t); }
    if (pt_is_inf(u)) return KC_SUBGROUP;                   // [x^2]P = O: not -phi(P), which is finite
    // [x^2]P = -phi(P) = (beta a.x, -a.y), compared without leaving the projective form
    const fe bx = fe_mul(a.x, pr_const(PAIR_GAMMA2[2]));
    const bool ex = pr_zero(fe_sub<2>(u.X, fe_mul(bx, u.ZZ)));
    const bool ey = pr_zero(fe_add(u.Y, fe_mul(a.y, u.ZZZ)));
    return ex && ey ? -1 : KC_SUBGROUP;
}
#else
__device__ __forceinline__ cf kc_conj(const cf& a) { cf r; r.c0 = a.c0; r.c1 = fe_renorm(fe_sub<8>(fe_zero(), a.c1)); return r; }   // a <= 8q
// psi on an affine or XYZZ point (the denominators are conjugated with the numerators)
__device__ __forceinline__ cf kc_psi_x(const cf& x) {
    if (PAIR_DTYPE) return cf_mul(kc_conj(x), cf_const(PAIR_GAMMA1[2]));
    return cf_scale(kc_conj(cf_mul(x, cf_const(PAIR_GAMMA1[2]))), pr_const(PAIR_GAMMA2[4]));
}
__device__ __forceinline__ cf kc_psi_y(const cf& y) {
    if (PAIR_DTYPE) return cf_mul(kc_conj(y), cf_const(PAIR_GAMMA1[3]));
    return cf_neg(kc_conj(cf_mul(y, cf_const(PAIR_GAMMA1[3]))));
}
__device__ __noinline__ xyzz kc_psi(const xyzz& p) {
    xyzz r; r.X = kc_psi_x(p.X); r.Y = kc_psi_y(p.Y); r.ZZ = kc_conj(p.ZZ); r.ZZZ = kc_conj(p.ZZZ);
    return r;
}
__device__ __forceinline__ bool kc_same(const xyzz& p, const xyzz& q) {
    const bool pi = pt_is_inf(p), qi = pt_is_inf(q);
    if (pi || qi) return pi && qi;
    return cf_zero_any(cf_sub<2>(cf_mul(p.X, q.ZZ), cf_mul(q.X, p.ZZ))) && cf_zero_any(cf_sub<2>(cf_mul(p.Y, q.ZZZ), cf_mul(q.Y, p.ZZZ)));
}
__device__ __forceinline__ int kc_classify(const u32* __restrict__ w, int plain, int canon) {
    if (pr_all_zero(w, 2 * CW_STD)) return KC_INFINITY;
    bool ok[4];
    aff a;
    a.x.c0 = kc_load_fe(w, canon, ok[0]); a.x.c1 = kc_load_fe(w + NL, canon, ok[1]);
    a.y.c0 = kc_load_fe(w + 2 * NL, canon, ok[2]); a.y.c1 = kc_load_fe(w + 3 * NL, canon, ok[3]);
    if (!(ok[0] && ok[1] && ok[2] && ok[3])) return KC_RANGE;
    const cf rhs = cf_add(cf_mul(cf_sqr(a.x), a.x), cf_const(PAIR_TWIST_B));
    if (!cf_zero_any(cf_sub<4>(cf_sqr(a.y), rhs))) return KC_CURVE;
    xyzz t = pt_inf();
    if (plain) {
        for (int b = 255; b >= 0; --b) { t = pt_dbl(t); if (pr_r_bit(b)) t = pt_madd(t, a); }
        return pt_is_inf(t) ? -1 : KC_SUBGROUP;
    }
    for (int b = 63; b >= 0; --b) { t = pt_dbl(t); if (kc_x_bit(b)) t = pt_madd(t, a); }   // [|x|]Q
    if (!PAIR_BN) {                                         // x < 0: psi(Q) = -[|x|]Q
        if (pt_is_inf(t)) return KC_SUBGROUP;
        const cf px = kc_psi_x(a.x), py = kc_psi_y(a.y);
        const bool ex = cf_zero_any(cf_sub<2>(t.X, cf_mul(px, t.ZZ)));
        const bool ey = cf_zero_any(cf_add(t.Y, cf_mul(py, t.ZZZ)));
        return ex && ey ? -1 : KC_SUBGROUP;
    }
    const xyzz p1 = kc_psi(t), p2 = kc_psi(p1), p3 = kc_psi(p2);
    const xyzz lhs = pt_add(pt_add(pt_madd(t, a), p1), p2);
    return kc_same(lhs, pt_dbl(p3)) ? -1 : KC_SUBGROUP;
}
#endif

__global__ __launch_bounds__(64) void points_check_init_kernel(unsigned long long* __restrict__ out) {
    if (threadIdx.x < 2 * KC_CLASSES) out[threadIdx.x] = (threadIdx.x & 1) ? ~0ull : 0ull;
}
// out[2 c] = the number of points of class c, out[2 c + 1] = the smallest index of one (all ones: none)
__global__ __launch_bounds__(64) void points_check_kernel(const u32* __restrict__ pts, u64 stride, u64 n, int plain, int canon,
                                                          unsigned long long* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * 64 + threadIdx.x;
    int cls = -1;
    if (i < n) cls = kc_classify(pts + i * stride, plain, canon);
#pragma unroll
    for (int c = 0; c < KC_CLASSES; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (m != 0 && threadIdx.x == 0) {                   // the block is one wave; lane 0 holds its first index
            atomicAdd(out + 2 * c, (unsigned long long)__popcll(m));
            atomicMin(out + 2 * c + 1, (unsigned long long)(i + (u64)(__ffsll((long long)m) - 1)));
        }
    }
}
void points_check_dev(const void* pts, u64 stride_words, u64 n, int plain, int canon, u64* d_out, hipStream_t st) {
    hipLaunchKernelGGL(points_check_init_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)d_out);
    ZK_HIP(hipGetLastError());
    if (!n) return;
    ZK_REQUIRE(n < (1ull << 37), "points check: more than 2^37 points");
    hipLaunchKernelGGL(points_check_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const u32*)pts, stride_words, n, plain, canon,
                       (unsigned long long*)d_out);
    ZK_HIP(hipGetLastError());
}
