// Coordinate field `cf` (Fq for G1; Fq2 for G2 with MSM_G2) and the XYZZ point formulas shared by the sums (msm_impl.hip.h) and the
// pairing (pairing_impl.hip.h).  Included inside a curve's namespace after its constants; no include guard on purpose.
#include "fe29_impl.hip.h"

// ---- coordinate field `cf`: Fq for G1; Fq2 = Fq[u]/(u^2 + 1) for G2 (MSM_G2), built from the Fq operations
// with every component brought back below 2q after a product (one extra product with R' mod q), so that the
// bounds of the point formulas below hold for both.
#ifndef MSM_G2
typedef fe cf;
constexpr int CW_STD = NL, CW_INT = NR;   // words per coordinate: external layout / internal limbs
__device__ __forceinline__ cf cf_zero() { return fe_zero(); }
__device__ __forceinline__ cf cf_one() { return fe_one(); }
__device__ __forceinline__ cf cf_add(const cf& a, const cf& b) { return fe_add(a, b); }
__device__ __forceinline__ cf cf_dbl(const cf& a) { return fe_dbl(a); }
template <int M> __device__ __forceinline__ cf cf_sub(const cf& a, const cf& b) { return fe_sub<M>(a, b); }
__device__ __forceinline__ cf cf_mul(const cf& a, const cf& b) { return fe_mul(a, b); }
__device__ __forceinline__ cf cf_sqr(const cf& a) { return fe_sqr(a); }
__device__ __forceinline__ bool cf_is_zero_m(const cf& a) { return fe_is_zero_m(a); }
__device__ __forceinline__ cf cf_inv(const cf& a) { return fe_inv(a); }
__device__ __forceinline__ cf cf_from_std(const u32* w) {
    u32 t[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) t[i] = w[i];
    return fe_from_std(t);
}
__device__ __forceinline__ void cf_to_std(const cf& a, u32* w) {
    u32 t[NL];
    fe_to_std(a, t);
#pragma unroll
    for (int i = 0; i < NL; ++i) w[i] = t[i];
}
__device__ __forceinline__ cf cf_load_int(const u32* p) {
    cf a;
#pragma unroll
    for (int k = 0; k < NR; ++k) a.l[k] = p[k];
    return a;
}
__device__ __forceinline__ void cf_store_int(const cf& a, u32* p) {
#pragma unroll
    for (int k = 0; k < NR; ++k) p[k] = a.l[k];
}
#else
struct cf { fe c0, c1; };                 // c0 + c1 u, u^2 = -1 (both BN254 and BLS12-381 build Fq2 this way)
constexpr int CW_STD = 2 * NL, CW_INT = 2 * NR;
__device__ __forceinline__ fe fe_renorm(const fe& a) { return fe_mul(a, fe_one()); }   // < 168q -> < 2q, same residue
__device__ __forceinline__ cf cf_zero() { cf r; r.c0 = fe_zero(); r.c1 = fe_zero(); return r; }
__device__ __forceinline__ cf cf_one() { cf r; r.c0 = fe_one(); r.c1 = fe_zero(); return r; }
__device__ __forceinline__ cf cf_add(const cf& a, const cf& b) { cf r; r.c0 = fe_add(a.c0, b.c0); r.c1 = fe_add(a.c1, b.c1); return r; }
__device__ __forceinline__ cf cf_dbl(const cf& a) { return cf_add(a, a); }
template <int M> __device__ __forceinline__ cf cf_sub(const cf& a, const cf& b) { cf r; r.c0 = fe_sub<M>(a.c0, b.c0); r.c1 = fe_sub<M>(a.c1, b.c1); return r; }
// (a0 b0 - a1 b1) + (a0 b1 + a1 b0) u with one reduction per component (fe_mul2): the subtrahend enters as
// a1 (8q - b1).  Requires b.c1 <= 8q and, for components a < Aq, b < Bq, A (B + 8) <= 168 (BN254; every call site
// below keeps the operand with the larger bound first: the worst is 10q x 6q = 140).  Components of the result < 2q.
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
#ifdef MSM_G2_INLINE_CF
#define CF_MUL_ATTR __forceinline__
#define PT_COLD_ATTR __noinline__
#else
#define CF_MUL_ATTR __noinline__
#define PT_COLD_ATTR
#endif
__device__ CF_MUL_ATTR cf cf_mul(const cf& a, const cf& b) {
    cf r;
    r.c0 = fe_mul2(a.c0, b.c0, a.c1, fe_sub<8>(fe_zero(), b.c1));
    r.c1 = fe_mul2(a.c0, b.c1, a.c1, b.c0);
    return r;
}
__device__ CF_MUL_ATTR cf cf_sqr(const cf& a) {   // a <= 8q (or c0 < 10q with c1 < 2q): a0^2 + a1 (8q - a1), 2 a0 a1
    cf r;
    r.c0 = fe_mul2(a.c0, a.c0, a.c1, fe_sub<8>(fe_zero(), a.c1));
    r.c1 = fe_mul(fe_dbl(a.c0), a.c1);
    return r;
}
__device__ __forceinline__ bool cf_is_zero_m(const cf& a) { return fe_is_zero_m(a.c0) && fe_is_zero_m(a.c1); }
__device__ cf cf_inv(const cf& a) {       // (a0 - a1 u) / (a0^2 + a1^2), a < 2q
    const fe n = fe_inv(fe_renorm(fe_add(fe_sqr(a.c0), fe_sqr(a.c1))));
    cf r; r.c0 = fe_mul(a.c0, n); r.c1 = fe_mul(fe_sub<2>(fe_zero(), a.c1), n);
    return r;
}
__device__ __forceinline__ cf cf_from_std(const u32* w) {
    u32 t0[NL], t1[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) { t0[i] = w[i]; t1[i] = w[NL + i]; }
    cf r; r.c0 = fe_from_std(t0); r.c1 = fe_from_std(t1);
    return r;
}
__device__ __forceinline__ void cf_to_std(const cf& a, u32* w) {
    u32 t0[NL], t1[NL];
    fe_to_std(a.c0, t0); fe_to_std(a.c1, t1);
#pragma unroll
    for (int i = 0; i < NL; ++i) { w[i] = t0[i]; w[NL + i] = t1[i]; }
}
__device__ __forceinline__ cf cf_load_int(const u32* p) {
    cf a;
#pragma unroll
    for (int k = 0; k < NR; ++k) { a.c0.l[k] = p[k]; a.c1.l[k] = p[NR + k]; }
    return a;
}
__device__ __forceinline__ void cf_store_int(const cf& a, u32* p) {
#pragma unroll
    for (int k = 0; k < NR; ++k) { p[k] = a.c0.l[k]; p[NR + k] = a.c1.l[k]; }
}
#endif

// XYZZ coordinates: x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2; infinity <=> ZZ == 0.
// Invariants of every stored point: X < 8q, Y <= 4q, ZZ, ZZZ < 2q (products), limbs normalised.
struct xyzz { cf X, Y, ZZ, ZZZ; };
struct aff { cf x, y; };  // x, y < 2q

__device__ __forceinline__ xyzz pt_inf() {
    xyzz p; p.X = cf_zero(); p.Y = cf_zero(); p.ZZ = cf_zero(); p.ZZZ = cf_zero();
    return p;
}
__device__ __forceinline__ bool pt_is_inf(const xyzz& p) { return cf_is_zero_m(p.ZZ); }
// shared tail of the addition formulas: given U1 (= X1 scaled, < 8q), S1 (<= 4q), P, R and PP = P^2
__device__ __forceinline__ void pt_finish(xyzz& r, const cf& U1, const cf& S1, const cf& P, const cf& Rr, const cf& PP) {
    const cf PPP = cf_mul(P, PP), Q = cf_mul(U1, PP);                      // < 2q each
    r.X = cf_sub<4>(cf_sub<2>(cf_sqr(Rr), PPP), cf_dbl(Q));                 // < 2q + 2q + 4q = 8q
#ifdef MSM_G2
    r.Y = cf_sub<2>(cf_mul(cf_sub<8>(Q, r.X), Rr), cf_mul(S1, PPP));        // (Q - X3 < 10q) first, Rr < 6q ; Y3 < 4q
#else
    // round 6: (Q - X3) R - S1 PPP as ONE sum of two products with one Montgomery reduction (fe_mul2; bounds 10 * 6 + 4 * 2 = 68 <= 168):
    // a reduction less per point addition, 110 of ~2 700 instructions.  Y3 < 2q.
    r.Y = fe_mul2(cf_sub<8>(Q, r.X), Rr, cf_sub<4>(cf_zero(), S1), PPP);
#endif
}
#ifndef PT_COLD_ATTR
#define PT_COLD_ATTR
#endif
__device__ PT_COLD_ATTR xyzz pt_dbl_aff(const aff& a) {  // mdbl-2008-s-1 (a = 0)
    const cf U = cf_dbl(a.y), V = cf_sqr(U), W = cf_mul(U, V), S = cf_mul(a.x, V);
    const cf xx = cf_sqr(a.x), M = cf_add(cf_dbl(xx), xx);                  // < 6q
    xyzz r;
    r.X = cf_sub<4>(cf_sqr(M), cf_dbl(S));                                  // < 6q
    r.Y = cf_sub<2>(cf_mul(cf_sub<8>(S, r.X), M), cf_mul(W, a.y));
    r.ZZ = V; r.ZZZ = W;
    return r;
}
__device__ PT_COLD_ATTR xyzz pt_dbl(const xyzz& p) {  // dbl-2008-s-1 (a = 0)
    if (pt_is_inf(p)) return p;
    const cf U = cf_dbl(p.Y), V = cf_sqr(U), W = cf_mul(U, V), S = cf_mul(p.X, V);   // U <= 8q
    const cf xx = cf_sqr(p.X), M = cf_add(cf_dbl(xx), xx);                  // < 6q
    xyzz r;
    r.X = cf_sub<4>(cf_sqr(M), cf_dbl(S));                                  // < 6q
    r.Y = cf_sub<2>(cf_mul(cf_sub<8>(S, r.X), M), cf_mul(W, p.Y));
    r.ZZ = cf_mul(V, p.ZZ); r.ZZZ = cf_mul(W, p.ZZZ);
    return r;
}
__device__ __forceinline__ xyzz pt_madd(const xyzz& p, const aff& a) {  // madd-2008-s
    if (pt_is_inf(p)) { xyzz r; r.X = a.x; r.Y = a.y; r.ZZ = cf_one(); r.ZZZ = cf_one(); return r; }
    const cf U2 = cf_mul(a.x, p.ZZ), S2 = cf_mul(a.y, p.ZZZ);
    cf P = cf_sub<8>(U2, p.X);                                              // < 10q
    const cf Rr = cf_sub<4>(S2, p.Y);                                       // < 6q
#ifdef MSM_G2
    P.c1 = fe_renorm(P.c1);                                                 // cf_sqr's bound: c0 < 10q needs c1 < 2q
#endif
    const cf PP = cf_sqr(P);
    if (cf_is_zero_m(PP)) return cf_is_zero_m(cf_sqr(Rr)) ? pt_dbl_aff(a) : pt_inf();  // q prime: P^2 = 0 <=> P = 0
    xyzz r;
    pt_finish(r, p.X, p.Y, P, Rr, PP);
    r.ZZ = cf_mul(p.ZZ, PP); r.ZZZ = cf_mul(p.ZZZ, cf_mul(P, PP));
    return r;
}
__device__ PT_COLD_ATTR xyzz pt_add(const xyzz& p, const xyzz& q) {  // add-2008-s
    if (pt_is_inf(p)) return q;
    if (pt_is_inf(q)) return p;
    const cf U1 = cf_mul(p.X, q.ZZ), U2 = cf_mul(q.X, p.ZZ), S1 = cf_mul(p.Y, q.ZZZ), S2 = cf_mul(q.Y, p.ZZZ);
    const cf P = cf_sub<2>(U2, U1), Rr = cf_sub<2>(S2, S1);                 // < 4q
    const cf PP = cf_sqr(P);
    if (cf_is_zero_m(PP)) return cf_is_zero_m(cf_sqr(Rr)) ? pt_dbl(p) : pt_inf();
    xyzz r;
    pt_finish(r, U1, S1, P, Rr, PP);
    r.ZZ = cf_mul(cf_mul(p.ZZ, q.ZZ), PP); r.ZZZ = cf_mul(cf_mul(p.ZZZ, q.ZZZ), cf_mul(P, PP));
    return r;
}
__device__ __forceinline__ xyzz pt_neg(const xyzz& p) {
    xyzz r = p;
    r.Y = cf_sub<4>(cf_zero(), p.Y);                                        // 4q - Y <= 4q
    return r;
}
// ---- four lanes per point operation -------------------------------------------------------------------------------------------
// The tails of a sum -- the bucket hierarchy and the final walk over the windows -- are chains of a few hundred dependent point
// operations on a handful of lanes: latency, not throughput.  A doubling is 9 field products in 3 dependent stages, a full addition
// 14 in 4; here the lanes of a quad hold the same point and lane q computes the q-th product of each stage, the results travel by
// DPP quad broadcasts (a move per limb, no LDS).  The same formulas, the same operands, the same bounds: bit-identical results
// (tests/test_gpu_ecpt.py compares them limb for limb), in a third of the dependent products.  Called by all four lanes of a quad with identical arguments.
__device__ __forceinline__ u32 quad_word(u32 v, int k) {            // lane k's value in every lane of the quad (k is uniform)
    switch (k) {
        case 0: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x00, 0xF, 0xF, false);
        case 1: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xF, 0xF, false);
        case 2: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xF, 0xF, false);
        default: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xF, 0xF, false);
    }
}
__device__ __forceinline__ fe quad_fe(const fe& v, int k) {
    fe r;
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = quad_word(v.l[i], k);
    return r;
}
__device__ __forceinline__ fe pick_fe(int q, const fe& a0, const fe& a1, const fe& a2, const fe& a3) {
    // by masks, not by `?:` -- the compiler turns a select between structures into four branches under EXEC, each with its own
    // copy of the product that follows, and the four lanes then take their turns
    u32 m0 = q == 0 ? ~0u : 0u, m1 = q == 1 ? ~0u : 0u, m2 = q == 2 ? ~0u : 0u, m3 = q == 3 ? ~0u : 0u;
    asm volatile("" : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3));
    fe r;
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = (a0.l[i] & m0) | (a1.l[i] & m1) | (a2.l[i] & m2) | (a3.l[i] & m3);
    return r;
}
__device__ __forceinline__ void fe_opaque(fe& v) {
#pragma unroll
    for (int i = 0; i < NR; ++i) asm volatile("" : "+v"(v.l[i]));
}
#ifndef MSM_G2
__device__ __forceinline__ void cf_opaque(cf& v) { fe_opaque(v); }
__device__ __forceinline__ cf quad_cf(const cf& v, int k) { return quad_fe(v, k); }
__device__ __forceinline__ cf pick_cf(int q, const cf& a0, const cf& a1, const cf& a2, const cf& a3) { return pick_fe(q, a0, a1, a2, a3); }
#else
__device__ __forceinline__ void cf_opaque(cf& v) { fe_opaque(v.c0); fe_opaque(v.c1); }
__device__ __forceinline__ cf quad_cf(const cf& v, int k) { cf r; r.c0 = quad_fe(v.c0, k); r.c1 = quad_fe(v.c1, k); return r; }
__device__ __forceinline__ cf pick_cf(int q, const cf& a0, const cf& a1, const cf& a2, const cf& a3) {
    cf r; r.c0 = pick_fe(q, a0.c0, a1.c0, a2.c0, a3.c0); r.c1 = pick_fe(q, a0.c1, a1.c1, a2.c1, a3.c1); return r;
}
#endif
// one stage: lane q multiplies (a_q, b_q); out[k] = the product of lane k, in every lane
__device__ PT_COLD_ATTR void quad_stage(const cf& a0, const cf& b0, const cf& a1, const cf& b1, const cf& a2, const cf& b2, const cf& a3, const cf& b3,
                                        cf& o0, cf& o1, cf& o2, cf& o3) {
    const int q = threadIdx.x & 3;
    cf prod = cf_mul(pick_cf(q, a0, a1, a2, a3), pick_cf(q, b0, b1, b2, b3));
    cf_opaque(prod);                                                       // (the broadcasts read exactly this value)
    o0 = quad_cf(prod, 0); o1 = quad_cf(prod, 1); o2 = quad_cf(prod, 2); o3 = quad_cf(prod, 3);
    cf_opaque(o0); cf_opaque(o1); cf_opaque(o2); cf_opaque(o3);
}
#ifndef MSM_G2
// G1's last stage of an addition: pt_finish has Y3 as ONE sum of two products (fe_mul2), so the quad does too -- lanes 0 and 1 compute
// a b + c d, lanes 2 and 3 e f (fe_mul2 with a zero second product: the column sums, hence the limbs, of fe_mul(e, f))
__device__ PT_COLD_ATTR void quad_stage_y(const cf& a, const cf& b, const cf& c, const cf& d, const cf& e, const cf& f, cf& o0, cf& o2) {
    const int q = threadIdx.x & 3;
    const cf z = cf_zero();
    cf prod = fe_mul2(pick_cf(q, a, a, e, e), pick_cf(q, b, b, f, f), pick_cf(q, c, c, z, z), pick_cf(q, d, d, z, z));
    cf_opaque(prod);
    o0 = quad_cf(prod, 0); o2 = quad_cf(prod, 2);
    cf_opaque(o0); cf_opaque(o2);
}
#endif
__device__ PT_COLD_ATTR xyzz pt_dbl4(const xyzz& p) {   // pt_dbl, three stages
    if (pt_is_inf(p)) return p;
    const cf U = cf_dbl(p.Y);
    cf V, xx, W, S, MM, t1, t2, d0, d1;
    quad_stage(U, U, p.X, p.X, U, U, U, U, V, xx, d0, d1);                      // V = U^2, xx = X^2
    const cf M = cf_add(cf_dbl(xx), xx);
    quad_stage(U, V, p.X, V, M, M, U, V, W, S, MM, d0);                          // W = U V, S = X V, M^2
    xyzz r;
    r.X = cf_sub<4>(MM, cf_dbl(S));
    quad_stage(cf_sub<8>(S, r.X), M, W, p.Y, V, p.ZZ, W, p.ZZZ, t1, t2, r.ZZ, r.ZZZ);
    r.Y = cf_sub<2>(t1, t2);
    return r;
}
__device__ PT_COLD_ATTR xyzz pt_add4(const xyzz& p, const xyzz& q) {   // pt_add, four stages
    if (pt_is_inf(p)) return q;
    if (pt_is_inf(q)) return p;
    cf U1, U2, S1, S2, PP, RR, ZZ12, ZZZ12, PPP, Q, d0;
    quad_stage(p.X, q.ZZ, q.X, p.ZZ, p.Y, q.ZZZ, q.Y, p.ZZZ, U1, U2, S1, S2);
    const cf P = cf_sub<2>(U2, U1), Rr = cf_sub<2>(S2, S1);                      // < 4q
    quad_stage(P, P, Rr, Rr, p.ZZ, q.ZZ, p.ZZZ, q.ZZZ, PP, RR, ZZ12, ZZZ12);
    if (cf_is_zero_m(PP)) return cf_is_zero_m(RR) ? pt_dbl4(p) : pt_inf();
    xyzz r;
    quad_stage(P, PP, U1, PP, ZZ12, PP, P, PP, PPP, Q, r.ZZ, d0);
    r.X = cf_sub<4>(cf_sub<2>(RR, PPP), cf_dbl(Q));
#ifdef MSM_G2
    cf t1, t2;
    quad_stage(cf_sub<8>(Q, r.X), Rr, S1, PPP, ZZZ12, PPP, S1, PPP, t1, t2, r.ZZZ, d0);
    r.Y = cf_sub<2>(t1, t2);
#else
    quad_stage_y(cf_sub<8>(Q, r.X), Rr, cf_sub<4>(cf_zero(), S1), PPP, ZZZ12, PPP, r.Y, r.ZZZ);   // Y3 as pt_finish has it: < 2q
#endif
    return r;
}
// affine (external layout) of a finite point: x = X/ZZ, y = Y/ZZZ; 1/ZZ = (ZZ/ZZZ)^2 because ZZ^3 = ZZZ^2
__device__ void pt_to_std(const xyzz& p, u32* x, u32* y) {   // CW_STD words each
    const cf izzz = cf_inv(p.ZZZ), t = cf_mul(p.ZZ, izzz), izz = cf_sqr(t);
    cf_to_std(cf_mul(p.X, izz), x); cf_to_std(cf_mul(p.Y, izzz), y);
}
