// Goldilocks field (p = 2^64 - 2^32 + 1) and its cubic extension for gfx950 device code.
//
// Representation: canonical u64 (NOT Montgomery).  The reference stores a*2^64 mod p
// (fields/src/field_gl.rs:16,454-458,525-538) but every observable artefact is the canonical
// as_int() (:542-544); its own SIMD path also computes in canonical form with the
// 2^64 = 2^32 - 1 reduction (fields/src/arch/x86_64/avx2_field_gl.rs:361,460), which is what
// maps best onto CDNA4: a 64x64->128 product is four v_mad_u64_u32 and the reduction is a
// handful of 32-bit add/sub-with-carry -- no second multiply as Montgomery would need.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ZK-JIT-BEGIN  (the region up to ZK-JIT-END is also the prelude of the run-time compiled
// constraint kernels, csrc/expr_jit.hip; keep it free of #include and host-only code)
typedef unsigned long long u64;
typedef unsigned int u32;
#define GL_P 0xFFFFFFFF00000001ULL
#define GL_EPS 0xFFFFFFFFULL

namespace gl {

// add/sub are written on 32-bit limbs with explicit carries: on gfx950 v_add_co/v_addc_co are
// double-rate VALU ops while 64-bit compares + selects are not (tools/ubench_valu.hip,
// tools/field_probe.hip measured the variants: -20 % cycles on an NTT-shaped workload).
//
// GL_OPAQUE: every operation makes its operands opaque to the optimiser first.  Without it hipcc
// (ROCm 7.2, LLVM 22) folds a producer's plain add/sub into a consumer's carry op
// ("addcarry (add x, y), 0, cc -> addcarry x, y, cc") although the carry-OUT is used, which changes
// the carry and silently corrupts e.g. add(sub(a, b), 0) -- found by tests/test_gpu_stark_steps.py,
// reproduced in tools/dbg/dbg_f3b.hip.  The empty asm costs no instruction.
#define GL_OPAQUE(x) asm("" : "+v"(x))
__device__ __forceinline__ u64 mk64(u32 lo, u32 hi) { return ((u64)hi << 32) | lo; }
__device__ __forceinline__ u64 add(u64 a, u64 b) {  // field_gl.rs:385-388; canonical in -> canonical out
    GL_OPAQUE(a); GL_OPAQUE(b);
    u32 c0, c1, d0, d1;
    u32 s0 = __builtin_addc((u32)a, (u32)b, 0u, &c0);
    u32 s1 = __builtin_addc((u32)(a >> 32), (u32)(b >> 32), c0, &c1);
    u32 t0 = __builtin_addc(s0, 0xFFFFFFFFu, 0u, &d0);  // t = s - p = s + 2^32 - 1 (mod 2^64)
    u32 t1 = __builtin_addc(s1, 0u, d0, &d1);           // d1 <=> s >= p
    const bool sel = (c1 | d1) != 0;
    return mk64(sel ? t0 : s0, sel ? t1 : s1);
}
__device__ __forceinline__ u64 sub(u64 a, u64 b) {  // field_gl.rs:395-403
    GL_OPAQUE(a); GL_OPAQUE(b);
    u32 b0, b1, e0, e1;
    u32 d0 = __builtin_subc((u32)a, (u32)b, 0u, &b0);
    u32 d1 = __builtin_subc((u32)(a >> 32), (u32)(b >> 32), b0, &b1);
    u32 m = 0u - b1;                                      // borrow ? 2^32 - 1 : 0;  d + p == d - (2^32 - 1)
    u32 r0 = __builtin_subc(d0, m, 0u, &e0);
    u32 r1 = __builtin_subc(d1, 0u, e0, &e1);
    return mk64(r0, r1);
}
__host__ __device__ __forceinline__ u64 neg(u64 a) { return a ? GL_P - a : 0; }

// x = hi*2^64 + lo  ->  x mod p, canonical.  2^64 = 2^32 - 1, 2^96 = -1 (mod p).
__host__ __device__ __forceinline__ u64 reduce128(u64 lo, u64 hi) {
    u64 hi_hi = hi >> 32, hi_lo = hi & GL_EPS;
    u64 t0 = lo - hi_hi;
    if (lo < hi_hi) t0 -= GL_EPS;
    u64 t1 = (hi_lo << 32) - hi_lo;  // hi_lo * (2^32 - 1)
    u64 t2 = t0 + t1;
    if (t2 < t1) t2 += GL_EPS;
    return t2 >= GL_P ? t2 - GL_P : t2;
}
// a*b mod p, any u64 inputs, canonical output (field_gl.rs:454-458, observable value).
//   product : four v_mad_u64_u32 (the compiler's a*b + __umul64hi(a,b) spends seven multiplies)
//   reduce  : x = lo + r2*2^64 + r3*2^96 = lo - r3 + r2*(2^32-1); the r2 term is ONE
//             v_mad_u64_u32 whose carry-out (vcc) selects the +2^32-1 fix-up.
// t + r2*(2^32-1) mod p, canonical: ONE v_mad_u64_u32 whose carry-out (vcc) selects the +2^32-1 fix-up
__device__ __forceinline__ u64 mad_eps(u32 r2, u64 t) {
    u64 u; u32 m;
    asm("v_mad_u64_u32 %0, vcc, %2, -1, %3\n\ts_nop 1\n\tv_cndmask_b32_e64 %1, 0, -1, vcc"
                 : "=&v"(u), "=v"(m) : "v"(r2), "v"(t) : "vcc");
    u += m;                                              // carried: u += 2^32 - 1 (cannot carry again)
    u32 d0, d1;
    const u32 v0 = __builtin_addc((u32)u, 0xFFFFFFFFu, 0u, &d0);
    const u32 v1 = __builtin_addc((u32)(u >> 32), 0u, d0, &d1);  // d1 <=> u >= p
    return mk64(d1 ? v0 : (u32)u, d1 ? v1 : (u32)(u >> 32));
}
// lo + r2*2^64 + r3*2^96 mod p = lo - r3 + r2*(2^32-1), canonical; any 32-bit words
// (w1:w0) - r3, minus 2^32 - 1 more if that borrowed: five instructions with the borrows travelling as carry-ins.  Written as asm
// because the compiler lowers `subc(w1, 0, borrow)` to a v_cndmask + v_sub_co pair (one instruction more per field product: round 5);
// the wait states between a flag's producer and its consumer are the compiler's own (s_nop 1), which it cannot add inside asm.
__device__ __forceinline__ u64 sub_word_fold(u32 w0, u32 w1, u32 r3) {
    u32 t0, t1, mb;
    asm("v_sub_co_u32 %0, vcc, %3, %5\n\ts_nop 1\n\t"
        "v_subbrev_co_u32 %1, vcc, 0, %4, vcc\n\ts_nop 1\n\t"
        "v_cndmask_b32_e64 %2, 0, -1, vcc\n\t"
        "v_sub_co_u32 %0, vcc, %0, %2\n\ts_nop 1\n\t"
        "v_subbrev_co_u32 %1, vcc, 0, %1, vcc"
        : "=&v"(t0), "=&v"(t1), "=&v"(mb) : "v"(w0), "v"(w1), "v"(r3) : "vcc");
    return mk64(t0, t1);
}
__device__ __forceinline__ u64 reduce_words(u32 w0, u32 w1, u32 r2, u32 r3) { return mad_eps(r2, sub_word_fold(w0, w1, r3)); }
__device__ __forceinline__ u64 mul(u64 a, u64 b) {
    GL_OPAQUE(a); GL_OPAQUE(b);
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u64 p0 = (u64)a0 * b0;
    const u64 p1 = (u64)a0 * b1 + (p0 >> 32);
    const u64 p2 = (u64)a1 * b0 + (u32)p1;
    const u64 p3 = (u64)a1 * b1 + (p1 >> 32) + (p2 >> 32);
    return reduce_words((u32)p0, (u32)p2, (u32)p3, (u32)(p3 >> 32));
}
// a*b + c mod p, any u64 inputs, canonical output: c rides on the product's multiply-adds
__device__ __forceinline__ u64 mul_add(u64 a, u64 b, u64 c) {
    GL_OPAQUE(a); GL_OPAQUE(b); GL_OPAQUE(c);
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u64 p0 = (u64)a0 * b0 + (u32)c;
    const u64 p1 = (u64)a0 * b1 + (p0 >> 32) + (c >> 32);   // <= (2^32-1)^2 + 2(2^32-1) = 2^64 - 1
    const u64 p2 = (u64)a1 * b0 + (u32)p1;
    const u64 p3 = (u64)a1 * b1 + (p1 >> 32) + (p2 >> 32);
    return reduce_words((u32)p0, (u32)p2, (u32)p3, (u32)(p3 >> 32));
}
__device__ __forceinline__ u64 sqr(u64 a) { return mul(a, a); }
__device__ __forceinline__ u64 pow(u64 a, u64 e) {  // field_gl.rs:467-479
    u64 r = 1;
    while (e) { if (e & 1) r = mul(r, a); a = mul(a, a); e >>= 1; }
    return r;
}
// a^(p - 2), p - 2 = 0xFFFFFFFE_FFFFFFFF = (2^31 - 1) 2^33 + (2^32 - 1): an addition chain of 64 squarings and 10 products (field_gl.rs:415-449
// walks its own chain of 72); square-and-multiply over the 63 one-bits took 125 -- an inversion is a single dependent chain wherever it occurs
__device__ __forceinline__ u64 sqr_n(u64 a, int n) {
#pragma unroll 1
    for (int i = 0; i < n; ++i) a = mul(a, a);
    return a;
}
__device__ __forceinline__ u64 inv(u64 a) {
    const u64 t2 = mul(mul(a, a), a);                 // a^(2^2 - 1)
    const u64 t3 = mul(mul(t2, t2), a);               // a^(2^3 - 1)
    const u64 t6 = mul(sqr_n(t3, 3), t3);
    const u64 t7 = mul(mul(t6, t6), a);
    const u64 t14 = mul(sqr_n(t7, 7), t7);
    const u64 t15 = mul(mul(t14, t14), a);
    const u64 t30 = mul(sqr_n(t15, 15), t15);
    const u64 t31 = mul(mul(t30, t30), a);            // a^(2^31 - 1)
    const u64 t32 = mul(mul(t31, t31), a);            // a^(2^32 - 1)
    return mul(sqr_n(t31, 33), t32);
}

// GF(p^3) = GF(p)[x]/(x^3 - x - 1)  (starky/src/f3g.rs).  Device values never carry the
// reference's runtime `dim` tag: the width (1 or 3 words) is a static property of each buffer.
struct f3 { u64 v[3]; };
__device__ __forceinline__ f3 f3_add(f3 a, f3 b) { return f3{{add(a.v[0], b.v[0]), add(a.v[1], b.v[1]), add(a.v[2], b.v[2])}}; }
__device__ __forceinline__ f3 f3_sub(f3 a, f3 b) { return f3{{sub(a.v[0], b.v[0]), sub(a.v[1], b.v[1]), sub(a.v[2], b.v[2])}}; }
__device__ __forceinline__ f3 f3_muls(f3 a, u64 s) { return f3{{mul(a.v[0], s), mul(a.v[1], s), mul(a.v[2], s)}}; }
__device__ __forceinline__ f3 f3_mul(f3 a, f3 b) {  // f3g.rs:420-430
    u64 A = mul(add(a.v[0], a.v[1]), add(b.v[0], b.v[1]));
    u64 B = mul(add(a.v[0], a.v[2]), add(b.v[0], b.v[2]));
    u64 C = mul(add(a.v[1], a.v[2]), add(b.v[1], b.v[2]));
    u64 D = mul(a.v[0], b.v[0]), E = mul(a.v[1], b.v[1]), F = mul(a.v[2], b.v[2]);
    u64 G = sub(D, E);
    return f3{{sub(add(C, G), F), sub(sub(sub(add(A, C), E), E), D), sub(B, G)}};
}
__device__ __forceinline__ f3 f3_inv(f3 x) {  // f3g.rs:207-235
    u64 a = x.v[0], b = x.v[1], c = x.v[2];
    u64 aa = mul(a, a), ac = mul(a, c), ba = mul(b, a), bb = mul(b, b), bc = mul(b, c), cc = mul(c, c);
    u64 aaa = mul(aa, a), aac = mul(aa, c), abc = mul(ba, c), abb = mul(ba, b);
    u64 acc = mul(ac, c), bbb = mul(bb, b), bcc = mul(bc, c), ccc = mul(cc, c);
    u64 t = neg(aaa);
    t = sub(t, aac); t = sub(t, aac);
    t = add(t, abc); t = add(t, abc); t = add(t, abc);
    t = add(t, abb); t = sub(t, acc); t = sub(t, bbb); t = add(t, bcc); t = sub(t, ccc);
    u64 ti = inv(t);
    u64 i1 = neg(aa);
    i1 = sub(i1, ac); i1 = sub(i1, ac); i1 = add(i1, bc); i1 = add(i1, bb); i1 = sub(i1, cc);
    u64 i2 = sub(ba, cc);
    u64 i3 = add(sub(ac, bb), cc);
    return f3{{mul(i1, ti), mul(i2, ti), mul(i3, ti)}};
}

// ZK-JIT-END

// ---- non-canonical ("nc") variants: results are SOME u64 congruent to the value, not necessarily < p.  Every
// operation here accepts such operands wherever it says "any u64"; chains of them (the Poseidon permutation)
// canonicalise once at the end instead of after every step (4-5 instructions per operation).
__device__ __forceinline__ u64 mad_eps_nc(u32 r2, u64 t) {          // t + r2*(2^32-1), any u64 representative
    u64 u; u32 m;
    asm("v_mad_u64_u32 %0, vcc, %2, -1, %3\n\ts_nop 1\n\tv_cndmask_b32_e64 %1, 0, -1, vcc"
                 : "=&v"(u), "=v"(m) : "v"(r2), "v"(t) : "vcc");
    return u + m;                                                    // carried: += 2^32 - 1 (cannot carry again)
}
__device__ __forceinline__ u64 reduce_words_nc(u32 w0, u32 w1, u32 r2, u32 r3) { return mad_eps_nc(r2, sub_word_fold(w0, w1, r3)); }
// acc + x for a 32-bit word x as ONE multiply-add (x * 1 + acc) instead of a zero-extending move and a 64-bit addition
__device__ __forceinline__ u64 add_word(u64 acc, u32 x) {
    u64 d, carry;
    asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=v"(d), "=s"(carry) : "v"(x), "v"(acc));
    return d;
}
__device__ __forceinline__ u64 mul_nc(u64 a, u64 b) {                // any u64 in, nc out
    GL_OPAQUE(a); GL_OPAQUE(b);
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u64 p0 = (u64)a0 * b0;
    const u64 p1 = (u64)a0 * b1 + (p0 >> 32);
    const u64 p2 = (u64)a1 * b0 + (u32)p1;
    const u64 p3 = (u64)a1 * b1 + (p1 >> 32) + (p2 >> 32);
    return reduce_words_nc((u32)p0, (u32)p2, (u32)p3, (u32)(p3 >> 32));
}
// A squaring with the cross product a0 a1 taken once (round 4): three multiply-adds instead of four, the second use of the cross
// product a 64-bit addition.  The same number of instructions as the plain product, a cheaper mix: 2^22 x 19 tree 9.39-9.44 ms against
// 9.54-9.70 (profiles/r04/poseidon_variants.md).  Half of the S-box's products are squarings (x^2, x^6).
__device__ __forceinline__ u64 sqr_nc(u64 a) {
    GL_OPAQUE(a);
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32);
    const u64 p0 = (u64)a0 * a0;
    const u64 c = (u64)a0 * a1;
    const u64 p1 = c + (p0 >> 32);
    const u64 p2 = c + (u32)p1;
    const u64 p3 = (u64)a1 * a1 + (p1 >> 32) + (p2 >> 32);
    return reduce_words_nc((u32)p0, (u32)p2, (u32)p3, (u32)(p3 >> 32));
}
__device__ __forceinline__ u64 mul_add_nc(u64 a, u64 b, u64 c) {     // a*b + c, any u64 in, nc out
    GL_OPAQUE(a); GL_OPAQUE(b); GL_OPAQUE(c);
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u64 p0 = (u64)a0 * b0 + (u32)c;
    const u64 p1 = (u64)a0 * b1 + (p0 >> 32) + (c >> 32);
    const u64 p2 = (u64)a1 * b0 + (u32)p1;
    const u64 p3 = (u64)a1 * b1 + (p1 >> 32) + (p2 >> 32);
    return reduce_words_nc((u32)p0, (u32)p2, (u32)p3, (u32)(p3 >> 32));
}
// a + b for any u64 a and CANONICAL b (< p): a + b - 2^64 <= p - 2, so the 2^32 - 1 fix-up cannot carry again
__device__ __forceinline__ u64 add_nc(u64 a, u64 b) {
    GL_OPAQUE(a); GL_OPAQUE(b);
    u32 c0, c1, d0, d1;
    const u32 s0 = __builtin_addc((u32)a, (u32)b, 0u, &c0);
    const u32 s1 = __builtin_addc((u32)(a >> 32), (u32)(b >> 32), c0, &c1);
    const u32 m = 0u - c1;
    const u32 r0 = __builtin_addc(s0, m, 0u, &d0);
    const u32 r1 = __builtin_addc(s1, 0u, d0, &d1);
    return mk64(r0, r1);
}

// ---- the NTT passes' sums, differences and canonicalising tail, with the fix-ups as multiply-adds.  A multiply-add adds a 64-bit pair in
// ONE instruction and hands out its carry as a lane mask, where the two-limb forms spend a v_add_co / v_addc_co (v_sub_co / v_subb_co)
// pair; bit for bit what gl::add, gl::sub and gl::mad_eps return.  One instruction fewer per call; in the pass kernel that is 1 854 -> 1 688
// vector instructions per lane up to the last twiddles and 2 % of the 2^24 transform (profiles/r20/ntt_issue_slots.md, which also has why
// gl::sub itself stays as it is).  The wait states between a flag's producer and its consumer are written out (s_nop 1): the compiler
// cannot add them inside asm.  Every asm below is as opaque to the optimiser as GL_OPAQUE makes the operands of gl::add.
// a + b, canonical in -> canonical out.  t = s + 2^32 - 1 = s - p (mod 2^64) is `1 * (2^32 - 1) + s`; its carry-out <=> s >= p.
__device__ __forceinline__ u64 add_m(u64 a, u64 b) {
    u32 s0, s1, r0, r1; u64 c1, d1, t;
    asm("v_add_co_u32 %0, vcc, %3, %5\n\ts_nop 1\n\tv_addc_co_u32 %1, %2, %4, %6, vcc"
        : "=&v"(s0), "=&v"(s1), "=&s"(c1) : "v"((u32)a), "v"((u32)(a >> 32)), "v"((u32)b), "v"((u32)(b >> 32)) : "vcc");
    asm("v_mad_u64_u32 %0, %1, 1, -1, %2" : "=&v"(t), "=&s"(d1) : "v"(mk64(s0, s1)));
    asm("s_or_b64 %2, %2, %3\n\tv_cndmask_b32_e64 %0, %4, %6, %2\n\tv_cndmask_b32_e64 %1, %5, %7, %2"
        : "=&v"(r0), "=v"(r1), "+s"(d1) : "s"(c1), "v"(s0), "v"(s1), "v"((u32)t), "v"((u32)(t >> 32)) : "scc");
    return mk64(r0, r1);
}
// d - (2^32 - 1) if `borrowed` (a lane mask in vcc at the end of the asm that made d0, d1; m = borrowed ? -65537 : 0 comes from there):
// -(2^32 - 1) = -65537 * 65535, a product of two signed words, so the fix-up is ONE v_mad_i64_i32 on the pair
__device__ __forceinline__ u64 sub_eps_if(u32 m, u32 d0, u32 d1) {
    u64 r, cc;
    asm("v_mad_i64_i32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(cc) : "v"(m), "s"(65535), "v"(mk64(d0, d1)));
    return r;
}
// a - b, canonical in -> canonical out: d = a - b + 2^64 if it borrowed, and d + p = d - (2^32 - 1) (mod 2^64) then lies in [1, p - 1]
__device__ __forceinline__ u64 sub_m(u64 a, u64 b) {
    u32 d0, d1, m;
    asm("v_sub_co_u32 %0, vcc, %3, %5\n\ts_nop 1\n\tv_subb_co_u32 %1, vcc, %4, %6, vcc\n\ts_nop 1\n\tv_cndmask_b32_e64 %2, 0, %7, vcc"
        : "=&v"(d0), "=&v"(d1), "=v"(m) : "v"((u32)a), "v"((u32)(a >> 32)), "v"((u32)b), "v"((u32)(b >> 32)), "v"(-65537) : "vcc");
    return sub_eps_if(m, d0, d1);
}
// gl::mad_eps with the last step (u >= p ? u - p : u) as in add_m
__device__ __forceinline__ u64 mad_eps_m(u32 r2, u64 t) {
    const u64 u = mad_eps_nc(r2, t);
    u64 v, ge; u32 r0, r1;
    asm("v_mad_u64_u32 %0, %1, 1, -1, %2" : "=&v"(v), "=&s"(ge) : "v"(u));
    asm("s_nop 1\n\tv_cndmask_b32_e64 %0, %3, %5, %2\n\tv_cndmask_b32_e64 %1, %4, %6, %2"
        : "=&v"(r0), "=v"(r1) : "s"(ge), "v"((u32)u), "v"((u32)(u >> 32)), "v"((u32)v), "v"((u32)(v >> 32)));
    return mk64(r0, r1);
}

// ---- the NTT passes' twiddle product: a 64 x 64 product whose four multiply-adds take the 32-bit halves directly.
// gl::mul chains its multiply-adds through the HIGH word of the one before (p1 = a0 b1 + (p0 >> 32), ...): a 64-bit
// addend has to be a register pair, so every link costs a move beside a zero register (4 moves and a 64-bit add per product).
// Here only the two cross products chain (64-bit result into 64-bit addend, no move); the columns are then summed with
// 32-bit carry adds, and the last carry rides as the borrow-in of the 2^96 fold instead of being added to r3 first:
//   a b = L + 2^32 (c:M) + 2^64 H,  L = a0 b0, c:M = a0 b1 + a1 b0 (65 bits), H = a1 b1
//   w0 = L0, w1 = L1 + M0 -> k1, r2 = M1 + H0 + k1 -> k2, r3 = H1 + c + k2   (H1 <= 2^32 - 2: H1 + c cannot wrap)
// Returns (w1:w0) - r3 folded as sub_word_fold does (minus 2^32 - 1 more if that borrowed, as ONE multiply-add: sub_eps_if) and r2 for
// mad_eps_m / mad_eps_nc: 11 instructions where the plain product and sub_word_fold spend 14.  Any u64 operands.  The asm is as opaque to the
// optimiser as GL_OPAQUE makes the operands of gl::mul.  The cross products come first: their carry c, an SGPR pair, has the
// two other multiply-adds between its producer and its consumer.  That distance is load-bearing: on the gfx940 family (gfx950
// included) an SGPR written by a VALU instruction may be read by a VALU instruction only 2 wait states later, the compiler cannot
// add wait states inside asm, and the first instruction of the second block reads c.  Whoever reorders the four multiply-adds
// keeps two instructions after the one that writes c (or puts an `s_nop 1` there).
__device__ __forceinline__ u64 mul_fold96(u64 a, u64 b, u32& r2) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    u64 l, m, h, c;
    asm("v_mad_u64_u32 %1, vcc, %4, %7, 0\n\t"
        "v_mad_u64_u32 %1, %3, %5, %6, %1\n\t"
        "v_mad_u64_u32 %0, vcc, %4, %6, 0\n\t"
        "v_mad_u64_u32 %2, vcc, %5, %7, 0"
        : "=&v"(l), "=&v"(m), "=&v"(h), "=&s"(c) : "v"(a0), "v"(a1), "v"(b0), "v"(b1) : "vcc");
    u32 t0, t1, mb, h1, w1;
    asm("v_addc_co_u32 %3, vcc, 0, %10, %11\n\t"
        "v_add_co_u32 %4, vcc, %6, %7\n\t"
        "s_nop 1\n\t"
        "v_addc_co_u32 %5, vcc, %8, %9, vcc\n\t"
        "s_nop 1\n\t"
        "v_subb_co_u32 %0, vcc, %12, %3, vcc\n\t"
        "s_nop 1\n\t"
        "v_subbrev_co_u32 %1, vcc, 0, %4, vcc\n\t"
        "s_nop 1\n\t"
        "v_cndmask_b32_e64 %2, 0, %13, vcc"
        : "=&v"(t0), "=&v"(t1), "=&v"(mb), "=&v"(h1), "=&v"(w1), "=&v"(r2)
        : "v"((u32)(l >> 32)), "v"((u32)m), "v"((u32)(m >> 32)), "v"((u32)h), "v"((u32)(h >> 32)), "s"(c), "v"((u32)l), "v"(-65537) : "vcc");
    return sub_eps_if(mb, t0, t1);
}
// x * w mod p, any u64 in, canonical out: bit for bit what gl::mul returns (17 instructions against 21 and no zero register pair)
__device__ __forceinline__ u64 mul_tw(u64 x, u64 w) { u32 r2; const u64 t = mul_fold96(x, w, r2); return mad_eps_m(r2, t); }
// the same without the final canonicalisation (14 instructions): for a product that feeds only other products
__device__ __forceinline__ u64 mul_tw_nc(u64 x, u64 w) { u32 r2; const u64 t = mul_fold96(x, w, r2); return mad_eps_nc(r2, t); }

// x * 2^E mod p for a compile-time 0 <= E < 96, canonical x -> canonical result.  2 has order 192
// and 2^96 = -1, so every root of unity of order <= 64 is a power of two (MG.0[6] = 2^39,
// constant.rs:54-68): the butterflies' small twiddles are shifts, not field multiplications.
// Callers fold E >= 96 into a swapped subtraction.
template <int E>
__device__ __forceinline__ u64 mul_pow2(u64 x) {
    static_assert(E >= 0 && E < 96, "fold 2^96 = -1 first");
    GL_OPAQUE(x);
    if constexpr (E == 0) {
        return x;
    } else if constexpr (E <= 32) {                       // lo + top*2^64, top < 2^32
        return mad_eps_m((u32)(x >> (64 - E)), x << E);
    } else if constexpr (E < 64) {
        // E = 32 + r: x 2^r = t2:t1:t0 (t2 < 2^r), so x 2^E = t0 2^32 + t1 2^64 + t2 2^96 = t0 2^32 + t1 (2^32 - 1) - t2.  With the addend
        // (t0 : ~t2) = t0 2^32 + (2^32 - 1) - t2 one multiply-add gives u + carry 2^64 = value + 2^32 - 1, i.e. value = u if it carried
        // (2^64 = 2^32 - 1) and u - (2^32 - 1) if not.  Both are already canonical: carried, u <= (2^32 - 1) 2^33 - 2^64 < p; not carried,
        // u - (2^32 - 1) < 2^64 - (2^32 - 1) = p.  Only t0 = t1 = 0 makes the difference negative (-t2), which the fold's second step turns
        // into p - t2.  11 instructions; lo + hi 2^64 through reduce_words and a canonicalisation took 15.
        constexpr int r = E - 32;
        const u32 x0 = (u32)x, x1 = (u32)(x >> 32);
        const u32 t1 = __builtin_amdgcn_alignbit(x1, x0, 32 - r);
        const u64 addend = mk64(~(x1 >> (32 - r)), x0 << r);
        u64 u; u32 m;
        asm("v_mad_u64_u32 %0, vcc, %2, -1, %3\n\ts_nop 1\n\tv_cndmask_b32_e64 %1, -1, 0, vcc"
                     : "=&v"(u), "=v"(m) : "v"(t1), "v"(addend) : "vcc");
        return sub_word_fold((u32)u, (u32)(u >> 32), m);
    } else {                                              // E = 64 + r: t0*2^64 - (x*2^r >> 32), t0 = low word of x*2^r
        constexpr int r = E - 64;
        const u32 t0 = (u32)x << r;
        u64 m = ((u64)t0 << 32) - t0;                     // t0*(2^32-1) < p
        u64 s = r == 0 ? (x >> 32) : (x >> (32 - r));     // < p
        return sub_m(m, s);
    }
}

// ---- paired forms of the NTT passes' primitives: two (bfly2_m: four) independent carry chains whose instructions alternate, so that the
// instruction behind a flag's producer belongs to another chain and not to the flag's consumer.  The single forms above keep every
// dependent instruction right behind its producer and write the two wait states between a vector instruction that writes an SGPR pair
// and the vector instruction that reads it as `s_nop 1`; here the other chain's instructions are those wait states, every chain has
// carry and mask SGPR pairs of its own (the VOP3 forms), and vcc only ever takes a carry-out nobody reads.  Where two chains leave a
// single instruction between producer and consumer, the second wait state is a written `s_nop 0`, named at its place.
// A primitive is a short run of asm statements, not one: inline asm cannot name the halves of a 64-bit operand, so a value that 32-bit
// carry instructions write and a multiply-add reads as a pair (or the other way round) changes its shape between two statements; every
// statement holds all chains, and no wait state is counted across a statement's end (the compiler pads one state there, no more).
// Results are bit for bit those of the single forms (tests/test_gpu_ntt_pairs.py).
// sum = add_m(a, b), diff = sub_m(a, b); canonical in -> canonical out
__device__ __forceinline__ void bfly_m(u64 a, u64 b, u64& sum, u64& diff) {
    u32 s0, s1, e0, e1, m, r0, r1; u64 cA, cS, dA, t, rs;
    asm("v_sub_co_u32 %[e0], %[cS], %[a0], %[b0]\n\t"
        "v_add_co_u32 %[s0], %[cA], %[a0], %[b0]\n\t"
        "s_nop 0\n\t"                                             // two chains: the second wait state of both carries
        "v_subb_co_u32 %[e1], %[cS], %[a1], %[b1], %[cS]\n\t"
        "v_addc_co_u32 %[s1], %[cA], %[a1], %[b1], %[cA]"
        : [e0] "=&v"(e0), [s0] "=&v"(s0), [e1] "=&v"(e1), [s1] "=v"(s1), [cS] "=&s"(cS), [cA] "=&s"(cA)
        : [a0] "v"((u32)a), [a1] "v"((u32)(a >> 32)), [b0] "v"((u32)b), [b1] "v"((u32)(b >> 32)));
    asm("v_mad_u64_u32 %[t], %[dA], 1, -1, %[S]\n\t"              // (the borrow cS: the sum's last carry and this stand behind its producer)
        "v_cndmask_b32_e64 %[m], 0, %[k], %[cS]\n\t"
        "v_mad_i64_i32 %[rs], vcc, %[m], %[c], %[D]\n\t"
        "s_or_b64 %[dA], %[dA], %[cA]"
        : [t] "=&v"(t), [dA] "=&s"(dA), [m] "=&v"(m), [rs] "=v"(rs)
        : [S] "v"(mk64(s0, s1)), [D] "v"(mk64(e0, e1)), [cS] "s"(cS), [cA] "s"(cA), [k] "v"(-65537), [c] "s"(65535) : "vcc", "scc");
    asm("v_cndmask_b32_e64 %[r0], %[s0], %[t0], %[dA]\n\tv_cndmask_b32_e64 %[r1], %[s1], %[t1], %[dA]"
        : [r0] "=&v"(r0), [r1] "=v"(r1) : [s0] "v"(s0), [s1] "v"(s1), [t0] "v"((u32)t), [t1] "v"((u32)(t >> 32)), [dA] "s"(dA));
    sum = mk64(r0, r1); diff = rs;
}
// two butterflies on independent operands, four chains (A: a + b, S: a - b, C: c + d, T: c - d): no written wait state
__device__ __forceinline__ void bfly2_m(u64 a, u64 b, u64 c, u64 d, u64& sum_ab, u64& diff_ab, u64& sum_cd, u64& diff_cd) {
    u32 s0, s1, e0, e1, u0, u1, f0, f1, mS, mT, r0, r1, q0, q1; u64 cA, cS, cC, cT, dA, dC, tA, tC, rs, rt;
    asm("v_add_co_u32 %[s0], %[cA], %[a0], %[b0]\n\t"
        "v_sub_co_u32 %[e0], %[cS], %[a0], %[b0]\n\t"
        "v_add_co_u32 %[u0], %[cC], %[c0], %[d0]\n\t"
        "v_sub_co_u32 %[f0], %[cT], %[c0], %[d0]\n\t"
        "v_addc_co_u32 %[s1], %[cA], %[a1], %[b1], %[cA]\n\t"
        "v_subb_co_u32 %[e1], %[cS], %[a1], %[b1], %[cS]\n\t"
        "v_addc_co_u32 %[u1], %[cC], %[c1], %[d1], %[cC]\n\t"
        "v_subb_co_u32 %[f1], %[cT], %[c1], %[d1], %[cT]"
        : [s0] "=&v"(s0), [e0] "=&v"(e0), [u0] "=&v"(u0), [f0] "=&v"(f0), [s1] "=&v"(s1), [e1] "=&v"(e1), [u1] "=&v"(u1), [f1] "=v"(f1),
          [cA] "=&s"(cA), [cS] "=&s"(cS), [cC] "=&s"(cC), [cT] "=&s"(cT)
        : [a0] "v"((u32)a), [a1] "v"((u32)(a >> 32)), [b0] "v"((u32)b), [b1] "v"((u32)(b >> 32)),
          [c0] "v"((u32)c), [c1] "v"((u32)(c >> 32)), [d0] "v"((u32)d), [d1] "v"((u32)(d >> 32)));
    asm("v_mad_u64_u32 %[tA], %[dA], 1, -1, %[SA]\n\t"
        "v_mad_u64_u32 %[tC], %[dC], 1, -1, %[SC]\n\t"
        "v_cndmask_b32_e64 %[mS], 0, %[k], %[cS]\n\t"
        "v_cndmask_b32_e64 %[mT], 0, %[k], %[cT]\n\t"             // cT: the last instruction of the statement above, three behind
        "v_mad_i64_i32 %[rs], vcc, %[mS], %[c], %[DS]\n\t"
        "v_mad_i64_i32 %[rt], vcc, %[mT], %[c], %[DT]\n\t"
        "s_or_b64 %[dA], %[dA], %[cA]\n\t"
        "s_or_b64 %[dC], %[dC], %[cC]"
        : [tA] "=&v"(tA), [tC] "=&v"(tC), [dA] "=&s"(dA), [dC] "=&s"(dC), [mS] "=&v"(mS), [mT] "=&v"(mT), [rs] "=&v"(rs), [rt] "=v"(rt)
        : [SA] "v"(mk64(s0, s1)), [SC] "v"(mk64(u0, u1)), [DS] "v"(mk64(e0, e1)), [DT] "v"(mk64(f0, f1)),
          [cS] "s"(cS), [cT] "s"(cT), [cA] "s"(cA), [cC] "s"(cC), [k] "v"(-65537), [c] "s"(65535) : "vcc", "scc");
    asm("v_cndmask_b32_e64 %[r0], %[s0], %[t0], %[dA]\n\tv_cndmask_b32_e64 %[r1], %[s1], %[t1], %[dA]\n\t"
        "v_cndmask_b32_e64 %[q0], %[u0], %[v0], %[dC]\n\tv_cndmask_b32_e64 %[q1], %[u1], %[v1], %[dC]"
        : [r0] "=&v"(r0), [r1] "=&v"(r1), [q0] "=&v"(q0), [q1] "=v"(q1)
        : [s0] "v"(s0), [s1] "v"(s1), [t0] "v"((u32)tA), [t1] "v"((u32)(tA >> 32)), [dA] "s"(dA),
          [u0] "v"(u0), [u1] "v"(u1), [v0] "v"((u32)tC), [v1] "v"((u32)(tC >> 32)), [dC] "s"(dC));
    sum_ab = mk64(r0, r1); diff_ab = rs; sum_cd = mk64(q0, q1); diff_cd = rt;
}
// two differences, sub_m(a, b) and sub_m(c, d)
__device__ __forceinline__ void sub2_m(u64 a, u64 b, u64 c, u64 d, u64& diff_ab, u64& diff_cd) {
    u32 e0, e1, f0, f1, mS, mT; u64 cS, cT, rs, rt;
    asm("v_sub_co_u32 %[e0], %[cS], %[a0], %[b0]\n\t"
        "v_sub_co_u32 %[f0], %[cT], %[c0], %[d0]\n\t"
        "s_nop 0\n\t"                                             // two chains: the second wait state of both borrows
        "v_subb_co_u32 %[e1], %[cS], %[a1], %[b1], %[cS]\n\t"
        "v_subb_co_u32 %[f1], %[cT], %[c1], %[d1], %[cT]\n\t"
        "s_nop 0\n\t"                                             // the same
        "v_cndmask_b32_e64 %[mS], 0, %[k], %[cS]\n\t"
        "v_cndmask_b32_e64 %[mT], 0, %[k], %[cT]"
        : [e0] "=&v"(e0), [f0] "=&v"(f0), [e1] "=&v"(e1), [f1] "=&v"(f1), [mS] "=&v"(mS), [mT] "=v"(mT), [cS] "=&s"(cS), [cT] "=&s"(cT)
        : [a0] "v"((u32)a), [a1] "v"((u32)(a >> 32)), [b0] "v"((u32)b), [b1] "v"((u32)(b >> 32)),
          [c0] "v"((u32)c), [c1] "v"((u32)(c >> 32)), [d0] "v"((u32)d), [d1] "v"((u32)(d >> 32)), [k] "v"(-65537));
    asm("v_mad_i64_i32 %[rs], vcc, %[mS], %[c], %[DS]\n\tv_mad_i64_i32 %[rt], vcc, %[mT], %[c], %[DT]"
        : [rs] "=&v"(rs), [rt] "=v"(rt) : [mS] "v"(mS), [mT] "v"(mT), [DS] "v"(mk64(e0, e1)), [DT] "v"(mk64(f0, f1)), [c] "s"(65535) : "vcc");
    diff_ab = rs; diff_cd = rt;
}

// The tail of two products or shifts, t + r2 (2^32 - 1) mod p twice (mad_eps_nc / mad_eps_m).  The carried fix-up u += 2^32 - 1 is ONE
// multiply-add, m * 1 + u with m = 0 or 2^32 - 1, where mad_eps_nc leaves a 64-bit addition (two carry instructions) to the compiler.
// HEAD: both multiply-adds, then both masks; TAIL_NC / TAIL_M: the fix-up (and the canonicalising multiply-add, whose mask gA has the
// other chain's two instructions behind it, gB the first two selects of the last statement)
#define GL_TAIL2_HEAD \
        "v_mad_u64_u32 %[tA], %[kA], %[r2A], -1, %[tA]\n\t" \
        "v_mad_u64_u32 %[tB], %[kB], %[r2B], -1, %[tB]\n\t" \
        "s_nop 0\n\t"                                             /* two chains: the second wait state of both carries */ \
        "v_cndmask_b32_e64 %[r2A], 0, -1, %[kA]\n\t" \
        "v_cndmask_b32_e64 %[r2B], 0, -1, %[kB]\n\t"
#define GL_TAIL2_NC \
        "v_mad_u64_u32 %[tA], vcc, %[r2A], 1, %[tA]\n\t" \
        "v_mad_u64_u32 %[tB], vcc, %[r2B], 1, %[tB]"
#define GL_TAIL2_M \
        "v_mad_u64_u32 %[tA], vcc, %[r2A], 1, %[tA]\n\t" \
        "v_mad_u64_u32 %[vA], %[gA], 1, -1, %[tA]\n\t" \
        "v_mad_u64_u32 %[tB], vcc, %[r2B], 1, %[tB]\n\t" \
        "v_mad_u64_u32 %[vB], %[gB], 1, -1, %[tB]"
// the 2^96 fold's last step in front of the tail (sub_eps_if on both chains)
#define GL_FOLD2 \
        "v_mad_i64_i32 %[tA], vcc, %[bA], %[c], %[tA]\n\t" \
        "v_mad_i64_i32 %[tB], vcc, %[bB], %[c], %[tB]\n\t"
// Every value of a chain stays in the registers of the one it replaces (t -> u, r2 -> the mask): a pair of products holds no more
// registers than its operands and the two canonicalised candidates
__device__ __forceinline__ void canon_select2(u64 uA, u64 vA, u64 gA, u64 uB, u64 vB, u64 gB, u64& ra, u64& rb) {
    u32 r0 = (u32)uA, r1 = (u32)(uA >> 32), q0 = (u32)uB, q1 = (u32)(uB >> 32);
    asm("v_cndmask_b32_e64 %[r0], %[r0], %[v0], %[gA]\n\tv_cndmask_b32_e64 %[r1], %[r1], %[v1], %[gA]\n\t"
        "v_cndmask_b32_e64 %[q0], %[q0], %[y0], %[gB]\n\tv_cndmask_b32_e64 %[q1], %[q1], %[y1], %[gB]"
        : [r0] "+v"(r0), [r1] "+v"(r1), [q0] "+v"(q0), [q1] "+v"(q1)
        : [v0] "v"((u32)vA), [v1] "v"((u32)(vA >> 32)), [gA] "s"(gA), [y0] "v"((u32)vB), [y1] "v"((u32)(vB >> 32)), [gB] "s"(gB));
    ra = mk64(r0, r1); rb = mk64(q0, q1);
}
// mad_eps_m(r2a, ta) and mad_eps_m(r2b, tb)
__device__ __forceinline__ void mad_eps2_m(u32 r2a, u64 ta, u32 r2b, u64 tb, u64& ra, u64& rb) {
    u64 vA, vB, kA, kB, gA, gB;
    asm(GL_TAIL2_HEAD GL_TAIL2_M
        : [tA] "+v"(ta), [tB] "+v"(tb), [r2A] "+v"(r2a), [r2B] "+v"(r2b), [vA] "=&v"(vA), [vB] "=&v"(vB),
          [kA] "=&s"(kA), [kB] "=&s"(kB), [gA] "=&s"(gA), [gB] "=&s"(gB)
        : : "vcc");
    canon_select2(ta, vA, gA, tb, vB, gB, ra, rb);
}

// Two twiddle products, mul_fold96 twice: (t0 : t1), the fold's mask b and r2 of each, for the tail above
struct fold96_pair { u32 t0A, t1A, bA, r2A, t0B, t1B, bB, r2B; };
__device__ __forceinline__ fold96_pair mul_fold96_2(u64 x0, u64 w0, u64 x1, u64 w1) {
    u64 lA, mA, hA, lB, mB, hB, cA, cB;
    asm("v_mad_u64_u32 %[mA], vcc, %[xa0], %[wa1], 0\n\t"
        "v_mad_u64_u32 %[mB], vcc, %[xb0], %[wb1], 0\n\t"
        "v_mad_u64_u32 %[mA], %[cA], %[xa1], %[wa0], %[mA]\n\t"
        "v_mad_u64_u32 %[mB], %[cB], %[xb1], %[wb0], %[mB]\n\t"
        "v_mad_u64_u32 %[lA], vcc, %[xa0], %[wa0], 0\n\t"
        "v_mad_u64_u32 %[lB], vcc, %[xb0], %[wb0], 0\n\t"
        "v_mad_u64_u32 %[hA], vcc, %[xa1], %[wa1], 0\n\t"
        "v_mad_u64_u32 %[hB], vcc, %[xb1], %[wb1], 0"
        : [lA] "=&v"(lA), [mA] "=&v"(mA), [hA] "=&v"(hA), [lB] "=&v"(lB), [mB] "=&v"(mB), [hB] "=v"(hB), [cA] "=&s"(cA), [cB] "=&s"(cB)
        : [xa0] "v"((u32)x0), [xa1] "v"((u32)(x0 >> 32)), [wa0] "v"((u32)w0), [wa1] "v"((u32)(w0 >> 32)),
          [xb0] "v"((u32)x1), [xb1] "v"((u32)(x1 >> 32)), [wb0] "v"((u32)w1), [wb1] "v"((u32)(w1 >> 32)) : "vcc");
    // The column sums and the fold, as mul_fold96 orders them per chain, every result in the register of the word it replaces:
    // l0 -> t0, l1 -> w1 -> t1, m0 -> the fold's mask, m1 -> r2, h1 -> h1 + c.  h1 (no flag of its chain) fills a wait state of each side.
    u32 lA0 = (u32)lA, lA1 = (u32)(lA >> 32), mA0 = (u32)mA, mA1 = (u32)(mA >> 32), hA1 = (u32)(hA >> 32);
    u32 lB0 = (u32)lB, lB1 = (u32)(lB >> 32), mB0 = (u32)mB, mB1 = (u32)(mB >> 32), hB1 = (u32)(hB >> 32);
    u64 kA, kB;
    asm("v_add_co_u32 %[lA1], %[kA], %[lA1], %[mA0]\n\t"
        "v_add_co_u32 %[lB1], %[kB], %[lB1], %[mB0]\n\t"
        "v_addc_co_u32 %[hA1], vcc, 0, %[hA1], %[cA]\n\t"
        "v_addc_co_u32 %[mA1], %[kA], %[mA1], %[hA0], %[kA]\n\t"
        "v_addc_co_u32 %[mB1], %[kB], %[mB1], %[hB0], %[kB]\n\t"
        "v_addc_co_u32 %[hB1], vcc, 0, %[hB1], %[cB]\n\t"
        "v_subb_co_u32 %[lA0], %[kA], %[lA0], %[hA1], %[kA]\n\t"
        "v_subb_co_u32 %[lB0], %[kB], %[lB0], %[hB1], %[kB]\n\t"
        "s_nop 0\n\t"                                             // two chains, nothing else left to do: the second wait state of both borrows
        "v_subbrev_co_u32 %[lA1], %[kA], 0, %[lA1], %[kA]\n\t"
        "v_subbrev_co_u32 %[lB1], %[kB], 0, %[lB1], %[kB]\n\t"
        "s_nop 0\n\t"                                             // the same
        "v_cndmask_b32_e64 %[mA0], 0, %[k], %[kA]\n\t"
        "v_cndmask_b32_e64 %[mB0], 0, %[k], %[kB]"
        : [lA0] "+v"(lA0), [lA1] "+v"(lA1), [mA0] "+v"(mA0), [mA1] "+v"(mA1), [hA1] "+v"(hA1),
          [lB0] "+v"(lB0), [lB1] "+v"(lB1), [mB0] "+v"(mB0), [mB1] "+v"(mB1), [hB1] "+v"(hB1), [kA] "=&s"(kA), [kB] "=&s"(kB)
        : [hA0] "v"((u32)hA), [hB0] "v"((u32)hB), [cA] "s"(cA), [cB] "s"(cB), [k] "v"(-65537) : "vcc");
    return fold96_pair{lA0, lA1, mA0, mA1, lB0, lB1, mB0, mB1};
}
// r0 = mul_tw(x0, w0), r1 = mul_tw(x1, w1): any u64 in, canonical out
__device__ __forceinline__ void mul_tw2(u64 x0, u64 w0, u64 x1, u64 w1, u64& r0, u64& r1) {
    fold96_pair F = mul_fold96_2(x0, w0, x1, w1);
    u64 tA = mk64(F.t0A, F.t1A), tB = mk64(F.t0B, F.t1B), vA, vB, kA, kB, gA, gB;
    asm(GL_FOLD2 GL_TAIL2_HEAD GL_TAIL2_M
        : [tA] "+v"(tA), [tB] "+v"(tB), [r2A] "+v"(F.r2A), [r2B] "+v"(F.r2B), [vA] "=&v"(vA), [vB] "=&v"(vB),
          [kA] "=&s"(kA), [kB] "=&s"(kB), [gA] "=&s"(gA), [gB] "=&s"(gB)
        : [bA] "v"(F.bA), [bB] "v"(F.bB), [c] "s"(65535) : "vcc");
    canon_select2(tA, vA, gA, tB, vB, gB, r0, r1);
}
// r0 = mul_tw_nc(x0, w0), r1 = mul_tw_nc(x1, w1): some u64 congruent to the products
__device__ __forceinline__ void mul_tw2_nc(u64 x0, u64 w0, u64 x1, u64 w1, u64& r0, u64& r1) {
    fold96_pair F = mul_fold96_2(x0, w0, x1, w1);
    u64 tA = mk64(F.t0A, F.t1A), tB = mk64(F.t0B, F.t1B), kA, kB;
    asm(GL_FOLD2 GL_TAIL2_HEAD GL_TAIL2_NC
        : [tA] "+v"(tA), [tB] "+v"(tB), [r2A] "+v"(F.r2A), [r2B] "+v"(F.r2B), [kA] "=&s"(kA), [kB] "=&s"(kB)
        : [bA] "v"(F.bA), [bB] "v"(F.bB), [c] "s"(65535) : "vcc");
    r0 = tA; r1 = tB;
}
// one of each: r0 = mul_tw(x0, w0) is stored, r1 = mul_tw_nc(x1, w1) only feeds products (a chain step beside the use of the factor before)
__device__ __forceinline__ void mul_tw2_m_nc(u64 x0, u64 w0, u64 x1, u64 w1, u64& r0, u64& r1) {
    fold96_pair F = mul_fold96_2(x0, w0, x1, w1);
    u64 tA = mk64(F.t0A, F.t1A), tB = mk64(F.t0B, F.t1B), vA, kA, kB, gA;
    asm(GL_FOLD2
        "v_mad_u64_u32 %[tA], %[kA], %[r2A], -1, %[tA]\n\t"
        "v_mad_u64_u32 %[tB], %[kB], %[r2B], -1, %[tB]\n\t"
        "s_nop 0\n\t"                                             // two chains: the second wait state of both carries
        "v_cndmask_b32_e64 %[r2A], 0, -1, %[kA]\n\t"
        "v_mad_u64_u32 %[tA], vcc, %[r2A], 1, %[tA]\n\t"
        "v_mad_u64_u32 %[vA], %[gA], 1, -1, %[tA]\n\t"            // gA: the two instructions below stand behind it
        "v_cndmask_b32_e64 %[r2B], 0, -1, %[kB]\n\t"
        "v_mad_u64_u32 %[tB], vcc, %[r2B], 1, %[tB]"
        : [tA] "+v"(tA), [tB] "+v"(tB), [r2A] "+v"(F.r2A), [r2B] "+v"(F.r2B), [vA] "=&v"(vA), [kA] "=&s"(kA), [kB] "=&s"(kB), [gA] "=&s"(gA)
        : [bA] "v"(F.bA), [bB] "v"(F.bB), [c] "s"(65535) : "vcc");
    u32 q0 = (u32)tA, q1 = (u32)(tA >> 32);
    asm("v_cndmask_b32_e64 %[q0], %[q0], %[v0], %[gA]\n\tv_cndmask_b32_e64 %[q1], %[q1], %[v1], %[gA]"
        : [q0] "+v"(q0), [q1] "+v"(q1) : [v0] "v"((u32)vA), [v1] "v"((u32)(vA >> 32)), [gA] "s"(gA));
    r0 = mk64(q0, q1); r1 = tB;
}

// x0 2^E0 and x1 2^E1 (mul_pow2) with the two shifts' chains alternating where both exponents fall into the same of mul_pow2's cases
// (a layer's two blocks of the same j always do); exponents of different cases, and the case 32 < E < 64, run one behind the other
template <int E0, int E1>
__device__ __forceinline__ void mul_pow2_2(u64 x0, u64 x1, u64& r0, u64& r1) {
    static_assert(E0 >= 0 && E0 < 96 && E1 >= 0 && E1 < 96, "fold 2^96 = -1 first");
    if constexpr (E0 >= 1 && E0 <= 32 && E1 >= 1 && E1 <= 32) {
        GL_OPAQUE(x0); GL_OPAQUE(x1);
        mad_eps2_m((u32)(x0 >> (64 - E0)), x0 << E0, (u32)(x1 >> (64 - E1)), x1 << E1, r0, r1);
    } else if constexpr (E0 >= 64 && E1 >= 64) {
        GL_OPAQUE(x0); GL_OPAQUE(x1);
        constexpr int ra = E0 - 64, rb = E1 - 64;
        const u32 ta = (u32)x0 << ra, tb = (u32)x1 << rb;
        sub2_m(((u64)ta << 32) - ta, ra == 0 ? (x0 >> 32) : (x0 >> (32 - ra)), ((u64)tb << 32) - tb, rb == 0 ? (x1 >> 32) : (x1 >> (32 - rb)), r0, r1);
    } else {
        r0 = mul_pow2<E0>(x0); r1 = mul_pow2<E1>(x1);
    }
}

// host-side twins (used only to build twiddle tables at context creation)
inline u64 hmul(u64 a, u64 b) {
    unsigned __int128 x = (unsigned __int128)a * b;
    return reduce128((u64)x, (u64)(x >> 64));
}
inline u64 hpow(u64 a, u64 e) {
    u64 r = 1;
    while (e) { if (e & 1) r = hmul(r, a); a = hmul(a, a); e >>= 1; }
    return r;
}
inline u64 hinv(u64 a) { return hpow(a, GL_P - 2); }
inline u64 hroot(unsigned k) {  // MG.0[k], starky/src/constant.rs:54-68
    u64 w = hpow(7, 0xFFFFFFFFULL);
    for (unsigned n = 32; n > k; --n) w = hmul(w, w);
    return w;
}

}  // namespace gl
