// Micro-benchmark: issue cost of the integer VALU instructions a Goldilocks multiplier is built
// from, on gfx950.  Prints cycles per wave-instruction per SIMD (assuming 2.4 GHz, 1024 SIMDs).
// Build: hipcc --offload-arch=gfx950 -O3 tools/ubench_valu.hip -o tools/ubench_valu
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "../eigen-zkvm_amd/csrc/gl.hip.h"   // the paired forms of round 33 (kpair)
typedef unsigned long long u64;
typedef unsigned int u32;

#define REP8(x) x x x x x x x x
#define REP64(x) REP8(REP8(x))

template <int WHICH>
__global__ __launch_bounds__(256) void k(u64* out, int iters, u32 seed) {
    u32 a0 = threadIdx.x + seed, a1 = a0 * 3 + 1, a2 = a0 * 5 + 2, a3 = a0 * 7 + 3;
    u32 b0 = a0 ^ 0x55, b1 = a1 ^ 0x77, b2 = a2 ^ 0x99, b3 = a3 ^ 0xbb;
    u64 x0 = a0, x1 = a1, x2 = a2, x3 = a3;
    u64 c0 = b0, c1 = b1, c2 = b2, c3 = b3;
    for (int i = 0; i < iters; ++i) {
        if (WHICH == 0) {  // v_add_u32 (baseline full-rate), 4 independent chains
            REP64(asm volatile("v_add_u32 %0, %0, %4\n v_add_u32 %1, %1, %5\n v_add_u32 %2, %2, %6\n v_add_u32 %3, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 1) {  // v_mad_u64_u32
            REP64(asm volatile("v_mad_u64_u32 %0, s[10:11], %4, %5, %0\n v_mad_u64_u32 %1, s[10:11], %5, %6, %1\n"
                               "v_mad_u64_u32 %2, s[10:11], %6, %7, %2\n v_mad_u64_u32 %3, s[10:11], %7, %4, %3"
                               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "s10", "s11");)
        } else if (WHICH == 2) {  // v_mul_lo_u32
            REP64(asm volatile("v_mul_lo_u32 %0, %0, %4\n v_mul_lo_u32 %1, %1, %5\n v_mul_lo_u32 %2, %2, %6\n v_mul_lo_u32 %3, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 3) {  // v_mul_hi_u32
            REP64(asm volatile("v_mul_hi_u32 %0, %0, %4\n v_mul_hi_u32 %1, %1, %5\n v_mul_hi_u32 %2, %2, %6\n v_mul_hi_u32 %3, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 4) {  // v_lshl_add_u64 (64-bit add)
            REP64(asm volatile("v_lshl_add_u64 %0, %0, 0, %4\n v_lshl_add_u64 %1, %1, 0, %5\n v_lshl_add_u64 %2, %2, 0, %6\n v_lshl_add_u64 %3, %3, 0, %7"
                               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3) : "v"(c0), "v"(c1), "v"(c2), "v"(c3));)
        } else if (WHICH == 5) {  // add_co / addc pairs through vcc, interleaved 2 chains (hazard visible?)
            REP64(asm volatile("v_add_co_u32 %0, vcc, %0, %4\n v_addc_co_u32 %1, vcc, %1, %5, vcc\n"
                               "v_add_co_u32 %2, vcc, %2, %6\n v_addc_co_u32 %3, vcc, %3, %7, vcc"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "vcc");)
        } else if (WHICH == 6) {  // v_mul_u32_u24
            REP64(asm volatile("v_mul_u32_u24 %0, %0, %4\n v_mul_u32_u24 %1, %1, %5\n v_mul_u32_u24 %2, %2, %6\n v_mul_u32_u24 %3, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 7) {  // v_cmp_lt_u64 + cndmask x2 through sgpr pair
            REP64(asm volatile("v_cmp_lt_u64 s[10:11], %0, %2\n v_cmp_lt_u64 s[12:13], %1, %3\n"
                               "v_cndmask_b32 %4, %4, %5, s[10:11]\n v_cndmask_b32 %6, %6, %7, s[12:13]"
                               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "s10", "s11", "s12", "s13");)
        } else if (WHICH == 8) {  // v_add3_u32
            REP64(asm volatile("v_add3_u32 %0, %0, %4, %5\n v_add3_u32 %1, %1, %5, %6\n v_add3_u32 %2, %2, %6, %7\n v_add3_u32 %3, %3, %7, %4"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 9) {  // v_mad_u32_u24
            REP64(asm volatile("v_mad_u32_u24 %0, %0, %4, %5\n v_mad_u32_u24 %1, %1, %5, %6\n v_mad_u32_u24 %2, %2, %6, %7\n v_mad_u32_u24 %3, %3, %7, %4"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 10) {  // v_lshlrev_b64
            REP64(asm volatile("v_lshlrev_b64 %0, 3, %0\n v_lshlrev_b64 %1, 5, %1\n v_lshlrev_b64 %2, 7, %2\n v_lshlrev_b64 %3, 9, %3"
                               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));)
        } else if (WHICH == 12) {  // add_co / addc with the 2 wait states the compiler inserts
            REP64(asm volatile("v_add_co_u32 %0, vcc, %0, %4\n s_nop 1\n v_addc_co_u32 %1, vcc, %1, %5, vcc\n"
                               "v_add_co_u32 %2, vcc, %2, %6\n s_nop 1\n v_addc_co_u32 %3, vcc, %3, %7, vcc"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "vcc");)
        } else if (WHICH == 13) {  // two carry chains interleaved through distinct sgpr pairs (1 instr gap)
            REP64(asm volatile("v_add_co_u32 %0, s[10:11], %0, %4\n v_add_co_u32 %2, s[12:13], %2, %6\n s_nop 0\n"
                               "v_addc_co_u32 %1, s[10:11], %1, %5, s[10:11]\n v_addc_co_u32 %3, s[12:13], %3, %7, s[12:13]"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "s10", "s11", "s12", "s13");)
        } else if (WHICH == 14) {
            REP64(asm volatile("v_sub_u32 %0, %0, %4\n v_sub_u32 %1, %1, %5\n v_sub_u32 %2, %2, %6\n v_sub_u32 %3, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 15) {
            REP64(asm volatile("v_and_b32 %0, %0, %4\n v_xor_b32 %1, %1, %5\n v_or_b32 %2, %2, %6\n v_xor_b32 %3, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 16) {
            REP64(asm volatile("v_lshlrev_b32 %0, 3, %0\n v_lshrrev_b32 %1, 1, %1\n v_lshlrev_b32 %2, 5, %2\n v_lshrrev_b32 %3, 2, %3"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));)
        } else if (WHICH == 17) {
            REP64(asm volatile("v_mov_b32 %0, %4\n v_mov_b32 %1, %5\n v_mov_b32 %2, %6\n v_mov_b32 %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 18) {  // cndmask e32 (vcc set once)
            asm volatile("v_cmp_lt_u32 vcc, %0, %1" :: "v"(a0), "v"(b0) : "vcc");
            REP64(asm volatile("v_cndmask_b32 %0, %0, %4, vcc\n v_cndmask_b32 %1, %1, %5, vcc\n v_cndmask_b32 %2, %2, %6, vcc\n v_cndmask_b32 %3, %3, %7, vcc"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "vcc");)
        } else if (WHICH == 19) {  // add_co e32 independent (write vcc only)
            REP64(asm volatile("v_add_co_u32 %0, vcc, %0, %4\n v_add_co_u32 %1, vcc, %1, %5\n v_add_co_u32 %2, vcc, %2, %6\n v_add_co_u32 %3, vcc, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "vcc");)
        } else if (WHICH == 20) {  // v_add_u32 forced VOP3 encoding
            REP64(asm volatile("v_add_u32_e64 %0, %0, %4\n v_add_u32_e64 %1, %1, %5\n v_add_u32_e64 %2, %2, %6\n v_add_u32_e64 %3, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 21) {  // add_co, 2 filler adds, addc (hazard-free carry chain)
            REP64(asm volatile("v_add_co_u32 %0, vcc, %0, %4\n v_add_u32 %2, %2, %6\n v_add_u32 %3, %3, %7\n v_addc_co_u32 %1, vcc, %1, %5, vcc"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "vcc");)
        } else if (WHICH == 22) {  // v_lshl_add_u32 / v_lshl_or_b32 (VOP3, 32-bit)
            REP64(asm volatile("v_lshl_add_u32 %0, %0, 1, %4\n v_lshl_or_b32 %1, %1, 1, %5\n v_lshl_add_u32 %2, %2, 1, %6\n v_lshl_or_b32 %3, %3, 1, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        } else if (WHICH == 23) {  // v_mad_u64_u32 with inline-constant multiplier (zext-add form)
            REP64(asm volatile("v_mad_u64_u32 %0, s[10:11], %4, 1, %0\n v_mad_u64_u32 %1, s[10:11], %5, 1, %1\n"
                               "v_mad_u64_u32 %2, s[10:11], %6, -1, %2\n v_mad_u64_u32 %3, s[10:11], %7, -1, %3"
                               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "s10", "s11");)
        } else if (WHICH == 24) {  // v_mov_b64
            REP64(asm volatile("v_mov_b64 %0, %4\n v_mov_b64 %1, %5\n v_mov_b64 %2, %6\n v_mov_b64 %3, %7"
                               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3) : "v"(c0), "v"(c1), "v"(c2), "v"(c3));)
        } else if (WHICH == 25) {  // v_cmp_lt_u32 e32 (vcc) independent
            REP64(asm volatile("v_cmp_lt_u32 vcc, %0, %4\n v_cmp_lt_u32 vcc, %1, %5\n v_cmp_lt_u32 vcc, %2, %6\n v_cmp_lt_u32 vcc, %3, %7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "vcc");)
        } else if (WHICH == 11) {  // v_alignbit_b32
            REP64(asm volatile("v_alignbit_b32 %0, %0, %4, 7\n v_alignbit_b32 %1, %1, %5, 7\n v_alignbit_b32 %2, %2, %6, 7\n v_alignbit_b32 %3, %3, %7, 7"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3));)
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + x0 + x1 + x2 + x3;
}

// ---- Mixed streams (issue model of the NTT butterflies): one carry-class instruction followed by K plain 32-bit ones, four independent
// groups per block.  CARRY 0: v_add_co_u32 (vcc), 1: v_lshl_add_u64.  PLAIN 0: v_cndmask_b32 on an SGPR-pair mask, 1: v_mov_b32,
// 2: v_and_b32.  The plain instructions of a group write registers of their own (no chain through them).
#define G_ADDCO(d, s) "v_add_co_u32 %" #d ", vcc, %" #d ", %" #s "\n"
#define G_ADD64(d, s) "v_lshl_add_u64 %" #d ", %" #d ", 0, %" #s "\n"
#define P_CND(d, s) "v_cndmask_b32_e64 %" #d ", %" #d ", %" #s ", %28\n"
#define P_MOV(d, s) "v_mov_b32 %" #d ", %" #s "\n"
#define P_AND(d, s) "v_and_b32 %" #d ", %" #d ", %" #s "\n"
#define P_NONE(d, s) ""
#define MIXBLK(C, c0, c1, c2, c3, s0, s1, s2, s3, PA, PB) \
    C(c0, s0) PA(8, 24) PB(12, 24) C(c1, s1) PA(9, 25) PB(13, 25) C(c2, s2) PA(10, 26) PB(14, 26) C(c3, s3) PA(11, 27) PB(15, 27)
#define MIX32(PA, PB) MIXBLK(G_ADDCO, 0, 1, 2, 3, 16, 17, 18, 19, PA, PB)
#define MIX64(PA, PB) MIXBLK(G_ADD64, 4, 5, 6, 7, 20, 21, 22, 23, PA, PB)
#define MIXRUN(STR) REP64(asm volatile(STR : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3),              \
                                       "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3), "+v"(q4), "+v"(q5), "+v"(q6), "+v"(q7)                     \
                                       : "v"(b0), "v"(b1), "v"(b2), "v"(b3), "v"(c0), "v"(c1), "v"(c2), "v"(c3), "v"(r0), "v"(r1), "v"(r2), \
                                         "v"(r3), "s"(mask) : "vcc");)
#define MIXCASE(CM, P, K, PM) if constexpr (PLAIN == P && K == 1) { MIXRUN(CM(PM, P_NONE)) } else if constexpr (PLAIN == P && K == 2) { MIXRUN(CM(PM, PM)) }
template <int CARRY, int PLAIN, int K>
__global__ __launch_bounds__(256) void kmix(u64* out, int iters, u32 seed) {
    u32 a0 = threadIdx.x + seed, a1 = a0 * 3 + 1, a2 = a0 * 5 + 2, a3 = a0 * 7 + 3;
    u32 b0 = a0 ^ 0x55, b1 = a1 ^ 0x77, b2 = a2 ^ 0x99, b3 = a3 ^ 0xbb;
    u64 x0 = a0, x1 = a1, x2 = a2, x3 = a3, c0 = b0, c1 = b1, c2 = b2, c3 = b3;
    u32 q0 = a0 + 1, q1 = a1 + 1, q2 = a2 + 1, q3 = a3 + 1, q4 = a0 + 2, q5 = a1 + 2, q6 = a2 + 2, q7 = a3 + 2;
    u32 r0 = b0 + 1, r1 = b1 + 1, r2 = b2 + 1, r3 = b3 + 1;
    u64 mask;
    asm volatile("v_cmp_lt_u32_e64 %0, %1, %2" : "=s"(mask) : "v"(a0), "v"(b1));   // an arbitrary lane mask, written once
    for (int i = 0; i < iters; ++i) {
        if constexpr (CARRY == 0) {
            if constexpr (K == 0) { MIXRUN(MIX32(P_NONE, P_NONE)) }
            else MIXCASE(MIX32, 0, K, P_CND) else MIXCASE(MIX32, 1, K, P_MOV) else MIXCASE(MIX32, 2, K, P_AND)
        } else {
            if constexpr (K == 0) { MIXRUN(MIX64(P_NONE, P_NONE)) }
            else MIXCASE(MIX64, 0, K, P_CND) else MIXCASE(MIX64, 1, K, P_MOV) else MIXCASE(MIX64, 2, K, P_AND)
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + x0 + x1 + x2 + x3 + q0 + q1 + q2 + q3 + q4 + q5 + q6 + q7;
}

// ---- v_cndmask_b32 alone.  MODE 0: VOP3 form, the mask an SGPR pair written once; 1: VOP2 form on vcc, vcc written by a compare at
// the head of every block of four (the two wait states the hardware asks for between them as an s_nop 1).
template <int MODE>
__global__ __launch_bounds__(256) void kcnd(u64* out, int iters, u32 seed) {
    u32 a0 = threadIdx.x + seed, a1 = a0 * 3 + 1, a2 = a0 * 5 + 2, a3 = a0 * 7 + 3;
    u32 b0 = a0 ^ 0x55, b1 = a1 ^ 0x77, b2 = a2 ^ 0x99, b3 = a3 ^ 0xbb;
    u64 mask;
    asm volatile("v_cmp_lt_u32_e64 %0, %1, %2" : "=s"(mask) : "v"(a0), "v"(b1));
    for (int i = 0; i < iters; ++i) {
        if constexpr (MODE == 0) {
            REP64(asm volatile("v_cndmask_b32_e64 %0, %0, %4, %8\n v_cndmask_b32_e64 %1, %1, %5, %8\n v_cndmask_b32_e64 %2, %2, %6, %8\n v_cndmask_b32_e64 %3, %3, %7, %8"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3), "s"(mask));)
        } else {
            REP64(asm volatile("v_cmp_lt_u32 vcc, %4, %5\n s_nop 1\n"
                               "v_cndmask_b32 %0, %0, %4, vcc\n v_cndmask_b32 %1, %1, %5, vcc\n v_cndmask_b32 %2, %2, %6, vcc\n v_cndmask_b32 %3, %3, %7, vcc"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "vcc");)
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3;
}

// ---- The two forms of the Goldilocks subtraction a <- a - b mod p, back to back, two chains (v[40:45], v[46:51]) alternating.  The
// registers are named outright so that the halves of a 64-bit pair can be addressed; the wait states are the ones the compiler inserts.
// FORM 0: sub, subb, mask from the borrow, sub, subb (five carry-class).  FORM 1: sub, subb, one 64-bit add of p, two selects on the
// borrow (three carry-class, two plain).  FORM 2 (gl::sub_m): sub, subb, m = borrow ? -65537 : 0, one v_mad_i64_i32 a += m * 65535.
#define SUB_OLD(a0, a1, b0, b1, m) \
    "v_sub_co_u32 " a0 ", vcc, " a0 ", " b0 "\n s_nop 1\n v_subb_co_u32 " a1 ", vcc, " a1 ", " b1 ", vcc\n s_nop 1\n" \
    "v_cndmask_b32_e64 " m ", 0, -1, vcc\n v_sub_co_u32 " a0 ", vcc, " a0 ", " m "\n s_nop 1\n v_subbrev_co_u32 " a1 ", vcc, 0, " a1 ", vcc\n"
#define SUB_NEW(a0, a1, a01, b0, b1, e0, e1, e01) \
    "v_sub_co_u32 " a0 ", vcc, " a0 ", " b0 "\n s_nop 1\n v_subb_co_u32 " a1 ", vcc, " a1 ", " b1 ", vcc\n" \
    "v_lshl_add_u64 " e01 ", " a01 ", 0, %0\n s_nop 0\n v_cndmask_b32 " a1 ", " a1 ", " e1 ", vcc\n v_cndmask_b32 " a0 ", " a0 ", " e0 ", vcc\n"
#define SUB_MAD(a0, a1, a01, b0, b1, m) \
    "v_sub_co_u32 " a0 ", vcc, " a0 ", " b0 "\n s_nop 1\n v_subb_co_u32 " a1 ", vcc, " a1 ", " b1 ", vcc\n s_nop 1\n" \
    "v_cndmask_b32_e64 " m ", 0, %1, vcc\n v_mad_i64_i32 " a01 ", s[12:13], " m ", %2, " a01 "\n"
#define SUB_CLOBBERS "vcc", "s12", "s13", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51"
template <int FORM>
__global__ __launch_bounds__(256) void ksub(u64* out, int iters, u32 seed) {
    const u64 p = 0xFFFFFFFF00000001ull;
    const u32 t = threadIdx.x + seed;
    u32 lo, hi;
    asm volatile("v_mov_b32 v40, %0\n v_lshlrev_b32 v41, 7, %0\n v_mul_u32_u24 v42, %0, 11\n v_lshlrev_b32 v43, 9, %0\n v_mov_b32 v44, 0\n v_mov_b32 v45, 0\n"
                 "v_add_u32 v46, 5, %0\n v_lshlrev_b32 v47, 6, %0\n v_mul_u32_u24 v48, %0, 13\n v_lshlrev_b32 v49, 8, %0\n v_mov_b32 v50, 0\n v_mov_b32 v51, 0"
                 : : "v"(t) : SUB_CLOBBERS);
    for (int i = 0; i < iters; ++i) {
        if constexpr (FORM == 0) {
            REP64(asm volatile(SUB_OLD("v40", "v41", "v42", "v43", "v44") SUB_OLD("v46", "v47", "v48", "v49", "v50") : : "s"(p) : SUB_CLOBBERS);)
        } else if constexpr (FORM == 2) {
            REP64(asm volatile(SUB_MAD("v40", "v41", "v[40:41]", "v42", "v43", "v44") SUB_MAD("v46", "v47", "v[46:47]", "v48", "v49", "v50")
                               : : "s"(p), "v"(-65537), "s"(65535) : SUB_CLOBBERS);)
        } else {
            REP64(asm volatile(SUB_NEW("v40", "v41", "v[40:41]", "v42", "v43", "v44", "v45", "v[44:45]")
                               SUB_NEW("v46", "v47", "v[46:47]", "v48", "v49", "v50", "v51", "v[50:51]") : : "s"(p) : SUB_CLOBBERS);)
        }
    }
    asm volatile("v_xor_b32 %0, v40, v46\n v_xor_b32 %1, v41, v47" : "=v"(lo), "=v"(hi) : : SUB_CLOBBERS);
    out[blockIdx.x * blockDim.x + threadIdx.x] = ((u64)hi << 32) | lo;
}

// The paired forms of csrc/gl.hip.h against their single forms called back to back (round 33): two butterflies or two twiddle products on
// independent operands per step, 16 steps per iteration.  MODE 0: add_m, sub_m twice; 1: bfly_m twice; 2: bfly2_m; 3: mul_tw twice; 4: mul_tw2
template <int MODE>
__global__ __launch_bounds__(256) void kpair(u64* out, int iters, u32 seed) {
    const u64 p = 0xFFFFFFFF00000001ull;
    u64 a = (threadIdx.x + seed) * 0x9E3779B97F4A7C15ull % p, b = (a * 31 + 7) % p, c = (a * 131 + 5) % p, d = (b * 17 + 3) % p;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            u64 s0, d0, s1, d1;
            if constexpr (MODE == 0) { s0 = gl::add_m(a, b); d0 = gl::sub_m(a, b); s1 = gl::add_m(c, d); d1 = gl::sub_m(c, d); }
            else if constexpr (MODE == 1) { gl::bfly_m(a, b, s0, d0); gl::bfly_m(c, d, s1, d1); }
            else if constexpr (MODE == 2) gl::bfly2_m(a, b, c, d, s0, d0, s1, d1);
            else if constexpr (MODE == 3) { s0 = gl::mul_tw(a, b); s1 = gl::mul_tw(c, d); d0 = b; d1 = d; }
            else { gl::mul_tw2(a, b, c, d, s0, s1); d0 = b; d1 = d; }
            a = s0; b = d1; c = s1; d = d0;
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a ^ b ^ c ^ d;
}
// cycles of a SIMD per operation of one wave (a butterfly, a product): 32 of them per iteration
template <class Kern>
void run_ops(const char* name, Kern kern, u64* d, int waves_per_simd) {
    const int iters = 2000;
    dim3 grid(256 * waves_per_simd), block(256);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, grid, block, 0, 0, d, iters, 1u);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(kern, grid, block, 0, 0, d, iters, 1u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%-36s waves/SIMD=%d  %.3f ms  -> %.2f cycles per operation (at 2.4 GHz)\n", name, waves_per_simd, ms,
           ms * 1e-3 * 2.4e9 / ((double)iters * 32 * waves_per_simd));
}

template <int W>
void run(const char* name, u64* d, int waves_per_simd) {
    const int iters = 3000;
    dim3 grid(256 * waves_per_simd), block(256);  // 256-thread blocks: 1 wave per SIMD per block
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<W>, grid, block, 0, 0, d, 3000, 1u);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<W>, grid, block, 0, 0, d, iters, 1u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    double winst = (double)iters * 64 * 4 * waves_per_simd;  // wave-instructions per SIMD
    double cycles = ms * 1e-3 * 2.4e9;
    printf("%-28s waves/SIMD=%d  %.3f ms  -> %.2f cycles per wave-instruction per SIMD (at 2.4 GHz)\n", name, waves_per_simd, ms, cycles / winst);
}

// a kernel whose block of `insts` instructions holds `groups` units of interest (a carry-class instruction with its plain followers, one
// subtraction): cycles per instruction and per group
template <class Kern>
void run_blk(const char* name, Kern kern, u64* d, int waves_per_simd, int insts, int groups) {
    const int iters = 3000;
    dim3 grid(256 * waves_per_simd), block(256);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, grid, block, 0, 0, d, iters, 1u);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(kern, grid, block, 0, 0, d, iters, 1u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double blocks = (double)iters * 64 * waves_per_simd, cycles = ms * 1e-3 * 2.4e9;
    printf("%-36s waves/SIMD=%d  %.3f ms  -> %.2f cycles per wave-instruction, %.2f per group (at 2.4 GHz)\n", name, waves_per_simd, ms,
           cycles / (blocks * insts), cycles / (blocks * groups));
}

int main() {
    u64* d; hipMalloc(&d, 256 * 8 * 256 * sizeof(u64));
    if (getenv("UBENCH_PAIRS")) {   // the paired forms alone (tools/ubench_valu_pairs.txt)
        for (int w : {1, 2, 4, 5}) {
            run_ops("butterfly: add_m, sub_m", kpair<0>, d, w);
            run_ops("butterfly: bfly_m", kpair<1>, d, w);
            run_ops("butterfly: bfly2_m", kpair<2>, d, w);
            run_ops("product: mul_tw", kpair<3>, d, w);
            run_ops("product: mul_tw2", kpair<4>, d, w);
        }
        return 0;
    }
    for (int w : {8}) {
        run<0>("v_add_u32", d, w);
        run<1>("v_mad_u64_u32", d, w);
        run<2>("v_mul_lo_u32", d, w);
        run<3>("v_mul_hi_u32", d, w);
        run<4>("v_lshl_add_u64", d, w);
        run<5>("v_add_co+v_addc (vcc)", d, w);
        run<6>("v_mul_u32_u24", d, w);
        run<7>("v_cmp_lt_u64+cndmask", d, w);
        run<8>("v_add3_u32", d, w);
        run<9>("v_mad_u32_u24", d, w);
        run<10>("v_lshlrev_b64", d, w);
        run<11>("v_alignbit_b32", d, w);
        run<12>("add_co+s_nop1+addc", d, w);
        run<13>("2 chains sgpr carry", d, w);
        run<14>("v_sub_u32", d, w);
        run<15>("v_and/xor/or_b32", d, w);
        run<16>("v_lshl/lshr_b32", d, w);
        run<17>("v_mov_b32", d, w);
        run<18>("v_cndmask_b32 e32 vcc", d, w);
        run<19>("v_add_co_u32 e32 indep", d, w);
        run<20>("v_add_u32_e64", d, w);
        run<21>("add_co,2 fill,addc", d, w);
        run<22>("v_lshl_add_u32/lshl_or", d, w);
        run<23>("v_mad_u64_u32 x*1/-1+acc", d, w);
        run<24>("v_mov_b64", d, w);
        run<25>("v_cmp_lt_u32 e32", d, w);
    }
    // mixed streams: group = one carry-class instruction + k plain ones
    for (int w : {5, 8}) {
        run_blk("add_co", kmix<0, 0, 0>, d, w, 4, 4);
        run_blk("add_co + 1 cndmask(sgpr)", kmix<0, 0, 1>, d, w, 8, 4);
        run_blk("add_co + 2 cndmask(sgpr)", kmix<0, 0, 2>, d, w, 12, 4);
        run_blk("add_co + 1 mov", kmix<0, 1, 1>, d, w, 8, 4);
        run_blk("add_co + 2 mov", kmix<0, 1, 2>, d, w, 12, 4);
        run_blk("add_co + 1 and", kmix<0, 2, 1>, d, w, 8, 4);
        run_blk("add_co + 2 and", kmix<0, 2, 2>, d, w, 12, 4);
        run_blk("lshl_add_u64", kmix<1, 0, 0>, d, w, 4, 4);
        run_blk("lshl_add_u64 + 1 cndmask(sgpr)", kmix<1, 0, 1>, d, w, 8, 4);
        run_blk("lshl_add_u64 + 2 cndmask(sgpr)", kmix<1, 0, 2>, d, w, 12, 4);
        run_blk("lshl_add_u64 + 1 mov", kmix<1, 1, 1>, d, w, 8, 4);
        run_blk("lshl_add_u64 + 2 mov", kmix<1, 1, 2>, d, w, 12, 4);
        run_blk("lshl_add_u64 + 1 and", kmix<1, 2, 1>, d, w, 8, 4);
        run_blk("lshl_add_u64 + 2 and", kmix<1, 2, 2>, d, w, 12, 4);
        run_blk("v_cndmask_b32 e64, sgpr-pair mask", kcnd<0>, d, w, 4, 4);
        run_blk("v_cmp (vcc) + 4 v_cndmask_b32 e32", kcnd<1>, d, w, 5, 1);
        run_blk("gl::sub, five carry-class", ksub<0>, d, w, 10, 2);
        run_blk("gl::sub, three carry-class + two", ksub<1>, d, w, 10, 2);
        run_blk("gl::sub_m, sub, subb, cnd, mad_i64", ksub<2>, d, w, 8, 2);
    }
    return 0;
}
