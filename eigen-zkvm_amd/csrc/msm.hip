// Multi-scalar multiplication (Pippenger bucket method) on G1 and G2 of BN254 and BLS12-381 for gfx950.
//
// Stands behind groth16/src/groth16.rs:88-96 (Groth16::prove -> bellman_ce::create_random_proof ->
// multiexp; the arithmetic itself is third-party).  Data layout = bellman's / pairing_ce's:
// bases n x 64 B (BN254 G1) affine (x, y), Fq in Montgomery form (R = 2^256), little-endian limbs; scalars
// n x 32 B canonical little-endian; result affine + infinity flag.  96 B points for BLS12-381, twice that for G2.
//
// Pipeline (msm_impl.hip.h; all on the device, one stream):
//   0. bases: external 32-bit-limb Montgomery form -> internal 29-bit limbs (one product per coordinate)
//   1. bucket sort of the 16 n (point, window) pairs by key = window * 2^16 + digit (c = 16): two LDS-histogram
//      partition passes, no device-scope atomics
//   2. bucket ids ordered by decreasing size (counting sort), so that the lanes of a wave finish together
//   3. bucket accumulation: one lane per bucket, XYZZ += affine (8M + 2S per point), points gathered by index
//   4. per-window reduction sum_k k*B_k: radix-16 hierarchy of (S, A) block summaries, 4 levels,
//      2^16 .. 2^4 lanes; the serial chain per lane is 47 point additions
//   5. Horner over the windows + conversion to affine (one lane)
// Field: 29-bit limbs with 64-bit column accumulators, lazily reduced (fe29_impl.hip.h); Fq2 on top of it for G2.
// Integer-ALU bound (about 10 Fq products per point and window); HBM traffic is 96 B per point.
#include "curve.h"
#include "curve_consts.hip.h"
#include <map>
#include <mutex>

// fe29_impl.hip.h: the sums keep squaring as fe_mul(a, a).  The dedicated squaring of the scalar-field hashes was measured here
// (tools/gpu_sqr_ab.sh, profiles/r05/sqr_ab_raw.txt): G1 +-1 %, BN254 G2 3 % slower -- the accumulation kernels sit at a register edge.
#define ZK_FE_SQR_PLAIN 1

namespace zk {

namespace bn254 {
namespace g1 {
__host__ __device__ constexpr u32 GEN_X(int i) {  // G = (1, 2), external Montgomery form: R mod q
    constexpr u32 r[8] = {0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, 0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};
    return r[i];
}
__host__ __device__ constexpr u32 GEN_Y(int i) {  // 2R mod q
    constexpr u32 y[8] = {0x8b1e1b3au, 0xa6ba871bu, 0xeb8e167bu, 0x14f1d651u, 0xf0f28c58u, 0xccdd46deu, 0x340fbe5eu, 0x1c14ef83u};
    return y[i];
}
}  // namespace g1
namespace g1half {   // the same group with 128-bit scalars (8 windows, 4 words apart): the sum behind the endomorphism split of g1
using g1::GEN_X; using g1::GEN_Y;
#define MSM_N_WIN 8
#define MSM_SC_WORDS 4
namespace {
#include "msm_impl.hip.h"
}
}  // namespace g1half
namespace g1 {
// the endomorphism split: constants and derivation in glv_split.hip.h
#define GLV_CURVE_BN254
#define MSM_GLV g1half
namespace {
#include "msm_impl.hip.h"
}
#undef MSM_GLV
#undef GLV_CURVE_BN254
}  // namespace g1
namespace g2 {   // the twist y^2 = x^3 + 3/(9 + u) over Fq2 = Fq[u]/(u^2 + 1); generator of EIP-197, x = c0 + c1 u
__host__ __device__ constexpr u32 GEN_X(int i) {
    constexpr u32 v[16] = {0x02bc2026u, 0x8e83b5d1u, 0x497b0172u, 0xdceb1935u, 0x97811adfu, 0xfbb82647u, 0xaf96503bu, 0x19573841u,
                           0xa84c6140u, 0xafb4737du, 0x5802d8c4u, 0x6043dd5au, 0x52a02f86u, 0x09e950fcu, 0x3aea7b6bu, 0x14fef083u};
    return v[i];
}
__host__ __device__ constexpr u32 GEN_Y(int i) {
    constexpr u32 v[16] = {0x886be9f6u, 0x619dfa9du, 0xf59e9b78u, 0xfe7fd297u, 0x231b7dfeu, 0xff9e1a62u, 0xae9e4206u, 0x28fd7eebu,
                           0xc71856eeu, 0x64095b56u, 0x327d3cbbu, 0xdc57f922u, 0x33351076u, 0x55f935beu, 0x93fd6482u, 0x0da4a0e6u};
    return v[i];
}
// Code-size hazard: with everything inlined, as for G1, a G2 point addition built from six-product Fq2 multiplications
// was > 128 KB of code, beyond the reach of s_branch, and kernels of that size built by hipcc (ROCm 7.2) did not
// terminate on the device (seen twice: 12 x 32-bit limbs inlined for BLS12-381 G1, and this).  With the two-reduction
// Fq2 product (fe_mul2) a BN254 addition is ~70 KB: the Fq2 products are inlined into the point formulas, the hot
// mixed addition into the accumulate kernel, and the cold formulas (pt_add, pt_dbl, pt_dbl_aff) stay real functions.
// BLS12-381 (14 limbs, 2.4 x the code) keeps cf_mul / cf_sqr as functions.
#define MSM_G2_INLINE_CF   // 9 x 29-bit limbs: the Fq2 products are small enough to inline; the rare point formulas stay out of line
#define MSM_G2
namespace {
#include "msm_impl.hip.h"
}
#undef MSM_G2_INLINE_CF
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
#undef MSM_G2
#undef FQ_MUL_ATTR
}  // namespace g2
}  // namespace bn254

namespace bls12_381 {
namespace g1 {
// the G1 generator of the BLS12-381 specification, external Montgomery form (R = 2^384)
__host__ __device__ constexpr u32 GEN_X(int i) {
    constexpr u32 x[12] = {0xfd530c16u, 0x5cb38790u, 0x9976fff5u, 0x7817fc67u, 0x143ba1c1u, 0x154f95c7u,
                           0xf3d0e747u, 0xf0ae6acdu, 0x21dbf440u, 0xedce6eccu, 0x9e0bfb75u, 0x12017741u};
    return x[i];
}
__host__ __device__ constexpr u32 GEN_Y(int i) {
    constexpr u32 y[12] = {0x0ce72271u, 0xbaac93d5u, 0x7918fd8eu, 0x8c22631au, 0x570725ceu, 0xdd595f13u,
                           0x50405194u, 0x51ac5829u, 0xad0059c0u, 0x0e1c8c3fu, 0x5008a26au, 0x0bbc3efcu};
    return y[i];
}
}  // namespace g1
namespace g1half {   // 128-bit scalars, 8 windows: the sum behind the endomorphism split of g1
using g1::GEN_X; using g1::GEN_Y;
#define MSM_N_WIN 8
#define MSM_SC_WORDS 4
namespace {
#include "msm_impl.hip.h"
}
}  // namespace g1half
namespace g1 {
#define GLV_CURVE_BLS12_381
#define MSM_GLV g1half
namespace {
#include "msm_impl.hip.h"
}
#undef MSM_GLV
#undef GLV_CURVE_BLS12_381
}  // namespace g1
namespace g2 {   // the twist y^2 = x^3 + 4(1 + u) over Fq2 = Fq[u]/(u^2 + 1); G2 generator of the BLS12-381 specification
__host__ __device__ constexpr u32 GEN_X(int i) {
    constexpr u32 v[24] = {0x02940a10u, 0xf5f28fa2u, 0x87b4961au, 0xb3f5fb26u, 0x3e2ae580u, 0xa1a893b5u, 0x1a3caee9u, 0x9894999du, 0x1863366bu, 0x6f67b763u, 0x4350bcd7u, 0x05819192u,
                           0x9e23f606u, 0xa5a9c075u, 0xbccd60c3u, 0xaaa0c59du, 0xe2867806u, 0x3bb17e18u, 0x8541b367u, 0x1b1ab6ccu, 0xf2158547u, 0xc2b6ed0eu, 0x7360edf3u, 0x11922a09u};
    return v[i];
}
__host__ __device__ constexpr u32 GEN_Y(int i) {
    constexpr u32 v[24] = {0x60494c4au, 0x4c730af8u, 0x5e369c5au, 0x597cfa1fu, 0xaa0a635au, 0xe7e6856cu, 0x6e0d495fu, 0xbbefb5e9u, 0xf0ef25a2u, 0x07d3a975u, 0x7e80dae5u, 0x0083fd8eu,
                           0xdf64b05du, 0xadc0fc92u, 0x2b1461dcu, 0x18aa270au, 0x3be4eba0u, 0x86adac6au, 0xc93da33au, 0x79495c4eu, 0xa43ccaedu, 0xe7175850u, 0x63de1bf2u, 0x0b2bc2a1u};
    return v[i];
}
// Code-size hazard: with everything inlined, as for G1, a G2 point addition built from six-product Fq2 multiplications
// was > 128 KB of code, beyond the reach of s_branch, and kernels of that size built by hipcc (ROCm 7.2) did not
// terminate on the device (seen twice: 12 x 32-bit limbs inlined for BLS12-381 G1, and this).  With the two-reduction
// Fq2 product (fe_mul2) a BN254 addition is ~70 KB: the Fq2 products are inlined into the point formulas, the hot
// mixed addition into the accumulate kernel, and the cold formulas (pt_add, pt_dbl, pt_dbl_aff) stay real functions.
// BLS12-381 (14 limbs, 2.4 x the code) keeps cf_mul / cf_sqr as functions.
#define MSM_G2
namespace {
#include "msm_impl.hip.h"
}
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
#undef MSM_G2
#undef FQ_MUL_ATTR
}  // namespace g2
}  // namespace bls12_381

// the table's slice of this unit (curve.h)
#define ZK_GROUP_OPS(NS) {NS::msm_g1_dev, NS::g1_mul_generator_dev, NS::mul_generator_fr_dev, NS::msm_fixed_table_bytes, NS::msm_fixed_prepare_dev, NS::msm_fixed_dev, NS::generator_words}
const MsmOps& msm_ops(CurveId id) {
    static const MsmOps OPS[2] = {
        {{ZK_GROUP_OPS(bn254::g1), ZK_GROUP_OPS(bn254::g2)}, bn254::g1::fq_canon_to_mont_dev, bn254::g1::fq_mont_to_canon_dev},
        {{ZK_GROUP_OPS(bls12_381::g1), ZK_GROUP_OPS(bls12_381::g2)}, bls12_381::g1::fq_canon_to_mont_dev, bls12_381::g1::fq_mont_to_canon_dev},
    };
    return OPS[id];
}
#undef ZK_GROUP_OPS

}  // namespace zk
