// The endomorphism split of a G1 scalar: phi(x, y) = (beta x, y) = [lambda](x, y), and k = k1 + k2 lambda (mod r) with |k1|, |k2| < 2^128.
// Used by the sums (msm_impl.hip.h glv_split_kernel: n points with 254-bit scalars become 2n with 128-bit ones) and by the per-point
// scalar product (ecntt_impl.hip.h ecn_mul_scalars_glv_kernel: one joint walk over the two halves).  Included inside a curve's G1
// namespace after ecpt_impl.hip.h, with GLV_CURVE_BN254 or GLV_CURVE_BLS12_381 defined; no include guard on purpose.  The constants are
// this header's own: it defines them, uses them and takes them away again.  tools/glv_constants.py derives and checks them.
#if defined(GLV_CURVE_BN254)
// y^2 = x^3 + 3: beta = 2203960485148121921418603742825762020974279258880205651966 (beta^3 = 1 in Fq), lambda =
// 4407920970296243842393367215006156084916469457145843978461; lattice basis a1 = b2 = 9931322734385697763,
// -b1 = 147946756881789319000765030803803410728, a2 = 147946756881789319010696353538189108491
#define GLV_BETA_STD 0xd782e155u, 0x71930c11u, 0xffbe3323u, 0xa6bb947cu, 0xd4741444u, 0xaa303344u, 0x26594943u, 0x2c3b3f0du
#define GLV_G1 0xc7e0b3d7u, 0xd91d232eu, 0x00000002u
#define GLV_G2 0x391eb18du, 0x7a7bd9d4u, 0xa773d2cfu, 0x4ccef014u, 0x00000002u
#define GLV_A1 0x94d213e3u, 0x89d32568u
#define GLV_A2 0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u
#define GLV_NB1 0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u
#define GLV_B2 0x94d213e3u, 0x89d32568u
#elif defined(GLV_CURVE_BLS12_381)
// y^2 = x^3 + 4 with lambda = z^2 - 1 = 0xac45a4010001a40200000000ffffffff (z the curve parameter): lambda^2 + lambda + 1 = 0 mod r, so
// k = k1 + k2 lambda by division; beta =
// 4002409555221667392624310435006688643935503118305586438271171395842971157480381377015405980053539358417135540939436
#define GLV_BETA_STD 0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u
#define GLV_LAMBDA 0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u
#define GLV_G 0xf6cfee30u, 0x63f6e522u, 0xe01faaddu, 0x7c6becf1u, 0x00000001u
#define GLV_R 0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u
#else
#error "glv_split.hip.h: define GLV_CURVE_BN254 or GLV_CURVE_BLS12_381"
#endif

__device__ __forceinline__ cf glv_beta() { const u32 BETA[NL] = {GLV_BETA_STD}; return cf_from_std(BETA); }   // beta in the internal form

template <int NA, int NB, int NO>
__device__ __forceinline__ void glv_mul(const u32 (&a)[NA], const u32 (&b)[NB], u32 (&out)[NO], int from) {   // words [from, from + NO) of a * b
    u64 acc = 0;
    u32 carry_hi = 0;
    for (int k = 0; k < from + NO; ++k) {       // column k; (acc, carry_hi) is a 96-bit running sum
        for (int i = 0; i < NA; ++i) {
            const int j = k - i;
            if (j < 0 || j >= NB) continue;
            const u64 p = (u64)a[i] * b[j];
            acc += p;
            carry_hi += acc < p;
        }
        if (k >= from) out[k - from] = (u32)acc;
        acc = (acc >> 32) | ((u64)carry_hi << 32);
        carry_hi = 0;
    }
}
// k (8 words; brought below r where the split needs it) -> |k1|, |k2| (the low 4 words hold them) and their signs: k = +-|k1| +- |k2| lambda
__device__ __forceinline__ void glv_split(u32 (&k)[8], u32 (&k1)[8], u32 (&k2)[8], bool& n1, bool& n2) {
    n1 = false; n2 = false;
#ifdef GLV_LAMBDA
    // lambda^2 + lambda + 1 = 0 (mod r) with lambda < 2^128: k = k1 + k2 lambda by plain division, both halves non-negative.  A scalar
    // is brought below r first (k2 <= lambda + 1 needs it); the quotient from the reciprocal g = floor(2^256 / lambda) is at most
    // one short, made up by one conditional step
    const u32 LAMBDA[4] = {GLV_LAMBDA}, GG[5] = {GLV_G}, RMOD[8] = {GLV_R};
    for (int rep = 0; rep < 2; ++rep) {
        u32 t[8]; u64 br = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const u64 d = (u64)k[j] - RMOD[j] - br; t[j] = (u32)d; br = (d >> 32) & 1; }
        if (!br) { for (int j = 0; j < 8; ++j) k[j] = t[j]; }
    }
    u32 c[5], t8[8];
    glv_mul<8, 5, 5>(k, GG, c, 8);
    glv_mul<5, 4, 8>(c, LAMBDA, t8, 0);
    u64 br = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const u64 d = (u64)k[j] - t8[j] - br; k1[j] = (u32)d; br = (d >> 32) & 1; }
#pragma unroll
    for (int j = 0; j < 8; ++j) k2[j] = j < 5 ? c[j] : 0;
    {   // k1 >= lambda: one more lambda goes to k2
        u32 t[8]; u64 b2 = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const u64 d = (u64)k1[j] - (j < 4 ? LAMBDA[j] : 0u) - b2; t[j] = (u32)d; b2 = (d >> 32) & 1; }
        if (!b2) {
            for (int j = 0; j < 8; ++j) k1[j] = t[j];
            u64 cy = 1;
            for (int j = 0; j < 8; ++j) { cy += k2[j]; k2[j] = (u32)cy; cy >>= 32; }
        }
    }
#else
    // (k1, k2) = k - c1 (a1, b1) - c2 (a2, b2) with c1 = floor(k g1 / 2^256), c2 = floor(k g2 / 2^256), g1 = floor(2^256 b2 / r),
    // g2 = floor(-2^256 b1 / r) for the short basis (a1, b1), (a2, b2) of {(x, y): x + y lambda = 0 mod r}; any integers c1, c2 give
    // a correct split, these keep both halves below 2^128 (checked over the edge scalars and 2 * 10^5 random ones when the constants
    // were derived)
    const u32 G1[3] = {GLV_G1}, G2[5] = {GLV_G2}, A1[2] = {GLV_A1}, A2[4] = {GLV_A2}, NB1[4] = {GLV_NB1}, B2[2] = {GLV_B2};
    u32 c1[3], c2[5];
    glv_mul<8, 3, 3>(k, G1, c1, 8);
    glv_mul<8, 5, 5>(k, G2, c2, 8);
    u32 t1[8], t2[8];
    glv_mul<3, 2, 8>(c1, A1, t1, 0); glv_mul<5, 4, 8>(c2, A2, t2, 0);          // k1 = k - c1 a1 - c2 a2  (mod 2^256, two's complement)
    u64 br = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const u64 d = (u64)k[j] - t1[j] - t2[j] - br; k1[j] = (u32)d; br = (0 - (d >> 32)) & 3; }
    glv_mul<3, 4, 8>(c1, NB1, t1, 0); glv_mul<5, 2, 8>(c2, B2, t2, 0);         // k2 = c1 |b1| - c2 b2
    br = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const u64 d = (u64)t1[j] - t2[j] - br; k2[j] = (u32)d; br = (0 - (d >> 32)) & 1; }
    n1 = k1[7] >> 31; n2 = k2[7] >> 31;
    if (n1) { u64 c = 1; for (int j = 0; j < 8; ++j) { c += (u32)~k1[j]; k1[j] = (u32)c; c >>= 32; } }
    if (n2) { u64 c = 1; for (int j = 0; j < 8; ++j) { c += (u32)~k2[j]; k2[j] = (u32)c; c >>= 32; } }
#endif
}
#undef GLV_BETA_STD
#ifdef GLV_LAMBDA
#undef GLV_LAMBDA
#undef GLV_G
#undef GLV_R
#else
#undef GLV_G1
#undef GLV_G2
#undef GLV_A1
#undef GLV_A2
#undef GLV_NB1
#undef GLV_B2
#endif
