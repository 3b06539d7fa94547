// Transforms, column sums and scalar products over curve points (ecntt_impl.hip.h) for G1 and G2 of BN254 and BLS12-381 on gfx950,
// instantiated as msm.hip instantiates the point formulas: squaring as fe_mul(a, a), BN254's Fq2 products inlined, BLS12-381's kept as
// functions, and the unit compiled with msm.o's flags (Makefile) so that the out-of-line point formulas get a 64-lane workgroup's
// register budget.  The twiddles are made on the host (fr_host.h): n / 2 products in Fr, next to n / 2 log n scalar products in the group.
#include "curve.h"
#include "curve_consts.hip.h"
#include "fr_host.h"

#define ZK_FE_SQR_PLAIN 1

namespace zk {
namespace bn254 {
namespace ecntt_g1 {
#define GLV_CURVE_BN254             // G1 has the endomorphism split (glv_split.hip.h): the per-point product through it
namespace {
#include "ecpt_impl.hip.h"
#include "ecntt_impl.hip.h"
}
#undef GLV_CURVE_BN254
}  // namespace ecntt_g1
namespace ecntt_g2 {
#define MSM_G2_INLINE_CF
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "ecntt_impl.hip.h"
}
#undef MSM_G2_INLINE_CF
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
#undef MSM_G2
#undef FQ_MUL_ATTR
}  // namespace ecntt_g2
}  // namespace bn254
namespace bls12_381 {
namespace ecntt_g1 {
#define GLV_CURVE_BLS12_381
namespace {
#include "ecpt_impl.hip.h"
#include "ecntt_impl.hip.h"
}
#undef GLV_CURVE_BLS12_381
}  // namespace ecntt_g1
namespace ecntt_g2 {
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "ecntt_impl.hip.h"
}
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
#undef MSM_G2
#undef FQ_MUL_ATTR
}  // namespace ecntt_g2
}  // namespace bls12_381

// the table's slice of this unit (curve.h)
#define ZK_EC_OPS(NS) {NS::ntt_run, NS::mul_scalar_run, NS::mul_scalars_run, NS::mul_scalars_glv_run, NS::diff_run, NS::column_sums_run}
const EcOps& ec_ops(CurveId id) {
    static const EcOps OPS[2] = {{{ZK_EC_OPS(bn254::ecntt_g1), ZK_EC_OPS(bn254::ecntt_g2)}}, {{ZK_EC_OPS(bls12_381::ecntt_g1), ZK_EC_OPS(bls12_381::ecntt_g2)}}};
    return OPS[id];
}
#undef ZK_EC_OPS

// bellman's EvaluationDomain::{fft, ifft} with group elements: the omega of zk_fr_<curve>_ntt, natural order in and out, 1 / n in the inverse
void group_ntt_dev(const Curve& cv, Group g, void* d_points, int logn, bool inverse, hipStream_t st) {
    const FrHost F(cv);
    ZK_REQUIRE(logn >= 0 && logn <= F.two_adicity() && logn <= 26, "group transform: log_n out of range");
    ZK_REQUIRE(d_points, "group transform: null points");
    if (logn == 0) return;                                          // one point: the identity, forward and inverse
    const u64 half = 1ull << (logn - 1);
    std::vector<u64> tw((half + 1) * 4);                            // the n / 2 twiddles, then 1 / n; canonical
    u64 w[4], cur[4];
    F.omega(logn, w);
    if (inverse) F.inv(w, w);
    std::memcpy(cur, F.one, 32);
    for (u64 k = 0; k < half; ++k) { F.from_mont(cur, &tw[4 * k]); F.mul(cur, w, cur); }
    if (inverse) {
        u64 nn[4] = {1ull << logn, 0, 0, 0}, t[4];
        F.to_mont(nn, t); F.inv(t, t); F.from_mont(t, &tw[4 * half]);
    }
    DevBuf d_tw; d_tw.reserve(tw.size() * 8);
    h2d_sync(d_tw.p, tw.data(), tw.size() * 8);
    const u32* p = (const u32*)d_tw.p;
    cv.ec().g[g].ntt(d_points, logn, p, inverse ? p + 8 * half : nullptr, st);
}

}  // namespace zk
