// Test hooks for the coordinate field `cf` and the XYZZ point formulas (ecpt_impl.hip.h), instantiated as msm.hip instantiates them:
// G1 and G2 (MSM_G2) of BN254 and BLS12-381, squaring as fe_mul(a, a), BN254's Fq2 products inlined (MSM_G2_INLINE_CF), BLS12-381's
// kept as functions, and the unit compiled with msm.o's flags (Makefile).  Every primitive is applied to operands from the host and
// what it returned is written back as raw internal limbs, unreduced (tests/test_gpu_ecpt.py; the families are in
// ecpt_probe_impl.hip.h).  Not part of include/zkgpu.h; the tests bind the function by name.
// Code size (msm.hip): one primitive per kernel; every kernel here is smaller than the largest msm.o has for the same curve and group.
#include "zk_internal.h"
#include "curve_consts.hip.h"

#define ZK_FE_SQR_PLAIN 1

namespace zk {
namespace bn254 {
namespace ecpt_probe_g1 {
namespace {
#include "ecpt_impl.hip.h"
#include "ecpt_probe_impl.hip.h"
}
}  // namespace ecpt_probe_g1
namespace ecpt_probe_g2 {
#define MSM_G2_INLINE_CF
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "ecpt_probe_impl.hip.h"
}
#undef MSM_G2_INLINE_CF
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
#undef MSM_G2
#undef FQ_MUL_ATTR
}  // namespace ecpt_probe_g2
}  // namespace bn254
namespace bls12_381 {
namespace ecpt_probe_g1 {
namespace {
#include "ecpt_impl.hip.h"
#include "ecpt_probe_impl.hip.h"
}
}  // namespace ecpt_probe_g1
namespace ecpt_probe_g2 {
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "ecpt_probe_impl.hip.h"
}
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
#undef MSM_G2
#undef FQ_MUL_ATTR
}  // namespace ecpt_probe_g2
}  // namespace bls12_381
}  // namespace zk

// curve: 0 BN254, 1 BLS12-381.  group: 1 or 2.  family: ecpt_probe_impl.hip.h's E_*.  in / out: n elements of the family's operand /
// result words, element-major.
extern "C" int zk_ecpt_probe(int curve, int group, int family, const uint32_t* in, uint32_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(in && out && n > 0 && n <= ((size_t)1 << 16) && (curve == 0 || curve == 1) && (group == 1 || group == 2), "zk_ecpt_probe: bad arguments");
        if (curve == 0 && group == 1) bn254::ecpt_probe_g1::run(family, in, out, n);
        else if (curve == 0) bn254::ecpt_probe_g2::run(family, in, out, n);
        else if (group == 1) bls12_381::ecpt_probe_g1::run(family, in, out, n);
        else bls12_381::ecpt_probe_g2::run(family, in, out, n);
    });
}
