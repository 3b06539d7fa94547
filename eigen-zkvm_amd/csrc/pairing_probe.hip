// Test hooks for the pairing tower (pairing_impl.hip.h), instantiated as pairing.hip's pg2 namespaces instantiate it: ecpt_impl.hip.h and
// pairing_impl.hip.h with MSM_G2 for BN254 and BLS12-381, fe_mul and fe_sqr real functions (FQ_MUL_ATTR __noinline__, the dedicated
// squaring), the Fq2 product a real function (no MSM_G2_INLINE_CF), and the unit compiled with pairing.o's flags (Makefile).  Every
// primitive -- cf_mul_xi / cf_red / cf_neg, the line steps, the Fq12 products on groups of eight lanes, the canonical words, the line
// tables and the final exponentiation as their entry points run them -- is applied to operands from the host and what it returned is
// written back as raw internal limbs, unreduced (tests/test_gpu_pairing_tower.py; the families are in pairing_probe_impl.hip.h).
// Not part of include/zkgpu.h; the tests bind the function by name.
#include "curve.h"
#include "curve_consts.hip.h"
#include "pairing_consts.hip.h"

namespace zk {
#define FQ_MUL_ATTR __noinline__

namespace bn254 {
namespace pairing_probe {
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "pairing_impl.hip.h"
#include "pairing_probe_impl.hip.h"
}
#undef MSM_G2
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
}  // namespace pairing_probe
}  // namespace bn254
namespace bls12_381 {
namespace pairing_probe {
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "pairing_impl.hip.h"
#include "pairing_probe_impl.hip.h"
}
#undef MSM_G2
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
}  // namespace pairing_probe
}  // namespace bls12_381
#undef FQ_MUL_ATTR
}  // namespace zk

// curve: 0 BN254, 1 BLS12-381.  family: pairing_probe_impl.hip.h's T_*.  in / out: n elements of the family's operand / result words,
// element-major.
extern "C" int zk_pairing_probe(int curve, int family, const uint32_t* in, uint32_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(in && out && n > 0 && n <= ((size_t)1 << 16) && (curve == 0 || curve == 1), "zk_pairing_probe: bad arguments");
        if (curve == 0) bn254::pairing_probe::run(family, in, out, n);
        else bls12_381::pairing_probe::run(family, in, out, n);
    });
}
