// Test hooks for the 29-bit-limb field layer (fe29_impl.hip.h), instantiated for the four moduli the library uses: Fq of BN254 and
// BLS12-381 (curve_consts.hip.h) and their scalar fields (fr29_consts.hip.h).  Every primitive is applied to operands from the host and
// what it returned is written back unreduced, as raw internal limbs, so that the test decides the exact lazy representative -- top-limb
// excess and limbs equal to 2^29 included (tests/test_gpu_fe29.py; the families and their rows are in fe_probe_impl.hip.h).  A host-only
// probe returns a field's constant tables.  Not part of include/zkgpu.h; the tests bind the two functions by name.
// Squaring is the dedicated fe_sqr here (as in the hashes); the mul row fe_mul(a, a) is what msm.hip's ZK_FE_SQR_PLAIN makes of it.
#include "zk_internal.h"
#include "curve_consts.hip.h"

namespace zk {
namespace bn254 {
namespace fe_probe_fq {
namespace {
#include "fe29_impl.hip.h"
#include "fe_probe_impl.hip.h"
}
}  // namespace fe_probe_fq
}  // namespace bn254
namespace bls12_381 {
namespace fe_probe_fq {
namespace {
#include "fe29_impl.hip.h"
#define FE_PROBE_NO_WIDE   // 14 limbs: (FE_WIDE_MAX + 1) NR products of 2^58 do not fit a 64-bit column
#include "fe_probe_impl.hip.h"
#undef FE_PROBE_NO_WIDE
}
}  // namespace fe_probe_fq
}  // namespace bls12_381
namespace fe_probe_fr254 {
namespace {
#define ZK_FR29_FIELD 254
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#include "fe_probe_impl.hip.h"
}
}  // namespace fe_probe_fr254
namespace fe_probe_fr381 {
namespace {
#define ZK_FR29_FIELD 381
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#include "fe_probe_impl.hip.h"
}
}  // namespace fe_probe_fr381
}  // namespace zk

// field: 0 BN254 Fq, 1 BLS12-381 Fq, 2 BN254 Fr, 3 BLS12-381 Fr.  family: fe_probe_impl.hip.h's F_*.  in / out: n elements of the
// family's operand / result words, element-major.
extern "C" int zk_fe29_probe(int field, int family, const uint32_t* in, uint32_t* out, size_t n) {
    using namespace zk;
    return guard([&] {
        ZK_REQUIRE(in && out && n > 0 && n <= ((size_t)1 << 20) && field >= 0 && field < 4, "zk_fe29_probe: bad arguments");
        switch (field) {
            case 0: bn254::fe_probe_fq::run(family, in, out, n); break;
            case 1: bls12_381::fe_probe_fq::run(family, in, out, n); break;
            case 2: fe_probe_fr254::run(family, in, out, n); break;
            default: fe_probe_fr381::run(family, in, out, n); break;
        }
    });
}

// Host only, no device: out[0..3) = NL, NR, QINV29, then nine tables of NR words (fe_probe_impl.hip.h consts); out holds 3 + 9 * 14 words
extern "C" int zk_fe29_consts_probe(int field, uint32_t* out) {
    using namespace zk;
    if (!out || field < 0 || field >= 4) return -1;
    switch (field) {
        case 0: bn254::fe_probe_fq::consts(out); break;
        case 1: bls12_381::fe_probe_fq::consts(out); break;
        case 2: fe_probe_fr254::consts(out); break;
        default: fe_probe_fr381::consts(out); break;
    }
    return 0;
}
