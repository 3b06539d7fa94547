// Optimal ate pairing on BN254 and BLS12-381 and Groth16 verification for gfx950: what `zkit groth16_verify` computes
// (zkit/src/main.rs:221-230, groth16/src/api.rs:302-341 -> bellman's prepare_verifying_key + verify_proof -> pairing_ce).
//
// Tower: Fq2 = Fq[u]/(u^2 + 1), Fq12 = Fq2[w]/(w^6 - xi); BN254: xi = 9 + u, D-type twist, loop count 6t + 2 and the two
// Frobenius steps; BLS12-381: xi = 1 + u, M-type twist, loop count |x|, the Miller value conjugated because x < 0.
// Pipeline (pairing_impl.hip.h), all on one stream:
//   1. g2_lines_kernel    one lane per twist point: the line coefficients of every step (Jacobian, no inversion) -- once per
//                         key for -gamma and -delta (the part of prepare_verifying_key), once per proof for B
//   2. miller_kernel      eight lanes per item (six own the Fq2 coefficients of w^0..w^5): one squaring per step shared by
//                         up to three pairs, the lines multiplied in as sparse elements
//   3. final_exp_kernel   the same lanes: easy part with one inversion, hard part (q^4 - q^2 + 1)/r in a 4-bit window over
//                         Granger-Scott squarings; the exact reduced pairing
// and around them the input checks (curve, subgroup by [r]P = O, canonical public inputs), acc = IC_0 + sum x_j IC_j, and
// the comparison with e(alpha, beta); the point checks at the scale of a proving key are key_check_impl.hip.h.  Stricter than the reference, which reads points unchecked (json_utils.rs:163-198).
// Fq, Fq2 and the point formulas are the sums' (fe29_impl.hip.h, ecpt_impl.hip.h); fe_mul and the Fq2 product are real
// functions here, and the loops over exponent bits stay loops: the code-size hazard recorded in msm.hip.
#include "curve.h"
#include "curve_consts.hip.h"
#include "pairing_consts.hip.h"
#include "json_min.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace zk {

#define FQ_MUL_ATTR __noinline__

namespace bn254 {
namespace pg1 {
namespace {
#include "ecpt_impl.hip.h"
#include "pairing_impl.hip.h"
#include "key_check_impl.hip.h"
}
}  // namespace pg1
namespace pg2 {
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "pairing_impl.hip.h"
#include "key_check_impl.hip.h"
}
#undef MSM_G2
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
}  // namespace pg2
static const PairingOps OPS = {"30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47",
                               pg1::g1_check_dev, pg1::g16_acc_dev, pg2::g2_check_dev, pg2::g2_lines_bytes, pg2::g2_lines_dev, pg2::f12_bytes,
                               pg2::final_exp_tab_bytes, pg2::miller_dev, pg2::final_exp_dev, pg2::g16_verdict_dev,
                               pg2::f12_prod_scratch_bytes, pg2::f12_prod_dev, {pg1::points_check_dev, pg2::points_check_dev}};
}  // namespace bn254
namespace bls12_381 {
namespace pg1 {
namespace {
#include "ecpt_impl.hip.h"
#include "pairing_impl.hip.h"
#include "key_check_impl.hip.h"
}
}  // namespace pg1
namespace pg2 {
#define MSM_G2
namespace {
#include "ecpt_impl.hip.h"
#include "pairing_impl.hip.h"
#include "key_check_impl.hip.h"
}
#undef MSM_G2
#undef CF_MUL_ATTR
#undef PT_COLD_ATTR
}  // namespace pg2
static const PairingOps OPS = {"1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab",
                               pg1::g1_check_dev, pg1::g16_acc_dev, pg2::g2_check_dev, pg2::g2_lines_bytes, pg2::g2_lines_dev, pg2::f12_bytes,
                               pg2::final_exp_tab_bytes, pg2::miller_dev, pg2::final_exp_dev, pg2::g16_verdict_dev,
                               pg2::f12_prod_scratch_bytes, pg2::f12_prod_dev, {pg1::points_check_dev, pg2::points_check_dev}};
}  // namespace bls12_381
#undef FQ_MUL_ATTR

const PairingOps& pairing_ops(CurveId id) { return id == CURVE_BN254 ? bn254::OPS : bls12_381::OPS; }   // the table's slice of this unit (curve.h)
struct PoolBuf {   // a block of the pool for the length of one call; freeing is ordered on the call's stream (devmem.hip)
    void* p;
    explicit PoolBuf(size_t n) : p(pool_alloc(n ? n : 4)) {}
    ~PoolBuf() { pool_free(p); }
    PoolBuf(const PoolBuf&) = delete; PoolBuf& operator=(const PoolBuf&) = delete;
};

// n pairs (G1 n x 2 NL words, G2 n x 4 NL words, external layout) -> n GT values of 12 canonical Fq
static void pairing_run(const Curve& cv, const void* d_g1, const void* d_g2, u64 n, void* d_gt, int with_final_exp, hipStream_t st) {
    if (!n) return;
    const PairingOps& o = cv.pairing();
    PoolBuf lines(o.lines_bytes(n)), inf(4 * n), f(o.f12_bytes(n)), tab(with_final_exp ? o.tab_bytes(n) : 4);
    o.g2_lines(d_g2, cv.point_words(G2), n, lines.p, inf.p, st);
    MillerArgs a{};
    a.np = 1;
    a.g1[0] = (const u32*)d_g1; a.g1_stride[0] = cv.point_words(G1);
    a.lines[0] = (const u32*)lines.p; a.lines_stride[0] = o.lines_bytes(1) / 4;
    a.inf[0] = (const u32*)inf.p; a.inf_stride[0] = 1;
    o.miller(a, n, f.p, st);
    o.final_exp(f.p, n, tab.p, d_gt, with_final_exp, st);
}
void pairing_dev(const Curve& cv, const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, hipStream_t st) {
    pairing_run(cv, d_g1, d_g2, n, d_gt, with_final_exp, st);
}

// ---- Groth16 -------------------------------------------------------------------------------------------------------------------
// a decimal or 0x string -> little-endian 32-bit words; false when it does not fit
static bool parse_int(const std::string& s, u32* w, int nw) {
    for (int i = 0; i < nw; ++i) w[i] = 0;
    const bool hex = s.size() > 2 && s[0] == '0' && (s[1] == 'x' || s[1] == 'X');
    ZK_REQUIRE(!s.empty() && (!hex || s.size() > 2), "groth16 verify: empty number");
    for (size_t i = hex ? 2 : 0; i < s.size(); ++i) {
        const char ch = s[i];
        u32 d;
        if (ch >= '0' && ch <= '9') d = (u32)(ch - '0');
        else if (hex && ch >= 'a' && ch <= 'f') d = (u32)(ch - 'a' + 10);
        else if (hex && ch >= 'A' && ch <= 'F') d = (u32)(ch - 'A' + 10);
        else throw Error("groth16 verify: '" + s + "' is not a number");
        uint64_t carry = d;
        for (int k = 0; k < nw; ++k) { const uint64_t v = (uint64_t)w[k] * (hex ? 16 : 10) + carry; w[k] = (u32)v; carry = v >> 32; }
        if (carry) return false;
    }
    return true;
}
static const std::string& jstr(const JVal& v) { ZK_REQUIRE(v.kind == JVal::Str || v.kind == JVal::Num, "groth16 verify: a number string expected"); return v.s; }
static void parse_fq(const Curve& cv, const JVal& v, u32* w) { ZK_REQUIRE(parse_int(jstr(v), w, (int)cv.fq_words), "groth16 verify: a coordinate does not fit the base field's width"); }
// {"x", "y"} -> 2 NL canonical words; pairing_ce's zero (0, 1) becomes the all-zero encoding (curve.h: groth16_key_check reads
// verification_key.json with these two as well)
void groth16_json_g1(const Curve& cv, const JVal& v, u32* w) {
    const int nl = (int)cv.fq_words;
    parse_fq(cv, v.at("x"), w); parse_fq(cv, v.at("y"), w + nl);
    bool zero = w[nl] == 1;
    for (int i = 0; i < 2 * nl; ++i) if (i != nl && w[i]) zero = false;
    if (zero) w[nl] = 0;
}
void groth16_json_g2(const Curve& cv, const JVal& v, u32* w, bool negate) {
    const int nl = (int)cv.fq_words;
    for (int c = 0; c < 2; ++c) { parse_fq(cv, v.at("x").at(c), w + c * nl); parse_fq(cv, v.at("y").at(c), w + (2 + c) * nl); }
    bool zero = w[2 * nl] == 1;
    for (int i = 0; i < 4 * nl; ++i) if (i != 2 * nl && w[i]) zero = false;
    if (zero) w[2 * nl] = 0;
    if (!negate || zero) return;
    std::vector<u32> q(nl);
    parse_int(std::string("0x") + cv.pairing().q_hex, q.data(), nl);
    for (int c = 2; c < 4; ++c) {                          // y -> q - y (a coordinate >= q stays as it is and fails the curve check)
        u32* y = w + c * nl;
        bool nz = false, lt = false;
        for (int i = 0; i < nl; ++i) nz |= y[i] != 0;
        for (int i = nl - 1; i >= 0; --i) if (y[i] != q[i]) { lt = y[i] < q[i]; break; }
        if (!nz || !lt) continue;
        uint64_t br = 0;
        for (int i = 0; i < nl; ++i) { const uint64_t d = (uint64_t)q[i] - y[i] - br; y[i] = (u32)d; br = (d >> 32) & 1; }
    }
}
static void* upload_mont(const Curve& cv, const std::vector<u32>& canon, hipStream_t st) {
    void* d = pool_alloc(canon.size() * 4);
    try {
        h2d_sync(d, canon.data(), canon.size() * 4);
        cv.msm().fq_canon_to_mont_dev(d, canon.size() / cv.fq_words, st);
    } catch (...) { pool_free(d); throw; }
    return d;
}

Groth16Vk* groth16_vk_new(const char* curve, const char* vk_json) {
    ZK_REQUIRE(vk_json, "groth16 verify: null verification key");
    const Curve& cv = curve_of(curve, PAIRING_NAMES);
    const PairingOps& o = cv.pairing();
    const JVal js = JParser::parse(vk_json);
    if (const JVal* c = js.find("curve")) ZK_REQUIRE(&curve_of(c->str().c_str(), PAIRING_NAMES) == &cv, "groth16 verify: the key is for curve " + c->str());
    const JVal& ic = js.at("IC");
    ZK_REQUIRE(ic.kind == JVal::Arr && ic.size() >= 1, "groth16 verify: IC must hold at least one point");
    const int nl = (int)cv.fq_words;
    std::vector<u32> g1((ic.size() + 1) * 2 * nl), g2(4 * 4 * nl);              // alpha, IC... ; beta, -gamma, -delta, -beta
    groth16_json_g1(cv, js.at("vk_alpha_1"), g1.data());
    for (size_t i = 0; i < ic.size(); ++i) groth16_json_g1(cv, ic.at(i), g1.data() + (i + 1) * 2 * nl);
    groth16_json_g2(cv, js.at("vk_beta_2"), g2.data(), false);
    groth16_json_g2(cv, js.at("vk_gamma_2"), g2.data() + 4 * nl, true);
    groth16_json_g2(cv, js.at("vk_delta_2"), g2.data() + 8 * nl, true);
    groth16_json_g2(cv, js.at("vk_beta_2"), g2.data() + 12 * nl, true);
    hipStream_t st = cur_stream();
    auto vk = std::make_unique<Groth16Vk>();
    vk->curve = &cv; vk->n_ic = (uint32_t)ic.size();
    PoolBuf dg1(g1.size() * 4), dg2(g2.size() * 4), status(4 * (g1.size() / (2 * nl) + 3));
    h2d_sync(dg1.p, g1.data(), g1.size() * 4); h2d_sync(dg2.p, g2.data(), g2.size() * 4);
    cv.msm().fq_canon_to_mont_dev(dg1.p, g1.size() / nl, st); cv.msm().fq_canon_to_mont_dev(dg2.p, g2.size() / nl, st);
    const u64 n1 = g1.size() / (2 * nl);
    ZK_HIP(hipMemsetD32Async((hipDeviceptr_t)status.p, 1, n1 + 3, st));
    o.g1_check(dg1.p, 2 * (u64)nl, n1, (int*)status.p, 1, st);
    o.g2_check(dg2.p, 4 * (u64)nl, 3, (int*)status.p + n1, 1, st);
    std::vector<int> hs(n1 + 3);
    d2h_sync(hs.data(), status.p, hs.size() * 4);
    for (size_t i = 0; i < hs.size(); ++i)
        ZK_REQUIRE(hs[i] == 1, std::string("groth16 verify: a point of the verification key is ") + (hs[i] == -3 ? "not on its curve" : "outside the subgroup of order r"));
    vk->d_ic = pool_alloc(ic.size() * 2 * nl * 4);
    ZK_HIP(hipMemcpyAsync(vk->d_ic, (const u32*)dg1.p + 2 * nl, ic.size() * 2 * nl * 4, hipMemcpyDeviceToDevice, st));
    vk->d_ab = pool_alloc(12 * nl * 4);
    pairing_run(cv, dg1.p, dg2.p, 1, vk->d_ab, 1, st);
    vk->d_lines = pool_alloc(o.lines_bytes(3)); vk->d_inf = pool_alloc(12);     // -gamma, -delta; -beta for the aggregate check
    o.g2_lines((const u32*)dg2.p + 4 * nl, 4 * (u64)nl, 3, vk->d_lines, vk->d_inf, st);
    vk->d_alpha = pool_alloc(2 * nl * 4);
    ZK_HIP(hipMemcpyAsync(vk->d_alpha, dg1.p, 2 * nl * 4, hipMemcpyDeviceToDevice, st));
    for (size_t i = 0; i < ic.size(); ++i) {
        const u32* w = g1.data() + (i + 1) * 2 * nl;
        if (std::all_of(w, w + 2 * nl, [](u32 v) { return v == 0; })) vk->ic_has_infinity = true;
    }
    ZK_HIP(hipStreamSynchronize(st));
    return vk.release();
}
void groth16_vk_info(const Groth16Vk* vk, uint32_t* n_public, uint32_t* proof_bytes, uint32_t* gt_bytes) {
    ZK_REQUIRE(vk, "groth16 verify: null key");
    if (n_public) *n_public = vk->n_ic - 1;
    if (proof_bytes) *proof_bytes = (uint32_t)(4 * vk->curve->proof_words());
    if (gt_bytes) *gt_bytes = (uint32_t)vk->curve->gt_bytes();
}
// proofs: n x (A | B | C) in the layout zk_groth16_prove writes; publics: n x n_public x 8 words canonical; verdicts: n ints
void groth16_verify_batch_dev(const Groth16Vk* vk, const void* d_proofs, const void* d_publics, uint64_t n, int* d_verdicts, hipStream_t st) {
    ZK_REQUIRE(vk, "groth16 verify: null key");
    if (!n) return;
    ZK_REQUIRE(d_proofs && d_verdicts && (d_publics || vk->n_ic == 1), "groth16 verify: null argument");
    const PairingOps& o = vk->curve->pairing();
    const u64 nl = vk->curve->fq_words, pw = 8 * nl;
    const u32* pr = (const u32*)d_proofs;
    PoolBuf status(4 * n), acc(n * 2 * nl * 4), lines(o.lines_bytes(n)), inf(4 * n), f(o.f12_bytes(n)), tab(o.tab_bytes(n)), gt(n * 12 * nl * 4);
    ZK_HIP(hipMemsetD32Async((hipDeviceptr_t)status.p, 1, n, st));
    o.g1_check(pr, pw, n, (int*)status.p, 1, st);
    o.g1_check(pr + 6 * nl, pw, n, (int*)status.p, 1, st);
    o.g2_check(pr + 2 * nl, pw, n, (int*)status.p, 1, st);
    o.g16_acc(vk->d_ic, vk->n_ic - 1, d_publics, n, acc.p, (int*)status.p, st);
    o.g2_lines(pr + 2 * nl, pw, n, lines.p, inf.p, st);
    const u64 lw = o.lines_bytes(1) / 4;
    MillerArgs a{};
    a.np = 3;
    a.g1[0] = pr; a.g1_stride[0] = pw; a.lines[0] = (const u32*)lines.p; a.lines_stride[0] = lw; a.inf[0] = (const u32*)inf.p; a.inf_stride[0] = 1;
    a.g1[1] = (const u32*)acc.p; a.g1_stride[1] = 2 * nl; a.lines[1] = (const u32*)vk->d_lines; a.lines_stride[1] = 0; a.inf[1] = (const u32*)vk->d_inf; a.inf_stride[1] = 0;
    a.g1[2] = pr + 6 * nl; a.g1_stride[2] = pw; a.lines[2] = (const u32*)vk->d_lines + lw; a.lines_stride[2] = 0; a.inf[2] = (const u32*)vk->d_inf + 1; a.inf_stride[2] = 0;
    o.miller(a, n, f.p, st);
    o.final_exp(f.p, n, tab.p, gt.p, 1, st);
    o.verdict(gt.p, vk->d_ab, n, (const int*)status.p, d_verdicts, st);
}
void groth16_verify_batch(const Groth16Vk* vk, const void* proofs, const void* publics, uint64_t n, int* verdicts) {
    ZK_REQUIRE(vk, "groth16 verify: null key");
    if (!n) return;
    ZK_REQUIRE(proofs && verdicts && (publics || vk->n_ic == 1), "groth16 verify: null argument");
    const size_t pb = 4 * vk->curve->proof_words(), ub = (size_t)(vk->n_ic - 1) * 32;
    PoolBuf dp(n * pb), du(n * ub), dv(n * 4);
    h2d_sync(dp.p, proofs, n * pb);
    if (ub) h2d_sync(du.p, publics, n * ub);
    groth16_verify_batch_dev(vk, dp.p, du.p, n, (int*)dv.p, cur_stream());
    d2h_sync(verdicts, dv.p, n * 4);
}
// the file-level form (api.rs:302-341): proof.json and public_input.json -> verdict
int groth16_verify_json(const Groth16Vk* vk, const char* proof_json, const char* public_json) {
    ZK_REQUIRE(vk && proof_json && public_json, "groth16 verify: null argument");
    const Curve& cv = *vk->curve;
    const int nl = (int)cv.fq_words;
    const JVal pj = JParser::parse(proof_json), uj = JParser::parse(public_json);
    ZK_REQUIRE(uj.kind == JVal::Arr, "groth16 verify: public_input.json must be an array");
    if (uj.size() != vk->n_ic - 1) return -2;
    std::vector<u32> pts(8 * nl), pub(8 * uj.size() + 8);
    groth16_json_g1(cv, pj.at("pi_a"), pts.data()); groth16_json_g2(cv, pj.at("pi_b"), pts.data() + 2 * nl, false); groth16_json_g1(cv, pj.at("pi_c"), pts.data() + 6 * nl);
    for (size_t i = 0; i < uj.size(); ++i) if (!parse_int(jstr(uj.at(i)), pub.data() + 8 * i, 8)) return -1;
    hipStream_t st = cur_stream();
    void* dp = upload_mont(cv, pts, st);
    int verdict = 0;
    try {
        PoolBuf du(pub.size() * 4), dv(4);
        h2d_sync(du.p, pub.data(), pub.size() * 4);
        groth16_verify_batch_dev(vk, dp, du.p, 1, (int*)dv.p, st);
        d2h_sync(&verdict, dv.p, 4);
    } catch (...) { pool_free(dp); throw; }
    pool_free(dp);
    return verdict;
}

// ---- many pairs, one value; many proofs, one check ------------------------------------------------------------------
// Proofs (or pairs) per chunk: the line tables and Miller values of one chunk are all that is ever allocated (about 20 KB a pair), and the
// running product is carried from chunk to chunk.  A chunk of 4096 was measured first and left the device idle: g2_lines_kernel is one lane
// per point, so 4096 points are 64 waves on 1024 SIMDs and every chunk costs the latency of one table (profiles/r15/verify_aggregate.md).  ZK_VERIFY_AGG_CHUNK, read once, overrides it so that a test meets chunk borders at small n.
constexpr u64 AGG_CHUNK = 65536;   // one lane of g2_lines_kernel per SIMD of the device and more; 1.3 GB (BN254) / 1.5 GB (BLS12-381) of tables
static u64 agg_chunk() {
    static const u64 c = [] { const char* e = getenv("ZK_VERIFY_AGG_CHUNK"); const long long v = e ? atoll(e) : 0; return v > 0 ? (u64)v : AGG_CHUNK; }();
    return c;
}
static thread_local double AGG_MS[6];
enum { AGG_T_CHECKS, AGG_T_MULS, AGG_T_MILLER, AGG_T_PRODUCT, AGG_T_SUMS, AGG_T_TAIL };
struct AggTimer {   // host milliseconds per phase, around stream synchronisations; off unless ZK_VERIFY_AGG_TIMING is set (read per call)
    using clk = std::chrono::steady_clock;
    hipStream_t st; bool on; clk::time_point t;
    explicit AggTimer(hipStream_t s) : st(s) {
        const char* e = getenv("ZK_VERIFY_AGG_TIMING");
        on = e && *e && strcmp(e, "0");
        if (on) { for (double& m : AGG_MS) m = 0; ZK_HIP(hipStreamSynchronize(st)); t = clk::now(); }
    }
    void lap(int phase) {
        if (!on) return;
        ZK_HIP(hipStreamSynchronize(st));
        const auto now = clk::now();
        AGG_MS[phase] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    }
};
void groth16_verify_aggregate_timing(double ms[6]) { for (int i = 0; i < 6; ++i) ms[i] = AGG_MS[i]; }

// n rows of `width` words, `stride` words apart -> packed (C out of the proofs, for the sum)
__global__ __launch_bounds__(256) void gather_rows_kernel(const u32* __restrict__ src, u64 stride, u32 width, u64 n, u32* __restrict__ dst) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * width) return;
    dst[t] = src[(t / width) * stride + (t % width)];
}
// acc <- acc x the Miller values of further pairs, chunk by chunk
struct MillerProduct {
    const Curve& cv; const PairingOps& o; hipStream_t st; AggTimer* tm;
    u64 chunk;
    PoolBuf lines, inf, f, scratch, acc;
    bool have = false;
    MillerProduct(const Curve& c, u64 n_max, hipStream_t s, AggTimer* t)
        : cv(c), o(c.pairing()), st(s), tm(t), chunk(std::max<u64>(1, std::min(n_max, agg_chunk()))), lines(o.lines_bytes(chunk)), inf(4 * chunk),
          f(o.f12_bytes(chunk + 1)), scratch(o.f12_prod_scratch(chunk + 1)), acc(o.f12_bytes(1)) {}
    // the m <= chunk values at the head of f, and the running product behind them, become the running product
    void fold(u64 m) {
        u64 k = m;
        if (have) { ZK_HIP(hipMemcpyAsync((uint8_t*)f.p + o.f12_bytes(m), acc.p, o.f12_bytes(1), hipMemcpyDeviceToDevice, st)); ++k; }
        o.f12_prod(f.p, k, scratch.p, acc.p, st);
        have = true;
        if (tm) tm->lap(AGG_T_PRODUCT);
    }
    void pairs(const u32* g1, u64 s1, const u32* g2, u64 s2, u64 n) {
        for (u64 off = 0; off < n; off += chunk) {
            const u64 m = std::min(chunk, n - off);
            o.g2_lines(g2 + off * s2, s2, m, lines.p, inf.p, st);
            MillerArgs a{};
            a.np = 1;
            a.g1[0] = g1 + off * s1; a.g1_stride[0] = s1;
            a.lines[0] = (const u32*)lines.p; a.lines_stride[0] = o.lines_bytes(1) / 4;
            a.inf[0] = (const u32*)inf.p; a.inf_stride[0] = 1;
            o.miller(a, m, f.p, st);
            if (tm) tm->lap(AGG_T_MILLER);
            fold(m);
        }
    }
};
void pairing_product_dev(const Curve& cv, const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, hipStream_t st) {
    if (!n) {                                                                            // the empty product: one
        const u32 one = 1;
        ZK_HIP(hipMemsetAsync(d_gt, 0, cv.gt_bytes(), st));
        ZK_HIP(hipMemcpyAsync(d_gt, &one, 4, hipMemcpyHostToDevice, st));
        ZK_HIP(hipStreamSynchronize(st));
        return;
    }
    const PairingOps& o = cv.pairing();
    MillerProduct mp(cv, n, st, nullptr);
    mp.pairs((const u32*)d_g1, cv.point_words(G1), (const u32*)d_g2, cv.point_words(G2), n);
    PoolBuf tab(with_final_exp ? o.tab_bytes(1) : 4);
    o.final_exp(mp.acc.p, 1, tab.p, d_gt, with_final_exp, st);
}

void groth16_verify_aggregate_dev(const Groth16Vk* vk, const void* d_proofs, const void* d_publics, uint64_t n, const uint8_t* seed, bool locate,
                                  int* verdict, uint64_t* first_bad, hipStream_t st) {
    ZK_REQUIRE(vk && verdict, "groth16 verify: null argument");
    *verdict = 1;
    if (first_bad) *first_bad = n;
    if (!n) return;
    ZK_REQUIRE(d_proofs && (d_publics || vk->n_ic == 1), "groth16 verify: null argument");
    ZK_REQUIRE(n < (1ull << 28), "groth16 verify: more than 2^28 proofs in one batch");
    const Curve& cv = *vk->curve;
    const PairingOps& o = cv.pairing();
    const u64 nl = cv.fq_words, pw = 8 * nl, P1 = 2 * nl;
    const u32 n_pub = vk->n_ic - 1;
    const u32* pr = (const u32*)d_proofs;
    AggTimer tm(st);
    // the per-proof path's answer: the first proof it does not accept.  refused: the aggregate has refused, so one must exist
    auto per_proof = [&](bool refused) {
        PoolBuf dv(4 * n);
        groth16_verify_batch_dev(vk, d_proofs, d_publics, n, (int*)dv.p, st);
        std::vector<int> v(n);
        d2h_sync(v.data(), dv.p, 4 * n);
        for (u64 i = 0; i < n; ++i)
            if (v[i] != 1) {
                *verdict = locate ? v[i] : 0;
                if (locate && first_bad) *first_bad = i;
                return;
            }
        ZK_REQUIRE(!refused, "groth16 verify: the aggregate check refused a batch whose proofs all pass one by one");
        *verdict = 1;
    };
    // 1. well-formedness: the classes of A, C (G1) and B (G2); the inputs' range comes with the sums below
    PoolBuf d_cls(3 * 64);
    u64 cls[3][8];
    o.points_check[G1](pr, pw, n, 0, 0, (u64*)d_cls.p, st);
    o.points_check[G2](pr + 2 * nl, pw, n, 0, 0, (u64*)d_cls.p + 8, st);
    o.points_check[G1](pr + 6 * nl, pw, n, 0, 0, (u64*)d_cls.p + 16, st);
    d2h_sync(cls, d_cls.p, sizeof cls);
    tm.lap(AGG_T_CHECKS);
    // What the sums cannot take, or where the per-proof path has a rule of its own, is answered by that path: a coordinate that is not below q
    // (it reduces it and goes on), C or an IC point at infinity (a term the sums would have to leave out).  None occurs in an honest batch.
    bool exotic = vk->ic_has_infinity || cls[2][0] != 0;
    bool malformed = false;
    for (int k = 0; k < 3; ++k) { exotic |= cls[k][2] != 0; malformed |= cls[k][4] != 0 || cls[k][6] != 0; }
    if (exotic) { per_proof(false); return; }
    // 2. the weights and the scalar side
    DevBuf d_rho;
    groth16_rho_dev(seed, n, d_rho, st, "groth16 verify");
    PoolBuf d_sums((size_t)vk->n_ic * 36);
    cv.groth16().verify_sums_dev(d_rho.p, d_publics, n, n_pub, d_sums.p, st);
    std::vector<u32> bad(vk->n_ic);
    d2h_sync(bad.data(), (const u32*)d_sums.p + (size_t)vk->n_ic * 8, (size_t)vk->n_ic * 4);
    for (u32 b : bad) malformed |= b != 0;
    tm.lap(AGG_T_SUMS);
    if (malformed) {
        if (locate) per_proof(true); else *verdict = 0;
        return;
    }
    // 3. prod e([rho_i] A_i, B_i), chunk by chunk
    MillerProduct mp(cv, n, st, &tm);
    {
        PoolBuf ra(mp.chunk * P1 * 4);
        for (u64 off = 0; off < n; off += mp.chunk) {
            const u64 m = std::min(mp.chunk, n - off);
            cv.ec().g[G1].mul_scalars(pr + off * pw, pw, m, (const u32*)d_rho.p + off * 8, ra.p, st);
            tm.lap(AGG_T_MULS);
            mp.pairs((const u32*)ra.p, P1, pr + off * pw + 2 * nl, pw, m);
        }
    }
    // 4. the tail: sum rho_i C_i, sum s_j IC_j, [s_0] alpha against -delta, -gamma, -beta
    const u64 TS = P1 + 4;                                                               // a point and its flag word, 16-byte aligned
    PoolBuf d_c(n * P1 * 4), d_t(3 * TS * 4);
    u32* t = (u32*)d_t.p;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n * P1 + 255) / 256)), dim3(256), 0, st, pr + 6 * nl, pw, (u32)P1, n, (u32*)d_c.p);
    ZK_HIP(hipGetLastError());
    cv.group(G1).msm_dev(vk->d_ic, d_sums.p, vk->n_ic, t, st);
    cv.group(G1).msm_dev(d_c.p, d_rho.p, n, t + TS, st);
    u32 flag[2];
    d2h_sync(&flag[0], t + P1, 4); d2h_sync(&flag[1], t + TS + P1, 4);
    for (int k = 0; k < 2; ++k) if (flag[k]) ZK_HIP(hipMemsetAsync(t + k * TS, 0, P1 * 4, st));          // a sum at infinity: the all-zero encoding
    tm.lap(AGG_T_SUMS);
    cv.ec().g[G1].mul_scalar(vk->d_alpha, 1, (const u32*)d_sums.p, t + 2 * TS, st);
    const u64 lw = o.lines_bytes(1) / 4;
    MillerArgs a{};
    a.np = 3;
    for (int k = 0; k < 3; ++k) {
        a.g1[k] = t + k * TS; a.g1_stride[k] = 0;
        a.lines[k] = (const u32*)vk->d_lines + k * lw; a.lines_stride[k] = 0;
        a.inf[k] = (const u32*)vk->d_inf + k; a.inf_stride[k] = 0;
    }
    o.miller(a, 1, mp.f.p, st);
    mp.tm = nullptr;
    mp.fold(1);
    PoolBuf tab(o.tab_bytes(1)), gt(12 * nl * 4);
    o.final_exp(mp.acc.p, 1, tab.p, gt.p, 1, st);
    std::vector<u32> g(12 * nl);
    d2h_sync(g.data(), gt.p, g.size() * 4);
    tm.lap(AGG_T_TAIL);
    bool is_one = g[0] == 1;
    for (size_t i = 1; i < g.size(); ++i) is_one &= g[i] == 0;
    if (is_one) return;
    if (locate) per_proof(true); else *verdict = 0;
}
void groth16_verify_aggregate(const Groth16Vk* vk, const void* proofs, const void* publics, uint64_t n, const uint8_t* seed, bool locate,
                              int* verdict, uint64_t* first_bad) {
    ZK_REQUIRE(vk && verdict, "groth16 verify: null argument");
    if (!n) { *verdict = 1; if (first_bad) *first_bad = 0; return; }
    ZK_REQUIRE(proofs && (publics || vk->n_ic == 1), "groth16 verify: null argument");
    const size_t pb = 4 * vk->curve->proof_words(), ub = (size_t)(vk->n_ic - 1) * 32;
    PoolBuf dp(n * pb), du(n * ub);
    h2d_sync(dp.p, proofs, n * pb);
    if (ub) h2d_sync(du.p, publics, n * ub);
    groth16_verify_aggregate_dev(vk, dp.p, du.p, n, seed, locate, verdict, first_bad, cur_stream());
}
int groth16_proof_words(const Groth16Vk* vk, const char* proof_json, const char* public_json, void* proof_out, void* public_out) {
    ZK_REQUIRE(vk && proof_json && public_json && proof_out && (public_out || vk->n_ic == 1), "groth16 verify: null argument");
    const Curve& cv = *vk->curve;
    const int nl = (int)cv.fq_words;
    const JVal pj = JParser::parse(proof_json), uj = JParser::parse(public_json);
    ZK_REQUIRE(uj.kind == JVal::Arr, "groth16 verify: public_input.json must be an array");
    if (uj.size() != vk->n_ic - 1) return -2;
    std::vector<u32> pts(8 * nl), pub(8 * uj.size());
    groth16_json_g1(cv, pj.at("pi_a"), pts.data()); groth16_json_g2(cv, pj.at("pi_b"), pts.data() + 2 * nl, false); groth16_json_g1(cv, pj.at("pi_c"), pts.data() + 6 * nl);
    for (size_t i = 0; i < uj.size(); ++i) if (!parse_int(jstr(uj.at(i)), pub.data() + 8 * i, 8)) return -1;
    void* dp = upload_mont(cv, pts, cur_stream());
    try { d2h_sync(proof_out, dp, pts.size() * 4); } catch (...) { pool_free(dp); throw; }
    pool_free(dp);
    if (!pub.empty()) std::memcpy(public_out, pub.data(), pub.size() * 4);
    return 1;
}

}  // namespace zk
