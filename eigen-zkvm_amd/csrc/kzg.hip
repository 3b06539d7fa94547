// KZG commitments over a powers-of-tau file on gfx950: commit, open, verify -- what every step of snarkjs's
// `ffs` / `fff` / `ffv` (test/snark_verifier.sh:67-106; PLONK, fflonk) is made of, over the tauG1 section zk_srs_open reads.
//   kzg_impl.hip.h   y = p(z) and q = (p - y) / (X - z) as a tiled scan, the gamma fold of polynomials, the scalars of the batched check --
//                    instantiated once per scalar field below
//   this file        the handle (the file's G1 powers on the device, window tables, Lagrange bases in the group per log n) and the layer that
//                    ties the scan to the existing sums (msm.hip), group transforms (ecntt.hip), point classes and pairing products (pairing.hip)
// Commitments are in G1 and are not hiding.
#include "curve.h"
#include "fr_host.h"
#include "../../include/zkgpu.h"
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>

namespace zk {
namespace kzg_bn254 {
#define ZK_FR29_FIELD 254
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#include "fr_rows_impl.hip.h"
#include "kzg_impl.hip.h"
}  // namespace kzg_bn254
namespace kzg_bls12381 {
#define ZK_FR29_FIELD 381
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#include "fr_rows_impl.hip.h"
#include "kzg_impl.hip.h"
}  // namespace kzg_bls12381

const KzgOps& kzg_ops(CurveId id) {   // the table's slice of this unit (curve.h)
    static const KzgOps OPS[2] = {{kzg_bn254::divide_dev, kzg_bn254::table_bytes, kzg_bn254::table_dev, kzg_bn254::lincomb_dev, kzg_bn254::weights_dev,
                                   kzg_bn254::divide_acc_dev, kzg_bn254::interleave_dev},
                                  {kzg_bls12381::divide_dev, kzg_bls12381::table_bytes, kzg_bls12381::table_dev, kzg_bls12381::lincomb_dev, kzg_bls12381::weights_dev,
                                   kzg_bls12381::divide_acc_dev, kzg_bls12381::interleave_dev}};
    return OPS[id];
}

namespace {
const u32* canon_words(const Curve& cv, const uint64_t* v, const char* what) {
    ZK_REQUIRE(v, std::string("kzg: null ") + what);
    ZK_REQUIRE(cv.fr_canonical((const u32*)v), std::string("kzg: ") + what + " is not below the scalar field's modulus");
    return (const u32*)v;
}
// a sum's result slot at infinity: the all-zero point and the flag word
void put_infinity(const Curve& cv, void* d_out, hipStream_t st) {
    const size_t B = cv.point_bytes(G1);
    const u32 one = 1;
    ZK_HIP(hipMemsetAsync(d_out, 0, B, st));
    ZK_HIP(hipMemcpyAsync((uint8_t*)d_out + B, &one, 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));                                   // `one` leaves scope
}
// sum_{i < n} s_i tauG1[i] for canonical scalars on the device
void powers_sum_dev(const Kzg& k, const void* d_scalars, u64 n, void* d_out, hipStream_t st) {
    const Curve& cv = *k.curve;
    if (n == 0) { put_infinity(cv, d_out, st); return; }
    if (k.d_table) cv.group(G1).fixed_dev(k.d_table, k.max_coeffs, 0, d_scalars, n, d_out, st);
    else cv.group(G1).msm_dev(k.d_tau, d_scalars, n, d_out, st);
}
void require_fits(const Kzg& k, u64 n) {
    ZK_REQUIRE(n <= k.max_coeffs, "kzg: a polynomial of " + std::to_string(n) + " coefficients exceeds the " + std::to_string(k.max_coeffs) + " powers the handle holds");
}
// m openings -> what the two sums take: bases C_j | W_j | G1 (2m + 1 points) with scalars rho_j | rho_j z_j | (filled in by the host), and
// rho_j again for the sum over W alone.  A point at infinity (all zero: a legal value) is a term the sums cannot take: G1 with scalar zero
__global__ __launch_bounds__(256) void kzg_terms_kernel(const u32* __restrict__ open, u64 stride, u32 pw, u64 m, const u32* __restrict__ rho,
                                                        const u32* __restrict__ rz, const u32* __restrict__ gen, u32* __restrict__ bases,
                                                        u32* __restrict__ scalars, u32* __restrict__ w_scalars) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * m) return;
    const u64 j = t % m;
    const bool is_w = t >= m;
    const u32* p = open + j * stride + (is_w ? pw + 16 : 0);
    u32 any = 0;
    for (u32 i = 0; i < pw; ++i) any |= p[i];
    for (u32 i = 0; i < pw; ++i) bases[t * pw + i] = any ? p[i] : gen[i];
    for (int i = 0; i < 8; ++i) {
        const u32 s = is_w ? rz[j * 8 + i] : rho[j * 8 + i];
        scalars[t * 8 + i] = any ? s : 0u;
        if (is_w) w_scalars[j * 8 + i] = any ? rho[j * 8 + i] : 0u;
    }
    if (t == 0)
        for (u32 i = 0; i < pw; ++i) bases[2 * m * pw + i] = gen[i];
}
std::vector<u32> hex_words(const char* hex, size_t n_words) {          // a modulus as little-endian words
    std::vector<u32> w(n_words, 0);
    const size_t len = std::strlen(hex);
    for (size_t i = 0; i < len && i < 8 * n_words; ++i) {
        const char c = hex[len - 1 - i];
        const u32 d = c >= '0' && c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
        w[i / 8] |= d << (4 * (i % 8));
    }
    return w;
}
}  // namespace

Kzg* kzg_new(const Srs* srs, uint64_t max_coeffs) {
    ZK_REQUIRE(srs, "kzg: null powers-of-tau handle");
    const Curve& cv = *srs->curve;
    const u64 have = (2ull << srs->power) - 1;
    if (max_coeffs == 0) max_coeffs = have;
    ZK_REQUIRE(max_coeffs <= have, "kzg: " + std::to_string(max_coeffs) + " coefficients asked for, the file of power " + std::to_string(srs->power) + " holds " +
                                       std::to_string(have) + " powers in G1");
    hipStream_t st = cur_stream();
    const size_t B1 = cv.point_bytes(G1), B2 = cv.point_bytes(G2);
    auto k = std::make_unique<Kzg>();
    k->curve = &cv; k->power = srs->power; k->max_coeffs = max_coeffs;
    k->d_tau = pool_alloc(max_coeffs * B1 + 4);
    h2d_sync(k->d_tau, srs->file.data() + srs->off[2], max_coeffs * B1);
    if (max_coeffs < (1ull << 24) && !getenv("ZK_KZG_NO_TABLES")) {     // zk_groth16_setup_new's policy; the knob keeps the plain sums testable
        k->d_table = pool_alloc(cv.group(G1).fixed_table_bytes(max_coeffs));
        cv.group(G1).fixed_prepare_dev(k->d_tau, max_coeffs, k->d_table, st);
    }
    std::vector<u32> gen(cv.point_words(G1));
    cv.group(G1).generator_words(gen.data());
    k->d_gen1 = pool_alloc(B1);
    h2d_sync(k->d_gen1, gen.data(), B1);
    if (srs->power >= 1) {                                              // G2 || -tauG2[1]; a file of power 0 has no tau in G2: it commits, it cannot verify
        std::vector<u32> g2(2 * cv.point_words(G2));
        std::memcpy(g2.data(), srs->file.data() + srs->off[3], 2 * B2);
        const std::vector<u32> q = hex_words(cv.pairing().q_hex, cv.fq_words);
        for (int c = 2; c < 4; ++c) {                                   // y.c0, y.c1 of the second point: Montgomery words, -v = q - v
            u32* v = g2.data() + cv.point_words(G2) + c * cv.fq_words;
            u32 any = 0;
            for (u32 i = 0; i < cv.fq_words; ++i) any |= v[i];
            if (!any) continue;
            uint64_t br = 0;
            for (u32 i = 0; i < cv.fq_words; ++i) { const uint64_t d = (uint64_t)q[i] - v[i] - br; v[i] = (u32)d; br = (d >> 32) & 1; }
        }
        k->d_g2 = pool_alloc(2 * B2);
        h2d_sync(k->d_g2, g2.data(), 2 * B2);
    }
    ZK_HIP(hipStreamSynchronize(st));
    return k.release();
}

void kzg_divide_dev(const Curve& cv, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_q, uint64_t* d_y, hipStream_t st) {
    ZK_REQUIRE((d_coeffs || n == 0) && d_y, "kzg: null argument");
    cv.kzg().divide_dev((const u64*)d_coeffs, n, canon_words(cv, z, "z"), nullptr, (u64*)d_q, false, (u32*)d_y, st);
}

void kzg_lincomb_dev(const Curve& cv, const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, const uint64_t* gamma, uint64_t* d_out, hipStream_t st) {
    ZK_REQUIRE(d_polys && n && k >= 1, "kzg: no polynomials");
    const u32* g = canon_words(cv, gamma, "gamma");
    u64 n_max = 0;
    for (u32 i = 0; i < k; ++i) {
        ZK_REQUIRE(d_polys[i] || n[i] == 0, "kzg: null polynomial");
        ZK_REQUIRE((uintptr_t)d_polys[i] % 16 == 0, "kzg: coefficient vectors must be 16-byte aligned");
        n_max = std::max<u64>(n_max, n[i]);
    }
    if (!n_max) return;
    ZK_REQUIRE(d_out && (uintptr_t)d_out % 16 == 0, "kzg: null or misaligned output");
    DevBuf d_ptrs, d_lens;
    d_ptrs.reserve(8 * (size_t)k); d_lens.reserve(8 * (size_t)k);
    h2d_sync(d_ptrs.p, d_polys, 8 * (size_t)k);
    h2d_sync(d_lens.p, n, 8 * (size_t)k);
    cv.kzg().lincomb_dev((const u64* const*)d_ptrs.p, (const u64*)d_lens.p, k, n_max, g, (u64*)d_out, st);
}

void kzg_commit_dev(Kzg& k, const uint64_t* d_coeffs, uint64_t n, void* d_out, hipStream_t st) {
    ZK_REQUIRE((d_coeffs || n == 0) && d_out, "kzg: null argument");
    require_fits(k, n);
    DevBuf s;
    if (n) { s.reserve(n * 32); k.curve->groth16().fr_to_canon_dev((const u64*)d_coeffs, n, (u32*)s.p, st); }
    powers_sum_dev(k, s.p, n, d_out, st);
}

void kzg_commit_evals_dev(Kzg& k, const uint64_t* d_evals, uint32_t log_n, void* d_out, hipStream_t st) {
    const Curve& cv = *k.curve;
    ZK_REQUIRE(d_evals && d_out, "kzg: null argument");
    ZK_REQUIRE(log_n <= k.power && log_n < 32, "kzg: a domain of 2^" + std::to_string(log_n) + " exceeds the file's power " + std::to_string(k.power));
    const u64 n = 1ull << log_n;
    require_fits(k, n);
    if (!k.d_lagrange[log_n]) {                                         // L_i(tau) G1 = iNTT(tauG1[0, n))_i: the same omega and 1 / n as zk_fr_<curve>_ntt
        const size_t bytes = n * cv.point_bytes(G1);
        void* p = pool_alloc(bytes + 4);
        try {
            ZK_HIP(hipMemcpyAsync(p, k.d_tau, bytes, hipMemcpyDeviceToDevice, st));
            if (log_n) group_ntt_dev(cv, G1, p, (int)log_n, true, st);
        } catch (...) { pool_free(p); throw; }
        ZK_HIP(hipStreamSynchronize(st));                               // once per log_n: a later call on another stream finds the basis finished
        k.d_lagrange[log_n] = p;
    }
    DevBuf s;
    s.reserve(n * 32);
    cv.groth16().fr_to_canon_dev((const u64*)d_evals, n, (u32*)s.p, st);
    cv.group(G1).msm_dev(k.d_lagrange[log_n], s.p, n, d_out, st);
}

// d_table: the powers table of z when the caller has one (kzg_open_many_dev), or null
static void open_with_table(Kzg& k, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, const void* d_table, uint64_t* d_y_out, void* d_w_out, hipStream_t st) {
    const Curve& cv = *k.curve;
    ZK_REQUIRE((d_coeffs || n == 0) && d_y_out && d_w_out, "kzg: null argument");
    const u32* zw = canon_words(cv, z, "z");
    require_fits(k, n);
    const u64 nq = n > 1 ? n - 1 : 0;
    DevBuf q;
    if (nq) q.reserve(nq * 32);
    cv.kzg().divide_dev((const u64*)d_coeffs, n, zw, d_table, (u64*)q.p, true, (u32*)d_y_out, st);
    powers_sum_dev(k, q.p, nq, d_w_out, st);
}
void kzg_open_dev(Kzg& k, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_y_out, void* d_w_out, hipStream_t st) {
    open_with_table(k, d_coeffs, n, z, nullptr, d_y_out, d_w_out, st);
}

void kzg_open_many_dev(Kzg& k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* z, const uint64_t* gamma, uint64_t* d_ys_out, void* d_w_out,
                       hipStream_t st) {
    const Curve& cv = *k.curve;
    ZK_REQUIRE(d_polys && n && n_polys >= 1 && d_ys_out && d_w_out, "kzg: null argument");
    const u32* zw = canon_words(cv, z, "z");
    (void)canon_words(cv, gamma, "gamma");
    u64 n_max = 0;
    for (u32 i = 0; i < n_polys; ++i) { require_fits(k, n[i]); ZK_REQUIRE(d_polys[i] || n[i] == 0, "kzg: null polynomial"); n_max = std::max<u64>(n_max, n[i]); }
    DevBuf f, y, tab;                                                   // one square chain and one powers table of z for the k evaluations and the opening
    tab.reserve(cv.kzg().table_bytes());
    cv.kzg().table_dev(zw, tab.p, st);
    for (u32 i = 0; i < n_polys; ++i) cv.kzg().divide_dev((const u64*)d_polys[i], n[i], zw, tab.p, nullptr, false, (u32*)d_ys_out + 8 * (size_t)i, st);
    y.reserve(32);
    if (n_max) { f.reserve(n_max * 32); kzg_lincomb_dev(cv, d_polys, n, n_polys, gamma, (uint64_t*)f.p, st); }
    open_with_table(k, (const uint64_t*)f.p, n_max, z, tab.p, (uint64_t*)y.p, d_w_out, st);
}

void kzg_fold_commitments(Kzg& k, const void* commitments, uint32_t n, const uint64_t* gamma, void* out) {
    const Curve& cv = *k.curve;
    ZK_REQUIRE(commitments && out && n >= 1, "kzg: null argument");
    const u32* g = canon_words(cv, gamma, "gamma");
    const size_t B1 = cv.point_bytes(G1), pw = cv.point_words(G1);
    hipStream_t st = cur_stream();
    const FrHost F(cv);
    std::vector<u32> bases((size_t)n * pw), sc((size_t)n * 8, 0), gen(pw);
    cv.group(G1).generator_words(gen.data());
    u64 gm[4], acc[4], c[4];
    F.to_mont((const u64*)g, gm);
    std::memcpy(acc, F.one, 32);
    for (u32 i = 0; i < n; ++i) {                                       // gamma^i; a commitment at infinity is a term left out
        const u32* p = (const u32*)commitments + (size_t)i * pw;
        u32 any = 0;
        for (size_t j = 0; j < pw; ++j) any |= p[j];
        std::memcpy(&bases[(size_t)i * pw], any ? p : gen.data(), B1);
        if (any) { F.from_mont(acc, c); std::memcpy(&sc[(size_t)i * 8], c, 32); }
        F.mul(acc, gm, acc);
    }
    DevBuf d_b, d_s, d_o;
    d_b.reserve(n * B1); d_s.reserve((size_t)n * 32); d_o.reserve(B1 + 4);
    h2d_sync(d_b.p, bases.data(), n * B1);
    h2d_sync(d_s.p, sc.data(), (size_t)n * 32);
    cv.group(G1).msm_dev(d_b.p, d_s.p, n, d_o.p, st);
    std::vector<u32> r(pw + 1);
    d2h_sync(r.data(), d_o.p, B1 + 4);
    if (r[pw]) std::memset(r.data(), 0, B1);
    std::memcpy(out, r.data(), B1);
}

namespace {
// One randomised check of m openings under the weights d_rho: ZK_VERDICT_ACCEPTED, ZK_VERDICT_REJECTED, or the code of a malformed opening
// (C before W, the points before the scalars).  Synchronises.
int kzg_check(Kzg& k, const u32* d_open, u64 m, const u32* d_rho, hipStream_t st) {
    const Curve& cv = *k.curve;
    const PairingOps& po = cv.pairing();
    const size_t pw = cv.point_words(G1), B1 = 4 * pw, ow = 2 * pw + 16;
    DevBuf d_cls, d_rz, d_y, d_flag, d_sums;
    d_cls.reserve(128); d_rz.reserve(m * 32); d_y.reserve(m * 32); d_flag.reserve(m * 4); d_sums.reserve(2 * 36);
    po.points_check[G1](d_open, ow, m, 0, 0, d_cls.u(), st);
    po.points_check[G1](d_open + pw + 16, ow, m, 0, 0, d_cls.u() + 8, st);
    cv.kzg().weights_dev(d_open, ow, pw, m, d_rho, (u32*)d_rz.p, (u32*)d_y.p, (u32*)d_flag.p, st);
    cv.groth16().verify_sums_dev(d_rho, d_y.p, m, 1, d_sums.p, st);   // sum rho_j | sum rho_j y_j | how many y_j are not below r
    u64 cls[2][8];
    u32 sums[18];
    std::vector<u32> flag(m);
    d2h_sync(cls, d_cls.p, sizeof cls); d2h_sync(sums, d_sums.p, sizeof sums); d2h_sync(flag.data(), d_flag.p, m * 4);
    for (int g = 0; g < 2; ++g) {
        if (cls[g][2 * ZK_POINT_COORDINATE_RANGE] || cls[g][2 * ZK_POINT_NOT_ON_CURVE]) return -3;     // ZK_VERDICT_NOT_ON_CURVE
        if (cls[g][2 * ZK_POINT_NOT_IN_SUBGROUP]) return -4;                                           // ZK_VERDICT_NOT_IN_SUBGROUP
    }
    if (sums[17]) return -1;                                                                            // ZK_VERDICT_INPUT_NOT_CANONICAL
    for (u32 f : flag) if (f) return -1;
    // L = sum rho_j C_j + sum (rho_j z_j) W_j + (r - sum rho_j y_j) G1, R = sum rho_j W_j
    u32 neg[8], any = 0;
    for (int i = 0; i < 8; ++i) any |= sums[8 + i];
    uint64_t br = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t d = (uint64_t)cv.r[i] - sums[8 + i] - br; neg[i] = any ? (u32)d : 0u; br = (d >> 32) & 1; }
    DevBuf d_bases, d_sc, d_wsc, d_lr, d_gt;
    const size_t slot = B1 + 16;                                        // a sum's point and flag word, 16-byte aligned
    d_bases.reserve((2 * m + 1) * B1); d_sc.reserve((2 * m + 1) * 32); d_wsc.reserve(m * 32); d_lr.reserve(2 * slot); d_gt.reserve(cv.gt_bytes());
    hipLaunchKernelGGL(kzg_terms_kernel, dim3((unsigned)((2 * m + 255) / 256)), dim3(256), 0, st, d_open, (u64)ow, (u32)pw, m, d_rho, (const u32*)d_rz.p,
                       (const u32*)k.d_gen1, (u32*)d_bases.p, (u32*)d_sc.p, (u32*)d_wsc.p);
    ZK_HIP(hipGetLastError());
    h2d_sync((uint8_t*)d_sc.p + 2 * m * 32, neg, 32);
    uint8_t* lr = (uint8_t*)d_lr.p;
    cv.group(G1).msm_dev(d_bases.p, d_sc.p, 2 * m + 1, lr, st);
    cv.group(G1).msm_dev((const uint8_t*)d_bases.p + m * B1, d_wsc.p, m, lr + slot, st);
    u32 fl[2];
    d2h_sync(&fl[0], lr + B1, 4); d2h_sync(&fl[1], lr + slot + B1, 4);
    DevBuf d_pair;
    d_pair.reserve(2 * B1);
    for (int i = 0; i < 2; ++i) {
        if (fl[i]) ZK_HIP(hipMemsetAsync((uint8_t*)d_pair.p + i * B1, 0, B1, st));
        else ZK_HIP(hipMemcpyAsync((uint8_t*)d_pair.p + i * B1, lr + i * slot, B1, hipMemcpyDeviceToDevice, st));
    }
    pairing_product_dev(cv, d_pair.p, k.d_g2, 2, d_gt.p, 1, st);       // e(L, G2) e(R, -tau G2): two Miller loops, one final exponentiation
    std::vector<u32> gt(cv.gt_bytes() / 4);
    d2h_sync(gt.data(), d_gt.p, cv.gt_bytes());
    bool is_one = gt[0] == 1;
    for (size_t i = 1; i < gt.size(); ++i) is_one &= gt[i] == 0;
    return is_one ? 1 : 0;
}
}  // namespace

void kzg_verify_dev(Kzg& k, const void* d_openings, uint64_t m, const uint8_t* seed, bool locate, int* verdict, uint64_t* first_bad, hipStream_t st) {
    ZK_REQUIRE(verdict, "kzg verify: null argument");
    *verdict = 1;
    if (first_bad) *first_bad = m;
    if (!m) return;
    ZK_REQUIRE(d_openings, "kzg verify: null argument");
    ZK_REQUIRE(k.d_g2, "kzg verify: a file of power 0 holds no tau in G2");
    ZK_REQUIRE(m < (1ull << 28), "kzg verify: more than 2^28 openings in one batch");
    const size_t ow = 2 * k.curve->point_words(G1) + 16;
    const u32* op = (const u32*)d_openings;
    const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    DevBuf d_one, d_rho;
    d_one.reserve(32);
    h2d_sync(d_one.p, one, 32);
    if (m > 1) groth16_rho_dev(seed, m, d_rho, st, "kzg verify");
    const int v = kzg_check(k, op, m, m > 1 ? (const u32*)d_rho.p : (const u32*)d_one.p, st);
    if (v == 1) return;
    if (!locate) { *verdict = 0; return; }
    if (m == 1) { *verdict = v; if (first_bad) *first_bad = 0; return; }
    for (u64 j = 0; j < m; ++j) {                                       // one by one, weight 1: the first opening that is not accepted
        const int vj = kzg_check(k, op + j * ow, 1, (const u32*)d_one.p, st);
        if (vj != 1) { *verdict = vj; if (first_bad) *first_bad = j; return; }
    }
    throw Error("kzg verify: the batched check refused openings that all pass one by one");
}

void kzg_verify(Kzg& k, const void* openings, uint64_t m, const uint8_t* seed, bool locate, int* verdict, uint64_t* first_bad) {
    ZK_REQUIRE(verdict, "kzg verify: null argument");
    if (!m) { *verdict = 1; if (first_bad) *first_bad = 0; return; }
    ZK_REQUIRE(openings, "kzg verify: null argument");
    const size_t ob = 4 * (2 * k.curve->point_words(G1) + 16);
    DevBuf d;
    d.reserve(m * ob);
    h2d_sync(d.p, openings, m * ob);
    kzg_verify_dev(k, d.p, m, seed, locate, verdict, first_bad, cur_stream());
}

// ---- several polynomials at several points in one two-point proof -------------------------------------------------
void kzg_divide_acc_dev(const Curve& cv, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, const uint64_t* w, uint64_t* d_acc, uint64_t* d_y, hipStream_t st) {
    ZK_REQUIRE((d_coeffs || n == 0) && d_y && (d_acc || n <= 1), "kzg: null argument");
    const u32* zw = canon_words(cv, z, "z");
    cv.kzg().divide_acc_dev((const u64*)d_coeffs, n, zw, nullptr, canon_words(cv, w, "w"), (const u64*)d_acc, (u64*)d_acc, (u32*)d_y, st);
}

void kzg_interleave_dev(const Curve& cv, const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, uint64_t* d_out, hipStream_t st) {
    ZK_REQUIRE(d_polys && n && k >= 1, "kzg: no polynomials");
    ZK_REQUIRE(k <= 65536, "kzg: more than 65536 polynomials to interleave");
    u64 n_max = 0;
    for (u32 i = 0; i < k; ++i) {
        ZK_REQUIRE(d_polys[i] || n[i] == 0, "kzg: null polynomial");
        ZK_REQUIRE((uintptr_t)d_polys[i] % 16 == 0, "kzg: coefficient vectors must be 16-byte aligned");
        n_max = std::max<u64>(n_max, n[i]);
    }
    if (!n_max) return;
    ZK_REQUIRE(n_max < (1ull << 38) / k, "kzg: more than 2^38 interleaved coefficients");
    ZK_REQUIRE(d_out && (uintptr_t)d_out % 16 == 0, "kzg: null or misaligned output");
    DevBuf d_ptrs, d_lens;
    d_ptrs.reserve(8 * (size_t)k); d_lens.reserve(8 * (size_t)k);
    h2d_sync(d_ptrs.p, d_polys, 8 * (size_t)k);
    h2d_sync(d_lens.p, n, 8 * (size_t)k);
    cv.kzg().interleave_dev((const u64* const*)d_ptrs.p, (const u64*)d_lens.p, k, n_max, (u64*)d_out, st);
}

namespace {
// The scalar field on the host for the few values a proof's sets give: Montgomery values of fr_host.h, by value
using Fr = std::array<u64, 4>;
struct FrM {
    FrHost F;
    explicit FrM(const Curve& cv) : F(cv) {}
    Fr in(const u64* canon) const { Fr o; F.to_mont(canon, o.data()); return o; }
    Fr out(const Fr& a) const { Fr o; F.from_mont(a.data(), o.data()); return o; }
    Fr one() const { Fr o; std::memcpy(o.data(), F.one, 32); return o; }
    static Fr zero() { return Fr{0, 0, 0, 0}; }
    static bool is_zero(const Fr& a) { return !(a[0] | a[1] | a[2] | a[3]); }
    Fr mul(const Fr& a, const Fr& b) const { Fr o; F.mul(a.data(), b.data(), o.data()); return o; }
    Fr add(const Fr& a, const Fr& b) const { Fr o; F.add(a.data(), b.data(), o.data()); return o; }
    Fr neg(const Fr& a) const {
        if (is_zero(a)) return a;
        Fr o; u64 br = 0;
        for (int i = 0; i < 4; ++i) { const FrHost::u128 d = (FrHost::u128)F.p[i] - a[i] - br; o[i] = (u64)d; br = (u64)(d >> 64) & 1; }
        return o;
    }
    Fr sub(const Fr& a, const Fr& b) const { return add(a, neg(b)); }
    Fr inv(const Fr& a) const { Fr o; F.inv(a.data(), o.data()); return o; }
};
// The sets of one proof: S_i, a_s = 1 / prod_(s' != s) (s - s') for s in S_i, and T, their union in order of first appearance
struct MultiSets {
    std::vector<std::vector<Fr>> S, A;
    std::vector<Fr> T;
    std::vector<u32> t_of;                                              // per point, sets one after another: its index in T
};
// points: the sets one after another, 4 canonical words each.  -> 1, or the verdict of a malformed proof with its reason
int multi_sets(const Curve& cv, const FrM& M, const u64* points, const u32* sizes, u32 k, MultiSets& out, std::string& why) {
    if (k == 0) { why = "no polynomials"; return ZK_VERDICT_INPUT_COUNT; }
    for (u32 i = 0; i < k; ++i) {
        if (sizes[i] == 0) { why = "set " + std::to_string(i) + " is empty"; return ZK_VERDICT_INPUT_COUNT; }
        if (sizes[i] > ZK_KZG_MULTI_MAX_POINTS) {
            why = "set " + std::to_string(i) + " has " + std::to_string(sizes[i]) + " points, more than ZK_KZG_MULTI_MAX_POINTS (" + std::to_string(ZK_KZG_MULTI_MAX_POINTS) + ")";
            return ZK_VERDICT_INPUT_COUNT;
        }
    }
    size_t at = 0;
    for (u32 i = 0; i < k; ++i)
        for (u32 s = 0; s < sizes[i]; ++s, ++at)
            if (!cv.fr_canonical((const u32*)(points + 4 * at))) { why = "a point of set " + std::to_string(i) + " is not below the scalar field's modulus"; return ZK_VERDICT_INPUT_NOT_CANONICAL; }
    out.S.assign(k, {}); out.A.assign(k, {}); out.T.clear(); out.t_of.clear();
    at = 0;
    for (u32 i = 0; i < k; ++i) {
        for (u32 s = 0; s < sizes[i]; ++s, ++at) {
            const Fr p = M.in(points + 4 * at);
            for (const Fr& o : out.S[i])
                if (o == p) { why = "set " + std::to_string(i) + " repeats a point"; return ZK_VERDICT_INPUT_COUNT; }
            out.S[i].push_back(p);
            size_t t = 0;
            while (t < out.T.size() && !(out.T[t] == p)) ++t;
            if (t == out.T.size()) out.T.push_back(p);
            out.t_of.push_back((u32)t);
        }
        for (u32 s = 0; s < sizes[i]; ++s) {
            Fr d = M.one();
            for (u32 o = 0; o < sizes[i]; ++o)
                if (o != s) d = M.mul(d, M.sub(out.S[i][s], out.S[i][o]));
            out.A[i].push_back(M.inv(d));
        }
    }
    return 1;
}
bool multi_in_t(const MultiSets& s, const Fr& z) {
    for (const Fr& t : s.T) if (t == z) return true;
    return false;
}
// What both sides derive from the sets, the values, gamma and a z outside T: w_i = gamma^i Z_(T \ S_i)(z), Z_T(z), sum_i w_i r_i(z) with
// r_i(z) = sum_(s in S_i) y_s a_s prod_(s' != s) (z - s') (Lagrange: no interpolant is built)
struct MultiScalars { std::vector<Fr> w; Fr zt, wr; };
MultiScalars multi_scalars(const FrM& M, const MultiSets& s, const u64* values, const Fr& gamma, const Fr& z) {
    MultiScalars o;
    std::vector<Fr> dz;
    o.zt = M.one();
    for (const Fr& t : s.T) { dz.push_back(M.sub(z, t)); o.zt = M.mul(o.zt, dz.back()); }
    o.wr = FrM::zero();
    Fr g = M.one();
    size_t at = 0;
    for (size_t i = 0; i < s.S.size(); ++i) {
        const size_t ns = s.S[i].size();
        std::vector<bool> mine(s.T.size(), false);
        for (size_t j = 0; j < ns; ++j) mine[s.t_of[at + j]] = true;
        Fr rest = M.one();
        for (size_t t = 0; t < s.T.size(); ++t) if (!mine[t]) rest = M.mul(rest, dz[t]);
        o.w.push_back(M.mul(g, rest));
        Fr ri = FrM::zero();
        for (size_t j = 0; j < ns; ++j) {
            Fr term = M.mul(M.in(values + 4 * (at + j)), s.A[i][j]);
            for (size_t j2 = 0; j2 < ns; ++j2) if (j2 != j) term = M.mul(term, dz[s.t_of[at + j2]]);
            ri = M.add(ri, term);
        }
        o.wr = M.add(o.wr, M.mul(o.w.back(), ri));
        g = M.mul(g, gamma);
        at += ns;
    }
    return o;
}
}  // namespace

KzgMulti* kzg_multi_begin(Kzg& k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* points, const uint32_t* set_sizes,
                          uint64_t* d_values_out, hipStream_t st) {
    const Curve& cv = *k.curve;
    ZK_REQUIRE(n_polys >= 1, "kzg multi: no polynomials");
    ZK_REQUIRE(d_polys && n && points && set_sizes, "kzg multi: null argument");
    const FrM M(cv);
    MultiSets s;
    std::string why;
    if (multi_sets(cv, M, (const u64*)points, set_sizes, n_polys, s, why) != 1) throw Error("kzg multi: " + why);
    for (u32 i = 0; i < n_polys; ++i) {
        require_fits(k, n[i]);
        ZK_REQUIRE(d_polys[i] || n[i] == 0, "kzg multi: null polynomial");
        ZK_REQUIRE((uintptr_t)d_polys[i] % 16 == 0, "kzg: coefficient vectors must be 16-byte aligned");
    }
    auto m = std::make_unique<KzgMulti>();
    m->k = &k;
    m->polys.assign(d_polys, d_polys + n_polys); m->n.assign(n, n + n_polys); m->sizes.assign(set_sizes, set_sizes + n_polys);
    const size_t total = s.t_of.size(), tb = (cv.kzg().table_bytes() + 255) / 256 * 256;
    m->points.assign(points, points + 4 * total);
    m->table_of = s.t_of;
    m->d_tables = pool_alloc(s.T.size() * tb);
    for (size_t t = 0; t < s.T.size(); ++t) {                           // one powers table per distinct point, for this stage and the next
        const Fr c = M.out(s.T[t]);
        cv.kzg().table_dev((const u32*)c.data(), (uint8_t*)m->d_tables + t * tb, st);
    }
    DevBuf own;
    if (!d_values_out) { own.reserve(total * 32); d_values_out = (uint64_t*)own.p; }
    size_t at = 0;
    for (u32 i = 0; i < n_polys; ++i)
        for (u32 j = 0; j < set_sizes[i]; ++j, ++at)                    // phases 1 and 2 alone: nothing but the value is written
            cv.kzg().divide_dev((const u64*)d_polys[i], n[i], (const u32*)(points + 4 * at), (const uint8_t*)m->d_tables + s.t_of[at] * tb, nullptr, false,
                                (u32*)(d_values_out + 4 * at), st);
    m->values.resize(4 * total);
    d2h_sync(m->values.data(), d_values_out, total * 32);
    m->stage = 1;
    return m.release();
}

void kzg_multi_quotient(KzgMulti& m, const uint64_t* gamma, void* d_w1_out, hipStream_t st) {
    Kzg& k = *m.k;
    const Curve& cv = *k.curve;
    ZK_REQUIRE(m.stage == 1, "kzg multi: the quotient comes once, after begin");
    ZK_REQUIRE(d_w1_out, "kzg multi: null argument");
    const u32* gw = canon_words(cv, gamma, "gamma");
    const FrM M(cv);
    MultiSets s;
    std::string why;
    const u32 np = (u32)m.n.size();
    if (multi_sets(cv, M, (const u64*)m.points.data(), m.sizes.data(), np, s, why) != 1) throw Error("kzg multi: internal error: " + why);
    m.gamma.assign(gamma, gamma + 4);
    const size_t tb = (cv.kzg().table_bytes() + 255) / 256 * 256;
    u64 nq = 0;
    for (u32 i = 0; i < np; ++i)                                        // a polynomial of at most |S_i| coefficients is its own interpolant
        if (m.n[i] > m.sizes[i]) nq = std::max<u64>(nq, m.n[i] - 1);
    m.nq = nq;
    DevBuf y, sc;
    y.reserve(32);
    if (nq) {
        m.d_q = pool_alloc(nq * 32);
        ZK_HIP(hipMemsetAsync(m.d_q, 0, nq * 32, st));
        const Fr g = M.in((const u64*)gw);
        Fr gi = M.one();
        size_t at = 0;
        for (u32 i = 0; i < np; ++i) {                                  // q += gamma^i a_s (f_i - f_i(s)) / (X - s)
            for (u32 j = 0; j < m.sizes[i]; ++j) {
                if (m.n[i] <= m.sizes[i]) continue;
                const Fr w = M.out(M.mul(gi, s.A[i][j]));
                cv.kzg().divide_acc_dev((const u64*)m.polys[i], m.n[i], (const u32*)(m.points.data() + 4 * (at + j)), (const uint8_t*)m.d_tables + m.table_of[at + j] * tb,
                                        (const u32*)w.data(), (const u64*)m.d_q, (u64*)m.d_q, (u32*)y.p, st);
            }
            at += m.sizes[i];
            gi = M.mul(gi, g);
        }
        sc.reserve(nq * 32);
        cv.groth16().fr_to_canon_dev((const u64*)m.d_q, nq, (u32*)sc.p, st);
    }
    powers_sum_dev(k, sc.p, nq, d_w1_out, st);
    ZK_HIP(hipStreamSynchronize(st));
    m.stage = 2;
}

void kzg_multi_finish(KzgMulti& m, const uint64_t* z, void* d_w2_out, hipStream_t st) {
    Kzg& k = *m.k;
    const Curve& cv = *k.curve;
    ZK_REQUIRE(m.stage == 2, "kzg multi: finish comes once, after the quotient");
    ZK_REQUIRE(d_w2_out, "kzg multi: null argument");
    const u32* zw = canon_words(cv, z, "z");
    const FrM M(cv);
    MultiSets s;
    std::string why;
    const u32 np = (u32)m.n.size();
    if (multi_sets(cv, M, (const u64*)m.points.data(), m.sizes.data(), np, s, why) != 1) throw Error("kzg multi: internal error: " + why);
    const Fr zf = M.in((const u64*)zw);
    ZK_REQUIRE(!multi_in_t(s, zf), "kzg multi: z is one of the opening points");
    const MultiScalars ms = multi_scalars(M, s, (const u64*)m.values.data(), M.in((const u64*)m.gamma.data()), zf);
    u64 nl = m.nq;
    for (u32 i = 0; i < np; ++i) nl = std::max<u64>(nl, m.n[i]);
    nl = nl > 1 ? nl - 1 : 0;
    DevBuf l, tab, ys, sc;
    tab.reserve(cv.kzg().table_bytes());
    cv.kzg().table_dev(zw, tab.p, st);
    ys.reserve((size_t)(np + 1) * 32);
    if (nl) { l.reserve(nl * 32); ZK_HIP(hipMemsetAsync(l.p, 0, nl * 32, st)); }
    // L / (X - z) = sum_i w_i (f_i - f_i(z)) / (X - z) - Z_T(z) (q - q(z)) / (X - z): constant terms do not enter a quotient
    for (u32 i = 0; i < np; ++i) {
        const Fr w = M.out(ms.w[i]);
        cv.kzg().divide_acc_dev((const u64*)m.polys[i], m.n[i], zw, tab.p, (const u32*)w.data(), (const u64*)l.p, (u64*)l.p, (u32*)ys.p + 8 * (size_t)i, st);
    }
    const Fr nzt = M.out(M.neg(ms.zt));
    cv.kzg().divide_acc_dev((const u64*)m.d_q, m.nq, zw, tab.p, (const u32*)nzt.data(), (const u64*)l.p, (u64*)l.p, (u32*)ys.p + 8 * (size_t)np, st);
    std::vector<u64> yh(4 * (size_t)(np + 1));
    d2h_sync(yh.data(), ys.p, yh.size() * 8);
    Fr lz = M.neg(M.add(ms.wr, M.mul(ms.zt, M.in(yh.data() + 4 * (size_t)np))));      // L(z) from the evaluations the divisions left
    for (u32 i = 0; i < np; ++i) lz = M.add(lz, M.mul(ms.w[i], M.in(yh.data() + 4 * (size_t)i)));
    if (!FrM::is_zero(lz)) throw Error("kzg multi: internal error: L(z) is not zero, the quotient and the values do not belong together");
    if (nl) { sc.reserve(nl * 32); cv.groth16().fr_to_canon_dev((const u64*)l.p, nl, (u32*)sc.p, st); }
    powers_sum_dev(k, sc.p, nl, d_w2_out, st);
    ZK_HIP(hipStreamSynchronize(st));
    m.stage = 3;
}

namespace {
struct MultiProof {                                                     // one proof of the flat layout (include/zkgpu.h), copied out of the caller's bytes
    u32 k = 0;
    int code = 1;                                                       // 1, or the verdict its scalars alone give
    std::vector<u32> sizes, points1;                                    // points1: C_0 .. C_(k-1) | W1 | W2, point_words each
    std::vector<u64> points, values;
    u64 gamma[4], z[4];
    std::vector<u32> scalars;                                           // (k + 2) x 8 canonical words: w_i | -sum w_i r_i(z) | -Z_T(z)
};
// -> the bytes the proof takes.  A buffer that ends inside it is an error of the call
size_t multi_parse(const Curve& cv, const FrM& M, const uint8_t* p, size_t left, u64 index, MultiProof& o) {
    const size_t B1 = cv.point_bytes(G1), pw = cv.point_words(G1);
    const std::string who = "kzg multi verify: proof " + std::to_string(index);
    size_t at = 0;
    auto take = [&](void* dst, size_t nbytes) {
        ZK_REQUIRE(nbytes <= left - at, who + " ends after " + std::to_string(left) + " bytes, inside the proof");
        std::memcpy(dst, p + at, nbytes);
        at += nbytes;
    };
    u64 k64 = 0;
    take(&k64, 8);
    ZK_REQUIRE(k64 <= (left - at) / (B1 + 8) && k64 < (1ull << 32), who + " states " + std::to_string(k64) + " polynomials, more than its bytes hold");
    o.k = (u32)k64;
    o.points1.resize((size_t)(o.k + 2) * pw);
    take(o.points1.data(), o.k * B1);
    std::vector<u64> sz(o.k);
    take(sz.data(), 8 * (size_t)o.k);
    size_t total = 0;
    for (u64 v : sz) {
        ZK_REQUIRE(v <= (left - at) / 64, who + " states a set of " + std::to_string(v) + " points, more than its bytes hold");
        total += (size_t)v;
    }
    for (u64 v : sz) o.sizes.push_back((u32)std::min<u64>(v, 0xffffffffu));
    o.points.resize(4 * total); o.values.resize(4 * total);
    take(o.points.data(), 32 * total);
    take(o.values.data(), 32 * total);
    take(o.gamma, 32);
    take(o.z, 32);
    take(o.points1.data() + (size_t)o.k * pw, 2 * B1);
    // the scalars: counts, ranges, then the sets themselves
    MultiSets s;
    std::string why;
    o.code = multi_sets(cv, M, o.points.data(), o.sizes.data(), o.k, s, why);
    if (o.code != 1) return at;
    bool canon = cv.fr_canonical((const u32*)o.gamma) && cv.fr_canonical((const u32*)o.z);
    for (size_t i = 0; i < total; ++i) canon = canon && cv.fr_canonical((const u32*)(o.values.data() + 4 * i));
    if (!canon) { o.code = ZK_VERDICT_INPUT_NOT_CANONICAL; return at; }
    const Fr zf = M.in(o.z);
    if (multi_in_t(s, zf)) { o.code = ZK_VERDICT_INPUT_COUNT; return at; }
    const MultiScalars ms = multi_scalars(M, s, o.values.data(), M.in(o.gamma), zf);
    o.scalars.resize((size_t)(o.k + 2) * 8);
    for (u32 i = 0; i < o.k; ++i) { const Fr c = M.out(ms.w[i]); std::memcpy(&o.scalars[(size_t)i * 8], c.data(), 32); }
    const Fr nwr = M.out(M.neg(ms.wr)), nzt = M.out(M.neg(ms.zt));
    std::memcpy(&o.scalars[(size_t)o.k * 8], nwr.data(), 32);
    std::memcpy(&o.scalars[(size_t)(o.k + 1) * 8], nzt.data(), 32);
    return at;
}
// One randomised check of m well-formed proofs under the weights d_rho: the classes of every point, F_j = sum w_i C_i - [sum w_i r_i(z)] G1 -
// Z_T(z) W1 as one small sum per proof, then the openings (F_j, z_j, 0, W2_j) through kzg_check.  Synchronises.
int multi_check(Kzg& k, const MultiProof* pr, u64 m, const u32* d_rho, hipStream_t st) {
    const Curve& cv = *k.curve;
    const size_t pw = cv.point_words(G1), B1 = 4 * pw, ow = 2 * pw + 16, slot = B1 + 16;
    size_t n_pts = 0;
    for (u64 j = 0; j < m; ++j) n_pts += pr[j].k + 2;
    std::vector<u32> pts(n_pts * pw), bases(n_pts * pw), sc(n_pts * 8), gen(pw);
    cv.group(G1).generator_words(gen.data());
    size_t at = 0;
    for (u64 j = 0; j < m; ++j) {                                       // bases C_i | G1 | W1; a point at infinity is a term the sums cannot take: G1, scalar zero
        const MultiProof& p = pr[j];
        std::memcpy(&pts[at * pw], p.points1.data(), (size_t)(p.k + 2) * B1);
        for (u32 i = 0; i < p.k + 2; ++i) {
            const u32* src = i < p.k ? &p.points1[(size_t)i * pw] : i == p.k ? gen.data() : &p.points1[(size_t)p.k * pw];
            u32 any = 0;
            for (size_t w = 0; w < pw; ++w) any |= src[w];
            std::memcpy(&bases[(at + i) * pw], any ? src : gen.data(), B1);
            if (any) std::memcpy(&sc[(at + i) * 8], &p.scalars[(size_t)i * 8], 32);
            else std::memset(&sc[(at + i) * 8], 0, 32);
        }
        at += p.k + 2;
    }
    DevBuf d_pts, d_cls, d_bases, d_sc, d_f, d_open;
    d_pts.reserve(n_pts * B1); d_cls.reserve(64);
    h2d_sync(d_pts.p, pts.data(), n_pts * B1);
    cv.pairing().points_check[G1](d_pts.p, pw, n_pts, 0, 0, d_cls.u(), st);
    u64 cls[8];
    d2h_sync(cls, d_cls.p, sizeof cls);
    if (cls[2 * ZK_POINT_COORDINATE_RANGE] || cls[2 * ZK_POINT_NOT_ON_CURVE]) return ZK_VERDICT_NOT_ON_CURVE;
    if (cls[2 * ZK_POINT_NOT_IN_SUBGROUP]) return ZK_VERDICT_NOT_IN_SUBGROUP;
    d_bases.reserve(n_pts * B1); d_sc.reserve(n_pts * 32); d_f.reserve(m * slot); d_open.reserve(m * ow * 4);
    h2d_sync(d_bases.p, bases.data(), n_pts * B1);
    h2d_sync(d_sc.p, sc.data(), n_pts * 32);
    at = 0;
    for (u64 j = 0; j < m; ++j) {
        cv.group(G1).msm_dev((const uint8_t*)d_bases.p + at * B1, (const uint8_t*)d_sc.p + at * 32, pr[j].k + 2, (uint8_t*)d_f.p + j * slot, st);
        at += pr[j].k + 2;
    }
    std::vector<u32> f(m * slot / 4), open(m * ow, 0);
    d2h_sync(f.data(), d_f.p, m * slot);
    for (u64 j = 0; j < m; ++j) {                                       // F_j || z_j || 0 || W2_j
        u32* o = &open[j * ow];
        if (!f[j * slot / 4 + pw]) std::memcpy(o, &f[j * slot / 4], B1);
        std::memcpy(o + pw, pr[j].z, 32);
        std::memcpy(o + pw + 16, &pr[j].points1[(size_t)(pr[j].k + 1) * pw], B1);
    }
    h2d_sync(d_open.p, open.data(), m * ow * 4);
    return kzg_check(k, (const u32*)d_open.p, m, d_rho, st);
}
}  // namespace

void kzg_multi_verify(Kzg& k, const void* proofs, uint64_t bytes, uint64_t m, const uint8_t* seed, bool locate, int* verdict, uint64_t* first_bad, hipStream_t st) {
    ZK_REQUIRE(verdict, "kzg multi verify: null argument");
    const Curve& cv = *k.curve;
    *verdict = ZK_VERDICT_ACCEPTED;
    if (first_bad) *first_bad = m;
    ZK_REQUIRE(proofs || !bytes, "kzg multi verify: null argument");
    ZK_REQUIRE(m < (1ull << 20), "kzg multi verify: more than 2^20 proofs in one batch");
    const FrM M(cv);
    std::vector<MultiProof> pr(m);
    size_t at = 0;
    u64 good = m;                                                       // the proofs before the first whose scalars alone refuse it
    for (u64 j = 0; j < m; ++j) {
        at += multi_parse(cv, M, (const uint8_t*)proofs + at, bytes - at, j, pr[j]);
        if (pr[j].code != 1 && good == m) good = j;
    }
    ZK_REQUIRE(at == bytes, "kzg multi verify: " + std::to_string(bytes - at) + " bytes follow the last proof");
    if (!m) return;
    ZK_REQUIRE(k.d_g2, "kzg verify: a file of power 0 holds no tau in G2");
    if (good < m && !locate) { *verdict = ZK_VERDICT_REJECTED; return; }
    const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    DevBuf d_one, d_rho;
    d_one.reserve(32);
    h2d_sync(d_one.p, one, 32);
    int v = ZK_VERDICT_ACCEPTED;
    if (good) {
        if (good > 1) groth16_rho_dev(seed, good, d_rho, st, "kzg multi verify");
        v = multi_check(k, pr.data(), good, good > 1 ? (const u32*)d_rho.p : (const u32*)d_one.p, st);
    }
    if (v == ZK_VERDICT_ACCEPTED) {
        if (good == m) return;
        *verdict = pr[good].code;
        if (first_bad) *first_bad = good;
        return;
    }
    if (!locate) { *verdict = ZK_VERDICT_REJECTED; return; }
    if (good == 1) { *verdict = v; if (first_bad) *first_bad = 0; return; }
    for (u64 j = 0; j < good; ++j) {                                    // one by one, weight 1: the first proof that is not accepted
        const int vj = multi_check(k, &pr[j], 1, (const u32*)d_one.p, st);
        if (vj != ZK_VERDICT_ACCEPTED) { *verdict = vj; if (first_bad) *first_bad = j; return; }
    }
    throw Error("kzg multi verify: the batched check refused proofs that all pass one by one");
}

}  // namespace zk
