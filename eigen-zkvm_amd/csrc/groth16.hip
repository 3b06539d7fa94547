// Groth16 around the multi-scalar sums on gfx950 -- SURVEY.md 8(f)-2: `zkit groth16_prove`
// (groth16/src/api.rs:144-205 -> groth16.rs:88-96 -> bellman_ce::groth16::create_random_proof, third-party) with
// everything after witness generation resident on the device:
//   file formats     .r1cs (algebraic/src/r1cs_file.rs:50-118, 185-270), .wtns (algebraic/src/reader.rs:86-137),
//                    bellman's Parameters (groth16/src/api.rs:545-550; pairing_ce's uncompressed points, the
//                    encoding of groth16/test-vectors/verification_key*.bin)
//   circuit          algebraic/src/circom_circuit.rs:94-160 + the `input * 0 = 0` rows bellman's prover appends
//   row evaluations  one lane per row of the three CSR matrices                 (frntt_impl.hip.h)
//   quotient         7 transforms over Fr + the pointwise step                  (frntt_impl.hip.h)
//   h, l, a, b_g1, b_g2 sums and the final assembly through msm.hip
// This unit owns the scalar field's transforms, so the polynomial layer that runs them batched in their own layout lives here too
// (frpoly_impl.hip.h, DESIGN.md 3.20: zk_fr_<curve>_poly_mul_dev and its siblings; no protocol), and after it the three kernels of the
// PLONK prover (plonk_impl.hip.h, DESIGN.md 3.21: the fused numerator of the quotient, the gate check, the gather) and its R1CS import
// (plonk_r1cs_impl.hip.h, DESIGN.md 3.22: the compile rule on the host, the auxiliary variables of a witness on the device), and the
// fflonk prover's three numerators in one launch (fflonk_impl.hip.h), and the lookup argument of the PLONK prover
// (plonk_lookup_impl.hip.h, DESIGN.md 3.24: the running sum, the hash table and the count, the denominators, the summand, the quotient's term),
// the tagged form of that argument for several tables (plonk_lookup_tagged_impl.hip.h),
// the four numerators of the fflonk prover with lookups in one launch (fflonk_lookup_impl.hip.h),
// and the same four with the tag column of several tables in the lookup term (fflonk_lookup_tagged_impl.hip.h).
//   proof.json       groth16/src/json_utils.rs:305-315
// Key generation (`zkit groth16_setup`, groth16/src/api.rs:42-66) over the same circuit: groth16_keygen_impl.hip.h with a trapdoor,
// groth16_srs.hip.h from a powers-of-tau file (and the contributions to such a key).
// r and s are taken from the caller (the reference draws them from OsRng, api.rs:172); everything else is a
// function of (key, circuit, witness).
#include "curve.h"
#include "fr_host.h"
#include "r1cs_file.h"
#include "json_min.h"
#include "ceremony_host.h"
#include "../../include/zkgpu.h"
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <sys/random.h>

namespace zk {
namespace g16 {

// Lc, Row, R1cs: r1cs_file.h
struct PointVec { uint64_t n = 0; std::vector<u32> w; std::vector<char> inf; };   // canonical little-endian words
struct Params { PointVec vk[6]; PointVec ic, h, l, a, b_g1, b_g2; };               // vk: alpha_g1 beta_g1 beta_g2 gamma_g2 delta_g1 delta_g2

namespace {
struct Reader {
    const uint8_t* p; size_t n, o = 0; const char* what;
    void need(size_t k) const { if (k > n - o) throw std::runtime_error(std::string(what) + ": truncated file"); }
    uint32_t u32le() { need(4); uint32_t v; std::memcpy(&v, p + o, 4); o += 4; return v; }
    uint64_t u64le() { need(8); uint64_t v; std::memcpy(&v, p + o, 8); o += 8; return v; }
    uint32_t u32be() { need(4); uint32_t v = ((uint32_t)p[o] << 24) | ((uint32_t)p[o + 1] << 16) | ((uint32_t)p[o + 2] << 8) | p[o + 3]; o += 4; return v; }
    const uint8_t* take(size_t k) { need(k); const uint8_t* q = p + o; o += k; return q; }
};
}  // namespace

std::string words_to_dec(const u32* w, int n) {
    std::vector<u32> v(w, w + n);
    std::string out;
    while (true) {
        bool zero = true;
        uint64_t rem = 0;
        for (int i = n - 1; i >= 0; --i) {
            const uint64_t cur = (rem << 32) | v[i];
            v[i] = (u32)(cur / 1000000000u); rem = cur % 1000000000u;
            zero = zero && v[i] == 0;
        }
        char buf[16];
        if (zero) { snprintf(buf, sizeof buf, "%u", (unsigned)rem); out = buf + out; break; }
        snprintf(buf, sizeof buf, "%09u", (unsigned)rem); out = buf + out;
    }
    return out;
}

// r1cs_file.rs:185-270 from_reader (sections may come in any order; custom gates are not supported there either)
R1cs parse_r1cs(const uint8_t* b, size_t len, const Curve& cv) {
    Reader rd{b, len, 0, "r1cs"};
    if (std::memcmp(rd.take(4), "r1cs", 4) != 0) throw std::runtime_error("r1cs: Invalid magic number");
    if (rd.u32le() != 1) throw std::runtime_error("r1cs: Unsupported version");
    const uint32_t n_sec = rd.u32le();
    std::map<uint32_t, std::pair<size_t, uint64_t>> sec;
    for (uint32_t i = 0; i < n_sec; ++i) {
        const uint32_t t = rd.u32le(); const uint64_t sz = rd.u64le();
        sec[t] = {rd.o, sz};
        rd.take(sz);
    }
    if (!sec.count(1) || !sec.count(2)) throw std::runtime_error("r1cs: header or constraint section missing");
    Reader h{b + sec[1].first, (size_t)sec[1].second, 0, "r1cs header"};
    const uint32_t fs = h.u32le();
    if (sec[1].second != 32 + (uint64_t)fs) throw std::runtime_error("r1cs: Invalid header section size");
    if (fs != 32) throw std::runtime_error("r1cs: field size " + std::to_string(fs) + " is not 32 bytes");
    const uint8_t* prime = h.take(fs);
    if (std::memcmp(prime, cv.r, 32) != 0) throw std::runtime_error("r1cs: the file's prime is not the scalar field of the selected curve");
    R1cs rc;
    rc.n_wires = h.u32le(); rc.n_pub_out = h.u32le(); rc.n_pub_in = h.u32le(); rc.n_prv_in = h.u32le();
    (void)h.u64le();
    const uint32_t n_cons = h.u32le();
    Reader c{b + sec[2].first, (size_t)sec[2].second, 0, "r1cs constraints"};
    rc.rows.resize(n_cons);
    for (uint32_t i = 0; i < n_cons; ++i)
        for (int w = 0; w < 3; ++w) {
            const uint32_t nv = c.u32le();
            std::vector<std::pair<uint32_t, const uint8_t*>> terms(nv);
            for (uint32_t k = 0; k < nv; ++k) { terms[k].first = c.u32le(); terms[k].second = c.take(32); }
            std::stable_sort(terms.begin(), terms.end(), [](const auto& x, const auto& y) { return x.first < y.first; });   // r1cs_file.rs:83
            Lc& lc = rc.rows[i].lc[w];
            for (auto& t : terms) {
                u32 v[8]; std::memcpy(v, t.second, 32);
                if (!cv.fr_canonical(v)) throw std::runtime_error("r1cs: coefficient is not a canonical field element");   // Fr::from_repr
                lc.col.push_back(t.first); lc.coeff.insert(lc.coeff.end(), v, v + 8);
            }
        }
    return rc;
}

// pairing_ce's uncompressed encoding: big-endian canonical coordinates (G2: x.c1, x.c0, y.c1, y.c0), bit 6 of the
// first byte = infinity, bit 7 = compressed (rejected)
static void parse_points(Reader& rd, uint64_t count, int coord_bytes, bool g2, PointVec& out) {
    const int nc = g2 ? 4 : 2, cw = coord_bytes / 4;
    out.n = count; out.w.assign(count * nc * cw, 0); out.inf.assign(count, 0);
    for (uint64_t i = 0; i < count; ++i) {
        const uint8_t* p = rd.take((size_t)nc * coord_bytes);
        if (p[0] & 0x80) throw std::runtime_error("proving key: compressed point where an uncompressed one is expected");
        if (p[0] & 0x40) { out.inf[i] = 1; continue; }
        for (int c = 0; c < nc; ++c) {
            const int dst = g2 ? (c ^ 1) : c;                       // swap c1/c0 within x and within y
            const uint8_t* q = p + (size_t)c * coord_bytes;
            u32* w = out.w.data() + (i * nc + dst) * cw;
            for (int k = 0; k < cw; ++k) {
                const uint8_t* e = q + coord_bytes - 4 * (k + 1);
                w[k] = ((u32)e[0] << 24) | ((u32)e[1] << 16) | ((u32)e[2] << 8) | e[3];
            }
        }
    }
}
// bellman groth16 Parameters::read (vk, then h, l, a, b_g1, b_g2, each with a big-endian u32 count)
static Params parse_params(const uint8_t* b, size_t len, int coord_bytes) {
    Reader rd{b, len, 0, "proving key"};
    Params P;
    const bool g2[6] = {false, false, true, true, false, true};
    for (int i = 0; i < 6; ++i) parse_points(rd, 1, coord_bytes, g2[i], P.vk[i]);
    parse_points(rd, rd.u32be(), coord_bytes, false, P.ic);
    parse_points(rd, rd.u32be(), coord_bytes, false, P.h);
    parse_points(rd, rd.u32be(), coord_bytes, false, P.l);
    parse_points(rd, rd.u32be(), coord_bytes, false, P.a);
    parse_points(rd, rd.u32be(), coord_bytes, false, P.b_g1);
    parse_points(rd, rd.u32be(), coord_bytes, true, P.b_g2);
    if (rd.o != len) throw std::runtime_error("proving key: trailing bytes");
    return P;
}

// The circuit algebraic/src/circom_circuit.rs:94-160 synthesises from an .r1cs, as the prover and key generation both see it: the rows
// that are enforced, bellman's `input_i * 0 = 0` rows behind them, the domain, the three matrices in CSR form (coef: 8 x u32 canonical
// per term) and what the density trackers record.  All three matrices stay on the host for the object's life, 36 B a term (about 150 MB at
// 2^20 rows of circom shape); key generation adds a column-major copy of one matrix at a time on top of that.
struct Circuit {
    uint32_t ni = 0, n_aux = 0, n_wires = 0;
    int logm = 0;
    u64 m = 0, n_rows = 0;
    struct Csr { std::vector<u64> ptr; std::vector<u32> cols, coef; } mat[3];
    std::vector<char> a_aux, b_any;
    explicit Circuit(const R1cs& rc) {
        ni = 1 + rc.n_pub_out + rc.n_pub_in;
        n_wires = rc.n_wires;
        ZK_REQUIRE(n_wires >= ni, "groth16: r1cs header: fewer wires than public signals");
        n_aux = n_wires - ni;
        // circom_circuit.rs:143-157: rows with (A or B empty) and C empty are not enforced; prover.rs then appends
        // one `input_i * 0 = 0` row per input
        std::vector<const Row*> rows;
        for (const auto& r : rc.rows)
            if (!((r.lc[0].col.empty() || r.lc[1].col.empty()) && r.lc[2].col.empty())) rows.push_back(&r);
        n_rows = rows.size() + ni;
        logm = 0;
        while ((1ull << logm) < n_rows) ++logm;
        m = 1ull << logm;
        a_aux.assign(n_wires, 0); b_any.assign(n_wires, 0);
        for (int w = 0; w < 3; ++w) {
            auto& ptr = mat[w].ptr; auto& cols = mat[w].cols; auto& coef = mat[w].coef;
            ptr.push_back(0);
            for (const Row* r : rows) {
                const auto& lc = r->lc[w];
                for (size_t k = 0; k < lc.col.size(); ++k) {
                    ZK_REQUIRE(lc.col[k] < n_wires, "groth16: r1cs: wire index out of range");
                    cols.push_back(lc.col[k]);
                    coef.insert(coef.end(), lc.coeff.begin() + 8 * k, lc.coeff.begin() + 8 * k + 8);
                    if (w == 0 && lc.col[k] >= ni) a_aux[lc.col[k]] = 1;
                    if (w == 1) b_any[lc.col[k]] = 1;
                }
                ptr.push_back(cols.size());
            }
            for (uint32_t i = 0; i < ni; ++i) {
                if (w == 0) { cols.push_back(i); const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0}; coef.insert(coef.end(), one, one + 8); }
                ptr.push_back(cols.size());
            }
        }
    }
};

// one matrix by columns, the rows of a column in increasing order: ptr (n_wires + 1 entries), the rows, and the coefficients (8 canonical words) beside them
static void csc_of(const Circuit::Csr& M, u64 nw, std::vector<u64>& ptr, std::vector<u32>& rows, std::vector<u32>& coef) {
    const size_t nt = M.cols.size();
    ptr.assign(nw + 1, 0);
    for (u32 c : M.cols) ++ptr[c + 1];
    for (u64 j = 0; j < nw; ++j) ptr[j + 1] += ptr[j];
    std::vector<u64> cur(ptr.begin(), ptr.end() - 1);
    rows.resize(nt); coef.resize(nt * 8);
    for (u64 r = 0; r + 1 < M.ptr.size(); ++r)
        for (u64 k = M.ptr[r]; k < M.ptr[r + 1]; ++k) {
            const u64 at = cur[M.cols[k]]++;
            rows[at] = (u32)r;
            std::memcpy(&coef[at * 8], &M.coef[k * 8], 32);
        }
}
static void os_random(void* p, size_t n, const char* who) {
    size_t got = 0;
    while (got < n) {
        const ssize_t k = getrandom((uint8_t*)p + got, n - got, 0);
        if (k < 0 && errno == EINTR) continue;                              // a signal arrived before any byte: ask again
        ZK_REQUIRE(k > 0, std::string(who) + ": the operating system gave no random bytes");
        got += (size_t)k;
    }
}
// uniform in [1, r): bytes from the operating system, cut to the modulus' bit length, drawn again while out of range
static void draw_fr(const Curve& cv, u32* v, const char* who) {
    const u32 top_mask = (1u << (cv.r_bits() - 224)) - 1;
    for (;;) {
        os_random(v, 32, who);
        v[7] &= top_mask;
        u32 any = 0; for (int i = 0; i < 8; ++i) any |= v[i];
        if (any && cv.fr_canonical(v)) break;
    }
}

// canonical little-endian coordinates (nc x cw words per point) -> pairing_ce's uncompressed encoding: every coordinate big-endian, G2 as
// x.c1 || x.c0 || y.c1 || y.c0; the all-zero point (no finite point has x = y = 0) is infinity: bit 6 of byte 0, zeros behind it
__global__ __launch_bounds__(256) void points_to_be_kernel(const u32* __restrict__ pts, u64 n, int cw, int g2, u32* __restrict__ out) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const int nc = g2 ? 4 : 2;
    const u32* p = pts + i * nc * cw;
    u32* o = out + i * nc * cw;
    u32 any = 0;
    for (int c = 0; c < nc; ++c) {
        const u32* q = p + (g2 ? (c ^ 1) : c) * cw;
        for (int k = 0; k < cw; ++k) { const u32 v = q[cw - 1 - k]; any |= v; o[c * cw + k] = __builtin_bswap32(v); }
    }
    if (!any) o[0] = 0x40u;
}
static void points_to_be_dev(const u32* d_pts, u64 n, int cw, bool g2, u32* d_out, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(points_to_be_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_pts, n, cw, g2 ? 1 : 0, d_out);
    ZK_HIP(hipGetLastError());
}
// Parameters::write from the key's points on the device (affine, Montgomery): pts1 = [alpha beta delta | x (ic, then l) | h | a | b] over all wires,
// pts2 = [beta gamma delta | b].  Canonical coordinates, then pairing_ce's uncompressed big-endian bytes; points at infinity are dropped from
// a, b_g1, b_g2 (generator.rs), in wire order.  Consumes pts1 and pts2.
static void write_params(const Curve& cv, const Circuit& C, DevBuf& pts1, DevBuf& pts2, std::vector<uint8_t>& out, hipStream_t st) {
    const MsmOps& M = cv.msm();
    const u64 nh = C.m - 1, nw = C.n_wires, n1 = 3 + 3 * nw + nh, n2 = 3 + nw;
    const u64 o_x = 3, o_h = o_x + nw, o_a = o_h + nh, o_b = o_a + nw;
    const size_t P1 = cv.point_words(G1), P2 = cv.point_words(G2);
    DevBuf be1, be2;
    M.fq_mont_to_canon_dev(pts1.p, n1 * 2, st); M.fq_mont_to_canon_dev(pts2.p, n2 * 4, st);
    be1.reserve(n1 * P1 * 4); be2.reserve(n2 * P2 * 4);
    points_to_be_dev((const u32*)pts1.p, n1, (int)cv.fq_words, false, (u32*)be1.p, st);
    points_to_be_dev((const u32*)pts2.p, n2, (int)cv.fq_words, true, (u32*)be2.p, st);
    ZK_HIP(hipStreamSynchronize(st));
    pts1.release(); pts2.release();
    std::vector<uint8_t> h1(n1 * P1 * 4), h2(n2 * P2 * 4);
    d2h_sync(h1.data(), be1.p, h1.size()); d2h_sync(h2.data(), be2.p, h2.size());
    const size_t B1 = P1 * 4, B2 = P2 * 4;
    out.clear();
    out.reserve(h1.size() + h2.size() + 24);
    auto put = [&](const std::vector<uint8_t>& src, size_t pb, u64 at, u64 n) { out.insert(out.end(), src.begin() + at * pb, src.begin() + (at + n) * pb); };
    auto count = [&](u64 n) { ZK_REQUIRE(n < (1ull << 32), "groth16 keygen: a query has 2^32 points or more"); const uint8_t b[4] = {(uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n}; out.insert(out.end(), b, b + 4); };
    auto put_finite = [&](const std::vector<uint8_t>& src, size_t pb, u64 at, u64 n) {   // generator.rs drops the zero points of a, b_g1, b_g2
        const size_t at_count = out.size();
        count(0);
        u64 kept = 0;
        for (u64 i = 0; i < n; ++i)
            if (!(src[(at + i) * pb] & 0x40)) { put(src, pb, at + i, 1); ++kept; }
        const uint8_t b[4] = {(uint8_t)(kept >> 24), (uint8_t)(kept >> 16), (uint8_t)(kept >> 8), (uint8_t)kept};
        std::memcpy(&out[at_count], b, 4);
    };
    put(h1, B1, 0, 2); put(h2, B2, 0, 2); put(h1, B1, 2, 1); put(h2, B2, 2, 1);   // alpha_g1 beta_g1 beta_g2 gamma_g2 delta_g1 delta_g2
    count(C.ni); put(h1, B1, o_x, C.ni);
    count(nh); put(h1, B1, o_h, nh);
    count(C.n_aux); put(h1, B1, o_x + C.ni, C.n_aux);
    put_finite(h1, B1, o_a, nw);
    put_finite(h1, B1, o_b, nw);
    put_finite(h2, B2, 3, nw);
}
// overwrite host memory that held a secret; the compiler may not drop the stores
static void wipe(void* p, size_t n) { volatile uint8_t* q = (volatile uint8_t*)p; for (size_t i = 0; i < n; ++i) q[i] = 0; }
}  // namespace g16

namespace bn254fr {
#define ZK_FR29_FIELD 254
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#define FRN_S 28
#define FRN_ROOT 0xb639feb8u, 0x9632c7c5u, 0x0d0ff299u, 0x985ce340u, 0x01b0ecd8u, 0xb2dd8800u, 0x6d98ce29u, 0x1d69070du   // 7^((r-1)/2^28) * 2^256
#define FRN_FN(name) name
#define FRP_CURVE CURVE_BN254
#include "frntt_impl.hip.h"
#include "frpoly_impl.hip.h"
#include "plonk_impl.hip.h"
#include "plonk_lookup_impl.hip.h"
#include "plonk_lookup_tagged_impl.hip.h"
#include "fflonk_impl.hip.h"
#include "fflonk_lookup_impl.hip.h"
#include "fflonk_lookup_tagged_impl.hip.h"
#include "plonk_r1cs_impl.hip.h"
#include "plonk_next_impl.hip.h"
#include "groth16_impl.hip.h"
#include "groth16_keygen_impl.hip.h"
#include "verify_sums_impl.hip.h"
#include "key_check_srs_impl.hip.h"
#include "ceremony_impl.hip.h"
#undef FRN_S
#undef FRN_ROOT
#undef FRP_CURVE
}  // namespace bn254fr

namespace bls12381fr {
#define ZK_FR29_FIELD 381
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#define FRN_S 32
#define FRN_ROOT 0x5f0e466au, 0xb9b58d8cu, 0x1819d7ecu, 0x5b1b4c80u, 0x52a31e64u, 0x0af53ae3u, 0x19e9b27bu, 0x5bf3addau   // 7^((r-1)/2^32) * 2^256
#define FRP_CURVE CURVE_BLS12_381
#include "frntt_impl.hip.h"
#include "frpoly_impl.hip.h"
#include "plonk_impl.hip.h"
#include "plonk_lookup_impl.hip.h"
#include "plonk_lookup_tagged_impl.hip.h"
#include "fflonk_impl.hip.h"
#include "fflonk_lookup_impl.hip.h"
#include "fflonk_lookup_tagged_impl.hip.h"
#include "plonk_r1cs_impl.hip.h"
#include "plonk_next_impl.hip.h"
#include "groth16_impl.hip.h"
#include "groth16_keygen_impl.hip.h"
#include "verify_sums_impl.hip.h"
#include "key_check_srs_impl.hip.h"
#include "ceremony_impl.hip.h"
}  // namespace bls12381fr

const Groth16Ops& groth16_ops(CurveId id) {   // the table's slice of this unit (curve.h)
    static const Groth16Ops OPS[2] = {{bn254fr::ntt_dev, bn254fr::quotient_dev, bn254fr::setup_new, bn254fr::keygen_run, bn254fr::verify_sums_dev, bn254fr::kc_coef_dev, bn254fr::kc_coeffs_dev, bn254fr::powers_dev, bn254fr::fr_to_canon_dev},
                                      {bls12381fr::ntt_dev, bls12381fr::quotient_dev, bls12381fr::setup_new, bls12381fr::keygen_run, bls12381fr::verify_sums_dev,
                                       bls12381fr::kc_coef_dev, bls12381fr::kc_coeffs_dev, bls12381fr::powers_dev, bls12381fr::fr_to_canon_dev}};
    return OPS[id];
}

const FrPolyOps& frpoly_ops(CurveId id) {     // frpoly_impl.hip.h, per scalar field
#define ZK_FRPOLY_OPS(NS) {NS::fp_prefix_product_dev, NS::fp_batch_inverse_dev, NS::fp_pointwise_dev, NS::fp_powers_dev, NS::fp_terms_dev, NS::fp_grand_product_dev, \
                           NS::fp_poly_mul_dev, NS::fp_divmod_zh_dev, NS::fp_divide_zh_coset_dev, NS::fp_prefix_sum_dev}
    static const FrPolyOps OPS[2] = {ZK_FRPOLY_OPS(bn254fr), ZK_FRPOLY_OPS(bls12381fr)};
#undef ZK_FRPOLY_OPS
    return OPS[id];
}

const PlonkOps& plonk_ops(CurveId id) {       // plonk_impl.hip.h, plonk_r1cs_impl.hip.h and plonk_next_impl.hip.h, per scalar field
#define ZK_PLONK_OPS(NS) {NS::pk_quotient_dev, NS::pk_gate_check_dev, NS::pk_gather_dev, NS::pk_r1cs_new, NS::pk_r1cs_extend_dev, \
                          NS::pn_quotient_dev, NS::pn_gate_check_dev, NS::pn_r1cs_new, NS::pn_r1cs_extend_dev}
    static const PlonkOps OPS[2] = {ZK_PLONK_OPS(bn254fr), ZK_PLONK_OPS(bls12381fr)};
#undef ZK_PLONK_OPS
    return OPS[id];
}

const FflonkOps& fflonk_ops(CurveId id) {     // fflonk_impl.hip.h, per scalar field
    static const FflonkOps OPS[2] = {{bn254fr::ff_quotients_dev}, {bls12381fr::ff_quotients_dev}};
    return OPS[id];
}

const FflonkLookupOps& fflonk_lookup_ops(CurveId id) {   // fflonk_lookup_impl.hip.h and fflonk_lookup_tagged_impl.hip.h, per scalar field
    static const FflonkLookupOps OPS[2] = {{bn254fr::fl_quotients_dev, bn254fr::flt_quotients_dev}, {bls12381fr::fl_quotients_dev, bls12381fr::flt_quotients_dev}};
    return OPS[id];
}

const PlonkLookupOps& plonk_lookup_ops(CurveId id) {   // plonk_lookup_impl.hip.h and plonk_lookup_tagged_impl.hip.h, per scalar field
#define ZK_PLONK_LOOKUP_OPS(NS) {NS::pl_table_new, NS::pl_count_dev, NS::pl_terms_dev, NS::pl_summands_dev, NS::pl_quotient_dev, \
                                 NS::plt_table_new, NS::plt_count_dev, NS::plt_terms_dev, NS::plt_quotient_dev}
    static const PlonkLookupOps OPS[2] = {ZK_PLONK_LOOKUP_OPS(bn254fr), ZK_PLONK_LOOKUP_OPS(bls12381fr)};
#undef ZK_PLONK_LOOKUP_OPS
    return OPS[id];
}

Groth16Setup* groth16_setup_new(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len) {
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(r1cs && params, "groth16: null input");
    const g16::R1cs rc = g16::parse_r1cs((const uint8_t*)r1cs, r1cs_len, cv);
    const g16::Params pk = g16::parse_params((const uint8_t*)params, params_len, 4 * (int)cv.fq_words);
    const g16::Circuit cir(rc);
    return cv.groth16().setup_new(cv, cir, pk);
}

// ---- key generation ---------------------------------------------------------------------------------------------------------------
Groth16Key* groth16_keygen_new(const char* curve, const void* r1cs, size_t r1cs_len, const uint64_t* trapdoor) {
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(r1cs, "groth16 keygen: null input");
    const u32* mod = cv.r;
    const g16::R1cs rc = g16::parse_r1cs((const uint8_t*)r1cs, r1cs_len, cv);
    const g16::Circuit cir(rc);
    u32 td[40];
    struct TdGuard { u32* p; ~TdGuard() { g16::wipe(p, 160); } } td_guard{td};
    static const char* const names[5] = {"tau", "alpha", "beta", "gamma", "delta"};
    if (trapdoor) {
        std::memcpy(td, trapdoor, 160);
        for (int c = 0; c < 5; ++c) {
            u32* v = td + 8 * c;
            while (!cv.fr_canonical(v)) { uint64_t br = 0; for (int i = 0; i < 8; ++i) { const uint64_t d = (uint64_t)v[i] - mod[i] - br; v[i] = (u32)d; br = (d >> 32) & 1; } }   // below r
            u32 any = 0; for (int i = 0; i < 8; ++i) any |= v[i];
            ZK_REQUIRE(any, std::string("groth16 keygen: trapdoor component ") + names[c] + " is zero");
        }
    } else {
        for (int c = 0; c < 5; ++c) g16::draw_fr(cv, td + 8 * c, "groth16 keygen");
    }
    auto key = std::make_unique<Groth16Key>();
    key->curve = &cv;
    cv.groth16().keygen_run(cv, cir, td, key->params, key->ms);
    return key.release();
}

// json_utils.rs:285-303 serialize_vk over the head of the key's bytes (VerifyingKey::write: alpha_g1 beta_g1 beta_g2 gamma_g2 delta_g1
// delta_g2, count, ic); a coordinate is render_scalar_to_str's decimal string, or with to_hex the fixed-width 0x string of its repr
std::string groth16_keygen_vk_json(const Groth16Key& k, bool to_hex) {
    const size_t cb = 4 * k.curve->fq_words;
    const uint8_t* p = k.params.data();
    size_t o = 0;
    auto coord = [&](const uint8_t* q) {
        if (to_hex) { std::string s = "\"0x"; char b[3]; for (size_t i = 0; i < cb; ++i) { snprintf(b, sizeof b, "%02x", q[i]); s += b; } return s + "\""; }
        std::vector<u32> w(cb / 4);
        for (size_t i = 0; i < cb / 4; ++i) { const uint8_t* e = q + cb - 4 * (i + 1); w[i] = ((u32)e[0] << 24) | ((u32)e[1] << 16) | ((u32)e[2] << 8) | e[3]; }
        return "\"" + g16::words_to_dec(w.data(), (int)w.size()) + "\"";
    };
    auto g1 = [&] {
        ZK_REQUIRE(o + 2 * cb <= k.params.size(), "groth16 keygen: truncated key");
        std::vector<uint8_t> pt(p + o, p + o + 2 * cb); o += 2 * cb;
        if (pt[0] & 0x40) { pt.assign(2 * cb, 0); pt[2 * cb - 1] = 1; }          // CurveAffine::zero() is (0, 1)
        return "{\"x\":" + coord(pt.data()) + ",\"y\":" + coord(pt.data() + cb) + "}";
    };
    auto g2 = [&] {                                                              // file: x.c1 x.c0 y.c1 y.c0; json: [c0, c1]
        ZK_REQUIRE(o + 4 * cb <= k.params.size(), "groth16 keygen: truncated key");
        const uint8_t* q = p + o; o += 4 * cb;
        return "{\"x\":[" + coord(q + cb) + "," + coord(q) + "],\"y\":[" + coord(q + 3 * cb) + "," + coord(q + 2 * cb) + "]}";
    };
    std::string js = std::string("{\"protocol\":\"groth16\",\"curve\":\"") + k.curve->name + "\"";
    js += ",\"vk_alpha_1\":" + g1(); js += ",\"vk_beta_1\":" + g1(); js += ",\"vk_beta_2\":" + g2(); js += ",\"vk_gamma_2\":" + g2();
    js += ",\"vk_delta_1\":" + g1(); js += ",\"vk_delta_2\":" + g2();
    ZK_REQUIRE(o + 4 <= k.params.size(), "groth16 keygen: truncated key");
    const u32 n_ic = ((u32)p[o] << 24) | ((u32)p[o + 1] << 16) | ((u32)p[o + 2] << 8) | p[o + 3]; o += 4;
    js += ",\"IC\":[";
    for (u32 i = 0; i < n_ic; ++i) { if (i) js += ","; js += g1(); }
    return js + "]}";
}

// ---- groth16_key_check: a proving key against its circuit, before the prover takes it on faith -----------------------------------------
// The one input of groth16_prove that is read unchecked (parse_params is the reference's read_pk_from_file(path, checked = false)).
// Findings in a fixed order: section lengths against the circuit's; the class of every point (key_check_impl.hip.h: infinity --
// bellman's Parameters::read refuses it in EVERY section, although the reference's own setup writes it for a wire no row mentions --,
// a coordinate >= q, off the curve, outside the subgroup) with exact counts and first indices; the G1 and G2 copies of beta, delta and the
// b query tied together by pairings (b: one random linear combination sum rho_i b_g1_i against sum rho_i b_g2_i, rho_i of 128 bits; a
// wrong pair survives with probability 2^-128; on failure the smallest failing prefix by bisection); verification_key.json field by field.
// What is NOT checked: h, l, ic and a against the circuit's polynomials -- that takes tau in G2 or the trapdoor.  "key ok" means well
// formed and self-consistent; the functional test remains groth16_prove --verify.
namespace g16 {
// rho_i = the first 128 bits of ChaCha20(key = seed, counter = i, nonce = 0) as a 32 B canonical scalar
__device__ __forceinline__ u32 kc_rotl(u32 v, int c) { return (v << c) | (v >> (32 - c)); }
#define KC_QR(a, b, c, d) a += b; d = kc_rotl(d ^ a, 16); c += d; b = kc_rotl(b ^ c, 12); a += b; d = kc_rotl(d ^ a, 8); c += d; b = kc_rotl(b ^ c, 7);
__global__ __launch_bounds__(256) void kc_rho_kernel(const u32* __restrict__ seed, u64 n, u32* __restrict__ out) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, seed[0], seed[1], seed[2], seed[3], seed[4], seed[5], seed[6], seed[7],
                  (u32)i, (u32)(i >> 32), 0u, 0u};
    u32 x[16];
    for (int k = 0; k < 16; ++k) x[k] = in[k];
    for (int r = 0; r < 10; ++r) {
        KC_QR(x[0], x[4], x[8], x[12]) KC_QR(x[1], x[5], x[9], x[13]) KC_QR(x[2], x[6], x[10], x[14]) KC_QR(x[3], x[7], x[11], x[15])
        KC_QR(x[0], x[5], x[10], x[15]) KC_QR(x[1], x[6], x[11], x[12]) KC_QR(x[2], x[7], x[8], x[13]) KC_QR(x[3], x[4], x[9], x[14])
    }
    for (int k = 0; k < 4; ++k) { out[i * 8 + k] = x[k] + in[k]; out[i * 8 + 4 + k] = 0; }
}
#undef KC_QR

static const char* const KC_CLASS_NAMES[4] = {"infinity", "coordinate_range", "not_on_curve", "not_in_subgroup"};
struct KcSection { const char* name; Group g; const PointVec* pv; DevBuf d; };

}  // namespace g16

std::string groth16_key_check(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const char* vk_json,
                              const uint8_t* seed, uint32_t max_findings) {
    using namespace g16;
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(r1cs && params, "groth16: null input");
    const auto t0 = clk::now();
    const R1cs rc = parse_r1cs((const uint8_t*)r1cs, r1cs_len, cv);
    const Params pk = parse_params((const uint8_t*)params, params_len, 4 * (int)cv.fq_words);
    const Circuit cir(rc);
    const auto t1 = clk::now();
    const int cw = (int)cv.fq_words;
    const size_t P1 = cv.point_words(G1), P2 = cv.point_words(G2);
    hipStream_t st = cur_stream();
    const PairingOps& po = cv.pairing();

    u64 na = cir.ni, nb = 0;
    for (uint32_t j = cir.ni; j < cir.n_wires; ++j) na += cir.a_aux[j] ? 1 : 0;
    for (uint32_t j = 0; j < cir.n_wires; ++j) nb += cir.b_any[j] ? 1 : 0;

    std::string found[7], skipped;                          // by kind: size, the four classes, g1_g2_mismatch, vk_mismatch -- the report lists
    u64 counts[7] = {};                                     // them kind by kind, whatever the order they are met in
    auto add = [&](int kind, const std::string& body) {
        if (counts[kind]++ < max_findings) { if (!found[kind].empty()) found[kind] += ","; found[kind] += body; }
    };
    auto skip = [&](const char* section, const char* reason) {
        if (!skipped.empty()) skipped += ",";
        skipped += std::string("{\"check\":\"g1_g2_mismatch\",\"section\":\"") + section + "\",\"reason\":\"" + reason + "\"}";
    };
    // 1. sizes
    const struct { const char* name; u64 have, want; } sizes[6] = {{"ic", pk.ic.n, cir.ni}, {"h", pk.h.n, cir.m - 1}, {"l", pk.l.n, cir.n_aux},
                                                                  {"a", pk.a.n, na}, {"b_g1", pk.b_g1.n, nb}, {"b_g2", pk.b_g2.n, nb}};
    for (const auto& s : sizes)
        if (s.have != s.want)
            add(0, std::string("{\"kind\":\"size\",\"section\":\"") + s.name + "\",\"have\":" + std::to_string(s.have) + ",\"want\":" + std::to_string(s.want) + "}");
    // 2. every point's class: canonical words up, one launch per section, 8 words per section back
    static const char* const vk_names[6] = {"alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "delta_g1", "delta_g2"};
    static const Group vk_group[6] = {G1, G1, G2, G2, G1, G2};
    KcSection sec[12];
    for (int i = 0; i < 6; ++i) { sec[i].name = vk_names[i]; sec[i].g = vk_group[i]; sec[i].pv = &pk.vk[i]; }
    const PointVec* qs[6] = {&pk.ic, &pk.h, &pk.l, &pk.a, &pk.b_g1, &pk.b_g2};
    for (int i = 0; i < 6; ++i) { sec[6 + i].name = sizes[i].name; sec[6 + i].g = i == 5 ? G2 : G1; sec[6 + i].pv = qs[i]; }
    DevBuf d_res; d_res.reserve(12 * 8 * 8);
    u64 n_g1 = 0, n_g2 = 0;
    for (int i = 0; i < 12; ++i) {
        KcSection& s = sec[i];
        const size_t pw = s.g == G1 ? P1 : P2;
        s.d.reserve(s.pv->n * pw * 4 + 4);
        if (s.pv->n) h2d_sync(s.d.p, s.pv->w.data(), s.pv->n * pw * 4);
        po.points_check[s.g](s.d.p, pw, s.pv->n, 0, 1, d_res.u() + 8 * i, st);
        (s.g == G1 ? n_g1 : n_g2) += s.pv->n;
    }
    u64 res[12][8];
    d2h_sync(res, d_res.p, sizeof res);
    const auto t2 = clk::now();
    bool bad[12];
    for (int i = 0; i < 12; ++i) {
        bad[i] = false;
        for (int c = 0; c < 4; ++c) {
            if (!res[i][2 * c]) continue;
            bad[i] = true;
            add(1 + c, std::string("{\"kind\":\"") + KC_CLASS_NAMES[c] + "\",\"section\":\"" + sec[i].name + "\",\"n_points\":" + std::to_string(res[i][2 * c]) +
                           ",\"first_index\":" + std::to_string(res[i][2 * c + 1]) + "}");
        }
    }
    // 3. the G1 and G2 copies.  e(P1, G2) = e(G1, P2) as two reduced pairings compared (the product form e(P1, -G2) e(G1, P2) = 1 asks the same)
    DevBuf d_gen1, d_gen2, d_one, d_p1, d_p2, d_gt;
    d_gen1.reserve(P1 * 4); d_gen2.reserve(P2 * 4); d_one.reserve(8); d_p1.reserve(2 * P1 * 4); d_p2.reserve(2 * P2 * 4); d_gt.reserve(2 * cv.gt_bytes());
    const u64 one = 1;
    h2d_sync(d_one.p, &one, 8);
    cv.group(G1).mul_generator_dev(d_one.u(), 1, d_gen1.p, st);
    cv.group(G2).mul_generator_dev(d_one.u(), 1, d_gen2.p, st);
    double ms_sum = 0, ms_pair = 0;
    u64 pairs = 0;
    // d_a: a G1 point, d_b: a G2 point (Montgomery; all zero = infinity) -> e(a, G2) == e(G1, b)
    auto same_pair = [&](const void* d_a, const void* d_b) {
        const auto ta = clk::now();
        ZK_HIP(hipMemcpyAsync(d_p1.p, d_a, P1 * 4, hipMemcpyDeviceToDevice, st));
        ZK_HIP(hipMemcpyAsync((u32*)d_p1.p + P1, d_gen1.p, P1 * 4, hipMemcpyDeviceToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_p2.p, d_gen2.p, P2 * 4, hipMemcpyDeviceToDevice, st));
        ZK_HIP(hipMemcpyAsync((u32*)d_p2.p + P2, d_b, P2 * 4, hipMemcpyDeviceToDevice, st));
        pairing_dev(cv, d_p1.p, d_p2.p, 2, d_gt.p, 1, st);
        std::vector<uint8_t> gt(2 * cv.gt_bytes());
        d2h_sync(gt.data(), d_gt.p, gt.size());
        ms_pair += since(ta, clk::now());
        return std::memcmp(gt.data(), gt.data() + cv.gt_bytes(), cv.gt_bytes()) == 0;
    };
    const int pair_idx[2][2] = {{1, 2}, {4, 5}};
    static const char* const pair_name[2] = {"beta", "delta"};
    for (int k = 0; k < 2; ++k) {
        const int i1 = pair_idx[k][0], i2 = pair_idx[k][1];
        if (bad[i1] || bad[i2]) { skip(pair_name[k], "an invalid point"); continue; }
        cv.msm().fq_canon_to_mont_dev(sec[i1].d.p, P1 / cw, st); cv.msm().fq_canon_to_mont_dev(sec[i2].d.p, P2 / cw, st);
        ++pairs;
        if (!same_pair(sec[i1].d.p, sec[i2].d.p)) add(5, std::string("{\"kind\":\"g1_g2_mismatch\",\"section\":\"") + pair_name[k] + "\",\"first_index\":0}");
    }
    if (pk.b_g1.n != pk.b_g2.n) skip("b", "b_g1 and b_g2 differ in length");
    else if (bad[10] || bad[11]) skip("b", "an invalid point");
    else if (pk.b_g1.n) {
        const u64 n = pk.b_g1.n;
        pairs += n;
        uint8_t sd[32];
        if (seed) std::memcpy(sd, seed, 32);
        else {
            size_t got = 0;
            while (got < 32) {
                const ssize_t k = getrandom(sd + got, 32 - got, 0);
                if (k < 0 && errno == EINTR) continue;
                ZK_REQUIRE(k > 0, "groth16 key check: the operating system gave no random bytes");
                got += (size_t)k;
            }
        }
        DevBuf d_seed, d_rho, d_s1, d_s2;
        d_seed.reserve(32); d_rho.reserve(n * 32); d_s1.reserve(P1 * 4 + 4); d_s2.reserve(P2 * 4 + 4);
        h2d_sync(d_seed.p, sd, 32);
        wipe(sd, 32);
        hipLaunchKernelGGL(kc_rho_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const u32*)d_seed.p, n, (u32*)d_rho.p);
        ZK_HIP(hipGetLastError());
        cv.msm().fq_canon_to_mont_dev(sec[10].d.p, n * P1 / cw, st); cv.msm().fq_canon_to_mont_dev(sec[11].d.p, n * P2 / cw, st);
        // the first len elements: sum rho_i b_g1_i against sum rho_i b_g2_i
        auto prefix_ok = [&](u64 len) {
            const auto ta = clk::now();
            cv.group(G1).msm_dev(sec[10].d.p, d_rho.p, len, d_s1.p, st);
            cv.group(G2).msm_dev(sec[11].d.p, d_rho.p, len, d_s2.p, st);
            u32 f1 = 0, f2 = 0;
            d2h_sync(&f1, (const u32*)d_s1.p + P1, 4); d2h_sync(&f2, (const u32*)d_s2.p + P2, 4);
            ms_sum += since(ta, clk::now());
            if (f1 || f2) return f1 && f2;
            return same_pair(d_s1.p, d_s2.p);
        };
        if (!prefix_ok(n)) {
            u64 lo = 0, hi = n;                             // the prefix of lo elements holds, that of hi fails
            while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if (prefix_ok(mid)) lo = mid; else hi = mid; }
            add(5, "{\"kind\":\"g1_g2_mismatch\",\"section\":\"b\",\"first_index\":" + std::to_string(hi - 1) + "}");
        }
    }
    // 4. verification_key.json against the embedded copy
    if (vk_json) {
        const JVal js = JParser::parse(vk_json);
        static const struct { const char* field; int idx; bool g2, optional; } f[6] = {{"vk_alpha_1", 0, false, false}, {"vk_beta_1", 1, false, true}, {"vk_beta_2", 2, true, false},
                                                                                       {"vk_gamma_2", 3, true, false}, {"vk_delta_1", 4, false, true}, {"vk_delta_2", 5, true, false}};
        auto mismatch = [&](const std::string& field) { add(6, "{\"kind\":\"vk_mismatch\",\"field\":\"" + field + "\"}"); };
        // the file's points through the verifier's own readers (pairing.hip; a field that is no point is their error), word for word
        std::vector<u32> w(P2);
        auto differs = [&](const JVal& v, bool g2, const u32* want) {
            if (g2) groth16_json_g2(cv, v, w.data(), false); else groth16_json_g1(cv, v, w.data());
            return std::memcmp(w.data(), want, (g2 ? P2 : P1) * 4) != 0;
        };
        for (const auto& e : f) {
            if (e.optional && !js.find(e.field)) continue;
            if (differs(js.at(e.field), e.g2, pk.vk[e.idx].w.data())) mismatch(e.field);
        }
        const JVal& ic = js.at("IC");
        if (ic.kind != JVal::Arr || ic.size() != pk.ic.n) mismatch("IC");
        else
            for (size_t i = 0; i < ic.size(); ++i)
                if (differs(ic.at(i), false, pk.ic.w.data() + i * P1)) mismatch("IC[" + std::to_string(i) + "]");
    }
    ZK_HIP(hipStreamSynchronize(st));
    static const char* const kinds[7] = {"size", "infinity", "coordinate_range", "not_on_curve", "not_in_subgroup", "g1_g2_mismatch", "vk_mismatch"};
    std::string js = std::string("{\"curve\":\"") + cv.name + "\",\"n_wires\":" + std::to_string(cir.n_wires) + ",\"n_public\":" + std::to_string(cir.ni - 1) +
                     ",\"domain_log\":" + std::to_string(cir.logm) + ",\"sections\":{";
    for (int i = 0; i < 6; ++i) js += std::string(i ? "," : "") + "\"" + sizes[i].name + "\":" + std::to_string(sizes[i].have);
    js += "},\"checked\":{\"g1_points\":" + std::to_string(n_g1) + ",\"g2_points\":" + std::to_string(n_g2) + ",\"pairs\":" + std::to_string(pairs) + "},\"skipped\":[" + skipped + "],\"counts\":{";
    for (int k = 0; k < 7; ++k) js += std::string(k ? "," : "") + "\"" + kinds[k] + "\":" + std::to_string(counts[k]);
    js += "},\"findings\":[";
    bool first = true;
    for (int k = 0; k < 7; ++k)
        if (!found[k].empty()) { js += (first ? "" : ",") + found[k]; first = false; }
    js += "]";
    // ZK_KEY_CHECK_TIMING (read per call, as ZK_STARK_TIMING is; tools/key_check_time.py sets it): the host's milliseconds of reading (both files
    // and the circuit's three matrices), the point checks, the sums and the pairings
    if (const char* env = getenv("ZK_KEY_CHECK_TIMING"); env && *env && strcmp(env, "0")) {
        char buf[160];
        snprintf(buf, sizeof buf, ",\"timing_ms\":{\"parse\":%.3f,\"point_checks\":%.3f,\"sums\":%.3f,\"pairings\":%.3f}", since(t0, t1), since(t1, t2), ms_sum, ms_pair);
        js += buf;
    }
    return js + "}";
}

#include "groth16_srs.hip.h"
#include "key_check_srs.hip.h"
#include "groth16_ceremony.hip.h"
// the weights of the aggregate verification (pairing.hip): rho_dev for a caller outside this unit
void groth16_rho_dev(const uint8_t* seed, uint64_t n, DevBuf& d_rho, hipStream_t st, const char* who) { g16::rho_dev(seed, n, d_rho, st, who); }

// reader.rs:86-137 load_witness_from_bin_reader: header checks, then n x 32 B little-endian canonical values
void groth16_wtns_payload(const void* wtns, size_t len, const char* curve, uint64_t* offset, uint64_t* n) {
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    g16::Reader rd{(const uint8_t*)wtns, len, 0, "wtns"};
    if (std::memcmp(rd.take(4), "wtns", 4) != 0) throw std::runtime_error("wtns: Invalid file header");
    if (rd.u32le() > 2) throw std::runtime_error("wtns: unsupported file version");
    if (rd.u32le() != 2) throw std::runtime_error("wtns: invalid num sections");
    if (rd.u32le() != 1) throw std::runtime_error("wtns: invalid section type");
    if (rd.u64le() != 4 + 32 + 4) throw std::runtime_error("wtns: invalid section len");
    if (rd.u32le() != 32) throw std::runtime_error("wtns: invalid field byte size");
    if (std::memcmp(rd.take(32), cv.r, 32) != 0) throw std::runtime_error("wtns: invalid curve prime");
    const uint32_t cnt = rd.u32le();
    if (rd.u32le() != 2) throw std::runtime_error("wtns: invalid section type");
    if (rd.u64le() != (uint64_t)cnt * 32) throw std::runtime_error("wtns: Invalid witness section size");
    rd.need((size_t)cnt * 32);
    *offset = rd.o; *n = cnt;
}

}  // namespace zk
