// wtns_check: a witness against its R1CS on the device -- what `snarkjs wtns check` answers, for the three fields of this pipeline.
//
// The object is the FILE: every constraint of section 2 as written and in file order (the rows circom_circuit.rs:143-157 leaves
// unenforced included, bellman's appended `input_i * 0 = 0` rows not), and, over Goldilocks, every use of the compressor's four
// custom gates (sections 4 and 5) with the meaning compressor12_pil.rs gives them.  No proving key is involved.
//
//   constraint   one lane per row: the three row sums as the prover takes them (fr_rows_impl.hip.h frn_row_sum; over Goldilocks a
//                chain of gl::mul_add), a b against c in canonical form
//   one_wire     w[0] != 1, looked at by the lane of row 0
//   gates        one lane per use: the outputs the inputs force, against the witness; the first position that differs is the finding
//                (Poseidon12: every transition row j -> j + 1 is checked from the witness' own row j, as the PIL's row constraint does)
//
// Reporting.  Every wave writes the 64-bit ballot of its failing lanes into a mask of ceil(n / 64) words (one vector store from lane 0;
// every word is written, so the mask needs no clearing) and, only when the ballot is not 0, adds its popcount to a counter: a satisfied
// witness issues no atomic.  Only when a counter is not 0 the host reads that mask, takes the lowest `max_findings` indices and one small
// launch computes the values of exactly those rows or uses.  The counts are exact whatever max_findings is.
#include "curve.h"
#include "r1cs_check.h"
#include "r1cs_file.h"
#include "poseidon_gl_constants.h"
#include "../../tools/poseidong_round_constants.h"   // the 360 plain round constants + the 12 zeros of the output row
#include <algorithm>
#include <cstring>
#include <memory>
#include <sstream>

namespace zk {

namespace {

typedef unsigned long long ull;
inline dim3 grid1(u64 n) { return dim3((unsigned)std::max<u64>(1, (n + 255) / 256)); }

struct Csr3 { const u64* ptr[3]; const u32* cols[3]; const void* coef[3]; };

// one wave's part of (mask, count): every lane of the wave calls it; `i` is the lane's index, n the number of live indices
__device__ __forceinline__ void wave_mask(bool bad, u64 i, u64 n, ull* __restrict__ mask, ull* __restrict__ count) {
    const ull m = __ballot(bad);
    if ((threadIdx.x & 63u) != 0) return;
    if (i < n) mask[i >> 6] = m;                          // i is the wave's first index: the word exists when that index is live
    if (m != 0) atomicAdd(count, (ull)__popcll(m));
}

// res: [0] the number of failing rows, [1] w[0] != 1
template <class F>
__global__ __launch_bounds__(256) void r1cs_check_kernel(Csr3 m, const typename F::word_t* __restrict__ wit, const typename F::word_t* __restrict__ canon, u64 n,
                                                         ull* __restrict__ mask, ull* __restrict__ res) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < n) {
        typename F::val a, b, c;
        F::row_abc(m, wit, i, a, b, c);
        bad = F::differs(a, b, c);
    }
    wave_mask(bad, i, n, mask, res);
    if (i == 0) res[1] = F::one_wire_bad(canon) ? 1 : 0;
}
// canonical a, b, c of the listed rows: out[k] = a | b | c
template <class F>
__global__ __launch_bounds__(64) void r1cs_values_kernel(Csr3 m, const typename F::word_t* __restrict__ wit, const u32* __restrict__ rows, uint32_t n_list,
                                                        typename F::word_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n_list) return;
    typename F::val a, b, c;
    F::row_abc(m, wit, rows[k], a, b, c);
    F::store(a, out + (size_t)k * 3 * F::CW);
    F::store(b, out + (size_t)k * 3 * F::CW + F::CW);
    F::store(c, out + (size_t)k * 3 * F::CW + 2 * F::CW);
}

struct GlField {
    typedef u64 word_t;
    static constexpr int CW = 1, IW = 1;
    struct val { u64 v; };
    static __device__ __forceinline__ u64 row_sum(const u64* __restrict__ ptr, const u32* __restrict__ cols, const u64* __restrict__ coef, const u64* __restrict__ wit, u64 i) {
        u64 acc = 0;
        for (u64 k = ptr[i]; k < ptr[i + 1]; ++k) acc = gl::mul_add(coef[k], wit[cols[k]], acc);
        return acc;
    }
    static __device__ __forceinline__ void row_abc(const Csr3& m, const u64* __restrict__ wit, u64 i, val& a, val& b, val& c) {
        a.v = row_sum(m.ptr[0], m.cols[0], (const u64*)m.coef[0], wit, i);
        b.v = row_sum(m.ptr[1], m.cols[1], (const u64*)m.coef[1], wit, i);
        c.v = row_sum(m.ptr[2], m.cols[2], (const u64*)m.coef[2], wit, i);
    }
    static __device__ __forceinline__ bool differs(const val& a, const val& b, const val& c) { return gl::mul(a.v, b.v) != c.v; }
    static __device__ __forceinline__ void store(const val& x, u64* __restrict__ out) { *out = x.v; }
    static __device__ __forceinline__ bool one_wire_bad(const u64* __restrict__ canon) { return canon[0] != 1; }
    static void to_internal(const u64*, u64*, u64, hipStream_t) {}        // canonical words are the internal form
    static std::string dec(const u64* v) { return std::to_string(*v); }
};

// ---- the compressor's custom gates (Goldilocks) -----------------------------------------------------------------------------------
enum GateKind { G_CMULADD = 0, G_POSEIDON12, G_FFT4, G_EVPOL4, N_GATE_KINDS };
const char* const GATE_NAME[N_GATE_KINDS] = {"cmuladd", "poseidon12", "fft4", "evpol4"};
constexpr uint32_t GATE_SIGNALS[N_GATE_KINDS] = {12, 31 * 12, 24, 21};
// sig: [n][GATE_SIGNALS]; tmpl / ftab: FFT4's template per use and the 12 row coefficients of each template (plonk_setup.rs:572-617);
// pc: the 372 row constants, then the 144 words of the matrix (out[i] = sum_k M[k * 12 + i] state[k])
struct GateArgs { const u32* sig; u64 n; const u32* tmpl; const u64* ftab; const u64* pc; };

__device__ __forceinline__ bool gate_differs(u64 expected, u64 value, uint32_t at, uint32_t& pos, u64& e, u64& v) {
    if (expected == value) return false;
    pos = at; e = expected; v = value;
    return true;
}
__device__ __forceinline__ gl::f3 load3(const u64* __restrict__ wit, const u32* __restrict__ s) { return gl::f3{{wit[s[0]], wit[s[1]], wit[s[2]]}}; }

// -> the use fails; pos, e, v: the first position that differs, what the inputs force there and what the witness holds
template <int K>
__device__ __forceinline__ bool gate_eval(const GateArgs& g, const u64* __restrict__ wit, u64 use, uint32_t& pos, u64& e, u64& v) {
    const u32* __restrict__ s = g.sig + use * GATE_SIGNALS[K];
    if constexpr (K == G_CMULADD) {                      // s[9..12) = s[0..3) s[3..6) + s[6..9)
        const gl::f3 r = gl::f3_add(gl::f3_mul(load3(wit, s), load3(wit, s + 3)), load3(wit, s + 6));
        for (uint32_t t = 0; t < 3; ++t)
            if (gate_differs(r.v[t], wit[s[9 + t]], t, pos, e, v)) return true;
        return false;
    } else if constexpr (K == G_EVPOL4) {                // Horner over s[0..12) at x = s[15..18), started from s[12..15)
        const gl::f3 x = load3(wit, s + 15);
        gl::f3 r = load3(wit, s + 12);
#pragma unroll 1
        for (int c = 9; c >= 0; c -= 3) r = gl::f3_add(gl::f3_mul(r, x), load3(wit, s + c));
        for (uint32_t t = 0; t < 3; ++t)
            if (gate_differs(r.v[t], wit[s[18 + t]], t, pos, e, v)) return true;
        return false;
    } else if constexpr (K == G_FFT4) {                  // the second 12 signals from the first 12 and the template's row coefficients
        const u64* __restrict__ C = g.ftab + (u64)g.tmpl[use] * 12;
        u64 a[12];
#pragma unroll
        for (int t = 0; t < 12; ++t) a[t] = wit[s[t]];
        // per output element q: the signs of the a[3..), a[6..), a[9..) terms and their coefficients (the four-point form), then
        // the two-point form's pair (C[6] a[x4..) +- C[c5] a[x5..)); the template's type leaves one of the two forms all zero
        constexpr int S1[4] = {1, -1, 1, -1}, C2[4] = {2, 4, 2, 4}, S2[4] = {1, 1, -1, -1}, C3[4] = {3, 5, 3, 5}, S3[4] = {1, -1, -1, 1};
        constexpr int X4[4] = {0, 0, 6, 6}, X5[4] = {3, 3, 9, 9}, C5[4] = {7, 7, 8, 8}, S5[4] = {1, -1, 1, -1};
        bool bad = false;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                u64 r = gl::mul(C[0], a[c]);
                const u64 t1 = gl::mul(C[1], a[3 + c]), t2 = gl::mul(C[C2[q]], a[6 + c]), t3 = gl::mul(C[C3[q]], a[9 + c]);
                r = S1[q] > 0 ? gl::add(r, t1) : gl::sub(r, t1);
                r = S2[q] > 0 ? gl::add(r, t2) : gl::sub(r, t2);
                r = S3[q] > 0 ? gl::add(r, t3) : gl::sub(r, t3);
                r = gl::mul_add(C[6], a[X4[q] + c], r);
                const u64 t5 = gl::mul(C[C5[q]], a[X5[q] + c]);
                r = S5[q] > 0 ? gl::add(r, t5) : gl::sub(r, t5);
                if (!bad) bad = gate_differs(r, wit[s[12 + 3 * q + c]], (uint32_t)(3 * q + c), pos, e, v);
            }
        return bad;
    } else {                                             // Poseidon12: row j + 1 = MDS(sbox(row j + C_j)); position = 12 j + column
        const u64* __restrict__ RC = g.pc;
        const u64* __restrict__ M = g.pc + 372;
#pragma unroll 1
        for (uint32_t j = 0; j < 30; ++j) {
            const bool full = j < 4 || j >= 26;
            u64 st[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const u64 x = gl::add(wit[s[12 * j + i]], RC[12 * j + i]);
                if (i == 0 || full) { const u64 x2 = gl::sqr(x), x4 = gl::sqr(x2); st[i] = gl::mul(gl::mul(x4, x2), x); }
                else st[i] = x;
            }
#pragma unroll 1
            for (uint32_t i = 0; i < 12; ++i) {
                u64 r = 0;
#pragma unroll
                for (int k = 0; k < 12; ++k) r = gl::mul_add(M[k * 12 + i], st[k], r);
                if (gate_differs(r, wit[s[12 * (j + 1) + i]], 12 * j + i, pos, e, v)) return true;
            }
        }
        return false;
    }
}
template <int K>
__global__ __launch_bounds__(256) void gate_check_kernel(GateArgs g, const u64* __restrict__ wit, ull* __restrict__ mask, ull* __restrict__ count) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < g.n) { uint32_t pos; u64 e, v; bad = gate_eval<K>(g, wit, i, pos, e, v); }
    wave_mask(bad, i, g.n, mask, count);
}
// out[k] = position | expected | value of the listed uses
template <int K>
__global__ __launch_bounds__(64) void gate_detail_kernel(GateArgs g, const u64* __restrict__ wit, const u32* __restrict__ list, uint32_t n_list, u64* __restrict__ out) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n_list) return;
    uint32_t pos = 0; u64 e = 0, v = 0;
    gate_eval<K>(g, wit, list[k], pos, e, v);
    out[3 * (size_t)k] = pos; out[3 * (size_t)k + 1] = e; out[3 * (size_t)k + 2] = v;
}

// the lowest `limit` set bits of a mask over n indices
std::vector<u32> lowest_set(const std::vector<ull>& mask, u64 n, uint32_t limit) {
    std::vector<u32> out;
    for (size_t w = 0; w < mask.size() && out.size() < limit; ++w) {
        ull m = mask[w];
        if (w == mask.size() - 1 && (n & 63)) m &= (1ull << (n & 63)) - 1;   // (lanes past n voted `false`; the cut is belt and braces)
        while (m && out.size() < limit) { out.push_back((u32)(w * 64 + (size_t)__builtin_ctzll(m))); m &= m - 1; }
    }
    return out;
}
// count words -> the mask when there is something in it -> the lowest failing indices
std::vector<u32> read_failing(const DevBuf& d_mask, u64 n, u64 n_failing, uint32_t limit) {
    if (!n_failing || !limit) return {};
    std::vector<ull> mask((n + 63) / 64);
    d2h_sync(mask.data(), d_mask.p, mask.size() * 8);
    return lowest_set(mask, n, limit);
}

u64 hmulp(u64 a, u64 b) { return gl::hmul(a, b); }

// the uses of section 5, sorted by kind; template names resolve as compressor12 setup resolves them (plonk_setup.rs:102-158)
struct Gates {
    struct Kind { std::vector<u32> sig, use_id, tmpl; DevBuf d_sig, d_tmpl, d_mask; u64 n = 0; } kind[N_GATE_KINDS];
    DevBuf d_ftab, d_pc, d_count;
    u64 n_uses = 0;

    Gates(const c12::R1csGL& rc) {
        constexpr u64 NO_GATE = ~0ull;
        u64 id_of[N_GATE_KINDS] = {NO_GATE, NO_GATE, NO_GATE, NO_GATE};
        std::map<u64, uint32_t> fft_tmpl;
        std::vector<u64> ftab;
        for (size_t i = 0; i < rc.gates.size(); ++i) {
            const c12::CustomGate& c = rc.gates[i];
            if (c.name == "FFT4") {
                ZK_REQUIRE(c.params.size() == 4, "r1cs check: FFT4 takes 4 parameters");
                ZK_REQUIRE(c.params[3] == 2 || c.params[3] == 4, "r1cs check: invalid FFT4 type: " + std::to_string(c.params[3]));
                const u64 first_w = c.params[0], inc_w = c.params[1], scale = c.params[2], first_w2 = hmulp(first_w, first_w);
                u64 R[12] = {};
                if (c.params[3] == 4) {
                    R[0] = scale; R[1] = hmulp(scale, first_w2); R[2] = hmulp(scale, first_w); R[3] = hmulp(R[2], first_w2);
                    R[4] = hmulp(R[2], inc_w); R[5] = hmulp(R[3], inc_w);
                } else {
                    R[6] = scale; R[7] = hmulp(scale, first_w); R[8] = hmulp(R[7], inc_w);
                }
                fft_tmpl[i] = (uint32_t)(ftab.size() / 12);
                ftab.insert(ftab.end(), R, R + 12);
                continue;
            }
            ZK_REQUIRE(c.name == "CMulAdd" || c.name == "Poseidon12" || c.name == "EvPol4", "r1cs check: Invalid custom gate " + c.name);
            ZK_REQUIRE(c.params.empty(), "r1cs check: " + c.name + " takes no parameter");
            id_of[c.name == "CMulAdd" ? G_CMULADD : c.name == "Poseidon12" ? G_POSEIDON12 : G_EVPOL4] = i;
        }
        n_uses = rc.uses.size();
        ZK_REQUIRE(n_uses < (1ull << 32), "r1cs check: more than 2^32 custom-gate uses");
        for (size_t ui = 0; ui < rc.uses.size(); ++ui) {
            const c12::CustomUse& u = rc.uses[ui];
            int k;
            if (u.id == id_of[G_POSEIDON12]) { k = G_POSEIDON12; ZK_REQUIRE(u.signals.size() == 31 * 12, "r1cs check: a Poseidon12 use has " + std::to_string(u.signals.size()) + " signals, not 372"); }
            else if (u.id == id_of[G_CMULADD]) { k = G_CMULADD; ZK_REQUIRE(u.signals.size() >= 12, "r1cs check: a CMulAdd use has fewer than 12 signals"); }
            else if (fft_tmpl.count(u.id)) { k = G_FFT4; ZK_REQUIRE(u.signals.size() >= 24, "r1cs check: an FFT4 use has fewer than 24 signals"); }
            else if (u.id == id_of[G_EVPOL4]) { k = G_EVPOL4; ZK_REQUIRE(u.signals.size() >= 21, "r1cs check: an EvPol4 use has fewer than 21 signals"); }
            else throw Error("r1cs check: Custom gate not defined " + std::to_string(u.id));
            Kind& K = kind[k];
            for (uint32_t t = 0; t < GATE_SIGNALS[k]; ++t) {
                ZK_REQUIRE(u.signals[t] < rc.n_wires, "r1cs check: wire index out of range in a custom gate");
                K.sig.push_back((u32)u.signals[t]);
            }
            K.use_id.push_back((u32)ui);
            if (k == G_FFT4) K.tmpl.push_back(fft_tmpl[u.id]);
            ++K.n;
        }
        auto up = [](DevBuf& d, const void* h, size_t bytes) { d.reserve(std::max<size_t>(8, bytes)); if (bytes) h2d_sync(d.p, h, bytes); };
        for (Kind& K : kind) {
            up(K.d_sig, K.sig.data(), K.sig.size() * 4);
            up(K.d_tmpl, K.tmpl.data(), K.tmpl.size() * 4);
            K.d_mask.reserve(std::max<size_t>(8, (K.n + 63) / 64 * 8));
        }
        up(d_ftab, ftab.data(), ftab.size() * 8);
        std::vector<u64> pc(POSEIDONG_C, POSEIDONG_C + 372);
        pc.insert(pc.end(), ZK_POSEIDON_M, ZK_POSEIDON_M + 144);
        up(d_pc, pc.data(), pc.size() * 8);
        d_count.reserve(N_GATE_KINDS * 8);
    }

    GateArgs args(int k) const { return GateArgs{(const u32*)kind[k].d_sig.p, kind[k].n, (const u32*)kind[k].d_tmpl.p, (const u64*)d_ftab.p, (const u64*)d_pc.p}; }

    // -> the counts of failing uses per kind; appends the findings to `o`
    void run(const u64* d_wit, uint32_t max_findings, hipStream_t st, u64 n_failing[N_GATE_KINDS], std::ostringstream& o, bool& any) {
        ZK_HIP(hipMemsetAsync(d_count.p, 0, N_GATE_KINDS * 8, st));
        ull* cnt = (ull*)d_count.p;
        if (kind[G_CMULADD].n) hipLaunchKernelGGL(gate_check_kernel<G_CMULADD>, grid1(kind[G_CMULADD].n), dim3(256), 0, st, args(G_CMULADD), d_wit, (ull*)kind[G_CMULADD].d_mask.p, cnt + G_CMULADD);
        if (kind[G_POSEIDON12].n) hipLaunchKernelGGL(gate_check_kernel<G_POSEIDON12>, grid1(kind[G_POSEIDON12].n), dim3(256), 0, st, args(G_POSEIDON12), d_wit, (ull*)kind[G_POSEIDON12].d_mask.p, cnt + G_POSEIDON12);
        if (kind[G_FFT4].n) hipLaunchKernelGGL(gate_check_kernel<G_FFT4>, grid1(kind[G_FFT4].n), dim3(256), 0, st, args(G_FFT4), d_wit, (ull*)kind[G_FFT4].d_mask.p, cnt + G_FFT4);
        if (kind[G_EVPOL4].n) hipLaunchKernelGGL(gate_check_kernel<G_EVPOL4>, grid1(kind[G_EVPOL4].n), dim3(256), 0, st, args(G_EVPOL4), d_wit, (ull*)kind[G_EVPOL4].d_mask.p, cnt + G_EVPOL4);
        ZK_HIP(hipGetLastError());
        d2h_sync(n_failing, d_count.p, N_GATE_KINDS * 8);
        for (int k = 0; k < N_GATE_KINDS; ++k) {
            const Kind& K = kind[k];
            const std::vector<u32> list = read_failing(K.d_mask, K.n, n_failing[k], max_findings);
            if (list.empty()) continue;
            const uint32_t nl = (uint32_t)list.size();
            DevBuf d_list, d_out;
            d_list.reserve(nl * 4); d_out.reserve((size_t)nl * 24);
            h2d_sync(d_list.p, list.data(), nl * 4);
            const dim3 g((nl + 63) / 64), b(64);
            const GateArgs a = args(k);
            if (k == G_CMULADD) hipLaunchKernelGGL(gate_detail_kernel<G_CMULADD>, g, b, 0, st, a, d_wit, (const u32*)d_list.p, nl, d_out.u());
            else if (k == G_POSEIDON12) hipLaunchKernelGGL(gate_detail_kernel<G_POSEIDON12>, g, b, 0, st, a, d_wit, (const u32*)d_list.p, nl, d_out.u());
            else if (k == G_FFT4) hipLaunchKernelGGL(gate_detail_kernel<G_FFT4>, g, b, 0, st, a, d_wit, (const u32*)d_list.p, nl, d_out.u());
            else hipLaunchKernelGGL(gate_detail_kernel<G_EVPOL4>, g, b, 0, st, a, d_wit, (const u32*)d_list.p, nl, d_out.u());
            ZK_HIP(hipGetLastError());
            std::vector<u64> det(3 * (size_t)nl);
            d2h_sync(det.data(), d_out.p, det.size() * 8);
            static const uint32_t OUT0[N_GATE_KINDS] = {9, 12, 12, 18};  // the signal a position 0 names
            for (uint32_t t = 0; t < nl; ++t) {
                const u64 pos = det[3 * t];
                if (any) o << ","; any = true;
                o << "{\"kind\":\"" << GATE_NAME[k] << "\",\"use\":" << K.use_id[list[t]];
                if (k == G_POSEIDON12) o << ",\"row\":" << pos / 12 << ",\"column\":" << pos % 12;
                else o << ",\"position\":" << pos;
                o << ",\"wire\":" << K.sig[(size_t)list[t] * GATE_SIGNALS[k] + OUT0[k] + pos] << ",\"expected\":\"" << det[3 * t + 1] << "\",\"value\":\"" << det[3 * t + 2] << "\"}";
            }
        }
    }
};

}  // namespace

struct R1csCheck {
    std::string field;
    uint32_t n_wires = 0, n_public = 0;
    u64 n_cons = 0, n_uses = 0;
    size_t value_bytes = 0;
    virtual ~R1csCheck() {}
    virtual bool canonical(const void* v) const = 0;
    virtual std::string run(const void* d_witness, uint32_t max_findings, hipStream_t st) = 0;
};

namespace {

template <class F>
struct Checker final : R1csCheck {
    typedef typename F::word_t word_t;
    // the three matrices in CSR form: on the host with canonical coefficients (the `wires` of a finding), on the device in internal form
    std::vector<u64> ptr[3];
    std::vector<u32> cols[3];
    std::vector<word_t> coef[3];
    DevBuf d_ptr[3], d_cols[3], d_coef[3], d_mask, d_res;
    std::unique_ptr<Gates> gates;
    const Curve* curve = nullptr;                                         // the scalar fields; null over Goldilocks

    bool canonical(const void* v) const override {
        if (curve) return curve->fr_canonical((const u32*)v);
        u64 x; std::memcpy(&x, v, 8); return x < GL_P;
    }
    // after the matrices are filled on the host
    void upload() {
        hipStream_t st = cur_stream();
        for (int w = 0; w < 3; ++w) {
            d_ptr[w].reserve(ptr[w].size() * 8); d_cols[w].reserve(cols[w].size() * 4 + 4); d_coef[w].reserve(cols[w].size() * F::IW * sizeof(word_t) + 8);
            h2d_sync(d_ptr[w].p, ptr[w].data(), ptr[w].size() * 8);
            if (cols[w].empty()) continue;
            h2d_sync(d_cols[w].p, cols[w].data(), cols[w].size() * 4);
            if (F::IW == F::CW) { h2d_sync(d_coef[w].p, coef[w].data(), coef[w].size() * sizeof(word_t)); continue; }
            DevBuf raw; raw.reserve(coef[w].size() * sizeof(word_t));
            h2d_sync(raw.p, coef[w].data(), coef[w].size() * sizeof(word_t));
            F::to_internal((const word_t*)raw.p, (word_t*)d_coef[w].p, cols[w].size(), st);
            ZK_HIP(hipStreamSynchronize(st));
        }
        d_mask.reserve(std::max<size_t>(8, (n_cons + 63) / 64 * 8));
        d_res.reserve(16);
    }
    Csr3 csr() const {
        Csr3 m;
        for (int w = 0; w < 3; ++w) { m.ptr[w] = (const u64*)d_ptr[w].p; m.cols[w] = (const u32*)d_cols[w].p; m.coef[w] = d_coef[w].p; }
        return m;
    }
    void side_json(std::ostringstream& o, int w, u64 row) const {
        o << "[";
        for (u64 k = ptr[w][row]; k < ptr[w][row + 1]; ++k)
            o << (k > ptr[w][row] ? "," : "") << "[" << cols[w][k] << ",\"" << F::dec(coef[w].data() + k * F::CW) << "\"]";
        o << "]";
    }

    std::string run(const void* d_witness, uint32_t max_findings, hipStream_t st) override {
        const word_t* d_canon = (const word_t*)d_witness;
        const word_t* d_wit = d_canon;
        DevBuf wit_fe;
        if (F::IW != F::CW) {                                             // once per run, not per term
            wit_fe.reserve((size_t)n_wires * F::IW * sizeof(word_t));
            F::to_internal(d_canon, (word_t*)wit_fe.p, n_wires, st);
            d_wit = (const word_t*)wit_fe.p;
        }
        ZK_HIP(hipMemsetAsync(d_res.p, 0, 16, st));
        hipLaunchKernelGGL(r1cs_check_kernel<F>, grid1(n_cons), dim3(256), 0, st, csr(), d_wit, d_canon, n_cons, (ull*)d_mask.p, (ull*)d_res.p);
        ZK_HIP(hipGetLastError());
        u64 res[2];
        d2h_sync(res, d_res.p, 16);
        std::ostringstream o;
        bool any = false;
        if (res[1] && max_findings) {
            word_t one[F::CW];
            d2h_sync(one, d_canon, sizeof one);
            o << "{\"kind\":\"one_wire\",\"value\":\"" << F::dec(one) << "\"}";
            any = true;
        }
        const std::vector<u32> rows = read_failing(d_mask, n_cons, res[0], max_findings);
        if (!rows.empty()) {
            const uint32_t nl = (uint32_t)rows.size();
            DevBuf d_list, d_out;
            d_list.reserve(nl * 4); d_out.reserve((size_t)nl * 3 * F::CW * sizeof(word_t));
            h2d_sync(d_list.p, rows.data(), nl * 4);
            hipLaunchKernelGGL(r1cs_values_kernel<F>, dim3((nl + 63) / 64), dim3(64), 0, st, csr(), d_wit, (const u32*)d_list.p, nl, (word_t*)d_out.p);
            ZK_HIP(hipGetLastError());
            std::vector<word_t> abc((size_t)nl * 3 * F::CW);
            d2h_sync(abc.data(), d_out.p, abc.size() * sizeof(word_t));
            for (uint32_t t = 0; t < nl; ++t) {
                if (any) o << ","; any = true;
                const word_t* v = abc.data() + (size_t)t * 3 * F::CW;
                o << "{\"kind\":\"constraint\",\"index\":" << rows[t] << ",\"a\":\"" << F::dec(v) << "\",\"b\":\"" << F::dec(v + F::CW) << "\",\"c\":\"" << F::dec(v + 2 * F::CW)
                  << "\",\"wires\":{\"a\":"; side_json(o, 0, rows[t]);
                o << ",\"b\":"; side_json(o, 1, rows[t]);
                o << ",\"c\":"; side_json(o, 2, rows[t]);
                o << "}}";
            }
        }
        u64 gf[N_GATE_KINDS] = {0, 0, 0, 0};
        if (gates) {
            if constexpr (F::CW == 1) gates->run((const u64*)d_wit, max_findings, st, gf, o, any);
        }
        std::ostringstream j;
        j << "{\"field\":\"" << field << "\",\"n_wires\":" << n_wires << ",\"n_constraints\":" << n_cons << ",\"checked\":{\"constraint\":" << n_cons;
        for (int k = 0; k < N_GATE_KINDS; ++k) j << ",\"" << GATE_NAME[k] << "\":" << (gates ? gates->kind[k].n : 0);
        j << "},\"n_failing\":{\"one_wire\":" << res[1] << ",\"constraint\":" << res[0];
        for (int k = 0; k < N_GATE_KINDS; ++k) j << ",\"" << GATE_NAME[k] << "\":" << gf[k];
        j << "},\"findings\":[" << o.str() << "]}";
        return j.str();
    }
};

// a 32-byte-field file that uses custom gates: neither the prover's circuit nor this check has a meaning for them
void refuse_custom_sections(const uint8_t* b, size_t len) {
    uint32_t n_sec; std::memcpy(&n_sec, b + 8, 4);                        // (the reader has accepted the section table)
    size_t o = 12;
    for (uint32_t i = 0; i < n_sec; ++i) {
        uint32_t t; uint64_t sz; std::memcpy(&t, b + o, 4); std::memcpy(&sz, b + o + 4, 8); o += 12;
        if (t == 4 || t == 5) {
            uint32_t count = 0;
            if (sz >= 4) std::memcpy(&count, b + o, 4);
            ZK_REQUIRE(count == 0, "r1cs check: custom gates in a file over a 32-byte field (only the compressor's Goldilocks circuits have them)");
        }
        o += sz;
    }
    (void)len;
}

}  // namespace

namespace r1cs_bn254fr {
#define ZK_FR29_FIELD 254
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#include "fr_rows_impl.hip.h"
#include "r1cs_check_impl.hip.h"
}  // namespace r1cs_bn254fr
namespace r1cs_bls12381fr {
#define ZK_FR29_FIELD 381
#include "fr29_consts.hip.h"
#include "fe29_impl.hip.h"
#include "fr_rows_impl.hip.h"
#include "r1cs_check_impl.hip.h"
}  // namespace r1cs_bls12381fr

namespace {

template <class F>
R1csCheck* new_fr(const Curve& cv, const uint8_t* b, size_t len) {
    const g16::R1cs rc = g16::parse_r1cs(b, len, cv);
    refuse_custom_sections(b, len);
    auto c = std::make_unique<Checker<F>>();
    c->field = cv.name; c->curve = &cv; c->value_bytes = 32;
    c->n_wires = rc.n_wires; c->n_public = rc.n_pub_out + rc.n_pub_in; c->n_cons = rc.rows.size();
    ZK_REQUIRE(c->n_wires >= 1, "r1cs check: the circuit has no wire");
    for (int w = 0; w < 3; ++w) {
        c->ptr[w].push_back(0);
        for (const g16::Row& r : rc.rows) {
            const g16::Lc& lc = r.lc[w];
            for (size_t k = 0; k < lc.col.size(); ++k) {
                ZK_REQUIRE(lc.col[k] < rc.n_wires, "groth16: r1cs: wire index out of range");
                c->cols[w].push_back(lc.col[k]);
            }
            c->coef[w].insert(c->coef[w].end(), lc.coeff.begin(), lc.coeff.end());
            c->ptr[w].push_back(c->cols[w].size());
        }
    }
    c->upload();
    return c.release();
}
R1csCheck* new_gl(const uint8_t* b, size_t len) {
    const c12::R1csGL rc = c12::parse_r1cs_gl(b, len);
    auto c = std::make_unique<Checker<GlField>>();
    c->field = "GL"; c->value_bytes = 8;
    c->n_wires = rc.n_wires; c->n_public = rc.n_pub_out + rc.n_pub_in; c->n_cons = rc.rows.size();
    ZK_REQUIRE(c->n_wires >= 1, "r1cs check: the circuit has no wire");
    for (int w = 0; w < 3; ++w) {
        c->ptr[w].push_back(0);
        for (const auto& r : rc.rows) {
            for (const auto& [wire, cf] : r[w]) { c->cols[w].push_back((u32)wire); c->coef[w].push_back(cf); }   // (the reader has checked the range)
            c->ptr[w].push_back(c->cols[w].size());
        }
    }
    c->upload();
    c->gates = std::make_unique<Gates>(rc);
    c->n_uses = c->gates->n_uses;
    return c.release();
}

}  // namespace

R1csCheck* r1cs_check_new(const char* field, const void* r1cs, size_t len) {
    ZK_REQUIRE(field && r1cs, "r1cs check: null argument");
    const std::string f = field;
    const uint8_t* b = (const uint8_t*)r1cs;
    if (f == "GL") return new_gl(b, len);
    if (f == curve(CURVE_BN254).name) return new_fr<r1cs_bn254fr::FrField>(curve(CURVE_BN254), b, len);
    if (f == curve(CURVE_BLS12_381).name) return new_fr<r1cs_bls12381fr::FrField>(curve(CURVE_BLS12_381), b, len);
    throw Error("r1cs check: unknown field \"" + f + "\" (BN128 | BLS12381 | GL)");
}
void r1cs_check_free(R1csCheck* c) { delete c; }
void r1cs_check_info(const R1csCheck* c, uint32_t* n_wires, uint64_t* n_constraints, uint64_t* n_custom_uses, uint32_t* n_public) {
    if (n_wires) *n_wires = c->n_wires;
    if (n_constraints) *n_constraints = c->n_cons;
    if (n_custom_uses) *n_custom_uses = c->n_uses;
    if (n_public) *n_public = c->n_public;
}
size_t r1cs_check_value_bytes(const R1csCheck* c) { return c->value_bytes; }
bool r1cs_check_value_canonical(const R1csCheck* c, const void* value) { return c->canonical(value); }
std::string r1cs_check_run_dev(R1csCheck* c, const void* d_witness, uint32_t max_findings, hipStream_t st) { return c->run(d_witness, max_findings, st); }

}  // namespace zk
