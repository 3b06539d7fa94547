// pil_verify: a trace against its PIL on the device, row by row.
//
// The reference checks a trace between building it and proving it: starkjs/src/pil_verifier.js:46 calls pilcom's
// verifyPil(FGL, pil, cmPols, constPols) and asserts that nothing comes back.  This is that check with pilcom's meaning (its
// message strings are not a target): the PIL's own constraints on domain n, none of the prover's rewriting, every value a
// base-field word, `next` = row (i + 1) mod N.
//
//   polynomial identity   one program for all of them (starkinfo_gen.hip check_program): each expression, then `check1`; the
//                         interpreter (expr_bytecode.hip) counts the failing rows and keeps the smallest, a second tiny launch
//                         leaves the value there
//   plookup               the identity's program writes f | selF | t | selT into a row-major scratch section [N][2k + 2]; the selected
//                         t rows go into an open-addressing table (a slot holds a representative row, equality compares the k
//                         words, the hash mixes every word with its position), the selected f rows probe it
//   permutation           the same table with a signed counter per representative: t rows add, f rows subtract (an f row whose
//                         tuple is absent claims a slot of its own); a pass over the rows of each side then gives, for
//                         c = #t - #f per distinct tuple, sum |c| over c < 0, sum c over c > 0 (added by the representative) and the
//                         smallest row of each side that holds such a tuple
//   selector              a selector value outside {0, 1}: a finding of its own (the prover blends with it as a 0/1 value); for
//                         the set checks a row is selected when the selector is not 0
//   connection            a table over the k N identity values k_j w^i (from the x_n table, k_0 = 1, k_j = 12275445934081160404^j:
//                         helper.rs:16-23) -> cell j N + i; every cell looks its S value up: no such cell is a `connection_value`
//                         finding, a partner that holds another word a `connection` finding
//
// Every count and first row is reduced per wave first (the ballot of the failing lanes; one atomicAdd and one atomicMin of the
// wave's lowest failing lane, whose row is the wave's smallest): a satisfied trace issues no atomic for them.  None of the numbers
// depends on the order of insertion.  The scratch section and the table are built for one set identity at a time and come from
// the pool (devmem.hip); tables hold at least 4 slots per key, a power of two, as calculate_h1h2_dev's.
#include "pil_check.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <sstream>

namespace zk {

namespace {

inline dim3 grid1(u64 n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }
typedef unsigned long long ull;

// one wave's part of (count, first): `key` grows with the lane
__device__ __forceinline__ void wave_report(bool bad, u64 key, u64* __restrict__ count, u64* __restrict__ first) {
    const ull m = __ballot(bad);
    if (m == 0) return;
    if ((threadIdx.x & 63u) == (unsigned)__ffsll(m) - 1) {
        atomicAdd((ull*)count, (ull)__popcll(m));
        atomicMin((ull*)first, (ull)key);
    }
}
__device__ __forceinline__ void wave_min(bool bad, u64 key, u64* __restrict__ first) {
    const ull m = __ballot(bad);
    if (m != 0 && (threadIdx.x & 63u) == (unsigned)__ffsll(m) - 1) atomicMin((ull*)first, (ull)key);
}
__device__ __forceinline__ void wave_sum(u64 v, u64* __restrict__ total) {     // every lane of the wave calls it
    if (__ballot(v != 0) == 0) return;
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor((ull)v, d);
    if ((threadIdx.x & 63u) == 0) atomicAdd((ull*)total, (ull)v);
}

// the hash of a tuple: every word and its position (the running value is multiplied between words, so (a, b) and (b, a) part)
__device__ __forceinline__ u64 tuple_hash(const u64* __restrict__ e, uint32_t k) {
    u64 h = 0x9E3779B97F4A7C15ull;
    for (uint32_t c = 0; c < k; ++c) {
        h = (h ^ (e[c] + 0x7F4A7C15ull * (c + 1))) * 0xD1B54A32D192ED03ull;
        h ^= h >> 29;
    }
    h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return h;
}
__device__ __forceinline__ bool tuple_eq(const u64* __restrict__ a, const u64* __restrict__ b, uint32_t k) {
    for (uint32_t c = 0; c < k; ++c) if (a[c] != b[c]) return false;
    return true;
}

// The scratch section of a plookup / permutation: row i = f[0..k) | selF | t[0..k) | selT.  A representative is row * 2 + side + 1
// (side 0 = f, 1 = t; 0 = an empty slot).
struct SetView {
    const u64* scratch; u64 n; uint32_t k, width;
    __device__ const u64* tuple(uint32_t side, u64 row) const { return scratch + row * width + (side ? k + 1 : 0); }
    __device__ u64 sel(uint32_t side, u64 row) const { return scratch[row * width + (side ? 2 * k + 1 : k)]; }
    __device__ const u64* tuple_of(uint32_t rep) const { return tuple((rep - 1) & 1u, (rep - 1) >> 1); }
};

__global__ __launch_bounds__(256) void set_selector_kernel(SetView v, uint32_t side, u64* __restrict__ res /* count, first */) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    wave_report(i < v.n && v.sel(side, i) > 1, i, res, res + 1);
}
// the selected rows of `side` find their tuple's slot or claim one; cnt (may be null): the signed counter of the slot moves by delta
__global__ __launch_bounds__(256) void set_insert_kernel(SetView v, uint32_t side, uint32_t* __restrict__ slots, u64 mask, int* __restrict__ cnt, int delta) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n || v.sel(side, i) == 0) return;
    const u64* e = v.tuple(side, i);
    const uint32_t me = (uint32_t)(2 * i + side + 1);
    for (u64 s = tuple_hash(e, v.k) & mask;; s = (s + 1) & mask) {
        const uint32_t cur = atomicCAS(&slots[s], 0u, me);
        if (cur == 0 || tuple_eq(v.tuple_of(cur), e, v.k)) { if (cnt) atomicAdd(&cnt[s], delta); return; }
    }
}
__global__ __launch_bounds__(256) void plookup_probe_kernel(SetView v, const uint32_t* __restrict__ slots, u64 mask, u64* __restrict__ res /* count, first */) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool missing = false;
    if (i < v.n && v.sel(0, i) != 0) {
        const u64* e = v.tuple(0, i);
        for (u64 s = tuple_hash(e, v.k) & mask;; s = (s + 1) & mask) {
            const uint32_t cur = slots[s];
            if (cur == 0) { missing = true; break; }
            if (tuple_eq(v.tuple_of(cur), e, v.k)) break;
        }
    }
    wave_report(missing, i, res, res + 1);
}
// res: n_f_unmatched, n_t_unmatched, first_f_row, first_t_row
__global__ __launch_bounds__(256) void permutation_scan_kernel(SetView v, uint32_t side, const uint32_t* __restrict__ slots, u64 mask, const int* __restrict__ cnt,
                                                               u64* __restrict__ res) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool first = false; u64 lost_f = 0, lost_t = 0;
    if (i < v.n && v.sel(side, i) != 0) {
        const u64* e = v.tuple(side, i);
        const uint32_t me = (uint32_t)(2 * i + side + 1);
        for (u64 s = tuple_hash(e, v.k) & mask;; s = (s + 1) & mask) {
            const uint32_t cur = slots[s];
            if (cur == 0) break;                                          // (every selected row was inserted)
            if (cur == me || tuple_eq(v.tuple_of(cur), e, v.k)) {
                const int c = cnt[s];
                first = side == 0 ? c < 0 : c > 0;
                if (cur == me) { if (c < 0) lost_f = (u64)(-(long long)c); else lost_t = (u64)c; }
                break;
            }
        }
    }
    wave_min(first, i, res + 2 + side);
    wave_sum(lost_f, res);
    wave_sum(lost_t, res + 1);
}

// ---- connections: the scratch row is pols[0..k) | connections[0..k); cell c = j N + i; a slot holds c + 1 ------------------------------
__device__ __forceinline__ u64 word_hash(u64 x) {
    u64 h = (x ^ 0x9E3779B97F4A7C15ull) * 0xD1B54A32D192ED03ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return h;
}
struct ConnView {
    const u64* scratch; const u64* x_n; const u64* ks; u64 n; uint32_t nbits, k;
    __device__ u64 id_value(u64 c) const { return gl::mul(ks[c >> nbits], x_n[c & (n - 1)]); }
    __device__ u64 pol(u64 c) const { return scratch[(c & (n - 1)) * (2 * k) + (c >> nbits)]; }
    __device__ u64 conn(u64 c) const { return scratch[(c & (n - 1)) * (2 * k) + k + (c >> nbits)]; }
};
__global__ __launch_bounds__(256) void conn_insert_kernel(ConnView v, uint32_t* __restrict__ slots, u64 mask) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (u64)v.k * v.n) return;
    for (u64 s = word_hash(v.id_value(c)) & mask;; s = (s + 1) & mask)
        if (atomicCAS(&slots[s], 0u, (uint32_t)(c + 1)) == 0) return;
}
// the cell a word names, or ~0
__device__ __forceinline__ u64 conn_find(const ConnView& v, const uint32_t* __restrict__ slots, u64 mask, u64 word) {
    for (u64 s = word_hash(word) & mask;; s = (s + 1) & mask) {
        const uint32_t cur = slots[s];
        if (cur == 0) return ~0ull;
        if (v.id_value(cur - 1) == word) return cur - 1;
    }
}
// res: n_unnamed, first_unnamed, n_differ, first_differ
__global__ __launch_bounds__(256) void conn_check_kernel(ConnView v, const uint32_t* __restrict__ slots, u64 mask, u64* __restrict__ res) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool unnamed = false, differ = false;
    if (c < (u64)v.k * v.n) {
        const u64 p = conn_find(v, slots, mask, v.conn(c));
        if (p == ~0ull) unnamed = true; else differ = v.pol(c) != v.pol(p);
    }
    wave_report(unnamed, c, res, res + 1);
    wave_report(differ, c, res + 2, res + 3);
}
// res[4..8): the partner of cell res[3], the two words
__global__ void conn_detail_kernel(ConnView v, const uint32_t* __restrict__ slots, u64 mask, u64* __restrict__ res) {
    const u64 c = res[3];
    if (c == ~0ull) return;
    const u64 p = conn_find(v, slots, mask, v.conn(c));
    res[4] = p; res[5] = v.pol(c); res[6] = p == ~0ull ? 0 : v.pol(p);
}
__global__ void gather_word_kernel(const u64* __restrict__ src, u64 at, u64* __restrict__ dst) { *dst = src[at]; }

u64 pow2_slots(u64 keys) { u64 m = 4; while (m < 4 * keys) m <<= 1; return m; }

struct Json {
    std::ostringstream o;
    static void str(std::ostringstream& o, const std::string& s) {
        o << '"';
        for (char c : s) { if (c == '"' || c == '\\') o << '\\'; o << c; }
        o << '"';
    }
    void words(const std::vector<u64>& v) { o << "["; for (size_t i = 0; i < v.size(); ++i) o << (i ? ",\"" : "\"") << v[i] << "\""; o << "]"; }
};

}  // namespace

struct PilCheck {
    PilCheckProgram prog;
    std::unique_ptr<Bytecode, void (*)(Bytecode*)> identities{nullptr, bytecode_free};
    std::vector<std::unique_ptr<Bytecode, void (*)(Bytecode*)>> publics, sets;
    std::string listing;
    DevBuf d_res, d_publics, d_scratch, d_table, d_x, d_ks;
    bool have_x = false;

    explicit PilCheck(const char* pil_json) : prog(pil_check_generate(pil_json)) {
        auto assemble = [](const std::vector<zk_instr>& c) {
            return std::unique_ptr<Bytecode, void (*)(Bytecode*)>(bytecode_assemble(c.data(), (uint32_t)c.size(), true), bytecode_free);
        };
        std::ostringstream o;
        for (size_t k = 0; k < prog.publics.size(); ++k) {
            publics.push_back(prog.publics[k].im ? assemble(prog.publics[k].code) : std::unique_ptr<Bytecode, void (*)(Bytecode*)>(nullptr, bytecode_free));
            if (publics.back()) o << "; public " << k << "\n" << bytecode_listing(publics.back().get());
        }
        identities = assemble(prog.identities);
        o << "; polIdentities\n" << bytecode_listing(identities.get());
        static const char* const KEY[3] = {"plookupIdentities", "permutationIdentities", "connectionIdentities"};
        for (const PilCheckSet& s : prog.sets) {
            sets.push_back(assemble(s.code));
            o << "; " << KEY[s.kind] << "[" << s.index << "]\n" << bytecode_listing(sets.back().get());
        }
        listing = o.str();
    }

    zk_eval_ctx ctx(const u64* d_const, const u64* d_cm) {
        zk_eval_ctx c; memset(&c, 0, sizeof c);
        c.bufs[PC_BUF_CM] = (uint64_t*)d_cm; c.bufs[PC_BUF_CONST] = (uint64_t*)d_const;
        c.bufs[PC_BUF_SCRATCH] = (uint64_t*)d_scratch.p; c.bufs[PC_BUF_PUBLICS] = (uint64_t*)d_publics.p; c.bufs[PC_BUF_RESULT] = (uint64_t*)d_res.p;
        c.publics = (const uint64_t*)d_publics.p;
        return c;
    }
    static void src(Json& j, const char* kind, uint32_t index, const PilCheckSrc& s) {
        j.o << "{\"kind\":\"" << kind << "\",\"index\":" << index << ",\"fileName\":"; Json::str(j.o, s.file); j.o << ",\"line\":" << s.line;
    }
    std::vector<u64> row_words(u64 row, uint32_t width, uint32_t off, uint32_t k) {
        std::vector<u64> w(k);
        d2h_sync(w.data(), d_scratch.u() + row * width + off, (size_t)k * 8);
        return w;
    }

    std::string run(const u64* d_const, const u64* d_cm, uint64_t n_rows, hipStream_t st) {
        const u64 N = prog.n;
        ZK_REQUIRE(n_rows == N, "pil_verify: the trace has " + std::to_string(n_rows) + " rows, the PIL's polDeg is " + std::to_string(N));
        ZK_REQUIRE((d_const || prog.n_const == 0) && (d_cm || prog.n_cm == 0), "pil_verify: null trace");
        const uint32_t n_ids = (uint32_t)prog.identity_src.size(), n_pub = (uint32_t)prog.publics.size();
        Json j;
        bool any = false;
        auto sep = [&] { if (any) j.o << ","; any = true; };

        // publics, as the prover computes them (stark_gen.rs:256-277)
        d_publics.reserve(std::max<size_t>(8, (size_t)n_pub * 8));
        d_res.reserve(std::max<size_t>(64, (size_t)n_ids * 24));
        for (uint32_t k = 0; k < n_pub; ++k) {
            const PilCheckPublic& p = prog.publics[k];
            if (p.im) { zk_eval_ctx c = ctx(d_const, d_cm); bytecode_run(publics[k].get(), &c, prog.nbits, 1, p.idx, 1, st); }
            else { hipLaunchKernelGGL(gather_word_kernel, dim3(1), dim3(1), 0, st, d_cm, p.idx * prog.n_cm + p.pol_id, d_publics.u() + k); ZK_HIP(hipGetLastError()); }
        }
        std::vector<u64> pub(n_pub);
        j.o << "{\"n\":" << N << ",\"publics\":";

        // polynomial identities
        std::vector<u64> res(3 * (size_t)n_ids);
        if (n_ids) {
            ZK_HIP(hipMemsetAsync(d_res.p, 0, (size_t)n_ids * 8, st));
            ZK_HIP(hipMemsetAsync(d_res.u() + n_ids, 0xFF, (size_t)n_ids * 8, st));
            ZK_HIP(hipMemsetAsync(d_res.u() + 2 * (size_t)n_ids, 0, (size_t)n_ids * 8, st));
            zk_eval_ctx c = ctx(d_const, d_cm);
            bytecode_run(identities.get(), &c, prog.nbits, 1, 0, N, st);
            d2h_sync(res.data(), d_res.p, (size_t)n_ids * 16);
            bool failed = false;
            for (uint32_t k = 0; k < n_ids; ++k) failed = failed || res[k] != 0;
            if (failed) {
                bytecode_run_first(identities.get(), &c, prog.nbits, 1, n_ids, st);
                d2h_sync(res.data() + 2 * (size_t)n_ids, d_res.u() + 2 * (size_t)n_ids, (size_t)n_ids * 8);
            }
        }
        d2h_sync(pub.data(), d_publics.p, (size_t)n_pub * 8);
        j.words(pub);
        uint32_t n_set[3] = {0, 0, 0};
        for (const PilCheckSet& s : prog.sets) ++n_set[s.kind];
        j.o << ",\"checked\":{\"polIdentities\":" << n_ids << ",\"plookupIdentities\":" << n_set[0] << ",\"permutationIdentities\":" << n_set[1]
            << ",\"connectionIdentities\":" << n_set[2] << "},\"findings\":[";
        for (uint32_t k = 0; k < n_ids; ++k) {
            if (res[k] == 0) continue;
            sep(); src(j, "identity", k, prog.identity_src[k]);
            j.o << ",\"n_rows\":\"" << res[k] << "\",\"first_row\":\"" << res[n_ids + k] << "\",\"value\":\"" << res[2 * (size_t)n_ids + k] << "\"}";
        }

        // set identities, one at a time: the scratch section, then the table
        for (size_t si = 0; si < prog.sets.size(); ++si) {
            const PilCheckSet& s = prog.sets[si];
            d_scratch.reserve((size_t)N * s.width * 8);
            zk_eval_ctx c = ctx(d_const, d_cm);
            bytecode_run(sets[si].get(), &c, prog.nbits, 1, 0, N, st);
            u64 r[8];
            u64* d_r = d_res.u();                                            // 8 words; the identities' results have been read
            auto reset = [&](std::initializer_list<int> minima) {
                for (int k = 0; k < 8; ++k) r[k] = 0;
                for (int k : minima) r[k] = ~0ull;
                h2d_sync(d_r, r, sizeof r);
            };
            if (s.kind == PC_CONNECTION) {
                if (!have_x) { d_x.reserve((size_t)N * 8); x_table_dev(prog.nbits, 1, d_x.u(), st); have_x = true; }
                std::vector<u64> ks(s.k, 1);
                for (uint32_t c2 = 1; c2 < s.k; ++c2) ks[c2] = c2 == 1 ? 12275445934081160404ull : (u64)(((unsigned __int128)ks[c2 - 1] * 12275445934081160404ull) % GL_P);
                d_ks.reserve((size_t)s.k * 8);
                h2d_sync(d_ks.p, ks.data(), (size_t)s.k * 8);
                const u64 cells = (u64)s.k * N, m = pow2_slots(cells);
                d_table.reserve((size_t)m * 4);
                ZK_HIP(hipMemsetAsync(d_table.p, 0, (size_t)m * 4, st));
                reset({1, 3});
                const ConnView v{d_scratch.u(), d_x.u(), d_ks.u(), N, prog.nbits, s.k};
                hipLaunchKernelGGL(conn_insert_kernel, grid1(cells), dim3(256), 0, st, v, (uint32_t*)d_table.p, m - 1);
                hipLaunchKernelGGL(conn_check_kernel, grid1(cells), dim3(256), 0, st, v, (const uint32_t*)d_table.p, m - 1, d_r);
                hipLaunchKernelGGL(conn_detail_kernel, dim3(1), dim3(1), 0, st, v, (const uint32_t*)d_table.p, m - 1, d_r);
                ZK_HIP(hipGetLastError());
                d2h_sync(r, d_r, sizeof r);
                if (r[0]) {
                    const u64 cell = r[1];
                    sep(); src(j, "connection_value", s.index, s.src);
                    j.o << ",\"n_cells\":\"" << r[0] << "\",\"col\":" << (cell >> prog.nbits) << ",\"row\":\"" << (cell & (N - 1)) << "\",\"value\":\""
                        << row_words(cell & (N - 1), s.width, s.k + (uint32_t)(cell >> prog.nbits), 1)[0] << "\"}";
                }
                if (r[2]) {
                    sep(); src(j, "connection", s.index, s.src);
                    j.o << ",\"n_cells\":\"" << r[2] << "\",\"col\":" << (r[3] >> prog.nbits) << ",\"row\":\"" << (r[3] & (N - 1)) << "\",\"partner_col\":" << (r[4] >> prog.nbits)
                        << ",\"partner_row\":\"" << (r[4] & (N - 1)) << "\",\"value\":\"" << r[5] << "\",\"partner_value\":\"" << r[6] << "\"}";
                }
                continue;
            }
            const SetView v{d_scratch.u(), N, s.k, s.width};
            const char* kind = s.kind == PC_PLOOKUP ? "plookup" : "permutation";
            for (uint32_t side = 0; side < 2; ++side) {
                if (!(side ? s.has_selt : s.has_self)) continue;
                reset({1});
                hipLaunchKernelGGL(set_selector_kernel, grid1(N), dim3(256), 0, st, v, side, d_r);
                ZK_HIP(hipGetLastError());
                d2h_sync(r, d_r, sizeof r);
                if (!r[0]) continue;
                sep(); src(j, "selector", s.index, s.src);
                j.o << ",\"identity\":\"" << kind << "\",\"side\":\"" << (side ? "t" : "f") << "\",\"n_rows\":\"" << r[0] << "\",\"first_row\":\"" << r[1]
                    << "\",\"value\":\"" << row_words(r[1], s.width, side ? 2 * s.k + 1 : s.k, 1)[0] << "\"}";
            }
            const u64 m = pow2_slots(s.kind == PC_PLOOKUP ? N : 2 * N);
            uint32_t* slots = nullptr; int* cnt = nullptr;
            d_table.reserve((size_t)m * (s.kind == PC_PLOOKUP ? 4 : 8));
            ZK_HIP(hipMemsetAsync(d_table.p, 0, (size_t)m * (s.kind == PC_PLOOKUP ? 4 : 8), st));
            slots = (uint32_t*)d_table.p;
            if (s.kind == PC_PLOOKUP) {
                reset({1});
                hipLaunchKernelGGL(set_insert_kernel, grid1(N), dim3(256), 0, st, v, 1u, slots, m - 1, cnt, 0);
                hipLaunchKernelGGL(plookup_probe_kernel, grid1(N), dim3(256), 0, st, v, (const uint32_t*)slots, m - 1, d_r);
                ZK_HIP(hipGetLastError());
                d2h_sync(r, d_r, sizeof r);
                if (!r[0]) continue;
                sep(); src(j, kind, s.index, s.src);
                j.o << ",\"n_rows\":\"" << r[0] << "\",\"first_row\":\"" << r[1] << "\",\"values\":"; j.words(row_words(r[1], s.width, 0, s.k)); j.o << "}";
            } else {
                cnt = (int*)(slots + m);
                reset({2, 3});
                hipLaunchKernelGGL(set_insert_kernel, grid1(N), dim3(256), 0, st, v, 1u, slots, m - 1, cnt, 1);
                hipLaunchKernelGGL(set_insert_kernel, grid1(N), dim3(256), 0, st, v, 0u, slots, m - 1, cnt, -1);
                hipLaunchKernelGGL(permutation_scan_kernel, grid1(N), dim3(256), 0, st, v, 0u, (const uint32_t*)slots, m - 1, (const int*)cnt, d_r);
                hipLaunchKernelGGL(permutation_scan_kernel, grid1(N), dim3(256), 0, st, v, 1u, (const uint32_t*)slots, m - 1, (const int*)cnt, d_r);
                ZK_HIP(hipGetLastError());
                d2h_sync(r, d_r, sizeof r);
                if (!r[0] && !r[1]) continue;
                sep(); src(j, kind, s.index, s.src);
                j.o << ",\"n_f_unmatched\":\"" << r[0] << "\",\"n_t_unmatched\":\"" << r[1] << "\"";
                j.o << ",\"first_f_row\":"; if (r[0]) j.o << "\"" << r[2] << "\""; else j.o << "null";
                j.o << ",\"first_t_row\":"; if (r[1]) j.o << "\"" << r[3] << "\""; else j.o << "null";
                j.o << ",\"f_values\":"; if (r[0]) j.words(row_words(r[2], s.width, 0, s.k)); else j.o << "null";
                j.o << ",\"t_values\":"; if (r[1]) j.words(row_words(r[3], s.width, s.k + 1, s.k)); else j.o << "null";
                j.o << "}";
            }
        }
        j.o << "]}";
        d_scratch.release(); d_table.release();
        return j.o.str();
    }
};

PilCheck* pil_check_new(const char* pil_json) { return new PilCheck(pil_json); }
void pil_check_free(PilCheck* p) { delete p; }
const char* pil_check_listing(const PilCheck* p) { return p->listing.c_str(); }
uint64_t pil_check_rows(const PilCheck* p) { return p->prog.n; }
void pil_check_widths(const PilCheck* p, uint32_t* n_const, uint32_t* n_cm) { *n_const = p->prog.n_const; *n_cm = p->prog.n_cm; }
std::string pil_check_run_dev(PilCheck* p, const u64* d_const, const u64* d_cm, uint64_t n_rows, hipStream_t st) { return p->run(d_const, d_cm, n_rows, st); }

}  // namespace zk
