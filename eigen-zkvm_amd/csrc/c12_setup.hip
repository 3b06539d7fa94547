// compressor12 setup on gfx950 -- `zkit compressor12_setup` (zkit/src/main.rs:140-151): a Goldilocks R1CS in, the compressor's
// .pil text, its .exec text and its [N][nConst] constant matrix out.
//   host    the R1CS reader (algebraic/src/r1cs_file.rs:50-270, 8-byte field, custom-gate sections 4 and 5), R1CS -> PLONK
//           (recursion/src/r1cs2plonk.rs:50-227: the order of gates and additions is part of the .exec format), the row packing
//           (recursion/src/compressor12/plonk_setup.rs:172-663), the .pil text (a generator of our own) and the .exec text
//           (compressor12_setup.rs:51-83)
//   device  everything of the size of the trace: the 12 S columns S[j][i] = w^i k_j, the copy-constraint wiring and the fill of
//           the row-major matrix.
// The wiring.  plonk_setup.rs:692-728 walks the cells in the order (row, column) and, at every repeat of a signal, swaps S there
// with S at the signal's FIRST cell.  For a signal whose cells in walk order are p_0 < p_1 < ... < p_k the chain of swaps leaves
//   S[p_m] = id[p_{m-1}] (m >= 1),  S[p_0] = id[p_k]
// (by induction: before the visit of p_m, S[p_0] = id[p_{m-1}]; the swap moves that into p_m and id[p_m] into p_0): a rotation of
// the run.  So: a stable sort of the (signal, position) pairs by signal puts every run in walk order, each element takes the
// identity value of its predecessor in the run and the head takes the tail's.  No cell is written twice and no order between
// signals matters.  The sort is a stable LSD radix sort over 32-bit keys, 8 bits a pass, one wave per tile.
#include "zk_internal.h"
#include "r1cs_file.h"
#include "poseidon_gl_constants.h"
#include "../../tools/poseidong_round_constants.h"   // the 360 plain round constants + the 12 zeros of the output row
#include <algorithm>
#include <array>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <vector>

namespace zk {
using namespace c12;                                      // Lc, CustomGate, CustomUse, R1csGL: r1cs_file.h
namespace {

constexpr u64 GLP = 0xFFFFFFFF00000001ULL;
constexpr u64 C12_K = 12275445934081160404ULL;          // helper.rs:16-23 get_ks: k_j = k^j
u64 fadd(u64 a, u64 b) { return (u64)(((unsigned __int128)a + b) % GLP); }
u64 fsub(u64 a, u64 b) { return a >= b ? a - b : a + (GLP - b); }
u64 fneg(u64 a) { return a ? GLP - a : 0; }
u64 fmul(u64 a, u64 b) { return (u64)((unsigned __int128)a * b % GLP); }

// ---- the R1CS file ------------------------------------------------------------------------------------------------------------
struct Rd {
    const uint8_t* p; size_t n, o = 0;
    void need(size_t k) const { if (k > n - o) throw Error("r1cs: truncated file"); }
    uint32_t u32le() { need(4); uint32_t v; std::memcpy(&v, p + o, 4); o += 4; return v; }
    uint64_t u64le() { need(8); uint64_t v; std::memcpy(&v, p + o, 8); o += 8; return v; }
    const uint8_t* take(size_t k) { need(k); const uint8_t* q = p + o; o += k; return q; }
    u64 field() { const u64 v = u64le(); if (v >= GLP) throw Error("r1cs: coefficient is not a canonical field element"); return v; }
};
}  // namespace

R1csGL c12::parse_r1cs_gl(const uint8_t* b, size_t len) {
    Rd rd{b, len};
    if (std::memcmp(rd.take(4), "r1cs", 4) != 0) throw Error("r1cs: Invalid magic number");
    if (rd.u32le() != 1) throw Error("r1cs: Unsupported version");
    const uint32_t n_sec = rd.u32le();
    std::map<uint32_t, std::pair<size_t, uint64_t>> sec;   // sections may come in any order (r1cs_file.rs:206-213)
    for (uint32_t i = 0; i < n_sec; ++i) {
        const uint32_t t = rd.u32le(); const uint64_t sz = rd.u64le();
        sec[t] = {rd.o, sz};
        rd.take(sz);
    }
    if (!sec.count(1) || !sec.count(2)) throw Error("r1cs: header or constraint section missing");
    Rd h{b + sec[1].first, (size_t)sec[1].second};
    const uint32_t fs = h.u32le();
    if (sec[1].second != 32 + (uint64_t)fs) throw Error("r1cs: Invalid header section size");
    if (fs != 8) throw Error("r1cs: Different prime: field size " + std::to_string(fs) + " bytes, the compressor's circuits are over Goldilocks (8)");
    if (h.u64le() != GLP) throw Error("r1cs: Different prime: the file's prime is not 0xFFFFFFFF00000001");
    R1csGL rc;
    rc.n_wires = h.u32le(); rc.n_pub_out = h.u32le(); rc.n_pub_in = h.u32le(); rc.n_prv_in = h.u32le();
    (void)h.u64le();
    const uint32_t n_cons = h.u32le();
    Rd c{b + sec[2].first, (size_t)sec[2].second};
    rc.rows.resize(n_cons);
    for (uint32_t i = 0; i < n_cons; ++i)
        for (int w = 0; w < 3; ++w) {
            const uint32_t nv = c.u32le();
            for (uint32_t k = 0; k < nv; ++k) {
                const u64 wire = c.u32le(), coef = c.field();
                if (wire >= rc.n_wires) throw Error("r1cs: wire index out of range in constraint " + std::to_string(i));
                if (!rc.rows[i][w].emplace(wire, coef).second) throw Error("r1cs: a wire appears twice in one linear combination");   // r1cs2plonk.rs:170
            }
        }
    if (sec.count(4)) {                                    // r1cs_file.rs:134-151
        Rd g{b + sec[4].first, (size_t)sec[4].second};
        const uint32_t n = g.u32le();
        for (uint32_t i = 0; i < n; ++i) {
            CustomGate cg;
            for (;;) { const uint8_t ch = *g.take(1); if (!ch) break; cg.name.push_back((char)ch); }
            const uint32_t np = g.u32le();
            for (uint32_t k = 0; k < np; ++k) cg.params.push_back(g.field());
            rc.gates.push_back(std::move(cg));
        }
    }
    if (sec.count(5)) {                                    // r1cs_file.rs:153-183: 32-bit words, signals as (LSB, MSB)
        Rd g{b + sec[5].first, (size_t)sec[5].second};
        const uint32_t n = g.u32le();
        for (uint32_t i = 0; i < n; ++i) {
            CustomUse cu; cu.id = g.u32le();
            const uint32_t ns = g.u32le();
            g.need((size_t)ns * 8);
            cu.signals.resize(ns);
            for (uint32_t k = 0; k < ns; ++k) { const u64 lsb = g.u32le(), msb = g.u32le(); cu.signals[k] = (msb << 32) | lsb; }
            rc.uses.push_back(std::move(cu));
        }
    }
    return rc;
}

namespace {

// ---- R1CS -> PLONK (r1cs2plonk.rs:50-227) ---------------------------------------------------------------------------------------
struct Gate { u64 s[3]; u64 q[5]; };                      // sl sr so | qm ql qr qo qc
struct Add { u64 a, b, ca, cb; };
struct Plonk { std::vector<Gate> gates; std::vector<Add> adds; u64 n_var = 0; };

struct Reduced { u64 k = 0; std::vector<u64> s, c; };
// :83-128.  The terms leave the FRONT of a list ordered by wire, the sum joins at the back
Reduced reduce_coefs(const Lc& lc, size_t max_c, Plonk& pl) {
    Reduced res;
    std::deque<std::pair<u64, u64>> cs;
    for (const auto& [key, val] : lc) {
        if (key == 0) res.k = fadd(res.k, val);
        else if (val != 0) cs.push_back({key, val});
    }
    while (cs.size() > max_c) {
        const auto c1 = cs.front(); cs.pop_front();
        const auto c2 = cs.front(); cs.pop_front();
        const u64 so = pl.n_var++;
        pl.gates.push_back(Gate{{c1.first, c2.first, so}, {0, fneg(c1.second), fneg(c2.second), 1, 0}});
        pl.adds.push_back(Add{c1.first, c2.first, c1.second, c2.second});
        cs.push_back({so, 1});
    }
    for (const auto& c : cs) { res.s.push_back(c.first); res.c.push_back(c.second); }
    while (res.c.size() < max_c) { res.s.push_back(0); res.c.push_back(0); }
    return res;
}
void add_constraint_sum(const Lc& lc, Plonk& pl) {         // :151-165
    const Reduced C = reduce_coefs(lc, 3, pl);
    pl.gates.push_back(Gate{{C.s[0], C.s[1], C.s[2]}, {0, C.c[0], C.c[1], C.c[2], C.k}});
}
void add_constraint_mul(const Lc& la, const Lc& lb, const Lc& lc, Plonk& pl) {   // :130-149
    const Reduced A = reduce_coefs(la, 1, pl), B = reduce_coefs(lb, 1, pl), C = reduce_coefs(lc, 1, pl);
    pl.gates.push_back(Gate{{A.s[0], B.s[0], C.s[0]},
                            {fmul(A.c[0], B.c[0]), fmul(A.c[0], B.k), fmul(A.k, B.c[0]), fneg(C.c[0]), fsub(fmul(A.k, B.k), C.k)}});
}
void normalize(Lc& lc) { for (auto it = lc.begin(); it != lc.end();) it = it->second == 0 ? lc.erase(it) : std::next(it); }
char lc_type(Lc& lc) {                                     // :176-197: 'n' some wire, 'k' a constant only, '0' nothing
    normalize(lc);
    size_t n = 0; u64 k = 0;
    for (const auto& [key, val] : lc) { if (key == 0) k = fadd(k, val); else ++n; }
    return n ? 'n' : k ? 'k' : '0';
}
Lc join(const Lc& lc1, u64 k, const Lc& lc2) {             // :59-81: k lc1 + lc2
    Lc res;
    for (const auto& [key, val] : lc1) res[key] = fadd(res.count(key) ? res[key] : 0, fmul(k, val));
    for (const auto& [key, val] : lc2) res[key] = fadd(res.count(key) ? res[key] : 0, val);
    normalize(res);
    return res;
}
Plonk r1cs2plonk(const R1csGL& r) {
    Plonk pl; pl.n_var = r.n_wires;                        // new wires count up from num_variables
    for (const auto& row : r.rows) {                       // :199-218
        Lc a = row[0], b = row[1], c = row[2];
        const char ta = lc_type(a), tb = lc_type(b);
        if (ta == '0' || tb == '0') { normalize(c); add_constraint_sum(c, pl); }
        else if (ta == 'k') add_constraint_sum(join(b, a[0], c), pl);
        else if (tb == 'k') add_constraint_sum(join(a, b[0], c), pl);
        else add_constraint_mul(a, b, c, pl);
    }
    return pl;
}

// ---- the row packing (plonk_setup.rs:172-663) ------------------------------------------------------------------------------------
// a used row of the constant matrix: C[0..12), then the selectors in the .pil's column order
enum { SEL_PARTIAL = 12, SEL_POSEIDON12, SEL_GATE, SEL_CMULADD, SEL_EVPOL4, SEL_FFT4, ROW_WORDS };
using ConstRow = std::array<u64, ROW_WORDS>;
constexpr u64 NO_GATE = ~0ull;

}  // namespace

struct C12Setup {
    uint32_t n_bits = 0, n_l = 0;
    u64 n_publics = 0, n_used = 0, n_const = 0;
    Plonk pl;
    std::vector<u32> s_map;                                // [n_used][12], the .exec order
    std::vector<ConstRow> rows;                            // [n_used]
    uint32_t key_bits = 32;                                // the radix passes the largest wire id needs
};

namespace {

void pack_rows(const R1csGL& r1cs, uint32_t force_n_bits, C12Setup& S) {
    const std::vector<Gate>& pg = S.pl.gates;
    // plonk_setup.rs:54-78.  The reference keys the gate map on a hex string of the five coefficients; the string's order only
    // fixes the iteration order of the "terminate the empty rows" loop below, and that order does not reach the output: every
    // half row the loop touches ends up in half_rows, and every row in half_rows has its second half zeroed the same way.
    using Key = std::array<u64, 5>;
    auto key_of = [](const Gate& g) { return Key{g.q[0], g.q[1], g.q[2], g.q[3], g.q[4]}; };
    std::map<Key, u64> uses;
    for (const Gate& g : pg) ++uses[key_of(g)];
    ZK_REQUIRE(!pg.empty(), "compressor12 setup: the circuit has no constraint");
    u64 n_plonk = 0;
    for (const auto& kv : uses) n_plonk += (kv.second - 1) / 2 + 1;
    n_plonk = (n_plonk - 1) / 2 + 1;
    // :102-158.  A template the circuit does not list has no id (the reference leaves it at 0, which then shadows gate 0)
    u64 poseidon_id = NO_GATE, cmuladd_id = NO_GATE, evpol_id = NO_GATE;
    std::map<u64, const std::vector<u64>*> fft_params;
    for (size_t i = 0; i < r1cs.gates.size(); ++i) {
        const CustomGate& c = r1cs.gates[i];
        if (c.name == "FFT4") {
            ZK_REQUIRE(c.params.size() == 4, "compressor12 setup: FFT4 takes 4 parameters");
            ZK_REQUIRE(c.params[3] == 2 || c.params[3] == 4, "compressor12 setup: invalid FFT4 type: " + std::to_string(c.params[3]));
            fft_params[i] = &c.params; continue;
        }
        ZK_REQUIRE(c.name == "CMulAdd" || c.name == "Poseidon12" || c.name == "EvPol4", "compressor12 setup: Invalid custom gate " + c.name);
        ZK_REQUIRE(c.params.empty(), "compressor12 setup: " + c.name + " takes no parameter");
        (c.name == "CMulAdd" ? cmuladd_id : c.name == "Poseidon12" ? poseidon_id : evpol_id) = i;
    }
    u64 custom_rows = 0;
    for (const CustomUse& u : r1cs.uses) {
        for (u64 s : u.signals) {
            ZK_REQUIRE(s < (1ull << 32), "compressor12 setup: wire id does not fit 32 bits");
            ZK_REQUIRE(s < r1cs.n_wires, "compressor12 setup: wire index out of range in a custom gate");
        }
        if (u.id == poseidon_id) { ZK_REQUIRE(u.signals.size() == 31 * 12, "compressor12 setup: a Poseidon12 use has " + std::to_string(u.signals.size()) + " signals, not 372"); custom_rows += 31; }
        else if (u.id == cmuladd_id) { ZK_REQUIRE(u.signals.size() >= 12, "compressor12 setup: a CMulAdd use has fewer than 12 signals"); custom_rows += 1; }
        else if (fft_params.count(u.id)) { ZK_REQUIRE(u.signals.size() >= 24, "compressor12 setup: an FFT4 use has fewer than 24 signals"); custom_rows += 2; }
        else if (u.id == evpol_id) { ZK_REQUIRE(u.signals.size() >= 21, "compressor12 setup: an EvPol4 use has fewer than 21 signals"); custom_rows += 2; }
        else throw Error("compressor12 setup: Custom gate not defined " + std::to_string(u.id));
    }
    ZK_REQUIRE(S.pl.n_var <= (1ull << 32), "compressor12 setup: wire id does not fit 32 bits");
    // :183-197
    S.n_publics = (u64)r1cs.n_pub_in + 2ull * r1cs.n_pub_out;          // num_inputs + num_outputs - 1 (reader.rs:200-208)
    ZK_REQUIRE(S.n_publics > 0, "compressor12 setup: the circuit has no public signal");
    ZK_REQUIRE(S.n_publics < r1cs.n_wires, "compressor12 setup: more public signals than wires");
    const u64 n_public_rows = (S.n_publics - 1) / 12 + 1;
    S.n_used = n_public_rows + n_plonk + custom_rows;
    uint32_t n_bits = 0;
    while ((1ull << n_bits) < S.n_used) ++n_bits;                       // log2(n_used - 1) + 1
    if (S.n_used == 1) n_bits = 1;                                      // helper::log2_any(0) + 1
    if (force_n_bits) n_bits = force_n_bits;
    ZK_REQUIRE(n_bits <= 32, "compressor12 setup: n_bits above 32");
    ZK_REQUIRE(S.n_used <= (1ull << n_bits), "compressor12 setup: force_n_bits " + std::to_string(force_n_bits) + " is too small for " + std::to_string(S.n_used) + " rows");
    S.n_bits = n_bits; S.n_l = (uint32_t)n_public_rows; S.n_const = n_public_rows + 12 + ROW_WORDS;

    const u64 n_used = S.n_used;
    S.s_map.assign(n_used * 12, 0);
    S.rows.assign(n_used, ConstRow{});
    auto sm = [&](u64 col, u64 row) -> u32& { return S.s_map[row * 12 + col]; };
    u64 r = 0;
    for (u64 i = 0; i < S.n_publics; ++i) sm(i % 12, i / 12) = (u32)(1 + i);                      // :253-258
    r += n_public_rows;
    struct ParRow { u64 row; int n_used; };
    std::map<Key, ParRow> partial;
    std::deque<ParRow> half;
    for (const Gate& c : pg) {                                                                    // :271-343
        const Key k = key_of(c);
        auto it = partial.find(k);
        if (it != partial.end()) {
            ParRow& pr = it->second;
            for (int t = 0; t < 3; ++t) sm(pr.n_used * 3 + t, pr.row) = (u32)c.s[t];
            ++pr.n_used;
            if (pr.n_used == 2) { half.push_back(pr); partial.erase(it); }
            else if (pr.n_used == 4) partial.erase(it);
        } else if (!half.empty()) {
            ParRow pr = half.front(); half.pop_front();
            ConstRow& R = S.rows[pr.row];
            R[9] = c.q[0]; R[6] = c.q[1]; R[7] = c.q[2]; R[8] = c.q[3]; R[10] = c.q[4]; R[11] = 0;
            for (int t = 0; t < 3; ++t) sm(pr.n_used * 3 + t, pr.row) = (u32)c.s[t];
            ++pr.n_used;
            partial[k] = pr;
        } else {
            // the count of :54-78 holds when at most one half row stays empty; a gate order that leaves more makes the reference index past its s_map
            ZK_REQUIRE(r + custom_rows < n_used, "compressor12 setup: the gates need more rows than plonk_setup's count gives (too many coefficient sets left with an odd gate)");
            ConstRow& R = S.rows[r];
            R[3] = c.q[0]; R[0] = c.q[1]; R[1] = c.q[2]; R[2] = c.q[3]; R[4] = c.q[4]; R[5] = 0;
            R[SEL_GATE] = 1;
            for (int t = 0; t < 3; ++t) sm(t, r) = (u32)c.s[t];
            partial[k] = ParRow{r, 1};
            ++r;
        }
    }
    for (auto& kv : partial) {                                                                    // :346-360: an odd gate is repeated
        ParRow& pr = kv.second;
        if (pr.n_used == 1) { for (int t = 0; t < 3; ++t) sm(3 + t, pr.row) = sm(t, pr.row); ++pr.n_used; half.push_back(pr); }
        else if (pr.n_used == 3) { for (int t = 0; t < 3; ++t) sm(9 + t, pr.row) = sm(6 + t, pr.row); }
        else throw Error("compressor12 setup: internal error while terminating the empty rows");
    }
    for (const ParRow& hr : half) {                                                               // :362-379
        for (int t = 6; t < 12; ++t) { sm(t, hr.row) = 0; S.rows[hr.row][t] = 0; }
    }
    for (const CustomUse& u : r1cs.uses) {                                                        // :383-663
        const u64 rows_needed = u.id == poseidon_id ? 31 : u.id == cmuladd_id ? 1 : 2;
        ZK_REQUIRE(r + rows_needed <= n_used, "compressor12 setup: internal error: more custom-gate rows than counted");
        if (u.id == poseidon_id) {
            for (u64 j = 0; j < 31; ++j) {
                ConstRow& R = S.rows[r + j];
                for (u64 k = 0; k < 12; ++k) { sm(k, r + j) = (u32)u.signals[j * 12 + k]; R[k] = POSEIDONG_C[j * 12 + k]; }
                R[SEL_POSEIDON12] = j < 30;
                R[SEL_PARTIAL] = j >= 4 && j < 26;
            }
            r += 31;
        } else if (u.id == cmuladd_id) {
            for (u64 k = 0; k < 12; ++k) sm(k, r) = (u32)u.signals[k];
            S.rows[r][SEL_CMULADD] = 1; S.rows[r][9] = 1; S.rows[r][10] = 1;
            r += 1;
        } else if (fft_params.count(u.id)) {
            for (u64 k = 0; k < 12; ++k) { sm(k, r) = (u32)u.signals[k]; sm(k, r + 1) = (u32)u.signals[12 + k]; }
            ConstRow& R = S.rows[r];
            R[SEL_FFT4] = 1;
            const std::vector<u64>& p = *fft_params[u.id];
            const u64 first_w = p[0], inc_w = p[1], scale = p[2], first_w2 = fmul(first_w, first_w);
            if (p[3] == 4) {
                R[0] = scale; R[1] = fmul(scale, first_w2); R[2] = fmul(scale, first_w); R[3] = fmul(fmul(scale, first_w), first_w2);
                R[4] = fmul(fmul(scale, first_w), inc_w); R[5] = fmul(fmul(fmul(scale, first_w), first_w2), inc_w);
            } else {
                R[6] = scale; R[7] = fmul(scale, first_w); R[8] = fmul(fmul(scale, first_w), inc_w);
            }
            r += 2;
        } else {
            for (u64 k = 0; k < 12; ++k) sm(k, r) = (u32)u.signals[k];
            for (u64 k = 0; k < 9; ++k) sm(k, r + 1) = (u32)u.signals[12 + k];
            S.rows[r][SEL_EVPOL4] = 1;
            r += 2;
        }
    }
    ZK_REQUIRE(r == n_used, "compressor12 setup: internal error: " + std::to_string(r) + " rows placed, " + std::to_string(n_used) + " counted");
    u64 max_id = 1;
    for (u32 v : S.s_map) max_id = std::max<u64>(max_id, v);
    S.key_bits = 8; while (S.key_bits < 32 && (max_id >> S.key_bits)) S.key_bits += 8;
}

// ---- the .pil text ---------------------------------------------------------------------------------------------------------------
// Written from the constraints the compressor states (compressor12_pil.rs:50- lists them), in the dialect tools/pilc.py compiles.
// Namespaces, column names, their order and the array lengths are interface: .const is indexed by them.
std::string render_pil(uint32_t n_bits, u64 n_publics) {
    std::string o;
    auto ln = [&](const std::string& s) { o += s; o += '\n'; };
    auto I = [](u64 v) { return std::to_string(v); };
    ln("let N: int = 2**" + I(n_bits) + ";");
    ln("");
    ln("namespace Global(N);");
    for (u64 i = 0; i < n_publics; i += 12) ln("    pol constant L" + I(i / 12 + 1) + ";");
    ln("");
    ln("namespace Compressor(N);");
    ln("    pol constant S[12];");
    ln("    pol constant C[12];");
    for (const char* s : {"PARTIAL", "POSEIDON12", "GATE", "CMULADD", "EVPOL4", "FFT4"}) ln(std::string("    pol constant ") + s + ";");
    ln("    pol commit a[12];");
    ln("");
    for (u64 i = 0; i < n_publics; ++i) ln("    public pub" + I(i) + " = a[" + I(i % 12) + "](" + I(i / 12) + ");");
    for (u64 i = 0; i < n_publics; ++i) ln("    Global.L" + I(i / 12 + 1) + " * (a[" + I(i % 12) + "] - :pub" + I(i) + ") = 0;");
    ln("");
    ln("    // four plain gates a row: two on the coefficients C[0..5), two on C[6..11)");
    for (int g = 0; g < 4; ++g) {
        const int a0 = 3 * g, c0 = g < 2 ? 0 : 6;
        const std::string n = "gate" + I(g);
        ln("    pol " + n + "_m = a[" + I(a0) + "]*a[" + I(a0 + 1) + "];");
        ln("    pol " + n + " = C[" + I(c0 + 3) + "]*" + n + "_m + C[" + I(c0) + "]*a[" + I(a0) + "] + C[" + I(c0 + 1) + "]*a[" + I(a0 + 1) + "] + C[" + I(c0 + 2) + "]*a[" + I(a0 + 2) + "] + C[" + I(c0 + 4) + "];");
        ln("    " + n + "*GATE = 0;");
    }
    ln("");
    ln("    // one Poseidon round a row: add the row's constants, x^7 (lanes 1..11 pass through in a partial round), the MDS matrix");
    for (int i = 0; i < 12; ++i) {
        const std::string p = "p" + I(i);
        ln("    pol " + p + "_1 = a[" + I(i) + "] + C[" + I(i) + "];");
        ln("    pol " + p + "_2 = " + p + "_1 * " + p + "_1;");
        ln("    pol " + p + "_4 = " + p + "_2 * " + p + "_2;");
        ln("    pol " + p + "_6 = " + p + "_4 * " + p + "_2;");
        ln("    pol " + p + "_7 = " + p + "_6 * " + p + "_1;");
        ln(i == 0 ? "    pol " + p + "_R = " + p + "_7;" : "    pol " + p + "_R = PARTIAL * (" + p + "_1 - " + p + "_7) + " + p + "_7;");
    }
    for (int i = 0; i < 12; ++i) {                      // out[i] = sum_j M[j][i] state[j]: the matrix our Poseidon uses (poseidon_gl_constants.h)
        std::string s = "    POSEIDON12 * (a[" + I(i) + "]' - (";
        for (int j = 0; j < 12; ++j) s += (j ? " + " : "") + I(ZK_POSEIDON_M[j * 12 + i]) + "*p" + I(j) + "_R";
        ln(s + ")) = 0;");
    }
    ln("");
    ln("    // CMulAdd: a[9..12) = a[0..3) * a[3..6) + a[6..9) in the cubic extension (x^3 = x - 1), Karatsuba form");
    for (int i = 0; i < 12; ++i) {
        const std::string e = "a[" + I(i) + "]", c = "C[" + I(i) + "]";
        if (i < 3) ln("    pol ca" + I(i) + " = (" + e + " + " + c + ")*C[9];");
        else if (i < 6) ln("    pol ca" + I(i) + " = " + e + " + " + c + ";");
        else if (i < 9) ln("    pol ca" + I(i) + " = (" + e + " + " + c + ")*C[10];");
        else ln("    pol ca" + I(i) + " = " + e + ";");
    }
    auto mul3 = [&](const std::string& n, const std::string a[3], const std::string b[3]) {        // the six products of a 3 x 3 Karatsuba
        ln("    pol " + n + "_A = (" + a[0] + " + " + a[1] + ") * (" + b[0] + " + " + b[1] + ");");
        ln("    pol " + n + "_B = (" + a[0] + " + " + a[2] + ") * (" + b[0] + " + " + b[2] + ");");
        ln("    pol " + n + "_C = (" + a[1] + " + " + a[2] + ") * (" + b[1] + " + " + b[2] + ");");
        ln("    pol " + n + "_D = " + a[0] + " * " + b[0] + ";");
        ln("    pol " + n + "_E = " + a[1] + " * " + b[1] + ";");
        ln("    pol " + n + "_F = " + a[2] + " * " + b[2] + ";");
    };
    {
        const std::string a[3] = {"ca0", "ca1", "ca2"}, b[3] = {"ca3", "ca4", "ca5"};
        mul3("cm", a, b);
        ln("    CMULADD * (ca9 - (cm_C + cm_D - cm_E - cm_F) - ca6) = 0;");
        ln("    CMULADD * (ca10 - (cm_A + cm_C - 2*cm_E - cm_D) - ca7) = 0;");
        ln("    CMULADD * (ca11 - (cm_B - cm_D + cm_E) - ca8) = 0;");
    }
    ln("");
    ln("    // FFT4: the next row is a 4-point (or two 2-point) transform of this row's four cubic-extension values");
    static const char* const fft_terms[4][6] = {           // sign and coefficient of (a[c], a[3+c], a[6+c], a[9+c], then the type-2 pair)
        {"+0", "+1", "+2", "+3", "+6:0", "+7:3"}, {"+0", "-1", "+4", "-5", "+6:0", "-7:3"},
        {"+0", "+1", "-2", "-3", "+6:6", "+8:9"}, {"+0", "-1", "-4", "+5", "+6:6", "-8:9"}};
    for (int q = 0; q < 4; ++q)
        for (int c = 0; c < 3; ++c) {
            std::string s = "    pol f" + I(3 * q + c) + " = ";
            for (int t = 0; t < 6; ++t) {
                const char* d = fft_terms[q][t];
                const int coef = d[1] - '0', col = t < 4 ? 3 * t : d[3] - '0';
                if (t) s += d[0] == '+' ? " + " : " - ";
                s += "C[" + I(coef) + "]*a[" + I(col + c) + "]";
            }
            ln(s + ";");
        }
    for (int i = 0; i < 12; ++i) ln("    FFT4 * (a[" + I(i) + "]' - f" + I(i) + ") = 0;");
    ln("");
    ln("    // EvPol4: Horner over four coefficients, ((((a[9..12) x + a[6..9)) x + a[3..6)) x + a[0..3)) with x = a'[3..6), started from a'[0..3)");
    {
        const std::string x[3] = {"a[3]'", "a[4]'", "a[5]'"};
        std::string acc[3] = {"a[0]'", "a[1]'", "a[2]'"};
        for (int step = 0; step < 4; ++step) {
            const std::string n = "ev" + I(step + 1);
            const int c = 9 - 3 * step;
            mul3(n, acc, x);
            ln("    pol " + n + "_0 = " + n + "_C + " + n + "_D - " + n + "_E - " + n + "_F + a[" + I(c) + "];");
            ln("    pol " + n + "_1 = " + n + "_A + " + n + "_C - 2*" + n + "_E - " + n + "_D + a[" + I(c + 1) + "];");
            ln("    pol " + n + "_2 = " + n + "_B - " + n + "_D + " + n + "_E + a[" + I(c + 2) + "];");
            for (int t = 0; t < 3; ++t) acc[t] = n + "_" + I(t);
        }
        for (int t = 0; t < 3; ++t) ln("    EVPOL4 * (a[" + I(6 + t) + "]' - " + acc[t] + ") = 0;");
    }
    ln("");
    std::string l = "    {", rr = "{";
    for (int i = 0; i < 12; ++i) { l += (i ? ", a[" : "a[") + I(i) + "]"; rr += (i ? ", S[" : "S[") + I(i) + "]"; }
    ln(l + "} connect " + rr + "};");
    return o;
}

std::string render_exec(const C12Setup& S) {               // compressor12_setup.rs:51-83, serde_json's compact array
    const u64 R = fmul(1ull << 32, 1ull << 32);            // 2^64 mod p: the raw word of an FGL is value * 2^64 (field_gl.rs:503-507)
    std::string o = "[" + std::to_string(S.pl.adds.size()) + "," + std::to_string(S.n_used);
    o.reserve(32 + S.pl.adds.size() * 60 + S.s_map.size() * 8);
    for (const Add& a : S.pl.adds) {
        o += ','; o += std::to_string(a.a); o += ','; o += std::to_string(a.b);
        o += ','; o += std::to_string(fmul(a.ca, R)); o += ','; o += std::to_string(fmul(a.cb, R));
    }
    for (u32 v : S.s_map) { o += ','; o += std::to_string(v); }
    o += ']';
    return o;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
// w^i from two tables: pw[i & 1023] = w^(i & 1023), pw[1024 + (i >> 10)] = w^(i & ~1023): no thread walks a power chain
constexpr uint32_t PW_LO = 1024;
struct Ks { u64 k[12]; };
__device__ __forceinline__ u64 s_identity(const u64* __restrict__ pw, const Ks& ks, u64 row, uint32_t col) {
    const u64 wi = gl::mul(pw[row & (PW_LO - 1)], pw[PW_LO + (row >> 10)]);
    return col ? gl::mul(wi, ks.k[col]) : wi;
}

// the 12 S columns alone: one thread a cell, 12 adjacent lanes write the 96 contiguous bytes of a row
__global__ __launch_bounds__(256) void c12_sigma_identity_kernel(const u64* __restrict__ pw, Ks ks, u64 n_rows, uint32_t n_const, uint32_t col0, u64* __restrict__ out) {
    const u64 c = blockIdx.x * 256ull + threadIdx.x;
    if (c >= n_rows * 12) return;
    const u64 row = c / 12; const uint32_t col = (uint32_t)(c - row * 12);
    out[row * n_const + col0 + col] = s_identity(pw, ks, row, col);
}

// the whole [N][n_const] matrix in one row-major pass: L_1..L_k | S (identity) | C and the selectors of the used rows, 0 below.
// block (32 columns, 8 rows): a lane per 8-byte cell, lanes adjacent along the row
__global__ __launch_bounds__(256) void c12_fill_kernel(const u64* __restrict__ pw, Ks ks, const u64* __restrict__ used_rows, u64 n_used, u64 n_rows,
                                                       uint32_t n_l, uint32_t n_const, u64* __restrict__ out) {
    const u64 row = blockIdx.x * 8ull + threadIdx.y;
    const uint32_t col = blockIdx.y * 32u + threadIdx.x;
    if (row >= n_rows || col >= n_const) return;
    u64 v;
    if (col < n_l) v = row == col;                                        // L_{col+1}: the unit vector of the public row `col`
    else if (col < n_l + 12) v = s_identity(pw, ks, row, col - n_l);
    else v = row < n_used ? used_rows[row * ROW_WORDS + (col - n_l - 12)] : 0;
    out[row * n_const + col] = v;
}

// ---- stable LSD radix sort of (key, position), 8 bits a pass.  A tile is SORT_TILE consecutive elements and belongs to ONE wave,
// which walks it 64 elements a round: the order inside a tile is (round, lane), the order of tiles is the block index.
constexpr uint32_t SORT_ITEMS = 32, SORT_TILE = 64 * SORT_ITEMS;
__global__ __launch_bounds__(64) void c12_sort_hist_kernel(const u32* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t n_tiles, u32* __restrict__ hist) {
    __shared__ u32 h[256];
    for (uint32_t d = threadIdx.x; d < 256; d += 64) h[d] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * SORT_TILE;
    for (uint32_t r = 0; r < SORT_ITEMS; ++r) {
        const uint32_t i = base + r * 64 + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);          // LDS atomics: a count has no order
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < 256; d += 64) hist[d * n_tiles + blockIdx.x] = h[d];   // digit-major: one scan gives every tile its offsets
}
// exclusive scan of m counts in place, one workgroup: a contiguous segment a thread, the 1024 segment sums scanned in LDS
__global__ __launch_bounds__(1024) void c12_sort_scan_kernel(u32* __restrict__ hist, uint32_t m) {
    __shared__ u32 s[2][1024];
    const uint32_t t = threadIdx.x, seg = (m + 1023) / 1024;
    const uint32_t lo = min(t * seg, m), hi = min(lo + seg, m);
    u32 sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += hist[i];
    int cur = 0;
    s[0][t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= off ? s[cur][t - off] : 0);
        cur ^= 1;
        __syncthreads();
    }
    u32 run = s[cur][t] - sum;
    for (uint32_t i = lo; i < hi; ++i) { const u32 c = hist[i]; hist[i] = run; run += c; }
}
__global__ __launch_bounds__(64) void c12_sort_scatter_kernel(const u32* __restrict__ keys, const u32* __restrict__ vals, uint32_t n, uint32_t shift, uint32_t n_tiles,
                                                              const u32* __restrict__ hist, u32* __restrict__ keys_out, u32* __restrict__ vals_out, int first_pass) {
    __shared__ u32 next[256];                                             // where the tile's next element of each digit goes
    for (uint32_t d = threadIdx.x; d < 256; d += 64) next[d] = hist[d * n_tiles + blockIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x, base = blockIdx.x * SORT_TILE;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t r = 0; r < SORT_ITEMS; ++r) {
        const uint32_t i = base + r * 64 + lane;
        const bool live = i < n;
        const u32 k = live ? keys[i] : 0, d = (k >> shift) & 255u;
        unsigned long long same = __ballot(live);                        // the lanes of this round that carry the same digit
        for (uint32_t b = 0; b < 8; ++b) {
            const unsigned long long set = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? set : ~set;
        }
        u32 dst = 0;
        if (live) dst = next[d] + (u32)__popcll(same & below);            // stable: lanes of a digit keep their order
        __syncthreads();
        if (live && (same & below) == 0) next[d] += (u32)__popcll(same); // the lowest lane of each digit moves its cursor
        __syncthreads();
        if (live && dst < n) { keys_out[dst] = k; vals_out[dst] = first_pass ? i : vals[i]; }
    }
}
// sorted (key, position): every element but the head of its run takes the identity of its predecessor's cell, the head the tail's
__global__ __launch_bounds__(256) void c12_wire_kernel(const u32* __restrict__ keys, const u32* __restrict__ pos, uint32_t n, const u64* __restrict__ pw, Ks ks,
                                                       uint32_t n_const, uint32_t col0, u64* __restrict__ out) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n) return;
    const u32 k = keys[e];
    if (k == 0) return;                                                   // 0 is "no wire"
    uint32_t src;
    if (e > 0 && keys[e - 1] == k) src = pos[e - 1];
    else {
        uint32_t lo = e, hi = n;                                          // the last element of the run: keys[lo] == k < keys[hi]
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (keys[mid] == k) lo = mid; else hi = mid; }
        if (lo == e) return;                                              // the signal's only cell keeps its own identity
        src = pos[lo];
    }
    const uint32_t p = pos[e], row = p / 12, col = p - row * 12, srow = src / 12;
    out[(u64)row * n_const + col0 + col] = s_identity(pw, ks, srow, src - srow * 12);
}

struct PowTable { DevBuf buf; Ks ks; };
void build_pow_table(uint32_t n_bits, PowTable& T) {
    const u64 w = gl::hroot(n_bits), n_hi = std::max<u64>(1, (1ull << n_bits) >> 10);
    std::vector<u64> h(PW_LO + n_hi);
    h[0] = 1;
    for (uint32_t i = 1; i < PW_LO; ++i) h[i] = gl::hmul(h[i - 1], w);
    const u64 w_hi = gl::hmul(h[PW_LO - 1], w);
    h[PW_LO] = 1;
    for (u64 i = 1; i < n_hi; ++i) h[PW_LO + i] = gl::hmul(h[PW_LO + i - 1], w_hi);
    T.buf.reserve(h.size() * 8);
    h2d_sync(T.buf.p, h.data(), h.size() * 8);
    T.ks.k[0] = 1;
    for (int j = 1; j < 12; ++j) T.ks.k[j] = gl::hmul(T.ks.k[j - 1], C12_K);
}

// the wiring of a [n_used][12] map onto S columns that already hold the identity
void wire_dev(const u32* d_s_map, u64 n_used, uint32_t key_bits, const PowTable& T, uint32_t n_const, uint32_t col0, u64* d_out, hipStream_t st) {
    const u64 n64 = n_used * 12;
    if (n64 == 0) return;
    ZK_REQUIRE(n64 < (1ull << 31), "compressor12 setup: more than 2^31 cells to wire");
    const uint32_t n = (uint32_t)n64, n_tiles = (n + SORT_TILE - 1) / SORT_TILE, m = 256 * n_tiles;
    DevBuf work;                                                          // keys and positions, twice; the tile histograms
    work.reserve(((size_t)n * 4 + m) * 4);
    u32* kbuf[2] = {(u32*)work.p, (u32*)work.p + n};
    u32* vbuf[2] = {(u32*)work.p + 2 * (size_t)n, (u32*)work.p + 3 * (size_t)n};
    u32* hist = (u32*)work.p + 4 * (size_t)n;
    const u32* k_in = d_s_map; const u32* v_in = vbuf[1];
    int cur = 0;
    for (uint32_t shift = 0; shift < key_bits; shift += 8) {
        hipLaunchKernelGGL(c12_sort_hist_kernel, dim3(n_tiles), dim3(64), 0, st, k_in, n, shift, n_tiles, hist);
        hipLaunchKernelGGL(c12_sort_scan_kernel, dim3(1), dim3(1024), 0, st, hist, m);
        hipLaunchKernelGGL(c12_sort_scatter_kernel, dim3(n_tiles), dim3(64), 0, st, k_in, v_in, n, shift, n_tiles, (const u32*)hist, kbuf[cur], vbuf[cur], shift == 0 ? 1 : 0);
        k_in = kbuf[cur]; v_in = vbuf[cur]; cur ^= 1;
    }
    hipLaunchKernelGGL(c12_wire_kernel, dim3((n + 255) / 256), dim3(256), 0, st, k_in, v_in, n, (const u64*)T.buf.p, T.ks, n_const, col0, d_out);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));                                     // the scratch goes back to the pool
}

}  // namespace

C12Setup* c12_setup_new(const void* r1cs, size_t len, uint32_t force_n_bits) {
    ZK_REQUIRE(r1cs, "compressor12 setup: null r1cs");
    const R1csGL rc = parse_r1cs_gl((const uint8_t*)r1cs, len);
    auto S = std::make_unique<C12Setup>();
    S->pl = r1cs2plonk(rc);
    pack_rows(rc, force_n_bits, *S);
    return S.release();
}
void c12_setup_free(C12Setup* s) { delete s; }
void c12_setup_info(const C12Setup* s, uint64_t out[6]) {
    out[0] = s->n_bits; out[1] = s->n_publics; out[2] = s->n_used; out[3] = s->n_const; out[4] = s->pl.gates.size(); out[5] = s->pl.adds.size();
}
void c12_setup_gates(const C12Setup* s, u64* out) {         // n_gates x (sl, sr, so, qm, ql, qr, qo, qc)
    for (const Gate& g : s->pl.gates) { std::memcpy(out, g.s, 24); std::memcpy(out + 3, g.q, 40); out += 8; }
}
std::string c12_setup_pil(const C12Setup* s) { return render_pil(s->n_bits, s->n_publics); }
std::string c12_setup_exec(const C12Setup* s) { return render_exec(*s); }

void c12_setup_consts_dev(const C12Setup* S, u64* d_out, hipStream_t st) {
    ZK_REQUIRE(S && d_out, "compressor12 setup: null argument");
    const u64 n_rows = 1ull << S->n_bits;
    PowTable T; build_pow_table(S->n_bits, T);
    DevBuf in;                                                            // the used rows, then the map
    const size_t rows_bytes = S->rows.size() * sizeof(ConstRow), map_bytes = S->s_map.size() * 4;
    in.reserve(rows_bytes + map_bytes);
    h2d_sync(in.p, S->rows.data(), rows_bytes);
    h2d_sync((char*)in.p + rows_bytes, S->s_map.data(), map_bytes);
    ZK_REQUIRE((n_rows + 7) / 8 < (1ull << 31), "compressor12 setup: too many rows");
    hipLaunchKernelGGL(c12_fill_kernel, dim3((unsigned)((n_rows + 7) / 8), (unsigned)((S->n_const + 31) / 32)), dim3(32, 8), 0, st,
                       (const u64*)T.buf.p, T.ks, (const u64*)in.p, S->n_used, n_rows, S->n_l, (uint32_t)S->n_const, d_out);
    ZK_HIP(hipGetLastError());
    wire_dev((const u32*)((char*)in.p + rows_bytes), S->n_used, S->key_bits, T, (uint32_t)S->n_const, S->n_l, d_out, st);
    ZK_HIP(hipStreamSynchronize(st));
}

void c12_sigma_dev(const u32* d_s_map, uint64_t n_used, uint32_t n_bits, uint32_t n_const, uint32_t col0, u64* d_out, hipStream_t st) {
    ZK_REQUIRE(d_out && (d_s_map || n_used == 0), "compressor12 sigma: null argument");
    ZK_REQUIRE(n_bits <= 32, "compressor12 sigma: n_bits above 32");
    ZK_REQUIRE(n_used <= (1ull << n_bits), "compressor12 sigma: the map has more rows than the trace");
    ZK_REQUIRE(n_const >= 12 && col0 <= n_const - 12, "compressor12 sigma: the 12 S columns do not fit the matrix");
    const u64 n_rows = 1ull << n_bits, blocks = (n_rows * 12 + 255) / 256;
    ZK_REQUIRE(blocks < (1ull << 31), "compressor12 sigma: too many rows");
    PowTable T; build_pow_table(n_bits, T);
    hipLaunchKernelGGL(c12_sigma_identity_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const u64*)T.buf.p, T.ks, n_rows, n_const, col0, d_out);
    ZK_HIP(hipGetLastError());
    wire_dev(d_s_map, n_used, 32, T, n_const, col0, d_out, st);
    ZK_HIP(hipStreamSynchronize(st));
}

}  // namespace zk
