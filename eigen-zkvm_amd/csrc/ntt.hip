// Goldilocks NTT / iNTT / LDE for gfx950 (MI355X).
//
// Replaces starky/src/fft_p.rs:174-355 (_fft, fft, ifft, interpolate) and fft_worker.rs:25-72.
// Same contract: row-major [1<<nbits][n_pols] matrix of canonical u64, natural order in and out,
// forward root w = MG.0[nbits] (constant.rs:54-68), inverse = 1/N * NTT with w^-1
// (== the reference's (n-BR(i))%n input permutation, fft_p.rs:124-142), LDE on the coset
// 49*<w_ext> (fft_p.rs:255-355).
//
// Design (not the reference's bit-reverse + blocked butterflies + transposes):
//   * Stockham auto-sort decomposition N = R_1*R_2*...; every pass reads R rows of `inner`
//     contiguous words (row stride N/R * n_pols) and writes runs of >= s*n_pols contiguous words,
//     so there is no bit-reversal pass and no transpose pass; natural order falls out.
//       pass with stride s (product of earlier radices), L = N/s, p < L/R, q < s:
//         out[(p*R + k)*s + q] = w_L^(p*k) * sum_j in[j*N/R + p*s + q] * w_R^(j*k)
//   * one workgroup = one tile of R (<=256) points x C = 4096/R adjacent lanes (a lane is one
//     (row-within-stride, column) pair, i.e. one contiguous u64 of the matrix row range);
//     each thread owns 16 points: radix-2^LOGA DIF in registers -> twiddle -> ONE LDS
//     transpose -> radix-2^LOGB DIF in registers -> inter-pass twiddle -> store.
//     A 2^24 transform is three such passes (8+8+8 bits), 2 LDS accesses / element / pass.
//   * twiddles w_N^e come from a two-level table (4096 + N/4096 entries, L2 resident); the
//     per-thread chain over the 16 outputs needs 2 lookups + 1 multiply per element.
//   * every table load of a tile goes out in one group right behind its data loads: no table address depends on the data.  A 16-lane
//     row shares its 16 entries of w256 (sub-step A) and, where 16 | s*n_pols, of the direct inter-pass table: one load per lane and a
//     DPP row broadcast at the use (2 + 2 table loads per lane where there were 15 + 16); the two-level look-ups of a chain ride along.
//     2^24 points 83.4 -> 85.7 GElem/s; the same loads in FRONT of the data loads gain nothing (profiles/r32/ntt_table_loads.md).
//   * the butterflies of a lane go two at a time through ntt_reg's paired form: the sums and differences of two butterflies as four carry
//     chains alternating inside one asm block, their shifts as two (gl::bfly2_m, gl::mul_pow2_2).  The single forms keep every dependent
//     instruction right behind its producer and write the wait states of each flag as s_nop; in a <4,4> kernel the vector instructions
//     that read what the one before them wrote fall from 56 % to 40 %, the written s_nop from 1 291 to 846, the same 2 802 vector
//     instructions (tools/asm_chain_stats.py).  2^24 points 84.8-86.8 -> 87.7-89.6 GElem/s, five
//     alternating runs each, slowest above the parent's fastest, 91 -> 93 VGPRs, five waves.  The twiddle products in the same form gained
//     nothing beside it and are not used here (profiles/r33/ntt_chains.md, tools/experiments/ntt_pair_products_r33.patch).
//   * HBM-bound: 16 B / element / pass; bytes per transform = 16 * passes * N * n_pols.  A pass reads every data word once, so the
//     sixteen data loads of a lane are non-temporal (the tables, which are re-read, and the stores are plain): 2^24 points 75.9 -> 82.3
//     GElem/s.  Measured on the same kernel and not kept: non-temporal stores (slower), LDS sized per launch, an XCD-contiguous
//     block -> tile order (slower), a raised wave priority up to the last data load (profiles/r10/ntt_stream.md).
#include "zk_internal.h"
#include "ntt_reg.hip.h"
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace zk {

namespace {

// elements per tile (a workgroup of NTT_TILE / 16 lanes, 8 bytes of LDS per element); tiles of 2048 and 1024 measured 24 % / 77 % slower
// (profiles/r05/ntt_bound.md; the switches of those runs: tools/experiments/rejected_switches_r02_r05.patch)
constexpr int NTT_TILE = 4096;
constexpr int TW_LO_BITS = 12;
constexpr int TW_LO = 1 << TW_LO_BITS;

struct PassParams {
    const u64* in;
    u64* out;
    const u64* w256;   // w_256^e, e < 256 (direction-specific)
    const u64* tw_lo;  // w_N^i, i < 4096
    const u64* tw_hi;  // w_N^(4096 i)
    const u64* tw_mid; // optional: w_N^(i << dshift), i < 2^16 -- direct inter-pass twiddles when L <= 2^16
    u64 pre_scale;     // constant folded into sub-step A (w256 is then the pre-scaled table); 1 = none
    u32 dshift;
    const u64* sc_lo;  // optional output scaling c * g^k (k = output row): g^i * c, i < 4096
    const u64* sc_hi;  // g^(4096 i)
    u64 sc_step;       // g^(RA * s)
    u64 out_scale;     // plain constant scaling (1 = none), used when sc_lo == nullptr
    u64 inner;         // (N/R) * n_pols : contiguous words per transform-axis index j
    u64 valid_in;      // words of `in` that exist; beyond that the input is implicit zero (LDE)
    u64 s_np;          // s * n_pols
    u32 np;
    u32 log_s;
    u32 has_tw;        // L > R (not the last pass)
    u32 row_p;         // tw_mid set, not the one-column thread order, 16 | s_np: the 16 lanes of a row share p (row-shared table loads)
};

// Lane SRC of every 16-lane row to the whole row: one DPP move per half (row_newbcast), no LDS and no memory.  Every lane of the row
// must be active.  Values entering and leaving a DPP move go through an empty asm (DESIGN_HISTORY.md section 3.9).  (The same by two
// ds_bpermute_b32 measured no faster and costs a wave of occupancy: profiles/r32/ntt_table_loads.md.)
__device__ __forceinline__ u32 dpp_opaque(u32 v) { asm volatile("" : "+v"(v)); return v; }
template <int SRC>
__device__ __forceinline__ u64 row_bcast(u64 v) {
    static_assert(SRC >= 0 && SRC < 16, "a lane of the row");
    const u32 v0 = dpp_opaque((u32)v), v1 = dpp_opaque((u32)(v >> 32));
    const u32 z0 = dpp_opaque((u32)__builtin_amdgcn_update_dpp(0, (int)v0, 0x150 + SRC, 0xF, 0xF, false));
    const u32 z1 = dpp_opaque((u32)__builtin_amdgcn_update_dpp(0, (int)v1, 0x150 + SRC, 0xF, 0xF, false));
    return gl::mk64(z0, z1);
}

template <int LOGA, int LOGB, bool KMODE, bool INV>
__global__ __launch_bounds__(NTT_TILE / 16) void ntt_pass_kernel(const PassParams P) {
    constexpr int LOGR = LOGA + LOGB, R = 1 << LOGR, RA = 1 << LOGA, RB = 1 << LOGB;
    constexpr int C = NTT_TILE / R;         // lanes per tile
    constexpr int GA = 16 / RA, GB = 16 / RB;  // independent sub-transforms per thread
    constexpr int TG = R / 16;                 // threads along the transform axis
    constexpr int PAD = KMODE ? 512 / R : 0;   // words; spreads kappa_a rows over banks (KMODE reads)
    constexpr int ROW = RB * C + PAD;
    static_assert(LOGR >= 4 && LOGR <= 8 && LOGA <= 4 && LOGB <= 4, "tile shape");
    __shared__ u64 lds[RA * ROW];

    const int t = threadIdx.x;
    const u64 u0 = (u64)blockIdx.x * C;

    // lane c of the tile -> (p, rem) = divmod(lane's word index within a transform-axis index, s n_pols); a dead lane is lane 0's.
    // p: a shift for one column; a 32-bit division when the matrix has fewer than 2^32 words per transform-axis index (every size
    // in use); the 64-bit division otherwise -- uniform branches, the general case cost ~100 instructions per lane
    auto lane_pos = [&](int c, u64& p, u64& rem) {
        const u64 u = u0 + c, uc = u < P.inner ? u : 0;
        if (P.np == 1) { p = uc >> P.log_s; rem = uc & (((u64)1 << P.log_s) - 1); }
        else if ((P.inner >> 32) == 0) { const u32 p32 = (u32)uc / (u32)P.s_np; p = p32; rem = (u32)uc - p32 * (u32)P.s_np; }
        else
        { p = uc / P.s_np; rem = uc - p * P.s_np; }
    };
    // sub-step B's thread order
    const int cb = KMODE ? t / TG : t % C, tb = KMODE ? t % TG : t / C;

    // ---- The table values of a tile.  No table address depends on the data, so every table load of a tile is requested in one group
    // right behind the data loads (request_tables, called below): one trip through the vector-memory pipe per tile.  Behind, not in
    // front: a wave's loads return in order, and a table load that misses L2 in front of the data holds the data back (measured).
    // The 16 lanes of a row (t / 16) share ta, and tb outside the one-column order, so a row's 16 entries of a table are fetched one per
    // lane and handed round by row_bcast at the point of use: two registers held per table, where sixteen per-lane values held from
    // the top would cost a wave of occupancy.
    static_assert(C % 16 == 0 && GA * RA == 16 && GB * RB == 16, "a 16-lane row shares ta and owns 16 table entries");
    const int r16 = t & 15;
    // sub-step A: entry (g, ka) = w256[(jb ka) << (8 - LOGR)], jb = ta GA + g, in lane g RA + ka of the row
    const bool shift_a = LOGR <= 6 && C >= 64 && LOGB > 0 && P.pre_scale == 1;   // the twiddles of sub-step A are shifts (below)
    u64 wa = 0;
    // sub-step B, direct table, p shared by the row (taken from the row's first lane): entry (g, kb) = tw_mid[(p kappa) << sh],
    // kappa = tb + g TG + RA kb, in lane g RB + kb.  (inner is a multiple of 16 here: a row is wholly live or wholly dead.)
    u64 wm = 0;
    const bool row_p = !KMODE && P.row_p;
    // sub-step B, two-level table w^e = hi[e >> 12] lo[e & 4095] (L > 2^16), or the scaled last pass of an extension: the first factor
    // of each chain and the chain's step.  The two halves of each look-up are requested with the rest and multiplied once sub-step A
    // is through.  The products are NOT canonical (some u64 congruent to them): every use is a factor of a further product
    // (gl::mul_tw / gl::mul_tw_nc take any u64), so the canonicalisation would be spent for nothing.
    const bool chain_tab = !P.tw_mid && (P.has_tw || P.sc_lo);
    u64 f0[GB], tw_step = 1, t2h[GB + 1], t2l[GB + 1];
    auto request_tables = [&]() {
        if (LOGB > 0 && !shift_a) wa = P.w256[(((t / C) * GA + r16 / RA) * (r16 % RA)) << (8 - LOGR)];
        if (row_p) {
            u64 p, rem;
            lane_pos(cb & ~15, p, rem);
            const u32 kappa = tb + (r16 / RB) * TG + RA * (r16 % RB);
            wm = *(const u64*)((const char*)P.tw_mid + (u32)((((u32)p * kappa) << (P.log_s - P.dshift)) * 8));
        }
        if (chain_tab) {
            u64 p, rem;
            lane_pos(cb, p, rem);
            const u64 row_q = !P.sc_lo ? 0 : P.np == 1 ? rem : (P.inner >> 32) == 0 ? (u64)((u32)rem / P.np) : rem / P.np;  // output row = kappa*s + row_q (last pass: p == 0)
            const u64 es = (p * RA) << P.log_s;
            t2h[GB] = P.has_tw ? P.tw_hi[es >> TW_LO_BITS] : 1; t2l[GB] = P.has_tw ? P.tw_lo[es & (TW_LO - 1)] : 1;
            const u64* __restrict__ hi = P.sc_lo ? P.sc_hi : P.tw_hi;
            const u64* __restrict__ lo = P.sc_lo ? P.sc_lo : P.tw_lo;
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const int ka = tb + g * TG;
                const u64 e = P.sc_lo ? ((u64)ka << P.log_s) + row_q : (p * ka) << P.log_s;
                t2h[g] = hi[e >> TW_LO_BITS]; t2l[g] = lo[e & (TW_LO - 1)];
            }
        }
    };
    u64 tw[GB][RB];   // per-lane entries of the direct table where p differs inside a row

    {   // ---- sub-step A: RA-point transforms over ja (j = ja*RB + jb), twiddle w_R^(jb*ka)
        const int c = t % C, ta = t / C;
        const u64 u = u0 + c;
        const bool live = u < P.inner;
        u64 x[GA][RA];
        // Whole tile inside the matrix and inside the rows that exist (wave-uniform test): sixteen unconditional loads,
        // issued back to back.  Otherwise (ragged last tile, or the zero-padded half of an extension's first forward
        // pass) every load still goes out unconditionally -- of word 0 where there is nothing to read -- and is zeroed afterwards: a
        // branch per element would serialise the loads behind each other's latency.
        // The data loads are non-temporal: a pass reads each word once, and lines that do not linger in L2 leave it to the tables.
        const bool full = u0 + C <= P.inner && (u64)(R - 1) * P.inner + u0 + C <= P.valid_in;
        const u64* __restrict__ base = P.in + (u64)(ta * GA) * P.inner + (live ? u : 0);
        if (full) {
#pragma unroll
            for (int g = 0; g < GA; ++g)
#pragma unroll
                for (int ja = 0; ja < RA; ++ja) x[g][ja] = __builtin_nontemporal_load(&base[(u64)(ja * RB + g) * P.inner]);
        } else {
#pragma unroll
            for (int g = 0; g < GA; ++g)
#pragma unroll
                for (int ja = 0; ja < RA; ++ja) {
                    const u64 off = (u64)(ja * RB + g) * P.inner;
                    const bool ok = live && (u64)(ta * GA) * P.inner + off + u < P.valid_in;
                    const u64 v = __builtin_nontemporal_load(ok ? base + off : P.in);      // word 0 always exists
                    x[g][ja] = ok ? v : 0;
                }
        }
        request_tables();
#pragma unroll
        for (int g = 0; g < GA; ++g) ntt_reg<LOGA, INV, true>(x[g]);
        // Passes of <= 6 bits: w_R is a power of two (w_64 = 2^39, ntt_reg.hip.h), so the twiddle w_R^(jb ka) between the two halves is a
        // shift like the butterflies' own -- once jb is a compile-time number.  jb = ta GA + g and ta = t / C with C = 4096 / R >= 64
        // lanes: the same in every lane of a wave, so a switch over ta (R / 16 <= 4 cases) costs no divergence and turns the 15 general
        // products of a lane into 15 shifts.  (Not for the pre-scaled last pass of a plain inverse transform: its 1/N rides on the table.)
        if (shift_a) {
            static_for<0, TG>([&](auto TA) {
                constexpr int ta_c = decltype(TA)::value;
                if (ta == ta_c) {
                    static_for<0, GA>([&](auto GI) {
                        constexpr int g = decltype(GI)::value, jb = ta_c * GA + g;
                        static_for<0, RA>([&](auto KA) {
                            constexpr int ka = decltype(KA)::value;
                            constexpr int e0 = (39 * (64 / (R > 64 ? 64 : R)) * jb * ka) % 192, e = INV ? (192 - e0) % 192 : e0;   // w_R^(+-jb ka) = 2^e
                            u64 v = x[g][bitrev_c(ka, LOGA)];
                            if constexpr (e >= 96) v = gl::neg(gl::mul_pow2<e - 96>(v));
                            else v = gl::mul_pow2<e>(v);
                            lds[ka * ROW + jb * C + c] = v;
                        });
                    });
                }
            });
        } else
        {   // the general products, by the row's entries of the table (dead lanes take part: a broadcast needs the whole row)
            static_for<0, GA>([&](auto GI) {
                constexpr int g = decltype(GI)::value;
                const int jb = ta * GA + g;   // entry (g, ka) of the row is w256[(jb ka) << (8 - LOGR)]
                static_for<0, RA>([&](auto KA) {
                    constexpr int ka = decltype(KA)::value;
                    u64 v = x[g][bitrev_c(ka, LOGA)];
                    if (LOGB > 0 && ka > 0) v = gl::mul_tw(v, row_bcast<g * RA + ka>(wa));
                    else if (P.pre_scale != 1) v = gl::mul_tw(v, P.pre_scale);
                    lds[ka * ROW + jb * C + c] = v;
                });
            });
        }
    }
    // per-lane entries of the direct table (p differs inside a row: the one-column thread order, s n_pols no multiple of 16): every
    // twiddle w_L^(p*kappa) is one load from the 512 KB table (L2), no chain; requested here, where sub-step A's registers are free
    // again, so that the barrier, the LDS reads and the radix-2^LOGB butterflies hide the latency.  Entry (p kappa) << (log_s - dshift)
    // of the table (it is only set where log_s >= dshift), below 2^16: linear in kb, so one 32-bit byte offset per ka and one add per entry
    auto load_mid = [&]() {
        u64 p, rem;
        lane_pos(cb, p, rem);
        const u32 sh = P.log_s - P.dshift, istep = (((u32)p * RA) << sh) * 8;
#pragma unroll
        for (int g = 0; g < GB; ++g) {
            const u32 ka = tb + g * TG, i0 = (((u32)p * ka) << sh) * 8;
#pragma unroll
            for (int kb = 0; kb < RB; ++kb) tw[g][kb] = *(const u64*)((const char*)P.tw_mid + (u32)(i0 + kb * istep));
        }
    };
    // (a uniform run-time branch on purpose: as `if constexpr` the compiler sinks these loads below the
    // butterflies to save registers and the L2 latency lands on the critical path again)
    if (P.tw_mid && !row_p) load_mid();
#pragma unroll
    for (int g = 0; g < GB; ++g) f0[g] = P.out_scale;
    if (chain_tab) {   // the two halves of each look-up arrived with the data
#pragma unroll
        for (int g = 0; g < GB; ++g) f0[g] = gl::mul_tw_nc(t2h[g], t2l[g]);
        if (P.has_tw) tw_step = gl::mul_tw_nc(t2h[GB], t2l[GB]);
    }
    __syncthreads();
    {   // ---- sub-step B: RB-point transforms over jb -> kappa = RA*kb + ka
        const int c = cb;
        const u64 u = u0 + c;
        u64 y[GB][RB];
#pragma unroll
        for (int g = 0; g < GB; ++g) {
            const int ka = tb + g * TG;
#pragma unroll
            for (int jb = 0; jb < RB; ++jb) y[g][jb] = lds[ka * ROW + jb * C + c];
        }
#pragma unroll
        for (int g = 0; g < GB; ++g) ntt_reg<LOGB, INV, true>(y[g]);
        if (row_p) {   // the inter-pass twiddles by the row's entries of the table, in front of the exit of the dead lanes
            static_for<0, GB>([&](auto GI) {
                constexpr int g = decltype(GI)::value;
                static_for<0, RB>([&](auto KB) {
                    constexpr int kb = decltype(KB)::value;
                    u64& v = y[g][bitrev_c(kb, LOGB)];
                    v = gl::mul_tw(v, row_bcast<g * RB + kb>(wm));
                });
            });
        }
        if (u >= P.inner) return;
        u64 p, rem;
        lane_pos(c, p, rem);

        // output kappa = RA kb + ka of the lane lies (RA kb + ka) s_np words past the lane's base: linear in kb.  Whole matrix under 4 GiB
        // (uniform): a lane's stores are then a uniform base plus a 32-bit byte offset, one add per store where the general form
        // multiplies and adds in 64 bits.  (The same for the data loads of sub-step A gained nothing: 40 against 37 instructions.)
        auto finish = [&](auto small_c) {
            constexpr bool SMALL = decltype(small_c)::value;
            u64* __restrict__ outp = P.out + p * R * P.s_np + rem;
            const u64 kstride = P.s_np;                    // words between the outputs kappa and kappa + 1 of a lane
            const u32 b0 = ((u32)p * R * (u32)P.s_np + (u32)rem) * 8, bstep = RA * (u32)P.s_np * 8;
            auto put = [&](u32 ka, int kb, u64 v) {
                if constexpr (SMALL) *(u64*)((char*)P.out + (u32)(b0 + ka * (u32)P.s_np * 8 + kb * bstep)) = v;
                else outp[(u64)(RA * kb + ka) * kstride] = v;
            };
            if (row_p) {   // twiddled above
#pragma unroll
                for (int g = 0; g < GB; ++g)
#pragma unroll
                    for (int kb = 0; kb < RB; ++kb) put(tb + g * TG, kb, y[g][bitrev_c(kb, LOGB)]);
                return;
            }
            if (P.tw_mid) {
#pragma unroll
                for (int g = 0; g < GB; ++g) {
                    const int ka = tb + g * TG;
#pragma unroll
                    for (int kb = 0; kb < RB; ++kb) {
                        u64 v = y[g][bitrev_c(kb, LOGB)];
                        v = gl::mul_tw(v, tw[g][kb]);
                        put(ka, kb, v);
                    }
                }
                return;
            }
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const int ka = tb + g * TG;
                u64 f = f0[g];                                              // the chain's first factor, looked up with the data
                const bool scaled = P.has_tw || P.sc_lo || P.out_scale != 1;
                const u64 fstep = P.sc_lo ? P.sc_step : tw_step;
#pragma unroll
                for (int kb = 0; kb < RB; ++kb) {
                    u64 v = y[g][bitrev_c(kb, LOGB)];
                    if (scaled) {
                        v = gl::mul_tw(v, f);                               // canonical: it is stored
                        if (kb + 1 < RB) f = gl::mul_tw_nc(f, fstep);       // the running factor only ever feeds products
                    }
                    put(ka, kb, v);
                }
            }
        };
        if (((P.inner * R) >> 29) == 0) finish(std::true_type{});
        else finish(std::false_type{});
    }
}

// Direct evaluation for transforms shorter than one register tile (nbits < 4): out[k][c] =
// scale(k) * sum_{i < n_in} in[i][c] * w^(i k).  A handful of rows; never on a hot path.
__global__ void ntt_small_kernel(const u64* in, u64* out, u32 np, u32 n_in, u32 n, u64 w, u64 g, u64 cst) {
    const u32 tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n * np) return;
    const u32 k = tid / np, c = tid % np;
    const u64 wk = gl::pow(w, k);
    u64 acc = 0, cur = 1;
    for (u32 i = 0; i < n_in; ++i) { acc = gl::add(acc, gl::mul(in[(u64)i * np + c], cur)); cur = gl::mul(cur, wk); }
    out[(u64)k * np + c] = gl::mul(acc, gl::mul(cst, gl::pow(g, k)));
}

// ---- host side: tables + plan -------------------------------------------------------------
struct Tables { DevConst w256, w256s, lo, hi, mid; u32 dshift = 0; };
struct ScaleTables { DevConst lo, hi; };

// kept for the life of the process, per device; the maps are never destroyed (DevConst, zk_internal.h)
std::mutex g_mu;
auto& g_tables = *new std::map<std::pair<int, std::pair<u32, int>>, Tables>;       // (device,(nbits,inverse))
auto& g_scales = *new std::map<std::pair<int, std::pair<u32, u64>>, ScaleTables>;  // (device,(nbits,g))

void two_level(u64 base, u64 cst, u32 nbits, std::vector<u64>& lo, std::vector<u64>& hi) {
    lo.resize(TW_LO);
    u64 c = cst;
    for (int i = 0; i < TW_LO; ++i) { lo[i] = c; c = gl::hmul(c, base); }
    size_t nh = nbits > (u32)TW_LO_BITS ? (size_t)1 << (nbits - TW_LO_BITS) : 1;
    hi.resize(nh);
    u64 step = gl::hpow(base, TW_LO);
    c = 1;
    for (size_t i = 0; i < nh; ++i) { hi[i] = c; c = gl::hmul(c, step); }
}

const Tables& get_tables(u32 nbits, bool inverse) {
    int dev; ZK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mu);
    auto key = std::make_pair(dev, std::make_pair(nbits, (int)inverse));
    auto it = g_tables.find(key);
    if (it != g_tables.end()) return it->second;
    u64 w = gl::hroot(nbits), w8 = gl::hroot(8);
    if (inverse) { w = gl::hinv(w); w8 = gl::hinv(w8); }
    std::vector<u64> t256(256), lo, hi;
    u64 c = 1;
    for (int i = 0; i < 256; ++i) { t256[i] = c; c = gl::hmul(c, w8); }
    two_level(w, 1, nbits, lo, hi);
    Tables T; T.w256 = DevConst(t256); T.lo = DevConst(lo); T.hi = DevConst(hi);
    if (inverse) {  // w_256^-e / N: folds the inverse transform's 1/N into sub-step A of its last pass
        const u64 ninv = gl::hinv((1ull << nbits) % GL_P);
        std::vector<u64> t256s(256);
        for (int i = 0; i < 256; ++i) t256s[i] = gl::hmul(t256[i], ninv);
        T.w256s = DevConst(t256s);
    }
    {   // direct table for passes with L <= 2^16: w_N^(i << dshift)
        T.dshift = nbits > 16 ? nbits - 16 : 0;
        const size_t nm = (size_t)1 << (nbits - T.dshift);
        std::vector<u64> mid(nm);
        const u64 step = gl::hpow(w, 1ull << T.dshift);
        c = 1;
        for (size_t i = 0; i < nm; ++i) { mid[i] = c; c = gl::hmul(c, step); }
        T.mid = DevConst(mid);
    }
    return g_tables.emplace(key, std::move(T)).first->second;
}

const ScaleTables& get_scale(u32 nbits, u64 g, u64 cst) {  // cst * g^k, k < 2^nbits
    int dev; ZK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mu);
    auto key = std::make_pair(dev, std::make_pair(nbits, g));
    auto it = g_scales.find(key);
    if (it != g_scales.end()) return it->second;
    std::vector<u64> lo, hi;
    two_level(g, cst, nbits, lo, hi);
    ScaleTables S; S.lo = DevConst(lo); S.hi = DevConst(hi);
    return g_scales.emplace(key, std::move(S)).first->second;
}

template <int LOGA, int LOGB>
void launch_pass(const PassParams& P, bool kmode, bool inverse, hipStream_t st) {
    constexpr int C = NTT_TILE >> (LOGA + LOGB);
    const u64 blocks = (P.inner + C - 1) / C;
    ZK_REQUIRE(blocks < (1ull << 31), "ntt: grid too large");
    const dim3 g((u32)blocks), b(NTT_TILE / 16);
    const int variant = (kmode ? 2 : 0) | (inverse ? 1 : 0);
#define ZK_PASS(K, I) hipLaunchKernelGGL((ntt_pass_kernel<LOGA, LOGB, K, I>), g, b, 0, st, P)
    switch (variant) {
        case 0: ZK_PASS(false, false); break; case 1: ZK_PASS(false, true); break;
        case 2: ZK_PASS(true, false); break;  default: ZK_PASS(true, true); break;
    }
#undef ZK_PASS
    ZK_HIP(hipGetLastError());
}

void launch_pass_logr(int logr, const PassParams& P, bool kmode, bool inverse, hipStream_t st) {
    switch (logr) {
        case 4: launch_pass<2, 2>(P, kmode, inverse, st); break;
        case 5: launch_pass<3, 2>(P, kmode, inverse, st); break;
        case 6: launch_pass<3, 3>(P, kmode, inverse, st); break;
        case 7: launch_pass<4, 3>(P, kmode, inverse, st); break;
        case 8: launch_pass<4, 4>(P, kmode, inverse, st); break;
        default: throw Error("ntt: unsupported pass radix");
    }
}

// radices of the passes of a 2^nbits transform (each 4..8 bits); empty for nbits < 4
std::vector<int> plan(u32 nbits) {
    std::vector<int> r;
    if (nbits < 4) return r;
    int np = (nbits + 7) / 8;
    int base = nbits / np, extra = nbits % np;
    for (int i = 0; i < np; ++i) r.push_back(base + (i < extra ? 1 : 0));
    return r;
}

// One transform of size 2^nbits whose input holds `valid_rows` rows (rest implicit zero).
// bufs: sequence of distinct buffers the passes ping-pong through, bufs[0] = input,
// bufs.back() = output.  scale: optional (g, cst) output scaling cst*g^row; out_scale: constant.
struct Scale { bool on = false; u64 g = 1, cst = 1; };

void run_transform(const u64* in, u64* a, u64* b, /* ping-pong, result must land in `a` */
                   u32 n_pols, u32 nbits, u64 valid_rows, bool inverse, Scale sc, u64 out_scale, hipStream_t st) {
    const u64 n = 1ull << nbits;
    if (nbits < 4) {
        u64 w = gl::hroot(nbits);
        if (inverse) w = gl::hinv(w);
        u64 cst = sc.on ? sc.cst : out_scale;
        u64 g = sc.on ? sc.g : 1;
        u32 total = (u32)(n * n_pols);
        hipLaunchKernelGGL(ntt_small_kernel, dim3((total + 255) / 256), dim3(256), 0, st, in, a, n_pols,
                           (u32)valid_rows, (u32)n, w, g, cst);
        ZK_HIP(hipGetLastError());
        return;
    }
    const std::vector<int> radices = plan(nbits);
    const int np = (int)radices.size();
    const Tables& T = get_tables(nbits, inverse);
    const ScaleTables* S = sc.on ? &get_scale(nbits, sc.g, sc.cst) : nullptr;
    u32 log_s = 0;
    const u64* cur = in;
    for (int i = 0; i < np; ++i) {
        const int logr = radices[i];
        u64* dstbuf = ((np - 1 - i) % 2 == 0) ? a : b;
        const bool last = (i == np - 1);
        PassParams P{};
        P.in = cur; P.out = dstbuf;
        P.w256 = T.w256.u(); P.tw_lo = T.lo.u(); P.tw_hi = T.hi.u();
        P.sc_lo = (last && sc.on) ? S->lo.u() : nullptr;
        P.sc_hi = (last && sc.on) ? S->hi.u() : nullptr;
        const int loga = (logr + 1) / 2;
        P.sc_step = (last && sc.on) ? gl::hpow(sc.g, (1ull << loga) << log_s) : 1;
        P.out_scale = 1; P.pre_scale = 1;
        if (last && !sc.on && out_scale != 1) {
            // the only constant scaling in use is the inverse transform's 1/N (ntt_dev)
            ZK_REQUIRE(inverse && out_scale == gl::hinv(n % GL_P), "ntt: unsupported constant scaling");
            P.w256 = T.w256s.u(); P.pre_scale = out_scale;
        }
        P.inner = (n >> logr) * n_pols;
        P.valid_in = (i == 0) ? valid_rows * n_pols : n * n_pols;
        P.s_np = ((u64)1 << log_s) * n_pols;
        P.np = n_pols;
        P.log_s = log_s;
        P.has_tw = last ? 0 : 1;
        P.dshift = T.dshift;
        P.tw_mid = (!last && log_s >= T.dshift) ? T.mid.u() : nullptr;  // L = N >> log_s <= 2^16
        const bool kmode = P.s_np < 16;
        P.row_p = (P.tw_mid && !kmode && P.s_np % 16 == 0) ? 1 : 0;
        launch_pass_logr(logr, P, kmode, inverse, st);
        cur = dstbuf;
        log_s += logr;
    }
}

}  // namespace

int ntt_num_passes(uint32_t nbits) { return nbits < 4 ? 1 : (int)plan(nbits).size(); }

const u64* ntt_w256_table(bool inverse) { return get_tables(8, inverse).w256.u(); }

void ntt_dev(const u64* d_src, u64* d_dst, u64* d_tmp, uint32_t n_pols, uint32_t nbits, bool inverse, hipStream_t st) {
    ZK_REQUIRE(nbits <= 32, "ntt: nbits > 32");
    if (n_pols == 0) return;
    ZK_REQUIRE(d_src != d_dst, "ntt: dst may not alias src");
    u64 out_scale = inverse ? gl::hinv((1ull << nbits) % GL_P) : 1;
    run_transform(d_src, d_dst, d_tmp, n_pols, nbits, 1ull << nbits, inverse, Scale{}, out_scale, st);
}

void lde_dev(const u64* d_src, u64* d_dst, u64* d_tmp, uint32_t n_pols, uint32_t nbits, uint32_t nbits_ext, hipStream_t st) {
    ZK_REQUIRE(nbits_ext <= 32 && nbits <= nbits_ext, "lde: need nbits <= nbits_ext <= 32");
    if (n_pols == 0) return;  // fft_p.rs:262-264
    ZK_REQUIRE(d_src != d_dst, "lde: dst may not alias src");
    const u64 n = 1ull << nbits;
    // (Blow-up 2 as two size-N coset transforms with interleaved output rows instead of one 2N-point transform over a half-zero input was
    // measured in round 3: bit-exact, 18.7 against 15.2 ms for 19 columns at 2^24 -- tools/experiments/rejected_switches_r02_r05.patch.)
    // coefficients * 49^i / N  (fft_p.rs:144-172): the inverse transform's last pass applies it.
    Scale sc; sc.on = true; sc.g = 49; sc.cst = gl::hinv(n % GL_P);
    const int fwd_passes = ntt_num_passes(nbits_ext);
    // forward transform must end in d_dst; its input (the coefficient buffer) must differ from
    // the first forward pass's output: forward pass i writes (fwd_passes-1-i)%2==0 ? dst : tmp.
    u64* first_fwd_out = ((fwd_passes - 1) % 2 == 0) ? d_dst : d_tmp;
    u64* coef = (first_fwd_out == d_dst) ? d_tmp : d_dst;
    u64* other = (coef == d_dst) ? d_tmp : d_dst;
    run_transform(d_src, coef, other, n_pols, nbits, n, true, sc, 1, st);
    run_transform(coef, d_dst, d_tmp, n_pols, nbits_ext, n, false, Scale{}, 1, st);
}

}  // namespace zk
