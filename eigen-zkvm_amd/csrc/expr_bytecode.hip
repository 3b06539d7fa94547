// Constraint-polynomial evaluation without run-time compilation: a bytecode interpreter.
//
// The second evaluator behind zk_program_t (the first: expr_jit.hip, which turns a step program into HIP text for hipRTC).
// Like the reference's own evaluator (starky/src/interpreter.rs:91-175 Block::eval, :187-225 compile_code) this one
// interprets; unlike it, the program is assembled once into fixed-width instructions for ONE kernel that hipcc compiles
// into libzkgpu.so, and one lane evaluates one row.  Assembling needs no GPU, no hipRTC and no helper process.
//
// The assembler (host):
//   * resolves the F3G `dim` of every value as Gen::instr does (f3g.rs:323-449): the opcode says add/sub/mul x {11, 13, 31, 33}
//     or copy1 / copy3, the kernel never tests a dim;
//   * rejects what the translator rejects, with its messages (tmp read before write, a column written at one row and read at
//     the next: zk_internal.h check_row_hazards, shared).  One difference: the translator hoists every read in front of every
//     store and therefore rejects "a read partially overlaps an earlier write of the same row"; the interpreter executes in
//     program order, a lane's own store followed by its own load is ordered, and that program is accepted here;
//   * renumbers temporaries to slots by liveness (the last use frees the slot): the slot count is the peak live width, not
//     the number of tmp ids.  Slots are 1 or 3 words.  BC_LDS_WORDS word-slots per wave live in LDS, laid out [slot][lane]
//     in 8-byte words (consecutive lanes, consecutive banks; a wave owns its region: no barrier); the shortest-lived values
//     are placed there first.  What does not fit lives in a pooled arena in HBM laid out [slot][lane of the grid] (coalesced):
//     no valid program is too large, only slower;
//   * gathers the wave-uniform operands (number, public, challenge, eval) into one table that lives in the program and is
//     refreshed on the stream in front of every run from the zk_eval_ctx pointers (with the section pointers in front of it);
//   * keeps plain evaluation: no Horner-chain or power-table rewriting.  Field arithmetic is exact: the same canonical words.
//
// The kernel: the instruction stream is wave-uniform and comes through a const __restrict__ pointer at a uniform index
// (scalar loads), dispatch is a switch that never diverges; section cells are read and written where the program has them,
// at offset + ((i + next * prime) & (n - 1)) * stride.  The grid is capped (BC_MAX_WAVES) and a wave walks its 64-row chunks,
// so the arena's size follows the grid, not the domain.
#include "zk_internal.h"
#include "pil_check.h"
#include "../../include/zkgpu.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <queue>
#include <set>
#include <sstream>
#include <tuple>
#include <vector>

namespace zk {

namespace {

// 40 word-slots x 64 lanes x 8 B = 20 KiB per wave (= per block): eight waves per CU out of its 160 KiB, two per SIMD --
// the interpreter waits on a scalar fetch and an LDS or memory round trip per instruction, a second wave fills those gaps
constexpr uint32_t BC_LDS_WORDS = 40;
constexpr uint32_t BC_MAX_WAVES = 4096;        // 16 waves per CU's worth of chunks in flight; 2 MiB of arena per word-slot
constexpr uint32_t BC_STRIDE_BITS = 27;        // a section cell's second word: stride | buf << 27 | prime << 31

enum : uint32_t { K_NONE = 0, K_LDS = 1, K_ARENA = 2, K_UNI = 3, K_MEM = 4, K_X = 5, K_ZI = 6, K_XDIV = 7, K_XDIVW = 8 };
// opcode = 4 * {add, sub, mul} + 2 * (first source is dim 3) + (second source is dim 3); then the two copies
enum : uint32_t { BC_COPY1 = 12, BC_COPY3 = 13 };
// the checker's instruction (pil_check.h): a live lane whose dim-1 source is not 0 counts in count[id] and lowers first[id] to its row
enum : uint32_t { BC_CHECK1 = 14 };
// the table a run reads its pointers and uniform values from, in words
enum : uint32_t { T_BUFS = 0, T_X = 16, T_ZI = 17, T_ZI_MASK = 18, T_XDIV = 19, T_XDIVW = 20, T_UNI = 21 };

struct alignas(32) BcInstr { uint32_t w[8]; };     // op | kinds of a, b, dest << 8, 12, 16;  a, b, dest: two words each
struct BcUni { uint32_t kind, id, off, words; u64 value; };   // one uniform operand: where it comes from, where it sits in the table

using gl::f3;

__global__ __launch_bounds__(64) void zk_bc_refresh_kernel(const zk_eval_ctx c, const BcUni* __restrict__ desc, uint32_t n_desc, u64* __restrict__ tab) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 16) {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) if (t == k) tab[T_BUFS + k] = (u64)c.bufs[k];
    } else if (t == T_X) tab[T_X] = (u64)c.x;
    else if (t == T_ZI) tab[T_ZI] = (u64)c.zi;
    else if (t == T_ZI_MASK) tab[T_ZI_MASK] = c.zi_mask;
    else if (t == T_XDIV) tab[T_XDIV] = (u64)c.xdivxsubxi;
    else if (t == T_XDIVW) tab[T_XDIVW] = (u64)c.xdivxsubwxi;
    else if (t >= 64 && t - 64 < n_desc) {
        const BcUni d = desc[t - 64];
        u64* o = tab + d.off;
        if (d.kind == ZK_OPND_NUMBER) o[0] = d.value;
        else if (d.kind == ZK_OPND_PUBLIC) o[0] = c.publics[d.id];
        else {
            const uint64_t* s = (d.kind == ZK_OPND_CHALLENGE ? c.challenges : c.evals) + 3 * (u64)d.id;
            o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        }
    }
}

struct BcLane {
    u64* lds;                    // this lane's column of the wave's slot file: slot s at lds[64 * s]
    u64* arena;                  // this lane's column of the arena: slot s at arena[stride * s]
    u64 arena_stride;
    const u64* __restrict__ tab;
    u64 i, ip;                   // this lane's row and the row `next` further on
};

// pointers that come out of the table are words: named global here, so that their loads and stores are global, not flat
typedef const u64 __attribute__((address_space(1)))* gcptr;
typedef u64 __attribute__((address_space(1)))* gptr;
__device__ __forceinline__ u64 bc_cell(const BcLane& L, uint32_t a0, uint32_t a1) {   // address of a section cell's first word
    return L.tab[T_BUFS + ((a1 >> BC_STRIDE_BITS) & 15u)] + 8 * (((a1 >> 31) ? L.ip : L.i) * (u64)(a1 & ((1u << BC_STRIDE_BITS) - 1)) + a0);
}
template <bool D3, class P>
__device__ __forceinline__ f3 bc_ld(P p, u64 step) { return D3 ? f3{{p[0], p[step], p[2 * step]}} : f3{{p[0], 0, 0}}; }
template <bool D3, class P>
__device__ __forceinline__ void bc_st(P p, u64 step, f3 r) { p[0] = r.v[0]; if (D3) { p[step] = r.v[1]; p[2 * step] = r.v[2]; } }

template <bool D3>
__device__ __forceinline__ f3 bc_load(const BcLane& L, uint32_t kind, uint32_t a0, uint32_t a1) {
    switch (kind) {
        case K_LDS: return bc_ld<D3>(L.lds + 64 * a0, 64);
        case K_ARENA: return bc_ld<D3>(L.arena + L.arena_stride * a0, L.arena_stride);
        case K_UNI: return bc_ld<D3>(L.tab + a0, 1);
        case K_MEM: return bc_ld<D3>((gcptr)bc_cell(L, a0, a1), 1);
        case K_X: return bc_ld<D3>((gcptr)L.tab[T_X] + L.i, 1);
        case K_ZI: return bc_ld<D3>((gcptr)L.tab[T_ZI] + (L.i & L.tab[T_ZI_MASK]), 1);
        case K_XDIV: return bc_ld<D3>((gcptr)L.tab[T_XDIV] + 3 * L.i, 1);
        default: return bc_ld<D3>((gcptr)L.tab[T_XDIVW] + 3 * L.i, 1);
    }
}

template <bool D3>
__device__ __forceinline__ void bc_store(const BcLane& L, uint32_t kind, uint32_t d0, uint32_t d1, f3 r, bool live) {
    switch (kind) {
        case K_LDS: bc_st<D3>(L.lds + 64 * d0, 64, r); break;
        case K_ARENA: bc_st<D3>(L.arena + L.arena_stride * d0, L.arena_stride, r); break;
        default: if (live) bc_st<D3>((gptr)bc_cell(L, d0, d1), 1, r); break;   // lanes past the range compute on rows that exist and store nothing
    }
}

// One lane, one row; the grid and the row0 / count contract of the compiled kernels (expr_jit.hip zk_eval_kernel), except that
// a wave goes on to the chunk gridDim.x * 64 rows further until the range ends.
//
// CHK: the checker's build of the kernel, the only one that knows check1.  The results live in bufs[PC_BUF_RESULT] as [3][n_ids] words:
// count, first, value.  A wave takes the ballot of its failing lanes and, only when there is one, issues one atomicAdd of the population
// count and one atomicMin of its smallest failing row (a checker's range starts at row 0 and does not wrap, so that is the row of the
// lowest failing lane): a satisfied trace issues no atomic.  With `at_first` the launch is the second, tiny one: block b evaluates the one
// row first[b] ends with (lane 0 alone is live) and check1 of identity b leaves its value there; identities nothing failed are skipped.
template <bool CHK>
__global__ __launch_bounds__(64) void zk_bc_eval_kernel(const BcInstr* __restrict__ code, uint32_t n_instr, const u64* __restrict__ tab, u64* __restrict__ arena,
                                                         u64 n, u64 next, u64 row0, u64 count, uint32_t at_first) {
    __shared__ u64 slots[BC_LDS_WORDS * 64];
    const unsigned lane = threadIdx.x;
    BcLane L;
    L.lds = slots + lane;
    L.arena_stride = (u64)gridDim.x * 64;
    L.arena = arena + (u64)blockIdx.x * 64 + lane;
    L.tab = tab;
    u64 k0 = (u64)blockIdx.x * 64;
    if (CHK && at_first) {
        const u64* res = (const u64*)tab[T_BUFS + PC_BUF_RESULT];
        if (res[blockIdx.x] == 0) return;
        row0 = res[gridDim.x + blockIdx.x]; k0 = 0; count = 1;
    }
    for (; k0 < count; k0 += L.arena_stride) {
        const unsigned i0 = (unsigned)(row0 + k0);                // first row of this chunk (the domain has at most 2^32 rows)
        const bool live = k0 + lane < count;
        L.i = (u64)((i0 + lane) & (unsigned)(n - 1));
        L.ip = (L.i + next) & (n - 1);
        for (uint32_t pc = 0; pc < n_instr; ++pc) {
            const BcInstr in = code[pc];
            const uint32_t op = in.w[0] & 255u, ka = (in.w[0] >> 8) & 15u, kb = (in.w[0] >> 12) & 15u, kd = (in.w[0] >> 16) & 15u;
            f3 r;
            if (op >= BC_COPY1) {
                if (CHK && op == BC_CHECK1) {
                    r = bc_load<false>(L, ka, in.w[1], in.w[2]);
                    u64* res = (u64*)tab[T_BUFS + PC_BUF_RESULT];
                    const uint32_t id = in.w[5], n_ids = in.w[6];
                    if (at_first) { if (lane == 0 && id == blockIdx.x) res[2 * n_ids + id] = r.v[0]; continue; }
                    const bool bad = live && r.v[0] != 0;
                    const unsigned long long m = __ballot(bad);
                    if (m != 0 && lane == (unsigned)__ffsll(m) - 1) {
                        atomicAdd((unsigned long long*)res + id, (unsigned long long)__popcll(m));
                        atomicMin((unsigned long long*)res + n_ids + id, (unsigned long long)L.i);
                    }
                    continue;
                }
                if (op == BC_COPY1) { r = bc_load<false>(L, ka, in.w[1], in.w[2]); bc_store<false>(L, kd, in.w[5], in.w[6], r, live); }
                else                { r = bc_load<true>(L, ka, in.w[1], in.w[2]);  bc_store<true>(L, kd, in.w[5], in.w[6], r, live); }
                continue;
            }
            const f3 a = (op & 2u) ? bc_load<true>(L, ka, in.w[1], in.w[2]) : bc_load<false>(L, ka, in.w[1], in.w[2]);
            const f3 b = (op & 1u) ? bc_load<true>(L, kb, in.w[3], in.w[4]) : bc_load<false>(L, kb, in.w[3], in.w[4]);
            switch (op) {
                case 0:  r = f3{{gl::add(a.v[0], b.v[0]), 0, 0}}; break;
                case 1:  r = f3{{gl::add(b.v[0], a.v[0]), b.v[1], b.v[2]}}; break;                       // f3g.rs:346-349
                case 2:  r = f3{{gl::add(a.v[0], b.v[0]), a.v[1], a.v[2]}}; break;                       // f3g.rs:338-341
                case 3:  r = gl::f3_add(a, b); break;
                case 4:  r = f3{{gl::sub(a.v[0], b.v[0]), 0, 0}}; break;
                case 5:  r = f3{{gl::sub(a.v[0], b.v[0]), gl::neg(b.v[1]), gl::neg(b.v[2])}}; break;     // f3g.rs:389-392
                case 6:  r = f3{{gl::sub(a.v[0], b.v[0]), a.v[1], a.v[2]}}; break;                       // f3g.rs:381-384
                case 7:  r = gl::f3_sub(a, b); break;
                case 8:  r = f3{{gl::mul(a.v[0], b.v[0]), 0, 0}}; break;
                case 9:  r = gl::f3_muls(b, a.v[0]); break;                                              // f3g.rs:436-441
                case 10: r = gl::f3_muls(a, b.v[0]); break;                                              // f3g.rs:412-416
                default: r = gl::f3_mul(a, b); break;
            }
            if (op & 3u) bc_store<true>(L, kd, in.w[5], in.w[6], r, live);
            else         bc_store<false>(L, kd, in.w[5], in.w[6], r, live);
        }
    }
}

const char* const OP_NAME[15] = {"add11", "add13", "add31", "add33", "sub11", "sub13", "sub31", "sub33", "mul11", "mul13", "mul31", "mul33", "copy1", "copy3", "check1"};

struct Ref { uint32_t kind = K_NONE, a0 = 0, a1 = 0, dim = 0; int value = -1; };   // value: the temporary it names, until slots are given out
struct Value { uint32_t dim, def, last; uint32_t kind = K_NONE, slot = 0; };

thread_local int t_eval_mode = -1;              // -1: not asked yet, $ZK_EVAL decides

}  // namespace

struct Bytecode {
    std::vector<BcInstr> code;
    std::vector<BcUni> uni;
    uint32_t tab_words = T_UNI, lds_words = 0, arena_words = 0;
    std::string listing;
    DevBuf d_code, d_uni, d_tab, d_arena;      // on the device from the first run on
    bool uploaded = false;
    bool checker = false;                      // assembled for pil_check.hip: runs the kernel that knows check1
};

namespace {

struct Assembler {
    std::vector<Value> values;
    std::map<uint32_t, int> tmp;                                  // tmp id -> its current value
    std::map<std::tuple<uint32_t, uint32_t, u64>, uint32_t> uni_at;   // (kind, id, value) -> word in the table
    std::vector<BcUni> uni;
    uint32_t tab_words = T_UNI;
    std::vector<EvalAccess> mem_reads, mem_writes;
    std::set<std::tuple<uint32_t, uint32_t, bool>> own_words;     // words this lane has stored so far: (buf, word, prime)
    std::set<std::tuple<uint32_t, uint32_t, uint32_t, bool>> read_seen;
    struct Enc { uint32_t op; Ref a, b, d; };
    std::vector<Enc> enc;

    Ref uniform(uint32_t kind, uint32_t id, u64 value, uint32_t dim) {
        auto key = std::make_tuple(kind, id, value);
        auto it = uni_at.find(key);
        if (it == uni_at.end()) {
            it = uni_at.emplace(key, tab_words).first;
            uni.push_back(BcUni{kind, id, tab_words, dim, value});
            tab_words += dim;
        }
        Ref r; r.kind = K_UNI; r.a0 = it->second; r.dim = dim;
        return r;
    }
    static Ref cell(const zk_operand& o, uint32_t dim) {
        ZK_REQUIRE(o.buf < 16, "eval program: buffer slot out of range");
        ZK_REQUIRE(o.stride < (1u << BC_STRIDE_BITS), "eval program: section row too wide");
        Ref r; r.kind = K_MEM; r.a0 = o.id; r.a1 = o.stride | ((uint32_t)o.buf << BC_STRIDE_BITS) | (o.prime ? 1u << 31 : 0u); r.dim = dim;
        return r;
    }
    Ref load(const zk_operand& o, uint32_t at) {
        ZK_REQUIRE(o.dim == 1 || o.dim == 3, "eval program: operand dim must be 1 or 3");
        switch (o.kind) {
            case ZK_OPND_TMP: {
                auto it = tmp.find(o.id);
                ZK_REQUIRE(it != tmp.end(), "eval program: tmp read before write");
                values[it->second].last = at;
                Ref r; r.value = it->second; r.dim = values[it->second].dim;
                return r;
            }
            case ZK_OPND_MEM: {
                Ref r = cell(o, o.dim);
                // a read this lane's own earlier stores of the same row cover entirely is ordered behind them (program order) and is
                // no other lane's business; anything else reaches memory other lanes may be writing
                bool own = true;
                for (uint32_t j = 0; j < o.dim; ++j) own = own && own_words.count(std::make_tuple((uint32_t)o.buf, o.id + j, o.prime != 0));
                if (!own && read_seen.insert(std::make_tuple((uint32_t)o.buf, o.id, (uint32_t)o.dim, o.prime != 0)).second)
                    mem_reads.push_back(EvalAccess{(uint32_t)o.buf, o.id, (uint32_t)o.dim, o.prime != 0});
                return r;
            }
            case ZK_OPND_NUMBER:
                ZK_REQUIRE(o.value < GL_P, "eval program: number not canonical");
                return uniform(ZK_OPND_NUMBER, 0, o.value, 1);
            case ZK_OPND_PUBLIC: return uniform(ZK_OPND_PUBLIC, o.id, 0, 1);
            case ZK_OPND_CHALLENGE: return uniform(ZK_OPND_CHALLENGE, o.id, 0, 3);
            case ZK_OPND_EVAL: return uniform(ZK_OPND_EVAL, o.id, 0, 3);
            case ZK_OPND_X: { Ref r; r.kind = K_X; r.dim = 1; return r; }
            case ZK_OPND_ZI: { Ref r; r.kind = K_ZI; r.dim = 1; return r; }
            case ZK_OPND_XDIVXSUBXI: { Ref r; r.kind = K_XDIV; r.dim = 3; return r; }
            case ZK_OPND_XDIVXSUBWXI: { Ref r; r.kind = K_XDIVW; r.dim = 3; return r; }
            default: throw Error("eval program: unknown operand kind");
        }
    }
    Ref store(const zk_operand& d, uint32_t dim, uint32_t at) {
        if (d.kind == ZK_OPND_TMP) {                                   // interpreter.rs:149-152: a tmp takes the value, whatever it held
            values.push_back(Value{dim, at, at});
            tmp[d.id] = (int)values.size() - 1;
            Ref r; r.value = (int)values.size() - 1; r.dim = dim;
            return r;
        }
        ZK_REQUIRE(d.kind == ZK_OPND_MEM && d.buf < 16, "eval program: destination must be tmp or a section cell");
        mem_writes.push_back(EvalAccess{(uint32_t)d.buf, d.id, dim, d.prime != 0});   // interpreter.rs:149-159
        for (uint32_t j = 0; j < dim; ++j) own_words.insert(std::make_tuple((uint32_t)d.buf, d.id + j, d.prime != 0));
        return cell(d, dim);
    }
    bool checker = false;                                         // bytecode_assemble for pil_check.hip: check1 is an instruction
    void instr(const zk_instr& in, uint32_t at) {
        Enc e;
        if (checker && in.op == ZK_OP_CHECK1) {
            e.a = load(in.src[0], at);
            ZK_REQUIRE(e.a.dim == 1, "check program: check1 takes a dim-1 value");
            ZK_REQUIRE(in.dest.id < in.dest.stride, "check program: identity index out of range");
            e.op = BC_CHECK1; e.d.a0 = in.dest.id; e.d.a1 = in.dest.stride;
        } else if (in.op == ZK_OP_COPY) {
            e.a = load(in.src[0], at);
            e.op = e.a.dim == 3 ? BC_COPY3 : BC_COPY1;
            e.d = store(in.dest, e.a.dim, at);
        } else {
            e.a = load(in.src[0], at); e.b = load(in.src[1], at);
            ZK_REQUIRE(in.op == ZK_OP_ADD || in.op == ZK_OP_SUB || in.op == ZK_OP_MUL, "eval program: unknown op");
            e.op = 4 * in.op + 2 * (e.a.dim == 3) + (e.b.dim == 3);
            e.d = store(in.dest, (e.a.dim == 3 || e.b.dim == 3) ? 3 : 1, at);
        }
        enc.push_back(e);
    }

    // Slots by liveness.  A value is busy from the instruction that writes it up to (not including) its last reader: an
    // instruction loads all its operands before it stores, so its result may take the slot of an operand that dies there.
    uint32_t lds_used = 0, arena_used = 0;
    void allocate() {
        auto end_of = [](const Value& v) { return std::max(v.last, v.def + 1); };
        // LDS: the shortest-lived values first (they are the ones touched most often per word-slot held), first fit over the
        // whole life of the value; busy[s] = the intervals word-slot s is taken for, start -> end
        std::vector<uint32_t> order(values.size());
        for (uint32_t k = 0; k < order.size(); ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return end_of(values[x]) - values[x].def < end_of(values[y]) - values[y].def; });
        std::vector<std::map<uint32_t, uint32_t>> busy(BC_LDS_WORDS);
        auto is_free = [&](uint32_t s, uint32_t b, uint32_t e) {
            const auto& m = busy[s];
            auto it = m.upper_bound(b);
            if (it != m.end() && it->first < e) return false;
            if (it != m.begin() && std::prev(it)->second > b) return false;
            return true;
        };
        for (uint32_t k : order) {
            Value& v = values[k];
            const uint32_t b = v.def, e = end_of(v);
            for (uint32_t s = 0; s + v.dim <= BC_LDS_WORDS; ++s) {
                bool ok = true;
                for (uint32_t j = 0; j < v.dim && ok; ++j) ok = is_free(s + j, b, e);
                if (!ok) continue;
                for (uint32_t j = 0; j < v.dim; ++j) busy[s + j][b] = e;
                v.kind = K_LDS; v.slot = s;
                lds_used = std::max(lds_used, s + v.dim);
                break;
            }
        }
        // the arena takes the rest, in program order: freed slots are reused, a freed 3-word slot is cut up when 1-word slots run out
        typedef std::pair<uint32_t, uint32_t> Rel;                                  // (end, value)
        std::priority_queue<Rel, std::vector<Rel>, std::greater<Rel>> active;
        std::vector<uint32_t> free1, free3;
        for (uint32_t k = 0; k < values.size(); ++k) {
            Value& v = values[k];
            if (v.kind == K_LDS) continue;
            while (!active.empty() && active.top().first <= v.def) {
                const Value& o = values[active.top().second];
                (o.dim == 3 ? free3 : free1).push_back(o.slot);
                active.pop();
            }
            if (v.dim == 1 && free1.empty() && !free3.empty()) {
                const uint32_t s = free3.back(); free3.pop_back();
                free1.push_back(s + 2); free1.push_back(s + 1); free1.push_back(s);
            }
            std::vector<uint32_t>& fl = v.dim == 3 ? free3 : free1;
            if (!fl.empty()) { v.slot = fl.back(); fl.pop_back(); }
            else { v.slot = arena_used; arena_used += v.dim; }
            v.kind = K_ARENA;
            active.push(Rel(end_of(v), k));
        }
    }
    void place(Ref& r) const {
        if (r.value < 0) return;
        r.kind = values[r.value].kind; r.a0 = values[r.value].slot; r.a1 = 0;
    }
    static void print(std::ostringstream& o, const Ref& r) {
        switch (r.kind) {
            case K_LDS: o << "L" << r.a0; break;
            case K_ARENA: o << "A" << r.a0; break;
            case K_UNI: o << "U" << r.a0 - T_UNI; break;
            case K_MEM: o << "M" << ((r.a1 >> BC_STRIDE_BITS) & 15u) << "[" << r.a0 << "/" << (r.a1 & ((1u << BC_STRIDE_BITS) - 1)) << "]" << ((r.a1 >> 31) ? "'" : ""); break;
            case K_X: o << "x"; break;
            case K_ZI: o << "Zi"; break;
            case K_XDIV: o << "xDivXSubXi"; break;
            case K_XDIVW: o << "xDivXSubWXi"; break;
            default: o << "-"; break;
        }
        if (r.kind != K_NONE) o << ":" << r.dim;
    }
};

}  // namespace

void bytecode_free(Bytecode* b) { delete b; }
const char* bytecode_listing(const Bytecode* b) { return b->listing.c_str(); }

int eval_mode() {
    if (t_eval_mode < 0) {
        const char* e = getenv("ZK_EVAL");
        t_eval_mode = e && !strcmp(e, "bytecode") ? ZK_EVAL_BYTECODE : ZK_EVAL_JIT;
    }
    return t_eval_mode;
}

void bytecode_run(Bytecode* b, const void* ctx, uint32_t nbits_domain, uint64_t next, uint64_t row0, uint64_t count, hipStream_t st) {
    if (b->code.empty() || count == 0) return;
    if (!b->uploaded) {   // assembling needs no GPU, running does
        b->d_code.reserve(b->code.size() * sizeof(BcInstr));
        h2d_sync(b->d_code.p, b->code.data(), b->code.size() * sizeof(BcInstr));
        b->d_uni.reserve(std::max<size_t>(1, b->uni.size()) * sizeof(BcUni));
        if (!b->uni.empty()) h2d_sync(b->d_uni.p, b->uni.data(), b->uni.size() * sizeof(BcUni));
        b->d_tab.reserve((size_t)b->tab_words * 8);
        b->uploaded = true;
    }
    const uint64_t waves = std::min<uint64_t>((count + 63) / 64, BC_MAX_WAVES);
    b->d_arena.reserve(std::max<size_t>(8, (size_t)b->arena_words * waves * 64 * 8));
    // this run's section pointers and uniform values, on the same stream
    const uint32_t n_uni = (uint32_t)b->uni.size();
    zk_bc_refresh_kernel<<<1 + (n_uni + 63) / 64, 64, 0, st>>>(*(const zk_eval_ctx*)ctx, (const BcUni*)b->d_uni.p, n_uni, b->d_tab.u());
    ZK_HIP(hipGetLastError());
    if (b->checker)
        zk_bc_eval_kernel<true><<<(unsigned)waves, 64, 0, st>>>((const BcInstr*)b->d_code.p, (uint32_t)b->code.size(), b->d_tab.u(), b->d_arena.u(),
                                                              1ull << nbits_domain, next, row0, count, 0u);
    else
        zk_bc_eval_kernel<false><<<(unsigned)waves, 64, 0, st>>>((const BcInstr*)b->d_code.p, (uint32_t)b->code.size(), b->d_tab.u(), b->d_arena.u(),
                                                               1ull << nbits_domain, next, row0, count, 0u);
    ZK_HIP(hipGetLastError());
}

void bytecode_run_first(Bytecode* b, const void* ctx, uint32_t nbits_domain, uint64_t next, uint32_t n_ids, hipStream_t st) {
    ZK_REQUIRE(b->checker && b->uploaded, "bytecode_run_first: a check program that has run");
    if (b->code.empty() || n_ids == 0) return;
    b->d_arena.reserve(std::max<size_t>(8, (size_t)b->arena_words * n_ids * 64 * 8));
    const uint32_t n_uni = (uint32_t)b->uni.size();
    zk_bc_refresh_kernel<<<1 + (n_uni + 63) / 64, 64, 0, st>>>(*(const zk_eval_ctx*)ctx, (const BcUni*)b->d_uni.p, n_uni, b->d_tab.u());
    ZK_HIP(hipGetLastError());
    zk_bc_eval_kernel<true><<<n_ids, 64, 0, st>>>((const BcInstr*)b->d_code.p, (uint32_t)b->code.size(), b->d_tab.u(), b->d_arena.u(),
                                                  1ull << nbits_domain, next, 0, 1, 1u);
    ZK_HIP(hipGetLastError());
}

// the assembler behind zk_program_assemble; `checker`: a program of pil_check.hip, which may hold check1
Bytecode* bytecode_assemble(const zk_instr* code, uint32_t n_instr, bool checker) {
    Assembler as;
    as.checker = checker;
    for (uint32_t k = 0; k < n_instr; ++k) as.instr(code[k], k);
    check_row_hazards(as.mem_writes, as.mem_reads);
    as.allocate();
    std::unique_ptr<Bytecode> b(new Bytecode());
    Bytecode* B = b.get();
    B->checker = checker;
    std::ostringstream o;
    for (uint32_t k = 0; k < n_instr; ++k) {
        Assembler::Enc& e = as.enc[k];
        as.place(e.a); as.place(e.b); as.place(e.d);
        BcInstr in; memset(&in, 0, sizeof in);
        in.w[0] = e.op | e.a.kind << 8 | e.b.kind << 12 | e.d.kind << 16;
        in.w[1] = e.a.a0; in.w[2] = e.a.a1; in.w[3] = e.b.a0; in.w[4] = e.b.a1; in.w[5] = e.d.a0; in.w[6] = e.d.a1;
        B->code.push_back(in);
        o << k << "  " << OP_NAME[e.op] << "  ";
        if (e.op == BC_CHECK1) o << "id" << e.d.a0; else Assembler::print(o, e.d);
        o << " <- "; Assembler::print(o, e.a);
        if (e.b.kind != K_NONE) { o << ", "; Assembler::print(o, e.b); }
        o << "\n";
    }
    B->uni = std::move(as.uni);
    B->tab_words = as.tab_words; B->lds_words = as.lds_used; B->arena_words = as.arena_used;
    o << "; slots: " << as.lds_used + as.arena_used << " words (lds " << as.lds_used << ", arena " << as.arena_used << "), values " << as.values.size()
      << ", uniforms " << as.tab_words - T_UNI << " words, instructions " << n_instr << "\n";
    B->listing = o.str();
    return b.release();
}

}  // namespace zk

using namespace zk;

extern "C" {

zk_program_t* zk_program_assemble(const zk_instr* code, uint32_t n_instr) {
    try {
        ZK_REQUIRE(code || n_instr == 0, "zk_program_assemble: null code");
        return program_of_bytecode(bytecode_assemble(code, n_instr, false));
    } catch (const std::exception& e) { set_error(e.what()); return nullptr; }
}
int zk_eval_set_mode(int mode) {
    const int prev = eval_mode();
    if (mode != ZK_EVAL_JIT && mode != ZK_EVAL_BYTECODE) { set_error("zk_eval_set_mode: mode must be ZK_EVAL_JIT or ZK_EVAL_BYTECODE"); return -1; }
    t_eval_mode = mode;
    return prev;
}

}  // extern "C"
