// Host-side driver of the GL-hash eSTARK prover: StarkSetup::new (starky/src/stark_setup.rs:27-66),
// StarkProof::stark_gen (stark_gen.rs:193-557), FRI::prove (fri.rs:84-184) and the zkin serialiser
// (serializer.rs:140-264), in C++ behind two C entry points (zk_stark_setup_new / zk_stark_gen).
//
// The reference's driver is Rust; this is its counterpart for callers that bind the C ABI.  Every field
// operation runs in the HIP kernels of this library (LDE, Merkle, transcript, run-time compiled
// constraint programs, Z, Q split, evals, x/(x-xi), FRI folds); the host only sequences launches,
// keeps the sections resident in HBM and formats the proof.  Inputs are the reference's own
// serialised StarkInfo + Program (serde field names, starkinfo.rs:27-95) and StarkStruct
// (types.rs): the reference's PIL front end and code generator stay in charge of them.
// calculate_H1H2 (stark_gen.rs:624-651), a host step in the reference, runs on the device as well (calculate_h1h2_dev, stark.hip).
#include "zk_internal.h"
#include "commit.h"
#include "../../include/zkgpu.h"
#include "json_min.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <array>
#include <cstring>
#include <atomic>
#include <future>
#include <map>
#include <memory>
#include <sstream>
#include <unordered_map>
#include <vector>

using namespace zk;

namespace {

enum Slot { S_CM1_N, S_CM2_N, S_CM3_N, S_TMPEXP_N, S_CONST_N, S_CM1_2NS, S_CM2_2NS, S_CM3_2NS, S_CM4_2NS,
            S_CONST_2NS, S_Q_2NS, S_F_2NS, S_SCRATCH, S_COUNT };
const char* const SLOT_NAME[S_COUNT] = {"cm1_n", "cm2_n", "cm3_n", "tmpexp_n", "const_n", "cm1_2ns", "cm2_2ns",
                                        "cm3_2ns", "cm4_2ns", "const_2ns", "q_2ns", "f_2ns", "scratch"};
int slot_of(const std::string& s) {
    for (int i = 0; i < S_COUNT; ++i) if (s == SLOT_NAME[i]) return i;
    return -1;  // e.g. cm4_n: listed by the map, never materialised by the prover (an error only if used)
}

void ck(int rc) { if (rc != 0) throw Error(zk_last_error()); }   // (the evaluator's and calculate_H1H2's entry points)
// the C ABI speaks uint64_t (unsigned long), the kernels u64 (unsigned long long): same 8 bytes
inline uint64_t* M(u64* p) { return reinterpret_cast<uint64_t*>(p); }
inline const uint64_t* C(const u64* p) { return reinterpret_cast<const uint64_t*>(p); }
inline const u64* K(const uint64_t* p) { return reinterpret_cast<const u64*>(p); }

struct PolRef { int slot; u64 width; u64 pos; u32 dim; };

struct ProgramDeleter { void operator()(zk_program_t* p) const { if (p) zk_program_free(p); } };
using ProgramPtr = std::unique_ptr<zk_program_t, ProgramDeleter>;
// The two instantiations of the reference's generics: StarkProof<MerkleTreeGL>::stark_gen::<TranscriptGL> and
// StarkProof<MerkleTreeBN128>::stark_gen::<TranscriptBN128> (prove.rs:47-91), chosen by verificationHashType: the trees and
// transcripts of commit.h.
using TreePtr = std::shared_ptr<const Tree>;       // shared: a setup lends its all-zero tree to every proof
struct AnyTranscript {
    std::unique_ptr<Transcript> own;                   // empty: a caller's TranscriptGL, borrowed
    Transcript* t; GlTranscript* gl;                   // gl: the sponge in device memory (deferred puts, squeezes into HBM), or nullptr
    explicit AnyTranscript(HashType h) : own(new_transcript(h)), t(own.get()), gl(t->gl()) {}
    explicit AnyTranscript(zk_transcript_t* callers) : t(callers), gl(callers) { ZK_REQUIRE(callers != nullptr, "null transcript"); }
    AnyTranscript(const AnyTranscript&) = delete; AnyTranscript& operator=(const AnyTranscript&) = delete;
    ~AnyTranscript() { if (!own) try { flush(); } catch (...) {} }   // (a borrowed sponge must not lose an absorbed word)
    // Goldilocks sponge: a put is DEFERRED until the next squeeze and rides in its launch (tr_put_get_kernel) -- "absorb a root, draw two
    // challenges" is one launch instead of three.  The absorbed words must stay in HBM until then: they are roots inside live trees, the
    // context's evaluations / publics, the last FRI polynomial.  Two puts in a row, or the end of the object, flush as a plain put.
    const u64* pend_src = nullptr; size_t pend_n = 0; hipStream_t pend_st = nullptr;
    void flush() {
        if (!pend_n) return;
        gl->put_dev(pend_src, pend_n, pend_st);
        pend_n = 0;
    }
    void defer(const u64* d, size_t n, hipStream_t st) { flush(); pend_src = d; pend_n = n; pend_st = st; }
    // n Goldilocks words, one transcript element each (publics, evals, the last FRI polynomial)
    void put_words_dev(const u64* d, size_t n, hipStream_t st) {
        if (!n) return;
        if (gl) { defer(d, n, st); return; }
        std::vector<u64> h(n);
        ZK_HIP(hipStreamSynchronize(st));
        ZK_HIP(hipMemcpy(h.data(), d, 8 * n, hipMemcpyDeviceToHost));
        t->put_words(h.data(), n);
    }
    void put_root(const Tree& tree, hipStream_t st) {   // a digest is ONE element of the scalar-field transcripts
        if (gl) { defer(tree.gl()->root_dev(), 4, st); return; }
        u64 r[4]; tree.root(r);
        t->put_digest(r);
    }
    // n_fields consecutive get_field()s into d_out (3 words each)
    void get_fields_dev(u64* d_out, u32 n_fields, hipStream_t st) {
        if (gl) {
            if (pend_n) ZK_REQUIRE(pend_st == st, "transcript: a deferred put moved streams");
            gl->put_get_async(pend_src, pend_n, d_out, 3 * n_fields, 0, st);
            pend_n = 0;
            return;
        }
        for (u32 k = 0; k < n_fields; ++k) {
            u64 f[3];
            t->get(f, 3);
            ZK_HIP(hipMemcpy(d_out + 3 * k, f, 24, hipMemcpyHostToDevice));
        }
    }
    void get_field_dev(u64* d_out3, hipStream_t st) { get_fields_dev(d_out3, 1, st); }
    void get_permutations_dev(u32 n, u32 nbits, u64* d_out, hipStream_t st) {   // Goldilocks transcript only: the indices stay in HBM
        ZK_REQUIRE(gl != nullptr, "get_permutations_dev: scalar-field transcripts keep their sponge on the host");
        ZK_REQUIRE(nbits >= 1 && nbits <= 63, "get_permutations: nbits out of range");
        gl->put_get_async(pend_src, pend_n, d_out, n, nbits, st);
        pend_n = 0;
    }
    void get_permutations(u32 n, u32 nbits, u64* out) { flush(); t->get_permutations(n, nbits, out); }
};

void zero(DevBuf& b, size_t words, hipStream_t st) { if (words) ZK_HIP(hipMemsetAsync(b.p, 0, words * 8, st)); }

// Per-stage device time of one proof, opt-in (ZK_STARK_TIMING=1): the reference's `#[time_profiler]` spans
// (stark_gen.rs:192,624,709,734,785, fri.rs:83) as HIP-event intervals on the proof's stream.  mark(name) closes the
// interval that began at the previous mark and gives it `name`; intervals of the same name add up.  Off: no events, no cost.
struct StageTimer {
    bool on = false, quiet = false;
    hipStream_t st = nullptr;
    std::vector<std::pair<std::string, hipEvent_t>> marks;
    std::chrono::steady_clock::time_point t0;
    StageTimer(hipStream_t s) : st(s) {
        const char* env = getenv("ZK_STARK_TIMING");      // read per proof: a caller may switch it on for one proof ("quiet": no stderr line)
        on = env && *env && strcmp(env, "0");
        quiet = on && !strcmp(env, "quiet");
        if (on) { t0 = std::chrono::steady_clock::now(); mark("begin"); }
    }
    ~StageTimer() { for (auto& m : marks) (void)hipEventDestroy(m.second); }
    void mark(const char* name) {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); on = false; return; }
        (void)hipEventRecord(e, st);
        marks.emplace_back(name, e);
    }
    // JSON object {"stage": ms, ..., "total_gpu_ms": .., "wall_ms": ..}; one line of it on stderr
    std::string finish(u32 nbits) {
        if (!on || marks.size() < 2) return "";
        (void)hipEventSynchronize(marks.back().second);
        std::vector<std::pair<std::string, double>> acc;
        for (size_t i = 1; i < marks.size(); ++i) {
            float ms = 0; (void)hipEventElapsedTime(&ms, marks[i - 1].second, marks[i].second);
            bool found = false;
            for (auto& a : acc) if (a.first == marks[i].first) { a.second += ms; found = true; }
            if (!found) acc.emplace_back(marks[i].first, ms);
        }
        float total = 0; (void)hipEventElapsedTime(&total, marks.front().second, marks.back().second);
        std::ostringstream o; o.setf(std::ios::fixed); o.precision(3);
        o << "{\"nBits\":" << nbits;
        for (auto& a : acc) o << ",\"" << a.first << "\":" << a.second;
        o << ",\"total_gpu_ms\":" << total << ",\"wall_ms\":" << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() << "}";
        if (!quiet) fprintf(stderr, "[zkgpu stark_gen] %s\n", o.str().c_str());
        return o.str();
    }
};

}  // namespace

struct zk_stark_setup {
    JVal info, prog, ss;
    u32 nbits = 0, nbits_ext = 0, n_queries = 0, n_constants = 0, q_dim = 0, q_deg = 0, n_cm1 = 0, n_cm2 = 0;
    std::vector<u32> steps;
    u64 sN[S_COUNT] = {};                 // map_sectionsN (words per row)
    std::vector<PolRef> var_pol_map;
    std::vector<u64> cm_n, cm_2ns, tmpexp_n;
    std::map<u64, u64> exp2pol;
    DevBuf const_n, const_2ns;
    HashType hash = HASH_GL;               // verificationHashType
    const FrField* fr = nullptr;           // its scalar field ("BN128" / "BLS12381"); nullptr = "GL"
    std::string prover_addr;               // StarkProof.prover_addr (serializer.rs:255-262), non-GL proofs only
    bool self_check = false;               // verify every proof before handing it out, as stark_prove does (prove.rs:124-132)
    TreePtr const_tree;
    TreePtr zero_tree;                     // the tree over a zero-width section (tree2 / tree3 of a PIL without such columns): the same in every proof
    DevBuf d_pub_pos;                      // word position in cm1_n of every public that is a cell of a committed column (~0: a computed public)
    DevBuf x_n, x_2ns, zi;                 // x over the domain and the extended coset, 1 / Z_H on the coset (stark_gen.rs:231-249): functions of the sizes only
    u64 const_root[4] = {};
    ProgramPtr step2prev, step3prev, step3, step42ns, step52ns;
    std::vector<ProgramPtr> public_programs;
    // step3 (the intermediate columns) and their extension may start before the first commitment is hashed when nothing
    // in stage 3 depends on a challenge: no plookup / permutation / connection columns and no challenge or
    // expression-section operand in step3 itself.  The transcript order is untouched (stark_gen below).
    bool early_stage3 = false;
    std::atomic<int> early_ctx_live{0};    // contexts that currently use side_stream / ev_inputs / ev_stage3 (at most one)
    hipStream_t side_stream = nullptr;     // memory-bound stage-3 work beside the ALU-bound hashing of tree 1
    hipEvent_t ev_inputs = nullptr, ev_stage3 = nullptr;
    int eval_mode = ZK_EVAL_JIT;           // which evaluator the step and public programs are built for: read once, on the thread that creates the setup
    std::string setup_timing;              // JSON: where StarkSetup::new's time went (zk_stark_setup_timing)
    std::string last_timing;               // JSON: the stages of the last proof, HIP-event milliseconds (ZK_STARK_TIMING=1)
    std::chrono::steady_clock::time_point t_json_begin, t_json_end;   // host time of the last proof's serialisation (timing runs only)
    ~zk_stark_setup() {
        if (side_stream) { forget_stream(side_stream); (void)hipStreamDestroy(side_stream); }
        if (ev_inputs) (void)hipEventDestroy(ev_inputs);
        if (ev_stage3) (void)hipEventDestroy(ev_stage3);
    }

    PolRef pol(u64 pol_id) const {
        ZK_REQUIRE(pol_id < var_pol_map.size(), "pol id out of range");
        ZK_REQUIRE(var_pol_map[pol_id].slot >= 0, "polynomial lives in a section the prover does not hold");
        return var_pol_map[pol_id];
    }

    // Node -> zk_operand, as interpreter.rs get_ref / set_ref / eval_map (:286-524) resolve addresses
    zk_operand resolve(const JVal& node, bool ext) const {
        zk_operand o; memset(&o, 0, sizeof o);
        o.dim = 1;
        const std::string& t = node.at("type_").str();
        const u32 id = node.find("id") && !node.at("id").is_null() ? (u32)node.at("id").u64() : 0;
        const bool prime = node.find("prime") && !node.at("prime").is_null() && node.at("prime").boolean();
        if (t == "tmp") { o.kind = ZK_OPND_TMP; o.id = id; }
        else if (t == "const") {
            o.kind = ZK_OPND_MEM; o.id = id; o.dim = 1; o.prime = prime; o.buf = ext ? S_CONST_2NS : S_CONST_N; o.stride = n_constants;
        } else if (t == "cm" || t == "tmpExp") {
            const std::vector<u64>& m = t == "cm" ? (ext ? cm_2ns : cm_n) : tmpexp_n;
            ZK_REQUIRE(id < m.size(), "cm id out of range");
            const PolRef p = pol(m[id]);
            o.kind = ZK_OPND_MEM; o.id = (u32)p.pos; o.dim = (uint8_t)p.dim; o.prime = prime; o.buf = (uint8_t)p.slot; o.stride = (u32)p.width;
        } else if (t == "q") { o.kind = ZK_OPND_MEM; o.id = id; o.dim = (uint8_t)q_dim; o.buf = S_Q_2NS; o.stride = q_dim; }
        else if (t == "f") { o.kind = ZK_OPND_MEM; o.id = id; o.dim = 3; o.buf = S_F_2NS; o.stride = 3; }
        else if (t == "number") { o.kind = ZK_OPND_NUMBER; o.value = parse_pil_number(node.at("value").str()); }
        else if (t == "public") { o.kind = ZK_OPND_PUBLIC; o.id = id; }
        else if (t == "challenge") { o.kind = ZK_OPND_CHALLENGE; o.id = id; }
        else if (t == "eval") { o.kind = ZK_OPND_EVAL; o.id = id; }
        else if (t == "x") o.kind = ZK_OPND_X;
        else if (t == "Zi") o.kind = ZK_OPND_ZI;
        else if (t == "xDivXSubXi") o.kind = ZK_OPND_XDIVXSUBXI;
        else if (t == "xDivXSubWXi") o.kind = ZK_OPND_XDIVXSUBWXI;
        else throw Error("Invalid reference type " + t);
        return o;
    }

    // compile_code (interpreter.rs:187-225): Segment.first -> one run-time compiled kernel, or bytecode for the interpreter kernel
    ProgramPtr compile_segment(const JVal& seg, bool ext, bool ret_to_scratch) const {
        const JVal& first = seg.at("first");
        std::vector<zk_instr> code;
        for (const JVal& c : first.arr) {
            zk_instr in; memset(&in, 0, sizeof in);
            const std::string& op = c.at("op").str();
            if (op == "add") in.op = ZK_OP_ADD; else if (op == "sub") in.op = ZK_OP_SUB;
            else if (op == "mul") in.op = ZK_OP_MUL; else if (op == "copy") in.op = ZK_OP_COPY;
            else throw Error("Invalid op " + op);  // the prover rejects muladd (interpreter.rs:208-216)
            in.dest = resolve(c.at("dest"), ext);
            const JVal& src = c.at("src");
            ZK_REQUIRE(src.size() >= 1 && src.size() <= 2, "instruction needs 1 or 2 sources");
            in.src[0] = resolve(src.at(0), ext);
            if (src.size() > 1) in.src[1] = resolve(src.at(1), ext);
            code.push_back(in);
        }
        if (ret_to_scratch && !code.empty()) {  // ret = true: the last destination is the result
            zk_instr in; memset(&in, 0, sizeof in);
            in.op = ZK_OP_COPY;
            in.dest.kind = ZK_OPND_MEM; in.dest.dim = 3; in.dest.buf = S_SCRATCH; in.dest.stride = 3;
            in.src[0] = resolve(first.arr.back().at("dest"), ext);
            code.push_back(in);
        }
        if (code.empty() && eval_mode != ZK_EVAL_BYTECODE) return ProgramPtr();   // (bytecode: an empty step is an empty program, a run of it does nothing: every program of the setup is the interpreter's)
        zk_program_t* p = eval_mode == ZK_EVAL_BYTECODE ? zk_program_assemble(code.data(), (u32)code.size()) : zk_program_compile(code.data(), (u32)code.size());
        if (!p) throw Error(zk_last_error());
        return ProgramPtr(p);
    }
};

namespace {

std::vector<u64> u64_list(const JVal& a) {
    std::vector<u64> v;
    for (const JVal& e : a.arr) v.push_back(e.u64());
    return v;
}

// The proof's JSON text is thousands of decimal words (every opening): written straight into one growing string --
// an ostringstream with a temporary std::string per number cost several hundred microseconds of a small proof.
struct Dec { u64 v; };
inline Dec dec(u64 v) { return Dec{v}; }
struct JOut {
    std::string s;
    JOut() { s.reserve(1 << 16); }
    JOut& operator<<(char c) { s.push_back(c); return *this; }
    JOut& operator<<(const char* t) { s.append(t); return *this; }
    JOut& operator<<(const std::string& t) { s.append(t); return *this; }
    JOut& operator<<(Dec d) {                            // two digits per division, appended in one piece
        static const char* const PAIRS =
            "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
        char buf[20]; int n = 20; u64 v = d.v;
        while (v >= 100) { const u64 q = v / 100; const unsigned r = (unsigned)(v - q * 100); v = q; buf[--n] = PAIRS[2 * r + 1]; buf[--n] = PAIRS[2 * r]; }
        if (v >= 10) { buf[--n] = PAIRS[2 * v + 1]; buf[--n] = PAIRS[2 * v]; } else buf[--n] = (char)('0' + v);
        s.append(buf + n, 20 - n);
        return *this;
    }
    JOut& operator<<(size_t v) { return *this << Dec{(u64)v}; }
    std::string str() { return std::move(s); }
};
// a scalar-field digest travels as the decimal of its canonical value, a GL digest as its words (digest.rs:84-112)
void put_digest(JOut& o, const u64* d, const FrField* fr) {
    if (fr) { o << '"' << fr->to_dec(d) << '"'; return; }
    if (d[1] == 0 && d[2] == 0 && d[3] == 0) { o << '"' << dec(d[0]) << '"'; return; }
    o << "[\"" << dec(d[0]) << "\",\"" << dec(d[1]) << "\",\"" << dec(d[2]) << "\",\"" << dec(d[3]) << "\"]";
}
void put_list(JOut& o, const u64* v, size_t n) {
    o << '[';
    for (size_t i = 0; i < n; ++i) { if (i) o << ','; o << '"' << dec(v[i]) << '"'; }
    o << ']';
}
void put_path(JOut& o, const u64* path, u32 depth, const FrField* fr) {   // path[depth][4], or [depth][64] of a scalar-field tree
    o << '[';
    for (u32 l = 0; l < depth; ++l) {
        if (l) o << ',';
        if (!fr) { put_list(o, path + 4 * l, 4); continue; }
        o << '[';                                        // the 16 nodes of the group, each an Fr (merklehash_bn128.rs:86-106)
        for (int k = 0; k < 16; ++k) { if (k) o << ','; o << '"' << fr->to_dec(path + 64 * l + 4 * k) << '"'; }
        o << ']';
    }
    o << ']';
}

// Device words the host needs for the proof's JSON (roots, evaluations, the last FRI polynomial): collected in one device
// block with asynchronous copies and fetched with ONE copy -- each of them on its own was a blocking round trip, and a
// small proof is a chain of those.
struct RbSegs { const u64* src[16]; u32 n[16]; u32 off[16]; };
__global__ __launch_bounds__(256) void rb_gather_kernel(const RbSegs G, u64* __restrict__ stage) {   // block b copies segment b
    const u64* __restrict__ s = G.src[blockIdx.x];
    u64* __restrict__ d = stage + G.off[blockIdx.x];
    for (u32 i = threadIdx.x; i < G.n[blockIdx.x]; i += blockDim.x) d[i] = s[i];
}
// A proof's preamble cleared eight small buffers and copied its publics with one hipMemsetAsync / hipMemcpyAsync each: a dozen launches of
// ~5 us before the first real kernel.  One launch clears up to sixteen buffers (block row y = buffer y), one gathers the publics.
struct ClearSegs { u64* p[16]; u64 n[16]; };
__global__ __launch_bounds__(256) void clear_list_kernel(const ClearSegs G) {
    u64* __restrict__ p = G.p[blockIdx.y];
    const u64 n = G.n[blockIdx.y];
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) p[i] = 0;
}
struct ClearList {
    ClearSegs G; u32 k = 0; u64 longest = 0; hipStream_t st;
    explicit ClearList(hipStream_t s) : st(s) {}
    void add(void* p, u64 words) { if (!words) return; G.p[k] = (u64*)p; G.n[k] = words; longest = std::max(longest, words); if (++k == 16) flush(); }
    void flush() {
        if (!k) return;
        const u32 bx = (u32)std::min<u64>(2048, (longest + 1023) / 1024);   // ~4 words per lane and trip at most; big sections get the whole chip
        hipLaunchKernelGGL(clear_list_kernel, dim3(std::max<u32>(1, bx), k), dim3(256), 0, st, G);
        ZK_HIP(hipGetLastError());
        k = 0; longest = 0;
    }
};
__global__ void gather_publics_kernel(const u64* __restrict__ cm, const u64* __restrict__ pos, u32 n, u64* __restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && pos[i] != ~0ull) out[i] = cm[pos[i]];
}
struct ReadBack {
    DevBuf stage; std::vector<u64> host; size_t words = 0, cap = 0; hipStream_t st;
    RbSegs segs; u32 n_segs = 0;                         // the pieces added since the last launch: one kernel copies sixteen of them
    ReadBack(size_t capacity, hipStream_t s) : cap(std::max<size_t>(1, capacity)), st(s) { stage.reserve(cap * 8); }
    void flush() {
        if (!n_segs) return;
        hipLaunchKernelGGL(rb_gather_kernel, dim3(n_segs), dim3(256), 0, st, segs, stage.u());
        ZK_HIP(hipGetLastError());
        n_segs = 0;
    }
    size_t add(const u64* d_src, size_t n) {
        ZK_REQUIRE(words + n <= cap && words + n < (1ull << 32), "ReadBack: capacity");
        if (n) { segs.src[n_segs] = d_src; segs.n[n_segs] = (u32)n; segs.off[n_segs] = (u32)words; if (++n_segs == 16) flush(); }
        const size_t off = words; words += n; return off;
    }
    u64* reserve(size_t n) { ZK_REQUIRE(words + n <= cap, "ReadBack: capacity"); u64* p = stage.u() + words; words += n; return p; }
    void fetch() {
        flush();
        host.resize(std::max<size_t>(1, words));
        if (words) ZK_HIP(hipMemcpyAsync(host.data(), stage.p, words * 8, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
    }
    const u64* at(size_t off) const { return host.data() + off; }
};

zk_stark_setup* setup_new(const char* json, const char* ss_json, const uint64_t* const_pols, uint64_t n_words) {
    std::unique_ptr<zk_stark_setup> S(new zk_stark_setup);
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const clk::time_point t_begin = clk::now();
    JVal root = JParser::parse(json);
    S->info = root.at("starkinfo"); S->prog = root.at("program");
    S->ss = JParser::parse(ss_json);
    const JVal& I = S->info;
    S->nbits = (u32)S->ss.at("nBits").u64(); S->nbits_ext = (u32)S->ss.at("nBitsExt").u64();
    S->n_queries = (u32)S->ss.at("nQueries").u64();
    S->hash = hash_type_of(S->ss.at("verificationHashType").str());
    S->fr = fr_field(S->hash);
    ZK_REQUIRE(S->nbits >= 1 && S->nbits <= S->nbits_ext && S->nbits_ext <= 32, "bad nBits / nBitsExt");
    for (const JVal& st : S->ss.at("steps").arr) S->steps.push_back((u32)st.at("nBits").u64());
    ZK_REQUIRE(!S->steps.empty(), "starkStruct without FRI steps");
    S->n_constants = (u32)I.at("n_constants").u64();
    S->q_dim = (u32)I.at("q_dim").u64(); S->q_deg = (u32)I.at("q_deg").u64();
    S->n_cm1 = (u32)I.at("n_cm1").u64(); S->n_cm2 = (u32)I.at("n_cm2").u64();
    const JVal& msn = I.at("map_sectionsN");
    for (int i = 0; i < S_COUNT; ++i) if (const JVal* v = msn.find(SLOT_NAME[i])) S->sN[i] = v->u64();
    S->sN[S_CONST_N] = S->sN[S_CONST_2NS] = S->n_constants;
    S->sN[S_Q_2NS] = S->q_dim; S->sN[S_F_2NS] = 3; S->sN[S_SCRATCH] = 3;
    for (const JVal& p : I.at("var_pol_map").arr) {
        PolRef r; r.slot = slot_of(p.at("section").str()); r.width = r.slot >= 0 ? S->sN[r.slot] : 0;
        r.pos = p.at("section_pos").u64(); r.dim = (u32)p.at("dim").u64();
        S->var_pol_map.push_back(r);
    }
    S->cm_n = u64_list(I.at("cm_n")); S->cm_2ns = u64_list(I.at("cm_2ns")); S->tmpexp_n = u64_list(I.at("tmpexp_n"));
    for (auto& kv : I.at("exp2pol").obj) S->exp2pol[strtoull(kv.first.c_str(), nullptr, 10)] = kv.second.u64();

    const u64 N = 1ull << S->nbits, Next = 1ull << S->nbits_ext, nc = S->n_constants;
    ZK_REQUIRE(n_words == nc * N, "const trace size mismatch");
    const clk::time_point t_parsed = clk::now();
    const JitStats j0 = jit_stats();
    const JVal& P = S->prog;
    // Every step program on a host thread of its own, each thread handing its text to a compiler process of its own: hipRTC takes
    // seconds per program, the programs are independent, and inside one process hipRTC compiles them one after the other whatever
    // the threads (serially the three of PoseidonG were 8.0 of an 8.4 s cold setup; the code-object cache keeps one compilation per text).
    // Round 6: they start HERE, before the constants are uploaded, extended and merkelized -- the compilers are other processes on
    // host cores, the constants are copies and kernels: 0.6 s of a 2^24-row cold setup that used to stand in front of the 2.1 s of hipRTC.
    // (The futures block in their destructors: an exception below still waits for the threads that read S.)
    S->eval_mode = eval_mode();                            // this thread's: the programs are built on threads of their own, which would see their own
    const zk_stark_setup* Sc = S.get();
    const bool spawn = S->eval_mode != ZK_EVAL_BYTECODE && !getenv("ZK_JIT_INPROCESS");        // side by side really means one compiler process each (expr_jit.hip); the switch keeps hipRTC in this process
    auto start = [Sc, spawn](const JVal& seg, bool ext, bool ret) {
        return std::async(std::launch::async, [Sc, &seg, ext, ret, spawn] {
            jit_prefer_spawn(spawn && seg.at("first").size() >= 32);            // (a handful of instructions compiles faster than a process starts)
            struct Off { ~Off() { jit_prefer_spawn(false); } } off;
            return Sc->compile_segment(seg, ext, ret);
        });
    };
    std::future<ProgramPtr> f2 = start(P.at("step2prev"), false, false), f3p = start(P.at("step3prev"), false, false), f3 = start(P.at("step3"), false, false),
                            f4 = start(P.at("step42ns"), true, false), f5 = start(P.at("step52ns"), true, false);
    std::vector<std::future<ProgramPtr>> fp;
    for (const JVal& seg : P.at("publics_code").arr) fp.push_back(start(seg, false, true));
    // Round 6 (round-5 verdict, 3b): pre-size the pool.  A proof's large buffers -- the sections, the extensions' workspaces, the trees, the
    // quotient's and the evaluations' buffers: their sizes follow from map_sectionsN -- are taken from the driver HERE, on a helper thread,
    // beside the compilers and the constants, and parked in the size-keyed pool.  VRAM that any process handed back is cleared by the driver
    // when it is allocated again (~30-90 ms per GB: DESIGN.md 3.5): without this the first stark_gen of a process pays it stage by stage
    // (1.0-1.5 s at 2^24 rows on a box that is not fresh, 4 x the steady state).
    std::future<void> prewarm;
    {
        std::vector<size_t> sizes;
        const u64 nodes_bytes = S->fr ? 0 : merkle_n_nodes(Next) * 32;                   // GL trees; the scalar-field trees size themselves
        auto sec = [&](u64 words) { if (words * 8 >= (64u << 20)) sizes.push_back(words * 8); };
        for (int k : {S_CM2_N, S_CM3_N, S_TMPEXP_N}) sec(S->sN[k] * N);
        for (int k : {S_CM1_2NS, S_CM2_2NS, S_CM3_2NS}) { sec(S->sN[k] * Next); sec(S->sN[k] * Next); }   // the section and its extension's workspace
        sec(S->sN[S_CM4_2NS] * Next); sec((u64)S->q_dim * Next); sec(3 * Next); sec(3 * Next);              // cm4, q, f, scratch
        sec((u64)S->q_dim * Next); sec((u64)S->q_dim * Next);                                              // the quotient's coefficients + workspace
        if (S->q_deg) { sec((u64)S->q_dim * S->q_deg * Next); sec((u64)S->q_dim * S->q_deg * Next); }     // ... split, + the forward transform's workspace
        sec(3 * Next); sec(3 * Next);                                                                      // x / (x - xi), x / (x - xi w)
        for (int k = 0; k < 5; ++k) sec(3 * N);                                                            // the evaluations' tables (LEv, LpEv and their transforms)
        const int n_trees = (S->sN[S_CM1_N] > 0) + (S->sN[S_CM2_N] > 0) + (S->sN[S_CM3_N] > 0) + 1;        // an empty section shares the setup's zero tree
        for (int k = 0; k < n_trees && nodes_bytes >= (64u << 20); ++k) sizes.push_back(nodes_bytes);
        size_t total = 0; for (size_t b : sizes) total += b;
        const char* pw = getenv("ZK_STARK_PREWARM");
        if (total >= (1ull << 30) && !(pw && !strcmp(pw, "0"))) {
            prewarm = pool_reserve_async(std::move(sizes));
        }
    }
    S->const_n.reserve(std::max<u64>(1, nc * N) * 8); S->const_2ns.reserve(std::max<u64>(1, nc * Next) * 8);
    if (nc) {
        h2d_sync(S->const_n.p, const_pols, nc * N * 8);
        DevBuf tmp; tmp.reserve(nc * Next * 8);
        lde_dev(S->const_n.u(), S->const_2ns.u(), tmp.u(), (u32)nc, S->nbits, S->nbits_ext, nullptr);
        ZK_HIP(hipStreamSynchronize(nullptr));
    }
    S->const_tree = build_tree(S->hash, S->const_2ns.u(), (u32)nc, Next, nullptr);
    S->const_tree->root(S->const_root);                    // (copies the root back: the tree is built when this returns)
    {   // what every proof of this setup would otherwise rebuild: the two x tables, 1 / Z_H, and the tree of an empty section
        const u32 ext = S->nbits_ext - S->nbits;
        S->x_n.reserve(N * 8); S->x_2ns.reserve(Next * 8); S->zi.reserve((1ull << ext) * 8);
        x_table_dev(S->nbits, 1, S->x_n.u(), nullptr); x_table_dev(S->nbits_ext, 49, S->x_2ns.u(), nullptr); zh_inv_dev(S->nbits, ext, S->zi.u(), nullptr);
        bool any_empty = false;
        for (int sec : {S_CM1_N, S_CM2_N, S_CM3_N}) any_empty |= S->sN[sec] == 0;
        if (any_empty) S->zero_tree = build_tree(S->hash, nullptr, 0, Next, nullptr);
        ZK_HIP(hipStreamSynchronize(nullptr));
    }
    {
        const JVal& pubs = I.at("publics");
        std::vector<u64> pos(std::max<size_t>(1, pubs.size()), ~0ull);
        for (size_t i = 0; i < pubs.size(); ++i)
            if (pubs.at(i).at("polType").str() == "cmP") pos[i] = pubs.at(i).at("idx").u64() * S->sN[S_CM1_N] + pubs.at(i).at("polId").u64();
        S->d_pub_pos.reserve(pos.size() * 8);
        h2d_sync(S->d_pub_pos.p, pos.data(), pos.size() * 8);
    }
    const clk::time_point t_tree = clk::now();
    {   // the step programs were started before the constants went up (above): collect them
        std::exception_ptr err;                           // wait for all of them before an error leaves this scope (they read S)
        auto take = [&](std::future<ProgramPtr>& f) -> ProgramPtr { try { return f.get(); } catch (...) { if (!err) err = std::current_exception(); return ProgramPtr(); } };
        S->step2prev = take(f2); S->step3prev = take(f3p); S->step3 = take(f3); S->step42ns = take(f4); S->step52ns = take(f5);
        for (auto& f : fp) S->public_programs.push_back(take(f));
        if (err) std::rethrow_exception(err);
    }
    const clk::time_point t_programs = clk::now();
    if (prewarm.valid()) prewarm.get();                   // the pool holds a proof's large buffers when the setup is handed out
    {   // where the time went (stark_setup.rs:26 `#[time_profiler("stark_setup")]` has one number; a caller deciding whether to keep a
        // setup alive wants the split): JSON parsing, upload + extension + tree of the constants, kernel generation / compilation
        const clk::time_point t_jit = clk::now();         // (includes the wait for the pool's pre-sizing, reported on its own)
        const JitStats j1 = jit_stats();
        u32 n_bytecode = 0;
        for (const ProgramPtr* p : {&S->step2prev, &S->step3prev, &S->step3, &S->step42ns, &S->step52ns}) n_bytecode += *p && zk_program_kind(p->get()) == ZK_EVAL_BYTECODE;
        for (const ProgramPtr& p : S->public_programs) n_bytecode += p && zk_program_kind(p.get()) == ZK_EVAL_BYTECODE;
        std::ostringstream o; o.setf(std::ios::fixed); o.precision(3);
        o << "{\"json_parse_ms\":" << ms(t_begin, t_parsed) << ",\"const_lde_merkle_ms\":" << ms(t_parsed, t_tree) << ",\"programs_ms\":" << ms(t_parsed, t_programs)
          << ",\"programs_wait_after_constants_ms\":" << ms(t_tree, t_programs) << ",\"pool_prewarm_wait_ms\":" << ms(t_programs, t_jit)
          << ",\"hiprtc_compiled\":" << (j1.compiled - j0.compiled) << ",\"hiprtc_processes\":" << (j1.spawned - j0.spawned) << ",\"code_cache_disk_hits\":" << (j1.disk_hits - j0.disk_hits)
          << ",\"code_cache_mem_hits\":" << (j1.mem_hits - j0.mem_hits)
          << ",\"eval_mode\":\"" << (S->eval_mode == ZK_EVAL_BYTECODE ? "bytecode" : "jit") << "\",\"bytecode_programs\":" << n_bytecode << ",\"total_ms\":" << ms(t_begin, t_jit) << "}";
        S->setup_timing = o.str();
        if (getenv("ZK_STARK_TIMING") && strcmp(getenv("ZK_STARK_TIMING"), "0")) fprintf(stderr, "[zkgpu stark_setup] %s\n", S->setup_timing.c_str());
    }
    {
        bool indep = S->n_cm2 == 0 && I.at("pu_ctx").size() == 0 && I.at("pe_ctx").size() == 0 && I.at("ci_ctx").size() == 0 &&
                     S->sN[S_CM3_N] > 0 && getenv("ZK_STARK_NO_OVERLAP") == nullptr;
        if (indep)
            for (const JVal& c : P.at("step3").at("first").arr) {
                auto fixed = [](const JVal& n) {
                    const std::string& t = n.at("type_").str();
                    return t == "tmp" || t == "cm" || t == "const" || t == "number" || t == "public" || t == "x";
                };
                indep = indep && fixed(c.at("dest"));
                for (const JVal& src : c.at("src").arr) indep = indep && fixed(src);
            }
        if (indep) {
            ZK_HIP(hipStreamCreateWithFlags(&S->side_stream, hipStreamNonBlocking));
            ZK_HIP(hipEventCreateWithFlags(&S->ev_inputs, hipEventDisableTiming));
            ZK_HIP(hipEventCreateWithFlags(&S->ev_stage3, hipEventDisableTiming));
            S->early_stage3 = true;
        }
    }
    return S.release();
}

// What a proof opens (fri.rs:160-181): every tree added here at every query index, reduced by the tree's mask.  Goldilocks trees are opened
// in device memory, all of them by one launch, into regions of the proof's ReadBack; a scalar-field tree takes one round trip
// (Tree::group_proofs) into arrays held here.  resolve() leaves one view per tree -- where row q and path q lie, whoever holds them -- and
// vals() / siblings() write the zkin lists from it.
struct Openings {
    struct View { const u64* rows; const u64* paths; size_t row_stride, path_stride; u32 depth, width, level_words; };
    std::vector<const Tree*> trees; std::vector<u64> masks;
    std::vector<size_t> off;                               // Goldilocks: tree j's region of the read-back block
    std::vector<std::vector<u64>> held;                    // scalar field: the rows and the paths of every tree
    std::vector<View> views;
    u32 n = 0;                                             // queries
    const FrField* fr = nullptr;
    void add(const Tree* t, u64 mask) { trees.push_back(t); masks.push_back(mask); }
    static size_t per(const Tree& t) { return (size_t)t.width + (size_t)t.level_words() * t.depth; }   // words of one opening
    size_t readback_words() const {
        size_t w = 0;
        if (!fr) for (const Tree* t : trees) w += n * per(*t);
        return w;
    }
    void queue(ReadBack& rb, const u64* d_ys) {            // Goldilocks only: the indices are in device memory
        std::vector<const GlTree*> mt; std::vector<u64*> mo;
        off.clear();
        for (const Tree* t : trees) { off.push_back(rb.words); mt.push_back(t->gl()); mo.push_back(rb.reserve(n * per(*t))); }
        rb.flush();                                        // (the pieces collected so far are copied before the openings' launch is queued: one order on `st`)
        GlTree::open_multi_async(mt.data(), masks.data(), mo.data(), (u32)mt.size(), d_ys, n, rb.st);   // every tree, one launch
    }
    void resolve(const ReadBack& rb, const std::vector<u64>& ys) {   // after rb.fetch()
        views.clear(); held.clear();
        for (size_t j = 0; j < trees.size(); ++j) {
            const Tree& t = *trees[j];
            View v{nullptr, nullptr, per(t), per(t), t.depth, t.width, t.level_words()};
            if (!fr) { v.rows = rb.at(off[j]); v.paths = v.rows + t.width; }
            else {   // the reduced indices on the host, one round trip per tree
                std::vector<u64> idx = ys;
                for (u64& y : idx) y &= masks[j];
                v.row_stride = t.width; v.path_stride = (size_t)v.level_words * t.depth;
                held.emplace_back(std::max<size_t>(1, n * v.row_stride)); held.emplace_back(std::max<size_t>(1, n * v.path_stride));
                v.rows = held[2 * j].data(); v.paths = held[2 * j + 1].data();
                t.group_proofs(idx.data(), n, held[2 * j].data(), held[2 * j + 1].data());
            }
            views.push_back(v);
        }
    }
    void vals(JOut& o, size_t j) const {
        const View& v = views[j];
        o << '[';
        for (u32 q = 0; q < n; ++q) { if (q) o << ','; put_list(o, v.rows + q * v.row_stride, v.width); }
        o << ']';
    }
    void siblings(JOut& o, size_t j) const {
        const View& v = views[j];
        o << '[';
        for (u32 q = 0; q < n; ++q) { if (q) o << ','; put_path(o, v.paths + q * v.path_stride, v.depth, fr); }
        o << ']';
    }
};

// FRI::prove (fri.rs:84-184) on a device polynomial, whoever owns the transcript.  commit() is its commit phase (:84-157) -- the folds, the
// trees over their groups, the last polynomial's absorption -- and the draw of the query indices (:158-159).  The queries (:160-181) follow
// in three steps around the caller's one ReadBack: queue() adds the fold roots, the last polynomial, the indices and the openings of every
// tree (its own, then the caller's: add_query_tree), resolve() reads them after the fetch, put_zkin() writes the FRI part of a zkin
// (serializer.rs:189-252).  Used by a proof context and by zk_fri_prove_dev.
struct FriState {
    std::vector<TreePtr> trees;                            // tree of step i+1's groups at [i]
    std::vector<u32> width, steps;
    std::vector<std::array<u64, 4>> roots;
    const u64* d_pol = nullptr;                            // the last polynomial, 3 << steps.back() words
    std::vector<u64> ys;
    DevBuf d_ys, d_sx;
    std::vector<std::unique_ptr<DevBuf>> keep;
    Openings open;                                         // the folded polynomials' trees, then the caller's query trees
    const FrField* fr = nullptr;
    std::vector<size_t> off_root; size_t off_last = 0, off_ys = 0;   // in the ReadBack
    void add_query_tree(const Tree* t) {                   // opened at the query indices themselves: step 0
        ZK_REQUIRE(t, "zk_fri_prove_dev: null query tree");
        ZK_REQUIRE(t->height >= (1ull << steps[0]), "zk_fri_prove_dev: a query tree is shorter than the first FRI step");
        open.add(t, (1ull << steps[0]) - 1);
    }
    size_t readback_words() const { return 4 * steps.size() + (3ull << steps.back()) + open.n + open.readback_words(); }
    void queue(ReadBack& rb) {
        off_root.assign(steps.size(), 0);
        if (!fr) for (size_t si = 0; si + 1 < steps.size(); ++si) off_root[si] = rb.add(trees[si]->gl()->root_dev(), 4);
        off_last = rb.add(d_pol, 3ull << steps.back());
        if (!fr) { off_ys = rb.add(d_ys.u(), open.n); open.queue(rb, d_ys.u()); }
    }
    void resolve(const ReadBack& rb) {
        for (size_t si = 0; si + 1 < steps.size(); ++si) {
            if (!fr) memcpy(roots[si].data(), rb.at(off_root[si]), 32); else trees[si]->root(roots[si].data());
        }
        if (!fr && open.n) memcpy(ys.data(), rb.at(off_ys), 8 * (size_t)open.n);
        open.resolve(rb, ys);
    }
    // s<k>_root / s<k>_vals / s<k>_siblings of the folded polynomials, s0_vals<name> / s0_siblings<name> of the query trees, finalPol
    void put_zkin(JOut& o, const ReadBack& rb, const std::vector<std::string>& names) const {
        const size_t n_steps = steps.size();
        for (size_t si = 1; si < n_steps; ++si) {
            o << ",\"s" << si << "_root\":"; put_digest(o, roots[si - 1].data(), fr);
            o << ",\"s" << si << "_vals\":"; open.vals(o, si - 1);
            o << ",\"s" << si << "_siblings\":"; open.siblings(o, si - 1);
        }
        for (size_t j = 0; j < names.size(); ++j) { o << ",\"s0_vals" << names[j] << "\":"; open.vals(o, n_steps - 1 + j); }
        for (size_t j = 0; j < names.size(); ++j) { o << ",\"s0_siblings" << names[j] << "\":"; open.siblings(o, n_steps - 1 + j); }
        const u64 n_last = 1ull << steps.back();
        o << ",\"finalPol\":[";
        for (u64 i = 0; i < n_last; ++i) { if (i) o << ','; put_list(o, rb.at(off_last) + 3 * i, 3); }
        o << ']';
    }
    void commit(AnyTranscript& tr, HashType hash, const u64* d_f, u32 nbits_ext, const std::vector<u32>& steps_, u32 n_queries, hipStream_t st, StageTimer* T) {
        steps = steps_; fr = fr_field(hash);
        const size_t n_steps = steps.size();
        u32 pol_bits = nbits_ext;
        u64 shift_inv = gl::hinv(49);
        trees.assign(n_steps, TreePtr()); width.assign(n_steps, 0); roots.resize(n_steps);
        d_sx.reserve(24);
        d_pol = d_f;
        for (size_t si = 0; si < n_steps; ++si) {
            const u32 step_bits = steps[si];
            ZK_REQUIRE(step_bits <= pol_bits, "FRI steps must not grow");
            tr.get_field_dev(d_sx.u(), st);                                            // special_x
            keep.emplace_back(new DevBuf); DevBuf& folded = *keep.back(); folded.reserve((3ull << step_bits) * 8);
            fri_fold_dev(d_pol, pol_bits, step_bits, d_sx.u(), shift_inv, folded.u(), st);
            d_pol = folded.u();
            if (si + 1 < n_steps) {
                const u32 nxt = steps[si + 1];
                ZK_REQUIRE(nxt <= step_bits, "FRI steps must not grow");
                const u64 n_groups = 1ull << nxt, group_size = (1ull << step_bits) >> nxt;
                keep.emplace_back(new DevBuf); DevBuf& tb = *keep.back(); tb.reserve((3ull << step_bits) * 8);
                fri_transpose_dev(d_pol, 1ull << step_bits, nxt, tb.u(), st);
                width[si] = (u32)(3 * group_size);
                trees[si] = build_tree(hash, tb.u(), width[si], n_groups, st);
                tr.put_root(*trees[si], st);                                           // (its words are read for the JSON below)
            } else {
                tr.put_words_dev(d_pol, 3ull << step_bits, st);                         // fri.rs:136-141
            }
            for (u32 k = 0; k < pol_bits - step_bits; ++k) shift_inv = gl::hmul(shift_inv, shift_inv);
            pol_bits = step_bits;
        }
        if (T) T->mark("fri_prove");
        // ---- queries (fri.rs:158-181)
        // Goldilocks hashing: the query indices are squeezed into HBM, every tree is opened there at (index mod its height) and ONE copy
        // brings back roots, evaluations, the last polynomial, the publics, the indices and all openings -- one host round trip where
        // the indices, the proof's words and the openings used to be three.  Scalar-field hashing keeps its host-side sponge and trees.
        ys.assign(n_queries, 0);
        if (tr.gl) { d_ys.reserve(std::max<u32>(1, n_queries) * 8); tr.get_permutations_dev(n_queries, steps[0], d_ys.u(), st); }
        else tr.get_permutations(n_queries, steps[0], ys.data());
        if (T) T->mark("fri_query_indices");
        open.n = n_queries; open.fr = fr;
        for (size_t si = 1; si < n_steps; ++si) open.add(trees[si - 1].get(), (1ull << steps[si]) - 1);
    }
};

// One proof in progress: the body of StarkProof::stark_gen (stark_gen.rs:193-557) cut at the reference's own seams -- the places where its
// stark_gen calls calculate_exps_parallel (:786-792), extend_and_merkelize (:709-750), the transcript, calculate_H1H2 / calculate_Z and
// FRI::prove (fri.rs:84-184).  `stark_gen` below runs the stages in the reference's order; the staged C entry points (zk_stark_new,
// zk_stark_eval, zk_stark_commit_stage, zk_stark_challenge / zk_stark_set_challenge, zk_stark_evals, zk_stark_fri_prove, zk_stark_finish:
// zkgpu.h) hand the same stages to a caller that keeps its own stark_gen.rs.  Every section stays in HBM between the calls.
enum Step { STEP_2PREV = 0, STEP_3PREV = 1, STEP_3 = 2, STEP_42NS = 3, STEP_52NS = 4 };
}  // namespace

struct zk_stark_ctx {
    zk_stark_setup& S;
    hipStream_t st;
    StageTimer T;
    const JVal& I;
    const u32 nbits, nbits_ext, ext;
    const u64 N, Next;
    const u64* sN;
    DevBuf B[S_COUNT];
    u64* ptr[S_COUNT] = {};
    DevBuf d_chal, d_evals, d_pub, xdiv, xdivw, d_pub_ext, z_checks;
    u32 n_ev = 0, n_pub = 0;
    std::vector<u64> publics;
    bool pub_on_device = false;
    const FrField* const fr;                              // the scalar field of the proof's hashes; nullptr: Goldilocks (openings and sponge stay in device memory)
    std::unique_ptr<AnyTranscript> tr;
    std::vector<std::unique_ptr<DevBuf>> keep;            // workspaces alive until the end
    TreePtr tree[4];
    u64 n_cm = 0;
    size_t n_z = 0, i_z = 0;
    const u64* d_qq2 = nullptr;                           // the split quotient's coefficients [N][q_dim q_deg] (kept for the evaluations)
    bool stage3_early = false, stage3_started = false;
    FriState F;
    bool fri_done = false;
    // what has happened so far (the staged entry points refuse calls out of the reference's order)
    int committed = 0;                                    // trees 1..committed exist
    bool ran[5] = {false, false, false, false, false};
    bool h1h2_done = false, z_done = false, evals_done = false;
    u32 chal_have = 0;                                    // bit i: challenge i was drawn from the transcript or set by the caller
    void need_challenges(u32 mask, const char* who) const {
        if ((chal_have & mask) == mask) return;
        char buf[16]; snprintf(buf, sizeof buf, "0x%02x", mask & ~chal_have);
        throw Error(std::string(who) + ": its challenges come first (zk_stark_challenge or zk_stark_set_challenge; bit i of the mask = challenge i: "
                    "0 u, 1 defVal, 2 gamma, 3 beta, 4 vc, 5 v1, 6 v2, 7 xi); missing " + buf);
    }
    bool holds_early = false;                             // this context owns the setup's side stream and its two events

    zk_stark_ctx(zk_stark_setup& s, const uint64_t* cm_pols, const u64* d_cm, uint64_t n_words, hipStream_t stream)
        : S(s), st(stream), T((on_stream(stream), stream)), I(s.info), nbits(s.nbits), nbits_ext(s.nbits_ext), ext(s.nbits_ext - s.nbits),
          N(1ull << s.nbits), Next(1ull << s.nbits_ext), sN(s.sN), fr(s.fr) {
        ZK_REQUIRE(n_words == N * sN[S_CM1_N], "cm trace size mismatch");
        ClearList clear_list(st); clr = &clear_list;
        // sections (stark_gen.rs:204-229); const_n / const_2ns belong to the setup
        if (d_cm) ptr[S_CM1_N] = const_cast<u64*>(d_cm);   // read-only for the prover: cm1_n is never a destination
        else {
            B[S_CM1_N].reserve(std::max<u64>(1, n_words) * 8); ptr[S_CM1_N] = B[S_CM1_N].u();
            ZK_HIP(hipStreamSynchronize(st));                 // the block's previous user is ordered before `st`, not before this copy
            if (n_words) h2d_sync(ptr[S_CM1_N], cm_pols, n_words * 8);
        }
        for (int sec : {S_CM2_N, S_CM3_N, S_TMPEXP_N}) alloc(sec, sN[sec] * N);
        // sections that a kernel writes in full before anything reads them are not cleared: the extended sections (LDE
        // output), cm4 (the forward NTT of the split quotient), q and f (every row written by step42ns / step52ns)
        for (int sec : {S_CM1_2NS, S_CM2_2NS, S_CM3_2NS}) alloc(sec, sN[sec] * Next, false);
        alloc(S_CM4_2NS, sN[S_CM4_2NS] * Next, S.q_deg == 0);
        alloc(S_Q_2NS, S.q_dim * Next, false); alloc(S_F_2NS, 3 * Next, false); alloc(S_SCRATCH, 3 * Next);
        ptr[S_CONST_N] = S.const_n.u(); ptr[S_CONST_2NS] = S.const_2ns.u();

        d_chal.reserve(24 * 8); zero_(d_chal, 24);                                           // challenge[8] (constant.rs:39-50)
        n_ev = (u32)I.at("ev_map").size();
        n_pub = (u32)I.at("publics").size();
        d_evals.reserve(std::max<u32>(1, n_ev) * 24); zero_(d_evals, std::max<u32>(1, n_ev) * 3);
        d_pub.reserve(std::max<u32>(1, n_pub) * 8); zero_(d_pub, std::max<u32>(1, n_pub));
        for (const char* ctx : {"pu_ctx", "pe_ctx", "ci_ctx"}) n_z += I.at(ctx).arr.size();
        z_checks.reserve(24 * std::max<size_t>(1, n_z));

        // publics (stark_gen.rs:256-270) and their absorption (:272-277)
        pub_on_device = d_cm != nullptr;                  // device-resident trace: no host round trip per public
        if (pub_on_device) {
            d_pub_ext.reserve(std::max<u32>(1, n_pub) * 16); zero_(d_pub_ext, 2 * (size_t)std::max<u32>(1, n_pub));   // words 1 and 2 of every computed public: checked to be zero at the end
        }
        clear_list.flush(); clr = nullptr;                // one launch for every clearing above
        if (pub_on_device && n_pub) {
            for (u32 i = 0; i < n_pub; ++i) {
                const JVal& pe = I.at("publics").at(i);
                const std::string& ty = pe.at("polType").str();
                if (ty == "cmP") ZK_REQUIRE(pe.at("idx").u64() * sN[S_CM1_N] + pe.at("polId").u64() < n_words, "public out of range");
                else if (ty != "imP") throw Error("Invalid public type " + ty);
            }
            hipLaunchKernelGGL(gather_publics_kernel, dim3((n_pub + 63) / 64), dim3(64), 0, st, d_cm, (const u64*)S.d_pub_pos.u(), n_pub, d_pub.u());   // every cell-of-a-column public, one launch
            ZK_HIP(hipGetLastError());
            for (u32 i = 0; i < n_pub; ++i) {
                const JVal& pe = I.at("publics").at(i);
                if (pe.at("polType").str() != "imP") continue;                         // calculate_exp_at_point :558-572
                const u64 idx = pe.at("idx").u64();
                ZK_REQUIRE(i < S.public_programs.size(), "missing public program");
                ZK_REQUIRE(idx < N, "public out of range");
                run(S.public_programs[i], false, nullptr, idx, 1);                     // its one row; reads the publics before it from d_pub
                ZK_HIP(hipMemcpyAsync(d_pub.u() + i, ptr[S_SCRATCH] + 3 * idx, 8, hipMemcpyDeviceToDevice, st));
                ZK_HIP(hipMemcpyAsync(d_pub_ext.u() + 2 * i, ptr[S_SCRATCH] + 3 * idx + 1, 16, hipMemcpyDeviceToDevice, st));
            }
        }
        for (u32 i = 0; i < n_pub && !pub_on_device; ++i) {
            const JVal& pe = I.at("publics").at(i);
            const std::string& ty = pe.at("polType").str();
            const u64 idx = pe.at("idx").u64();
            if (ty == "cmP") {
                const u64 pos = idx * sN[S_CM1_N] + pe.at("polId").u64();
                ZK_REQUIRE(pos < n_words, "public out of range");
                publics.push_back(cm_pols[pos]);
            } else if (ty == "imP") {                                                  // calculate_exp_at_point :558-572
                ZK_HIP(hipStreamSynchronize(st));                                      // (the clearing of d_pub is on `st`)
                if (!publics.empty()) ZK_HIP(hipMemcpy(d_pub.p, publics.data(), 8 * publics.size(), hipMemcpyHostToDevice));
                ZK_REQUIRE(i < S.public_programs.size(), "missing public program");
                ZK_REQUIRE(idx < N, "public out of range");
                run(S.public_programs[i], false, nullptr, idx, 1);                     // its one row, not the domain
                u64 v[3];
                ZK_HIP(hipStreamSynchronize(st));
                ZK_HIP(hipMemcpy(v, ptr[S_SCRATCH] + 3 * idx, 24, hipMemcpyDeviceToHost));
                // The reference absorbs ctx.publics[i].as_elements() (stark_gen.rs:272-277): one word for a base-field value.
                // Every operand a public calculator can see is base-field at this point (columns, numbers, earlier publics,
                // x; the challenges are still F3G::ZERO of dim 1), so an extension-valued result means a malformed program.
                ZK_REQUIRE(v[1] == 0 && v[2] == 0, "public " + std::to_string(i) + ": extension-field value (only base-field publics exist in the reference)");
                publics.push_back(v[0]);
            } else throw Error("Invalid public type " + ty);
        }
        if (!pub_on_device) {
            ZK_HIP(hipStreamSynchronize(st));
            if (!publics.empty()) ZK_HIP(hipMemcpy(d_pub.p, publics.data(), 8 * publics.size(), hipMemcpyHostToDevice));
        }
        tr.reset(new AnyTranscript(S.hash));
        tr->put_words_dev(d_pub.u(), n_pub, st);
        T.mark("inputs_publics");
        // the early stage 3 runs on the SETUP's side stream and is ordered by the setup's two events: one live context at a time may use them
        // (advisor finding, round 5); a second context on the same setup takes stage 3 in order on its own stream -- the same proof
        if (S.early_stage3) {
            if (S.early_ctx_live.fetch_add(1) == 0) holds_early = true; else S.early_ctx_live.fetch_sub(1);
        }
        stage3_early = holds_early;
        n_cm = S.n_cm1;
    }
    ~zk_stark_ctx() {
        if (holds_early) {
            if (stage3_started) (void)hipStreamSynchronize(S.side_stream);          // nothing of this proof is left on the shared stream
            S.early_ctx_live.fetch_sub(1);
        }
    }
    zk_stark_ctx(const zk_stark_ctx&) = delete; zk_stark_ctx& operator=(const zk_stark_ctx&) = delete;

    ClearList* clr = nullptr;                             // the constructor's clearings travel as one launch
    void zero_(DevBuf& b, size_t words) { if (clr) clr->add(b.p, words); else zero(b, words, st); }
    void alloc(int s, u64 words, bool zeroed = true) {
        B[s].reserve(std::max<u64>(1, words) * 8); if (zeroed) zero_(B[s], words); ptr[s] = B[s].u();
    }
    void run(const ProgramPtr& p, bool e, hipStream_t on = nullptr, u64 row0 = 0, u64 count = ~0ull) {
        if (!p) return;
        zk_eval_ctx c; memset(&c, 0, sizeof c);
        for (int s = 0; s < S_COUNT; ++s) c.bufs[s] = M(ptr[s]);
        c.publics = C(d_pub.u()); c.challenges = C(d_chal.u()); c.evals = C(d_evals.u());
        c.x = C(e ? S.x_2ns.u() : S.x_n.u()); c.zi = C(S.zi.u()); c.zi_mask = (1ull << ext) - 1;
        c.xdivxsubxi = C(xdiv.u()); c.xdivxsubwxi = C(xdivw.u());
        const u32 nb = e ? nbits_ext : nbits;
        ck(zk_program_run_rows_dev(p.get(), &c, nb, e ? (1ull << ext) : 1, row0, count == ~0ull ? 1ull << nb : count, on ? on : st));
        if (on) on_stream(st);                                                     // this thread goes on issuing on `st`
    }
    void get_pol(u64 pol_id, DevBuf& out) {                                        // stark_gen.rs:683-707
        const PolRef p = S.pol(pol_id);
        out.reserve(3 * N * 8);
        pol_get_dev(ptr[p.slot], p.width, p.pos, p.dim, N, out.u(), st);
    }
    void set_pol(u64 pol_id, const u64* d_pol3) {                                  // stark_gen.rs:594-622
        const PolRef p = S.pol(pol_id);
        pol_set_dev(ptr[p.slot], p.width, p.pos, p.dim, N, d_pol3, st);
    }
    u64 e2p(const JVal& v) const {
        auto it = S.exp2pol.find(v.u64());
        if (it == S.exp2pol.end()) throw Error("exp2pol: unknown expression");
        return it->second;
    }
    TreePtr extend_and_merkelize(int sec_n, int sec_2ns) {                         // stark_gen.rs:709-732
        const u64 width = sN[sec_n];
        if (width) {
            keep.emplace_back(new DevBuf); keep.back()->reserve(width * Next * 8);
            lde_dev(ptr[sec_n], ptr[sec_2ns], keep.back()->u(), (u32)width, nbits, nbits_ext, st);
        }
        T.mark("extend");                                                          // the two halves of extend_and_merkelize (:709, :734)
        if (!width && S.zero_tree) return S.zero_tree;                            // an empty section: every node is the all-zero digest of its level
        TreePtr t = build_tree(S.hash, ptr[sec_2ns], (u32)width, Next, st);
        T.mark("merkelize");
        return t;
    }
    // transcript.get_field() -> challenge i (u, defVal, gamma, beta, vc, v1, v2, xi: constant.rs:39-50), kept in HBM for the step programs
    // (count consecutive challenges in one launch, together with the root absorbed just before)
    // The transcript must hold what the reference has absorbed when it draws challenge i (stark_gen.rs:285-294, 313-321, 362-369, 407-414, 474-479):
    // u, defVal after root 1; gamma, beta after root 2; vc after root 3; xi after root 4; v1, v2 after the evaluations.
    void challenge_allowed(int i, int count) const {
        ZK_REQUIRE(i >= 0 && count >= 1 && i + count <= 8, "challenge index");
        for (int k = i; k < i + count; ++k) {
            const int need = k <= 1 ? 1 : k <= 3 ? 2 : k == 4 ? 3 : 4;
            ZK_REQUIRE(committed >= need, "challenge: the commitment it is drawn after comes first (u, defVal: 1; gamma, beta: 2; vc: 3; xi, v1, v2: 4)");
            if (k == 5 || k == 6) ZK_REQUIRE(evals_done, "challenge v1 / v2: the evaluations are absorbed first (stark_gen.rs:472-479)");
        }
    }
    void challenge(int i, int count = 1) {
        challenge_allowed(i, count);
        tr->get_fields_dev(d_chal.u() + 3 * i, (u32)count, st);
        chal_have |= ((1u << count) - 1) << i;
    }
    void set_challenge(int i, const u64 v[3]) {                                    // a caller with its own transcript
        challenge_allowed(i, 1);
        ZK_HIP(hipMemcpyAsync(d_chal.u() + 3 * i, v, 24, hipMemcpyHostToDevice, st));
        ZK_HIP(hipStreamSynchronize(st));                                          // (v is the caller's)
        chal_have |= 1u << i;
    }
    void get_challenge(int i, u64 out[3]) {
        ZK_REQUIRE(i >= 0 && i < 8, "challenge index");
        ZK_HIP(hipMemcpyAsync(out, d_chal.u() + 3 * i, 24, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
    }

    // Stage-3 columns that depend on no challenge (setup_new decided): evaluated and extended on the side stream while the
    // main stream hashes tree 1 -- memory-bound work beside ALU-bound work.  Values and transcript order are the same.
    void start_early_stage3() {
        if (!stage3_early || stage3_started) return;
        stage3_started = true;
        ZK_HIP(hipEventRecord(S.ev_inputs, st));                                   // tables, cleared sections, publics: issued on `st`
        ZK_HIP(hipStreamWaitEvent(S.side_stream, S.ev_inputs, 0));
        run(S.step3, false, S.side_stream);
        on_stream(S.side_stream);                                                  // the workspace below is used on the side stream
        keep.emplace_back(new DevBuf); keep.back()->reserve(sN[S_CM3_N] * Next * 8);
        lde_dev(ptr[S_CM3_N], ptr[S_CM3_2NS], keep.back()->u(), (u32)sN[S_CM3_N], nbits, nbits_ext, S.side_stream);
        ZK_HIP(hipEventRecord(S.ev_stage3, S.side_stream));
        on_stream(st);
    }

    // extend_and_merkelize of stage `stage` (1..3) or the Q split + tree 4 (stark_gen.rs:375-405), and the root's absorption
    void commit(int stage) {
        ZK_REQUIRE(stage == committed + 1 && stage >= 1 && stage <= 4, "commit_stage: stages are committed in order 1, 2, 3, 4");
        on_stream(st);
        if (stage == 1) {
            start_early_stage3();
            tree[0] = extend_and_merkelize(S_CM1_N, S_CM1_2NS);
        } else if (stage == 2) {
            ZK_REQUIRE(ran[STEP_2PREV] && h1h2_done, "commit_stage 2: step2prev and calculate_H1H2 come first (stark_gen.rs:296-311)");
            tree[1] = extend_and_merkelize(S_CM2_N, S_CM2_2NS);
        } else if (stage == 3) {
            ZK_REQUIRE(ran[STEP_3PREV] && z_done && ran[STEP_3], "commit_stage 3: step3prev, calculate_Z and step3 come first (stark_gen.rs:323-362)");
            if (stage3_early) {
                ZK_HIP(hipStreamWaitEvent(st, S.ev_stage3, 0));                    // cm3_n and its extension are ready
                T.mark("wait_side_stream");
                tree[2] = build_tree(S.hash, ptr[S_CM3_2NS], (u32)sN[S_CM3_N], Next, st);
                T.mark("merkelize");
            } else tree[2] = extend_and_merkelize(S_CM3_N, S_CM3_2NS);
        } else {
            ZK_REQUIRE(ran[STEP_42NS], "commit_stage 4: step42ns comes first (stark_gen.rs:371-373)");
            const u32 q_dim = S.q_dim, q_deg = S.q_deg;                            // Q split (stark_gen.rs:375-396)
            keep.emplace_back(new DevBuf); DevBuf& qq1 = *keep.back(); qq1.reserve(q_dim * Next * 8);
            keep.emplace_back(new DevBuf); DevBuf& tmpq = *keep.back(); tmpq.reserve(q_dim * Next * 8);
            ntt_dev(ptr[S_Q_2NS], qq1.u(), tmpq.u(), q_dim, nbits_ext, true, st);
            if (q_deg > 0) {
                keep.emplace_back(new DevBuf); DevBuf& qq2 = *keep.back(); qq2.reserve((u64)q_dim * q_deg * Next * 8);
                ZK_HIP(hipMemsetAsync(qq2.p, 0, (u64)q_dim * q_deg * Next * 8, st));
                qsplit_dev(qq1.u(), nbits, q_dim, q_deg, qq2.u(), st);
                d_qq2 = qq2.u();
                keep.emplace_back(new DevBuf); DevBuf& tmp4 = *keep.back(); tmp4.reserve((u64)q_dim * q_deg * Next * 8);
                ntt_dev(qq2.u(), ptr[S_CM4_2NS], tmp4.u(), q_dim * q_deg, nbits_ext, false, st);
            }
            T.mark("q_split_ntt");
            tree[3] = build_tree(S.hash, ptr[S_CM4_2NS], (u32)sN[S_CM4_2NS], Next, st);  // stark_gen.rs:399-405
            T.mark("merkelize");
        }
        tr->put_root(*tree[stage - 1], st);
        committed = stage;
    }

    // calculate_exps_parallel(ctx, starkinfo, segment, domain, step) (stark_gen.rs:786-792) for one of the five step programs
    void eval(int step) {
        ZK_REQUIRE(step >= 0 && step <= 4, "eval: step id");
        ZK_REQUIRE(!ran[step], "eval: every step program runs once per proof");
        on_stream(st);
        switch (step) {
            case STEP_2PREV:
                ZK_REQUIRE(committed >= 1, "step2prev follows the first commitment and the challenges u, defVal");
                need_challenges(0x03, "step2prev");
                run(S.step2prev, false); break;
            case STEP_3PREV:
                ZK_REQUIRE(committed >= 2, "step3prev follows the second commitment and the challenges gamma, beta");
                need_challenges(0x0c, "step3prev");
                zero(B[S_TMPEXP_N], sN[S_TMPEXP_N] * N, st);                       // an output-only section starts from zero (stark_gen.rs:944-951)
                run(S.step3prev, false); break;
            case STEP_3:
                ZK_REQUIRE(ran[STEP_3PREV] && z_done, "step3 follows step3prev and calculate_Z");
                if (!stage3_early) run(S.step3, false);                            // (early: already running on the side stream since commit 1)
                break;
            case STEP_42NS:
                ZK_REQUIRE(committed >= 3, "step42ns follows the third commitment and the challenge vc");
                need_challenges(0x10, "step42ns");
                run(S.step42ns, true); break;
            default:
                ZK_REQUIRE(evals_done, "step52ns follows the evaluations and the challenges v1, v2");
                need_challenges(0xe0, "step52ns");
                xdiv.reserve(3 * Next * 8); xdivw.reserve(3 * Next * 8);            // stark_gen.rs:481-522
                xdivxsub2_dev(d_chal.u() + 3 * 7, 1, gl::hroot(nbits), nbits_ext, xdiv.u(), xdivw.u(), st);   // both tables, one launch
                T.mark("xDivXSubXi");
                run(S.step52ns, true); break;
        }
        ran[step] = true;
        T.mark("calculate_exps_parallel");
    }
    void calculate_h1h2() {                                                        // stark_gen.rs:300-308, every plookup of the PIL
        ZK_REQUIRE(ran[STEP_2PREV] && !h1h2_done, "calculate_H1H2 follows step2prev, once");
        on_stream(st);
        n_cm = S.n_cm1;
        for (const JVal& pu : I.at("pu_ctx").arr) {
            DevBuf f, t, h1, h2;
            get_pol(e2p(pu.at("f_exp_id")), f); get_pol(e2p(pu.at("t_exp_id")), t);
            h1.reserve(24 * N); h2.reserve(24 * N);
            ck(zk_stark_calculate_h1h2_dev(C(f.u()), C(t.u()), N, M(h1.u()), M(h2.u()), st));
            set_pol(S.cm_n.at(n_cm++), h1.u()); set_pol(S.cm_n.at(n_cm++), h2.u());
            T.mark("calculate_H1H2");
        }
        h1h2_done = true;
    }
    // every z must close (grand product 1, stark_gen.rs:663-664): the products stay in HBM and come back with the proof's one
    // read-back -- checking each on the spot was a host round trip in the middle of the proof
    void calculate_z() {                                                           // stark_gen.rs:329-353
        ZK_REQUIRE(ran[STEP_3PREV] && !z_done, "calculate_Z follows step3prev, once");
        on_stream(st);
        n_cm = S.n_cm1 + S.n_cm2;
        for (const char* ctx : {"pu_ctx", "pe_ctx", "ci_ctx"}) {
            for (const JVal& o : I.at(ctx).arr) {
                DevBuf num, den, z, work;
                get_pol(e2p(o.at("num_id")), num); get_pol(e2p(o.at("den_id")), den);
                z.reserve(3 * N * 8); work.reserve((N + N / 1024 + 8) * 24);
                calculate_z_dev(num.u(), den.u(), N, z.u(), work.u(), z_checks.u() + 3 * i_z++, st);
                set_pol(S.cm_n.at(n_cm++), z.u());
                T.mark("calculate_Z");
            }
        }
        zero(B[S_TMPEXP_N], sN[S_TMPEXP_N] * N, st);
        z_done = true;
    }

    // Evaluations at xi and xi w (stark_gen.rs:416-466).  The reference weighs the rows k 2^ext of the EXTENDED sections with
    // LEv = ifft(powers of xi / shift).  The same values come from the sections themselves -- p(xi) = sum_k p(w^k) L'[k] with
    // L' = ifft(powers of xi), the shift-1 instance of the same identity -- and, for the quotient's pieces (which only exist
    // extended), from their coefficients qq2 and the powers of xi: every read is a contiguous row of an N-row buffer instead of
    // every other row of a 2N-row one, half the bytes.  Field arithmetic is exact: the evaluations, hence the proof, are the same words.
    // (cm4_2ns is the plain transform of qq2, i.e. the coset values of the polynomial with coefficients qq2_i / shift^i: its value at
    // xi is sum_i qq2_i (xi / shift)^i -- the weights of the coefficients are the powers the reference feeds its ifft.)
    void evals() {
        ZK_REQUIRE(committed == 4 && !evals_done, "the evaluations follow the fourth commitment and the challenge xi, once");
        need_challenges(0x80, "evals");
        on_stream(st);
        const u64* d_xi = d_chal.u() + 3 * 7;
        DevBuf LEv, LpEv, pw, pwp, lt1, lt1p, lt2;
        LEv.reserve(3 * N * 8); LpEv.reserve(3 * N * 8); lt1.reserve(3 * N * 8); lt1p.reserve(3 * N * 8); lt2.reserve(3 * N * 8);
        bool q_plain = false, q_prime = false;            // which openings of the quotient's pieces exist
        for (const JVal& ev : I.at("ev_map").arr)
            if (ev.at("type_").str() == "cm" && S.pol(S.cm_2ns.at(ev.at("id").u64())).slot == S_CM4_2NS) (ev.at("prime").boolean() ? q_prime : q_plain) = true;
        {   // every table of powers this stage needs in ONE launch (each is an exponentiation chain per lane: two to four launches stood in a row):
            // the powers of xi and xi w (-> LEv, LpEv by the inverse transforms below), of xi / 49 and xi w / 49 (the quotient's weights)
            bool prime[4] = {false, true, false, true}; u64 shift[4] = {1, 1, 49, 49}; u64* out[4] = {lt1.u(), lt1p.u(), nullptr, nullptr};
            u32 nt = 2;
            if (d_qq2 && q_plain) { pw.reserve(3 * N * 8); prime[nt] = false; shift[nt] = 49; out[nt++] = pw.u(); }
            if (d_qq2 && q_prime) { pwp.reserve(3 * N * 8); prime[nt] = true; shift[nt] = 49; out[nt++] = pwp.u(); }
            lev_pow_multi_dev(d_xi, nbits, nt, prime, shift, out, st);
            ntt_dev(lt1.u(), LEv.u(), lt2.u(), 3, nbits, true, st);                   // FFT::ifft over F3G == per-limb iNTT (base-field roots)
            ntt_dev(lt1p.u(), LpEv.u(), lt2.u(), 3, nbits, true, st);
        }
        if (n_ev) {
            std::vector<EvalDescKHost> descs;
            for (const JVal& ev : I.at("ev_map").arr) {
                const std::string& ty = ev.at("type_").str();
                const bool prime = ev.at("prime").boolean();
                EvalDescKHost d; d.rshift = 0; d.L = prime ? LpEv.u() : LEv.u();
                if (ty == "const") { d.buf = ptr[S_CONST_N]; d.width = S.n_constants; d.offset = ev.at("id").u64(); d.dim = 1; }
                else if (ty == "cm") {
                    const u64 id = ev.at("id").u64();
                    const PolRef p2 = S.pol(S.cm_2ns.at(id));
                    if (p2.slot == S_CM4_2NS) {                                    // a piece of the quotient: its coefficients (Q split above)
                        ZK_REQUIRE(d_qq2 != nullptr, "evaluation of a quotient piece without a split quotient");
                        d.buf = d_qq2; d.width = p2.width; d.offset = p2.pos; d.dim = p2.dim; d.L = prime ? pwp.u() : pw.u();
                    } else {
                        ZK_REQUIRE(id < S.cm_n.size(), "ev_map: cm id out of range");
                        const PolRef p = S.pol(S.cm_n.at(id));                     // the same column before its extension
                        ZK_REQUIRE(p.dim == p2.dim, "ev_map: section mismatch");
                        d.buf = ptr[p.slot]; d.width = p.width; d.offset = p.pos; d.dim = p.dim;
                    }
                } else throw Error("Invalid ev type: " + ty);
                descs.push_back(d);
            }
            evals_k_dev(descs.data(), n_ev, nbits, d_evals.u(), st);
            tr->put_words_dev(d_evals.u(), 3 * (size_t)n_ev, st);                      // stark_gen.rs:469-472
        }
        evals_done = true;
        T.mark("evals");
    }

    // ---- FRI::prove (fri.rs:84-184) over the polynomial step52ns left in f_2ns: folds, their trees, the last polynomial, the query indices;
    // its queries open the proof's five trees
    void fri_prove() {
        ZK_REQUIRE(ran[STEP_52NS] && !fri_done, "FRI::prove follows step52ns, once");
        on_stream(st);
        F.commit(*tr, S.hash, ptr[S_F_2NS], nbits_ext, S.steps, S.n_queries, st, &T);
        for (const Tree* t : {tree[0].get(), tree[1].get(), tree[2].get(), tree[3].get(), S.const_tree.get()}) F.add_query_tree(t);
        fri_done = true;
    }

    // ---- the openings, one read-back, proof -> zkin JSON (serializer.rs:146-261)
    std::string finish() {
        ZK_REQUIRE(fri_done, "finish follows FRI::prove");
        on_stream(st);
        ReadBack rb(4 * 4 + 3 * (size_t)n_ev + 3 * (size_t)n_pub + 3 * n_z + F.readback_words(), st);   // lives until the text is written: its words are read in place
        u64 r_host[4][4]; const u64* r[4];                // root1..4: in the read-back block, or fetched from a scalar-field tree
        size_t off_r[4] = {};
        if (!fr) for (int j = 0; j < 4; ++j) off_r[j] = rb.add(tree[j]->gl()->root_dev(), 4);
        const size_t off_ev = rb.add(d_evals.u(), 3 * (size_t)n_ev), off_z = rb.add(z_checks.u(), 3 * n_z);
        const size_t off_pub = pub_on_device ? rb.add(d_pub.u(), n_pub) : 0, off_ext = pub_on_device ? rb.add(d_pub_ext.u(), 2 * (size_t)n_pub) : 0;
        F.queue(rb);
        rb.fetch();
        for (size_t i = 0; i < n_z; ++i)
            ZK_REQUIRE(rb.at(off_z)[3 * i] == 1 && rb.at(off_z)[3 * i + 1] == 0 && rb.at(off_z)[3 * i + 2] == 0, "calculate_Z: z does not close (grand product != 1)");
        if (pub_on_device) {
            publics.assign(rb.at(off_pub), rb.at(off_pub) + n_pub);
            // The reference absorbs ctx.publics[i].as_elements() (stark_gen.rs:272-277): one word for a base-field value; a
            // computed public with extension words means a malformed program (see the host-trace path above)
            for (u32 i = 0; i < n_pub; ++i)
                ZK_REQUIRE(rb.at(off_ext)[2 * i] == 0 && rb.at(off_ext)[2 * i + 1] == 0,
                           "public " + std::to_string(i) + ": extension-field value (only base-field publics exist in the reference)");
        }
        for (int j = 0; j < 4; ++j) {
            if (!fr) r[j] = rb.at(off_r[j]); else { tree[j]->root(r_host[j]); r[j] = r_host[j]; }
        }
        F.resolve(rb);
        T.mark("openings_readback");
        S.last_timing = T.finish(nbits);
        S.t_json_begin = std::chrono::steady_clock::now();
        JOut o;
        o << "{\"rootC\":"; put_digest(o, S.const_root, fr);
        o << ",\"root1\":"; put_digest(o, r[0], fr); o << ",\"root2\":"; put_digest(o, r[1], fr);
        o << ",\"root3\":"; put_digest(o, r[2], fr); o << ",\"root4\":"; put_digest(o, r[3], fr);
        o << ",\"evals\":[";
        for (u32 e = 0; e < n_ev; ++e) { if (e) o << ','; put_list(o, rb.at(off_ev) + 3 * e, 3); }
        o << ']';
        F.put_zkin(o, rb, {"1", "2", "3", "4", "C"});
        o << ",\"publics\":"; put_list(o, publics.data(), publics.size());
        if (fr) {                                          // serializer.rs:255-262: non-GL proofs carry the prover address
            o << ",\"proverAddr\":\"";
            for (char c : S.prover_addr) { if (c == '"' || c == '\\') o << '\\'; o << c; }
            o << '"';
        }
        o << '}';
        S.t_json_end = std::chrono::steady_clock::now();
        return o.str();
    }
};

namespace {

// cm_pols: host trace, or nullptr when d_cm (device-resident trace, borrowed) is given.  The reference's stark_gen, stage by stage.
std::string stark_gen(zk_stark_setup& S, const uint64_t* cm_pols, const u64* d_cm, uint64_t n_words, hipStream_t st) {
    std::string zkin;
    {
        zk_stark_ctx P(S, cm_pols, d_cm, n_words, st);
        auto T = [&](const char* name) { P.T.mark(name); };
        P.commit(1); P.challenge(0, 2); T("transcript");                           // u, defVal (stark_gen.rs:279-294)
        P.eval(STEP_2PREV);
        P.calculate_h1h2();
        P.commit(2); P.challenge(2, 2); T("transcript");                           // gamma, beta (:310-321)
        P.eval(STEP_3PREV);
        P.calculate_z();
        P.eval(STEP_3);
        P.commit(3); P.challenge(4); T("transcript");                              // vc (:355-369)
        P.eval(STEP_42NS);
        P.commit(4); P.challenge(7); T("transcript");                              // xi (:399-414)
        P.evals();
        P.challenge(5, 2); T("transcript");                                        // v1, v2 (:474-479)
        P.eval(STEP_52NS);
        P.fri_prove();
        zkin = P.finish();
        pool_defer_begin();                               // nothing is launched from here on: the buffers and trees go back as one burst
    }
    return zkin;
}

// prove.rs:124-132: `assert!(stark_verify(...))` on the fresh proof, opt-in per setup (zk_stark_setup_set_self_check)
void self_check(const zk_stark_setup& S, const std::string& zkin) {
    if (!S.self_check) return;
    pool_defer_flush();                                   // the proof's buffers go back before the verifier asks for its own
    std::string why;
    if (!stark_verify_impl(S.info, S.prog, S.ss, S.const_root, zkin.c_str(), why)) throw Error("stark_gen: the proof does not verify: " + why);
}

}  // namespace

extern "C" {

zk_stark_setup_t* zk_stark_setup_new(const char* starkinfo_program_json, const char* stark_struct_json,
                                     const uint64_t* const_pols, uint64_t n_words) {
    zk_stark_setup* s = nullptr;
    if (guard([&] {
            ZK_REQUIRE(starkinfo_program_json && stark_struct_json, "zk_stark_setup_new: null json");
            ZK_REQUIRE(const_pols || n_words == 0, "zk_stark_setup_new: null constant trace");
            s = setup_new(starkinfo_program_json, stark_struct_json, const_pols, n_words);
        }) != 0) return nullptr;
    return s;
}

int zk_stark_setup_const_root(const zk_stark_setup_t* s, uint64_t out[4]) {
    return guard([&] { ZK_REQUIRE(s && out, "null argument"); memcpy(out, s->const_root, 32); });
}

char* zk_stark_gen(zk_stark_setup_t* s, const uint64_t* cm_pols, uint64_t n_words) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(s, "zk_stark_gen: null setup");
            ZK_REQUIRE(cm_pols || n_words == 0, "zk_stark_gen: null trace");
            const std::string z = stark_gen(*s, cm_pols, nullptr, n_words, nullptr);
            self_check(*s, z);
            out = (char*)malloc(z.size() + 1);
            ZK_REQUIRE(out, "out of memory");
            memcpy(out, z.c_str(), z.size() + 1);
        }) != 0) return nullptr;
    return out;
}

char* zk_stark_gen_dev(zk_stark_setup_t* s, const uint64_t* d_cm_pols, uint64_t n_words) {
    return zk_stark_gen_dev_on(s, d_cm_pols, n_words, nullptr);
}

char* zk_stark_gen_dev_on(zk_stark_setup_t* s, const uint64_t* d_cm_pols, uint64_t n_words, void* stream) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(s && d_cm_pols, "zk_stark_gen_dev: null argument");
            const auto t0 = std::chrono::steady_clock::now();
            const std::string z = stark_gen(*s, nullptr, K(d_cm_pols), n_words, (hipStream_t)stream);
            pool_defer_flush();                                        // stark_gen's locals are gone: their blocks are stamped with one set of events and released HERE,
            const auto t1 = std::chrono::steady_clock::now();          // inside host_release_ms (the call scope's flush only covers the error paths now)
            self_check(*s, z);
            const auto t2 = std::chrono::steady_clock::now();
            out = (char*)malloc(z.size() + 1);
            ZK_REQUIRE(out, "out of memory");
            memcpy(out, z.c_str(), z.size() + 1);
            if (!s->last_timing.empty() && s->last_timing.back() == '}') {   // a timing run: where the host time after the last launch went
                auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
                char buf[256];
                snprintf(buf, sizeof buf, ",\"host_json_ms\":%.3f,\"host_release_ms\":%.3f,\"self_check_ms\":%.3f,\"host_copy_ms\":%.3f,\"call_ms\":%.3f,\"zkin_bytes\":%zu}",
                         ms(s->t_json_begin, s->t_json_end), ms(s->t_json_end, t1), ms(t1, t2), ms(t2, std::chrono::steady_clock::now()), ms(t0, std::chrono::steady_clock::now()), z.size());
                s->last_timing.pop_back(); s->last_timing += buf;
            }
        }) != 0) return nullptr;
    return out;
}

const char* zk_stark_setup_timing(const zk_stark_setup_t* s) { return s ? s->setup_timing.c_str() : ""; }
const char* zk_stark_last_timing(const zk_stark_setup_t* s) { return s ? s->last_timing.c_str() : ""; }

int zk_stark_setup_set_prover_addr(zk_stark_setup_t* s, const char* prover_addr) {
    return guard([&] { ZK_REQUIRE(s && prover_addr, "null argument"); s->prover_addr = prover_addr; });
}

int zk_stark_setup_set_self_check(zk_stark_setup_t* s, int on) {
    return guard([&] { ZK_REQUIRE(s, "null argument"); s->self_check = on != 0; });
}

int zk_stark_verify(const zk_stark_setup_t* s, const char* zkin_json) {
    int ok = -1;
    if (guard([&] {
            ZK_REQUIRE(s && zkin_json, "zk_stark_verify: null argument");
            std::string why;
            ok = stark_verify_impl(s->info, s->prog, s->ss, s->const_root, zkin_json, why);
            if (!ok) set_error("stark_verify: " + why);
        }) != 0) return -1;
    return ok;
}

// ---- the staged prover (zk_stark_new / zk_stark_eval / zk_stark_commit_stage / zk_stark_set_challenge / zk_stark_evals / zk_fri_prove) ----
zk_stark_ctx_t* zk_stark_new(zk_stark_setup_t* s, const uint64_t* cm_pols, const uint64_t* d_cm_pols, uint64_t n_words, void* stream) {
    zk_stark_ctx* c = nullptr;
    if (guard([&] {
            ZK_REQUIRE(s, "zk_stark_new: null setup");
            ZK_REQUIRE((cm_pols != nullptr) != (d_cm_pols != nullptr) || n_words == 0, "zk_stark_new: the trace is given once, in host memory or in device memory");
            c = new zk_stark_ctx(*s, cm_pols, K(d_cm_pols), n_words, (hipStream_t)stream);
        }) != 0) return nullptr;
    return c;
}
int zk_stark_commit_stage(zk_stark_ctx_t* c, int stage, uint64_t root[4]) {
    return guard([&] {
        ZK_REQUIRE(c, "null context");
        c->commit(stage);
        if (root) { u64 r[4]; c->tree[stage - 1]->root(r); memcpy(root, r, 32); }
    });
}
int zk_stark_challenge(zk_stark_ctx_t* c, int i, uint64_t out[3]) {
    return guard([&] {
        ZK_REQUIRE(c, "null context");
        on_stream(c->st);
        c->challenge(i);
        if (out) { u64 v[3]; c->get_challenge(i, v); memcpy(out, v, 24); }
    });
}
int zk_stark_set_challenge(zk_stark_ctx_t* c, int i, const uint64_t v[3]) {
    return guard([&] { ZK_REQUIRE(c && v, "null argument"); on_stream(c->st); c->set_challenge(i, K(v)); });
}
int zk_stark_eval(zk_stark_ctx_t* c, int step) { return guard([&] { ZK_REQUIRE(c, "null context"); c->eval(step); }); }
int zk_stark_calculate_h1h2(zk_stark_ctx_t* c) { return guard([&] { ZK_REQUIRE(c, "null context"); c->calculate_h1h2(); }); }
int zk_stark_calculate_z(zk_stark_ctx_t* c) { return guard([&] { ZK_REQUIRE(c, "null context"); c->calculate_z(); }); }
int zk_stark_evals(zk_stark_ctx_t* c, uint64_t* evals_out, uint64_t cap_words) {
    int n = -1;
    if (guard([&] {
            ZK_REQUIRE(c, "null context");
            c->evals();
            if (evals_out) {
                ZK_REQUIRE(cap_words >= 3ull * c->n_ev, "zk_stark_evals: the output holds fewer than 3 words per evaluation");
                if (c->n_ev) ZK_HIP(hipMemcpyAsync(evals_out, c->d_evals.p, 24ull * c->n_ev, hipMemcpyDeviceToHost, c->st));
                ZK_HIP(hipStreamSynchronize(c->st));
            }
            n = (int)c->n_ev;
        }) != 0) return -1;
    return n;
}
int zk_stark_fri_prove(zk_stark_ctx_t* c) { return guard([&] { ZK_REQUIRE(c, "null context"); c->fri_prove(); }); }
char* zk_stark_finish(zk_stark_ctx_t* c) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(c, "null context");
            const std::string z = c->finish();
            self_check(c->S, z);
            out = (char*)malloc(z.size() + 1);
            ZK_REQUIRE(out, "out of memory");
            memcpy(out, z.c_str(), z.size() + 1);
        }) != 0) return nullptr;
    return out;
}
const uint64_t* zk_stark_fri_pol_dev(const zk_stark_ctx_t* c) { return c && c->ran[STEP_52NS] ? C(c->ptr[S_F_2NS]) : nullptr; }
const zk_merkle_t* zk_stark_tree(const zk_stark_ctx_t* c, int j) {
    if (!c || j < 1 || j > 5) return nullptr;
    const Tree* t = j == 5 ? c->S.const_tree.get() : (j <= c->committed ? c->tree[j - 1].get() : nullptr);
    return dynamic_cast<const zk_merkle_t*>(t);           // (scalar-field trees have no zk_merkle_t: NULL)
}
int zk_stark_free(zk_stark_ctx_t* c) { return guard([&] { if (c) { on_stream(c->st); pool_defer_begin(); delete c; } }); }

// FRI::prove(transcript, pol, query_pol) (fri.rs:84-184) on its own: the caller's TranscriptGL, a device polynomial of 2^nbits_ext extension
// values and the trees the queries open (the reference passes them as the `query_pol` closure).  -> JSON text, the FRI part of a zkin
// (serializer.rs:189-252) with the query trees numbered from 1: s<k>_root / s<k>_vals / s<k>_siblings for the folded polynomials,
// s0_vals<j> / s0_siblings<j> for query tree j, finalPol, plus "ys", the query indices.
char* zk_fri_prove_dev(zk_transcript_t* transcript, const uint64_t* d_pol, uint32_t nbits_ext, const uint32_t* steps, uint32_t n_steps,
                       uint32_t n_queries, const zk_merkle_t* const* query_trees, uint32_t n_query_trees, void* stream) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(transcript && d_pol && steps && n_steps >= 1 && (query_trees || n_query_trees == 0), "zk_fri_prove_dev: null argument");
            ZK_REQUIRE(nbits_ext <= 32 && steps[0] <= nbits_ext, "zk_fri_prove_dev: the first step cannot exceed the polynomial's size");
            hipStream_t st = (hipStream_t)stream;
            on_stream(st);
            const std::vector<u32> sv(steps, steps + n_steps);
            FriState F;                                    // declared BEFORE the borrowed transcript: on an exception the transcript goes first and
            AnyTranscript tr(transcript);                  // flushes its deferred put while the buffers it points into (F's) still exist
            F.commit(tr, HASH_GL, K(d_pol), nbits_ext, sv, n_queries, st, nullptr);
            std::vector<std::string> names;
            for (u32 j = 0; j < n_query_trees; ++j) { F.add_query_tree(query_trees[j]); names.push_back(std::to_string(j + 1)); }
            ReadBack rb(F.readback_words(), st);
            F.queue(rb);
            rb.fetch();
            F.resolve(rb);
            JOut o;
            o << "{\"ys\":"; put_list(o, F.ys.data(), n_queries);
            F.put_zkin(o, rb, names);
            o << '}';
            const std::string z = o.str();
            pool_defer_begin();
            out = (char*)malloc(z.size() + 1);
            ZK_REQUIRE(out, "out of memory");
            memcpy(out, z.c_str(), z.size() + 1);
        }) != 0) return nullptr;
    return out;
}

void zk_string_free(char* s) { free(s); }

int zk_stark_setup_free(zk_stark_setup_t* s) { return guard([&] { delete s; }); }

}  // extern "C"
