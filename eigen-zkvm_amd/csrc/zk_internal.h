// Internal plumbing shared by the HIP translation units of libzkgpu (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <future>
#include <string>
#include <stdexcept>
#include <vector>
#include "gl.hip.h"

struct zk_program;
namespace zk {

// ---- error handling: C ABI returns int status, message kept per thread (include/zkgpu.h) ----
void set_error(const std::string& msg);
const char* last_error();
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

#define ZK_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            throw zk::Error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" +     \
                            __FILE__ + ":" + std::to_string(__LINE__) + ")");                     \
    } while (0)

#define ZK_REQUIRE(cond, msg)                                                                     \
    do { if (!(cond)) throw zk::Error(std::string(msg)); } while (0)

// a number of a PIL program (types.rs:221-233): decimal or 0x hex, possibly negative, reduced mod p
inline u64 parse_pil_number(const std::string& s) {
    const bool neg = !s.empty() && s[0] == '-';
    size_t i = neg ? 1 : 0;
    const bool hex = s.size() > i + 1 && s[i] == '0' && (s[i + 1] == 'x' || s[i + 1] == 'X');
    unsigned __int128 v = 0;
    for (i += hex ? 2 : 0; i < s.size(); ++i) {
        const char c = s[i];
        const int d = c >= '0' && c <= '9' ? c - '0' : !hex ? -1 : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (d < 0) throw Error("bad PIL number " + s);
        v = (v * (hex ? 16 : 10) + d) % GL_P;
    }
    const u64 r = (u64)v;
    return neg && r ? GL_P - r : r;
}

// ---- device buffers ----
// Size-keyed free list in front of the driver's allocator (devmem.hip): a prover allocates the same
// multi-GB sections for every proof, and returning such buffers to the driver and asking for them again
// costs hundreds of ms and synchronises the device.  Reuse is ordered across streams: every host thread keeps the set of streams it has
// issued on (`on_stream`); pool_free records an event on the null stream and on each stream of the freeing thread,
// and pool_alloc makes the calling thread's current stream wait for the events of the block it hands out, so a
// block freed with kernels still in flight on stream A is never written early by stream B -- while provers running
// on different threads and streams never wait for each other.  With a single stream in use (the common case) no
// event is needed: reuse is stream ordered.
void* pool_alloc(size_t bytes, bool host_wait = false);   // host_wait: drain the previous users on the host (the block leaves the library)
void h2d_sync(void* d, const void* h, size_t n);            // copies of pooled buffers, ordered on the current stream and waited for
void d2h_sync(void* h, const void* d, size_t n);
void pool_free(void* p);
void pool_defer_begin();   // frees of this thread are collected until pool_defer_flush() stamps them with one set of events
void pool_defer_flush();
void pool_trim();  // everything cached goes back to the driver
// takes blocks of these sizes on a helper thread and parks them in the free list; until the future is ready an allocation
// that runs out of memory waits for the helper before it trims
std::future<void> pool_reserve_async(std::vector<size_t> sizes);
// registers `st` as a stream the library works on and makes it the calling thread's current stream (the one
// pool_alloc orders reuse against); returns st.  Every entry point that takes a stream goes through it.
hipStream_t on_stream(hipStream_t st);
hipStream_t cur_stream();
// Scope of one C-ABI call: a call from outside the library starts on the null stream, a call the prover makes on its own
// entry points inherits the prover's current stream; either way the caller's current stream is back when the call returns.
void set_device(int d);                // zk_init: the GPU of the process
void bind_device() noexcept;           // the calling thread onto the GPU zk_init selected (HIP's current device is per thread)
struct CallScope { hipStream_t saved; CallScope(); ~CallScope(); CallScope(const CallScope&) = delete; CallScope& operator=(const CallScope&) = delete; };
void forget_stream(hipStream_t st);  // call before destroying a registered stream, or when a side stream's work has been waited for
void on_side_stream(hipStream_t ss); // a helper stream inside one call (see devmem.hip); pairs with forget_stream

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) pool_free(p); }
    void reserve(size_t n) {  // grow-only workspace
        if (n <= bytes) return;
        if (p) { pool_free(p); p = nullptr; bytes = 0; }
        p = pool_alloc(n); bytes = n;
    }
    u64* u() const { return (u64*)p; }
    void release() { if (p) { pool_free(p); p = nullptr; bytes = 0; } }
};

// A device block that lives as long as the process: constant tables, built once per device.  Not the pool's: never recycled, and
// pool_trim() does not touch it.  The owner frees the block only when it is destroyed before it was published (an upload or a later
// table's construction threw); where it is kept for good it sits in an object that is never destroyed (`*new`), because a static
// destructor would give memory back after the HIP runtime's own teardown.
void* const_alloc(size_t bytes);
void const_free(void* p) noexcept;
struct DevConst {
    void* p = nullptr;
    DevConst() = default;
    explicit DevConst(size_t bytes) : p(const_alloc(bytes)) {}                           // filled by a kernel of the caller
    DevConst(const void* h, size_t bytes) : p(const_alloc(bytes)) {                      // filled from host memory, here
        const hipError_t e = bytes ? hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
        if (e != hipSuccess) { (void)hipGetLastError(); const_free(p); throw Error(std::string("uploading a constant table failed: ") + hipGetErrorString(e)); }
    }
    template <class T> explicit DevConst(const std::vector<T>& v) : DevConst(v.data(), v.size() * sizeof(T)) {}
    DevConst(DevConst&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevConst& operator=(DevConst&& o) noexcept { if (this != &o) { const_free(p); p = o.p; o.p = nullptr; } return *this; }
    ~DevConst() { const_free(p); }
    u64* u() const { return (u64*)p; }
};

// One C-ABI call that returns a status: the call's scope, and what it throws kept for zk_last_error()
template <class F>
int guard(F&& f) {
    CallScope scope;
    try { f(); return 0; }
    catch (const std::exception& e) { set_error(e.what()); return -1; }
    catch (...) { set_error("unknown error"); return -1; }
}

// ---- run-time compiled kernels (expr_jit.hip): what the code-object cache did so far in this process ----
struct JitStats { uint64_t compiled = 0, disk_hits = 0, mem_hits = 0, spawned = 0; double ms = 0; };   // spawned: compilations done by a helper process (of `compiled`)
JitStats jit_stats();
// the next compilations of this thread go to a helper process each (a setup compiling several step programs at once: hipRTC is serial inside one process)
void jit_prefer_spawn(bool on);

// ---- what both evaluators of a step program check (expr_jit.hip, expr_bytecode.hip) ----
// Rows are evaluated concurrently (one lane per row), the reference evaluates them in order inside a chunk
// (stark_gen.rs:752-783).  The two agree unless one row's lane reads a cell another row's lane writes: a write at row
// i and a read of an overlapping cell range at row i+next, in either order.  Reads a lane takes from its own earlier
// store are not recorded by either evaluator.
struct EvalAccess { uint32_t buf, id, dim; bool prime; };
inline bool eval_overlap(const EvalAccess& a, const EvalAccess& b) { return a.buf == b.buf && a.id < b.id + b.dim && b.id < a.id + a.dim; }
inline void check_row_hazards(const std::vector<EvalAccess>& mem_writes, const std::vector<EvalAccess>& mem_reads) {
    for (const EvalAccess& w : mem_writes) {
        for (const EvalAccess& r : mem_reads)
            ZK_REQUIRE(!(eval_overlap(w, r) && w.prime != r.prime), "eval program: a column is written at one row and read at the next row in the same step");
    }
}

// ---- the bytecode evaluator (expr_bytecode.hip): the same step program, assembled for one precompiled interpreter kernel ----
struct Bytecode;
void bytecode_free(Bytecode* b);
const char* bytecode_listing(const Bytecode* b);
// `ctx` is a zk_eval_ctx; the caller has checked the row range and made `st` the thread's current stream
void bytecode_run(Bytecode* b, const void* ctx, uint32_t nbits_domain, uint64_t next, uint64_t row0, uint64_t count, hipStream_t st);
struct ::zk_program* program_of_bytecode(Bytecode* b);   // expr_jit.hip owns zk_program: wraps b (and owns it from here on)
int eval_mode();                                       // the calling thread's ZK_EVAL_* (zk_eval_set_mode, initially $ZK_EVAL)

// ---- NTT (ntt.hip) ----
// natural-order batched NTT over a row-major [1<<nbits][n_pols] device matrix; dst != src.
// `tmp` must hold (1<<nbits)*n_pols words when the plan has more than one pass.
void ntt_dev(const u64* d_src, u64* d_dst, u64* d_tmp, uint32_t n_pols, uint32_t nbits, bool inverse, hipStream_t st);
// low-degree extension on the coset 49*<w_ext>: [1<<nbits][n_pols] -> [1<<nbits_ext][n_pols].
// tmp: (1<<nbits_ext)*n_pols words.
void lde_dev(const u64* d_src, u64* d_dst, u64* d_tmp, uint32_t n_pols, uint32_t nbits, uint32_t nbits_ext, hipStream_t st);
int ntt_num_passes(uint32_t nbits);

// ---- Poseidon / Merkle (poseidon.hip) ----
void poseidon_dev(const u64* d_in8, const u64* d_cap4, u64* d_out, int n_out, hipStream_t st);
void linearhash_rows_dev(const u64* d_rows, uint32_t width, uint64_t height, u64* d_digests, hipStream_t st);
uint64_t merkle_n_nodes(uint64_t height);
// nodes: merkle_n_nodes(height)*4 words, zero-filled by this call; leaves from [height][width] rows
void merkelize_dev(const u64* d_rows, uint32_t width, uint64_t height, u64* d_nodes, hipStream_t st);
// n paths: from leaf digest [n][4] and siblings [n][max_depth][4] (path q uses its first depth[q] levels) to the root each implies
void merkle_roots_from_paths_dev(const u64* d_leaves, const u64* d_paths, const uint32_t* d_depth, const u64* d_idx, uint32_t n, uint32_t max_depth,
                                 u64* d_roots, hipStream_t st);

// ---- device-resident transcript (poseidon.hip; transcript.rs:8-103) ----
size_t transcript_state_bytes();
std::string poseidon_tables_selfcheck();   // host only: the one-lane kernels' matrix-pipe tables and arithmetic against 128-bit arithmetic ("" = fine)
void transcript_init_dev(void* d_t, hipStream_t st);
void transcript_put_dev(void* d_t, const u64* d_src, uint64_t n, hipStream_t st);
void transcript_get_dev(void* d_t, u64* d_dst, uint32_t n_words, hipStream_t st);
void transcript_permutations_dev(void* d_t, uint32_t n, uint32_t nbits, u64* d_dst, hipStream_t st);
void transcript_put_get_dev(void* d_t, const u64* d_src, uint64_t n_put, u64* d_dst, uint32_t n_get, uint32_t bits, hipStream_t st);

// ---- prover glue (stark.hip) ----
const u64* ntt_w256_table(bool inverse);  // w_256^(+-e), e < 256, device pointer (ntt.hip)
struct EvalDescHost { const u64* buf; uint64_t width; uint64_t offset; uint32_t dim; uint32_t prime; };
void fri_fold_dev(const u64* d_pol, uint32_t pol_bits, uint32_t step_bits, const u64* d_special_x, u64 shift_inv, u64* d_out, hipStream_t st);
void fri_transpose_dev(const u64* d_pol, uint64_t n, uint32_t tbits, u64* d_out, hipStream_t st);
void x_table_dev(uint32_t nbits, u64 shift, u64* d_out, hipStream_t st);
void zh_inv_dev(uint32_t nbits, uint32_t extend_bits, u64* d_out, hipStream_t st);
void xdivxsub_dev(const u64* d_xi, u64 mulw, uint32_t nbits_ext, u64* d_out, hipStream_t st);
struct EvalDescKHost { const u64* buf; const u64* L; uint64_t width; uint64_t offset; uint32_t dim; uint32_t rshift; };   // L: weights per row; rows k << rshift
void lev_dev(const u64* d_xi, uint32_t nbits, bool prime, u64 shift, u64* d_out, u64* d_pow, u64* d_tmp2, hipStream_t st);
void lev_pow_dev(const u64* d_xi, uint32_t nbits, bool prime, u64 shift, u64* d_pow, hipStream_t st);
void lev_pow_multi_dev(const u64* d_xi, uint32_t nbits, uint32_t n_tables, const bool* prime, const u64* shift, u64* const* d_pow, hipStream_t st);
void xdivxsub2_dev(const u64* d_xi, u64 mulw0, u64 mulw1, uint32_t nbits_ext, u64* d_out0, u64* d_out1, hipStream_t st);
void evals_k_dev(const EvalDescKHost* descs, uint32_t n_ev, uint32_t nbits, u64* d_out, hipStream_t st);
void evals_dev(const EvalDescHost* descs, uint32_t n_ev, uint32_t nbits, uint32_t ext, const u64* d_LEv, const u64* d_LpEv, u64* d_out, hipStream_t st);
void pol_get_dev(const u64* d_buf, uint64_t width, uint64_t offset, uint32_t dim, uint64_t n, u64* d_out, hipStream_t st);
void pol_set_dev(u64* d_buf, uint64_t width, uint64_t offset, uint32_t dim, uint64_t n, const u64* d_in, hipStream_t st);
uint64_t h1h2_work_words(uint64_t n);
void calculate_h1h2_dev(const u64* d_f, const u64* d_t, uint64_t n, u64* d_h1, u64* d_h2, u64* d_work, u64** d_missing, hipStream_t st);
void calculate_z_dev(const u64* d_num, const u64* d_den, uint64_t n, u64* d_z, u64* d_work, u64* d_check, hipStream_t st);
// ---- BN128-field hashing (frhash.hip; reached through the field table of commit.h); digests = 4 raw (Montgomery, R = 2^256) limbs
void bn128_load_constants(const char* path);
std::string bn128_tables_selfcheck(const char* path);   // host only: the matrix-pipe tables (fr_mfma.hip.h) against the constants; "" or what is wrong
void bn128_poseidon_dev(const u64* d_inp, uint64_t n, uint32_t n_in, const u64* d_init, uint32_t n_out, u64* d_out, hipStream_t st);
uint64_t bn128_merkle_n_nodes(uint64_t height);
void bn128_linearhash_rows_dev(const u64* d_rows, uint32_t width, uint64_t height, u64* d_digests, hipStream_t st);
void bn128_merkelize_dev(const u64* d_rows, uint32_t width, uint64_t height, u64* d_nodes, hipStream_t st);
// the same over the BLS12-381 scalar field (verificationHashType "BLS12381")
void bls12381_load_constants(const char* path);
std::string bls12381_tables_selfcheck(const char* path);
void bls12381_poseidon_dev(const u64* d_inp, uint64_t n, uint32_t n_in, const u64* d_init, uint32_t n_out, u64* d_out, hipStream_t st);
uint64_t bls12381_merkle_n_nodes(uint64_t height);
void bls12381_linearhash_rows_dev(const u64* d_rows, uint32_t width, uint64_t height, u64* d_digests, hipStream_t st);
void bls12381_merkelize_dev(const u64* d_rows, uint32_t width, uint64_t height, u64* d_nodes, hipStream_t st);
// stark_verify (stark_verify.hip): 1 accepted, 0 rejected (`why` names the failed check); throws Error on malformed input
struct JVal;
int stark_verify_impl(const JVal& info, const JVal& prog, const JVal& ss, const u64 const_root[4], const char* zkin_json, std::string& why);
void qsplit_dev(const u64* d_qq1, uint32_t nbits, uint32_t q_dim, uint32_t q_deg, u64* d_qq2, hipStream_t st);

// ---- compressor12 exec (compressor12.hip): witness -> committed trace [n_rows][12]
struct C12Exec;
C12Exec* c12_exec_new(const char* exec_json, size_t len, uint64_t n_witness);
void c12_exec_free(C12Exec* e);
uint64_t c12_exec_levels(const C12Exec* e);
void c12_exec_dev(const C12Exec* e, const u64* d_witness, uint64_t n_witness, uint64_t n_rows, u64* d_cm, hipStream_t st);
// ---- compressor12 setup (c12_setup.hip): a Goldilocks R1CS -> .pil / .exec text and the [N][nConst] constant matrix
struct C12Setup;
C12Setup* c12_setup_new(const void* r1cs, size_t len, uint32_t force_n_bits);
void c12_setup_free(C12Setup* s);
void c12_setup_info(const C12Setup* s, uint64_t out[6]);   // n_bits, n_publics, n_used, n_const, gates, additions
void c12_setup_gates(const C12Setup* s, u64* out);         // gates x (sl, sr, so, qm, ql, qr, qo, qc)
std::string c12_setup_pil(const C12Setup* s);
std::string c12_setup_exec(const C12Setup* s);
void c12_setup_consts_dev(const C12Setup* s, u64* d_out, hipStream_t st);
// the 12 S columns of any [n_used][12] map (0 = no wire) into columns [col0, col0 + 12) of a [2^n_bits][n_const] matrix
void c12_sigma_dev(const u32* d_s_map, uint64_t n_used, uint32_t n_bits, uint32_t n_const, uint32_t col0, u64* d_out, hipStream_t st);
// (the curves -- multi-scalar sums, Groth16, pairings -- are declared in curve.h, for the four units that see it)

}  // namespace zk
