// C ABI of libzkgpu (include/zkgpu.h): thin extern "C" wrappers and host<->device staging for the host-pointer entry points.
// (Device memory, streams, error capture: devmem.hip.  Merkle trees and transcripts: commit.hip.)
#include "zk_internal.h"
#include "commit.h"
#include "curve.h"
#include "pil_check.h"
#include "r1cs_check.h"
#include "../../include/zkgpu.h"
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include <cstring>

namespace zk {
namespace {

std::mutex g_ws_mu;
// grow-only staging for the host-pointer API.  Never destroyed: a static DevBuf would go back to the pool from a static
// destructor, after the main thread's thread_local stream list is gone and possibly after the HIP runtime's own teardown
// (a process that still had a registered side stream at exit crashed there).
DevBuf &g_ws_a = *new DevBuf, &g_ws_b = *new DevBuf, &g_ws_c = *new DevBuf;

// synthetic words for benchmarks and size tests: word i = splitmix64(seed + i) folded below p (one conditional subtraction)
__global__ void fill_splitmix_kernel(u64* __restrict__ out, u64 n, u64 seed) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 z = seed + i + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; z ^= z >> 31;
    out[i] = z >= GL_P ? z - GL_P : z;
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zk_init(int device) {
    return guard([&] {
        int n = 0;
        ZK_HIP(hipGetDeviceCount(&n));
        ZK_REQUIRE(device >= 0 && device < n, "zk_init: no such device");
        ZK_HIP(hipSetDevice(device));
        set_device(device);                                  // ... and of every thread that calls into the library from now on
    });
}
const char* zk_last_error(void) { return last_error(); }
int zk_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
uint64_t zk_gl_modulus(void) { return GL_P; }
uint64_t zk_gl_root_of_unity(uint32_t k) { return k <= 32 ? gl::hroot(k) : 0; }

void* zk_dev_alloc(size_t bytes) {
    void* p = nullptr;
    // handed to the caller, who may write it on any stream: reuse is ordered on the host, not on the null stream of this call
    if (guard([&] { p = pool_alloc(bytes, /*host_wait=*/true); }) != 0) return nullptr;
    return p;
}
int zk_dev_free(void* p) { return guard([&] { pool_free(p); }); }
int zk_dev_trim(void) { return guard([&] { ZK_HIP(hipDeviceSynchronize()); pool_trim(); }); }
int zk_dev_upload(void* d, const void* h, size_t n) { return guard([&] { ZK_HIP(hipMemcpy(d, h, n, hipMemcpyHostToDevice)); }); }
int zk_dev_download(void* h, const void* d, size_t n) { return guard([&] { ZK_HIP(hipMemcpy(h, d, n, hipMemcpyDeviceToHost)); }); }
int zk_dev_sync(void) { return guard([&] { ZK_HIP(hipDeviceSynchronize()); }); }
void* zk_stream_new(void) {
    hipStream_t st = nullptr;
    if (guard([&] { ZK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }) != 0) return nullptr;
    return st;
}
int zk_stream_sync(void* stream) { return guard([&] { ZK_HIP(hipStreamSynchronize((hipStream_t)stream)); }); }
int zk_stream_free(void* stream) {
    return guard([&] {
        if (!stream) return;
        ZK_HIP(hipStreamSynchronize((hipStream_t)stream));
        forget_stream((hipStream_t)stream);
        ZK_HIP(hipStreamDestroy((hipStream_t)stream));
    });
}
int zk_dev_fill_splitmix(uint64_t* d, uint64_t n_words, uint64_t seed, void* stream) {
    return guard([&] {
        if (!n_words) return;
        ZK_REQUIRE(d != nullptr, "zk_dev_fill_splitmix: null buffer");
        ZK_REQUIRE((n_words + 255) / 256 < (1ull << 31), "zk_dev_fill_splitmix: too many words for one launch");
        hipLaunchKernelGGL(fill_splitmix_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, on_stream((hipStream_t)stream), (u64*)d, n_words, seed);
        ZK_HIP(hipGetLastError());
    });
}
int zk_dev_memset(void* d, int value, size_t n) { return guard([&] { if (n) ZK_HIP(hipMemset(d, value, n)); }); }

int zk_gl_ntt_passes(uint32_t nbits) { return ntt_num_passes(nbits); }

int zk_gl_ntt_dev(const uint64_t* d_src, uint64_t* d_dst, uint64_t* d_tmp, uint32_t n_pols, uint32_t nbits,
                  int inverse, void* stream) {
    return guard([&] {
        ZK_REQUIRE(nbits <= 32, "zk_gl_ntt: nbits > 32");
        ZK_REQUIRE(d_tmp != nullptr || ntt_num_passes(nbits) == 1 || n_pols == 0, "zk_gl_ntt_dev: d_tmp required");
        ntt_dev((const u64*)d_src, (u64*)d_dst, (u64*)d_tmp, n_pols, nbits, inverse != 0, on_stream((hipStream_t)stream));
    });
}

int zk_gl_lde_dev(const uint64_t* d_src, uint32_t n_pols, uint32_t nbits, uint64_t* d_dst, uint64_t* d_tmp,
                  uint32_t nbits_ext, void* stream) {
    return guard([&] {
        ZK_REQUIRE(d_tmp != nullptr || n_pols == 0, "zk_gl_lde_dev: d_tmp required");
        lde_dev((const u64*)d_src, (u64*)d_dst, (u64*)d_tmp, n_pols, nbits, nbits_ext, on_stream((hipStream_t)stream));
    });
}

int zk_gl_ntt(const uint64_t* src, uint64_t* dst, uint32_t n_pols, uint32_t nbits, int inverse) {
    return guard([&] {
        ZK_REQUIRE(nbits <= 32, "zk_gl_ntt: nbits > 32");
        if (n_pols == 0) return;
        ZK_REQUIRE(src && dst && src != dst, "zk_gl_ntt: bad buffers (dst may not alias src)");
        std::lock_guard<std::mutex> lk(g_ws_mu);
        const size_t bytes = ((size_t)1 << nbits) * n_pols * sizeof(u64);
        g_ws_a.reserve(bytes); g_ws_b.reserve(bytes); g_ws_c.reserve(bytes);
        ZK_HIP(hipMemcpy(g_ws_a.p, src, bytes, hipMemcpyHostToDevice));
        ntt_dev(g_ws_a.u(), g_ws_b.u(), g_ws_c.u(), n_pols, nbits, inverse != 0, nullptr);
        ZK_HIP(hipMemcpy(dst, g_ws_b.p, bytes, hipMemcpyDeviceToHost));
    });
}

int zk_gl_lde(const uint64_t* src, uint32_t n_pols, uint32_t nbits, uint64_t* dst, uint32_t nbits_ext) {
    return guard([&] {
        ZK_REQUIRE(nbits_ext <= 32 && nbits <= nbits_ext, "zk_gl_lde: need nbits <= nbits_ext <= 32");
        if (n_pols == 0) return;  // fft_p.rs:262-264: empty source is a no-op
        ZK_REQUIRE(src && dst, "zk_gl_lde: null buffer");
        std::lock_guard<std::mutex> lk(g_ws_mu);
        const size_t in_bytes = ((size_t)1 << nbits) * n_pols * sizeof(u64);
        const size_t out_bytes = ((size_t)1 << nbits_ext) * n_pols * sizeof(u64);
        g_ws_a.reserve(in_bytes); g_ws_b.reserve(out_bytes); g_ws_c.reserve(out_bytes);
        ZK_HIP(hipMemcpy(g_ws_a.p, src, in_bytes, hipMemcpyHostToDevice));
        lde_dev(g_ws_a.u(), g_ws_b.u(), g_ws_c.u(), n_pols, nbits, nbits_ext, nullptr);
        ZK_HIP(hipMemcpy(dst, g_ws_b.p, out_bytes, hipMemcpyDeviceToHost));
    });
}

int zk_gl_poseidon_selfcheck(void) {                                   // host arithmetic only: no CallScope, no device
    try {
        const std::string why = poseidon_tables_selfcheck();
        if (why.empty()) return 0;
        set_error(why);
    } catch (const std::exception& e) { set_error(e.what()); }
    return -1;
}

int zk_gl_poseidon(const uint64_t in[8], const uint64_t cap[4], uint64_t* out, uint32_t n_out) {
    return guard([&] {
        // poseidon_opt.rs:81-96 rejects wrong input/capacity lengths; with fixed-size C arrays the
        // remaining argument error is the output count.
        ZK_REQUIRE(in && cap && out, "zk_gl_poseidon: null buffer");
        ZK_REQUIRE(n_out >= 1 && n_out <= 12, "zk_gl_poseidon: n_out must be 1..12");
        std::lock_guard<std::mutex> lk(g_ws_mu);
        g_ws_a.reserve(24 * sizeof(u64));
        u64 h[12];
        memcpy(h, in, 64); memcpy(h + 8, cap, 32);
        ZK_HIP(hipMemcpy(g_ws_a.p, h, 96, hipMemcpyHostToDevice));
        poseidon_dev(g_ws_a.u(), g_ws_a.u() + 8, g_ws_a.u() + 12, (int)n_out, nullptr);
        ZK_HIP(hipMemcpy(out, g_ws_a.u() + 12, n_out * sizeof(u64), hipMemcpyDeviceToHost));
    });
}

int zk_gl_linearhash_rows_dev(const uint64_t* d_rows, uint32_t width, uint64_t height, uint64_t* d_digests, void* stream) {
    return guard([&] { linearhash_rows_dev((const u64*)d_rows, width, height, (u64*)d_digests, on_stream((hipStream_t)stream)); });
}

int zk_gl_linearhash(const uint64_t* v, size_t n, uint64_t out[4]) {
    return guard([&] {
        ZK_REQUIRE(out && (v || n == 0), "zk_gl_linearhash: null buffer");
        ZK_REQUIRE(n < (1ull << 32), "zk_gl_linearhash: row too wide");
        std::lock_guard<std::mutex> lk(g_ws_mu);
        g_ws_a.reserve((n + 8) * sizeof(u64));
        if (n) ZK_HIP(hipMemcpy(g_ws_a.p, v, n * sizeof(u64), hipMemcpyHostToDevice));
        u64* d_out = g_ws_a.u() + n;
        linearhash_rows_dev(g_ws_a.u(), (uint32_t)n, 1, d_out, nullptr);
        ZK_HIP(hipMemcpy(out, d_out, 32, hipMemcpyDeviceToHost));
    });
}

// ---- MerkleTreeGL / TranscriptGL (commit.hip) --------------------------------------------------------
uint64_t zk_merkle_n_nodes(uint64_t height) { return height ? merkle_n_nodes(height) : 0; }

zk_merkle_t* zk_gl_merkelize(const uint64_t* buff, uint32_t width, uint64_t height) {
    std::unique_ptr<zk_merkle> t;
    if (guard([&] {
            ZK_REQUIRE((buff || width == 0) && height >= 1, "zk_gl_merkelize: empty matrix");
            t.reset(new zk_merkle); t->build_host((const u64*)buff, width, height);
        }) != 0) return nullptr;
    return t.release();
}
zk_merkle_t* zk_gl_merkelize_dev(const uint64_t* d_buff, uint32_t width, uint64_t height, void* stream) {
    std::unique_ptr<zk_merkle> t;
    if (guard([&] {
            ZK_REQUIRE((d_buff || width == 0) && height >= 1, "zk_gl_merkelize_dev: empty matrix");
            t.reset(new zk_merkle); t->build_dev((const u64*)d_buff, width, height, (hipStream_t)stream);
        }) != 0) return nullptr;
    return t.release();
}
int zk_merkle_root(const zk_merkle_t* t, uint64_t out[4]) { return guard([&] { ZK_REQUIRE(t && out, "zk_merkle_root: null"); t->root((u64*)out); }); }
int zk_merkle_nodes(const zk_merkle_t* t, uint64_t* out) { return guard([&] { ZK_REQUIRE(t && out, "zk_merkle_nodes: null"); t->nodes_host((u64*)out); }); }
int zk_merkle_elements(const zk_merkle_t* t, uint64_t* out) { return guard([&] { ZK_REQUIRE(t && out, "zk_merkle_elements: null"); t->elements_host((u64*)out); }); }
uint32_t zk_merkle_depth(const zk_merkle_t* t) { return t ? t->depth : 0; }
int zk_merkle_group_proof(const zk_merkle_t* t, uint64_t idx, uint64_t* row_out, uint64_t* path_out) {
    return guard([&] {
        ZK_REQUIRE(t && row_out && (path_out || t->depth == 0), "zk_merkle_group_proof: null");
        t->group_proof(idx, (u64*)row_out, (u64*)path_out);
    });
}
int zk_merkle_group_proofs(const zk_merkle_t* t, const uint64_t* idx, uint32_t n, uint64_t* rows_out, uint64_t* paths_out) {
    return guard([&] {
        ZK_REQUIRE(t && (n == 0 || (idx && rows_out && (paths_out || t->depth == 0))), "zk_merkle_group_proofs: null");
        t->group_proofs((const u64*)idx, n, (u64*)rows_out, (u64*)paths_out);
    });
}
const uint64_t* zk_merkle_elements_dev(const zk_merkle_t* t) { return t ? (const uint64_t*)t->d_elements : nullptr; }
const uint64_t* zk_merkle_nodes_dev(const zk_merkle_t* t) { return t ? (const uint64_t*)t->nodes.p : nullptr; }
int zk_merkle_free(zk_merkle_t* t) { delete t; return 0; }

zk_transcript_t* zk_transcript_new(void) {
    zk_transcript_t* t = nullptr;
    if (guard([&] { t = new zk_transcript; }) != 0) return nullptr;
    return t;
}
int zk_transcript_put_dev(zk_transcript_t* t, const uint64_t* d_src, size_t n, void* stream) {
    return guard([&] { ZK_REQUIRE(t, "transcript: null"); t->put_dev((const u64*)d_src, n, (hipStream_t)stream); });
}
int zk_transcript_put(zk_transcript_t* t, const uint64_t* src, size_t n) {
    return guard([&] { ZK_REQUIRE(t && (src || n == 0), "transcript: null"); t->put_words((const u64*)src, n); });
}
int zk_transcript_get_field_dev(zk_transcript_t* t, uint64_t* d_out3, void* stream) {
    return guard([&] { ZK_REQUIRE(t && d_out3, "transcript: null"); t->get_dev((u64*)d_out3, 3, (hipStream_t)stream); });
}
int zk_transcript_get_field(zk_transcript_t* t, uint64_t out[3]) { return guard([&] { ZK_REQUIRE(t && out, "transcript: null"); t->get((u64*)out, 3); }); }
int zk_transcript_get_fields1(zk_transcript_t* t, uint64_t* out) { return guard([&] { ZK_REQUIRE(t && out, "transcript: null"); t->get((u64*)out, 1); }); }
int zk_transcript_get_permutations(zk_transcript_t* t, uint32_t n, uint32_t nbits, uint64_t* out) {
    return guard([&] { ZK_REQUIRE(t && out, "transcript: null"); t->get_permutations(n, nbits, (u64*)out); });
}
int zk_transcript_free(zk_transcript_t* t) { delete t; return 0; }

// ---- FRI / stark_gen glue ----------------------------------------------------------------------
int zk_fri_fold_dev(const uint64_t* d_pol, uint32_t pol_bits, uint32_t step_bits, const uint64_t* d_special_x,
                    uint64_t shift_inv, uint64_t* d_out, void* stream) {
    return guard([&] { fri_fold_dev((const u64*)d_pol, pol_bits, step_bits, (const u64*)d_special_x, shift_inv, (u64*)d_out, on_stream((hipStream_t)stream)); });
}
int zk_fri_transpose_dev(const uint64_t* d_pol, uint64_t n, uint32_t tbits, uint64_t* d_out, void* stream) {
    return guard([&] { fri_transpose_dev((const u64*)d_pol, n, tbits, (u64*)d_out, on_stream((hipStream_t)stream)); });
}
int zk_stark_x_table_dev(uint32_t nbits, uint64_t shift, uint64_t* d_out, void* stream) {
    return guard([&] { ZK_REQUIRE(nbits <= 32, "x_table: nbits > 32"); x_table_dev(nbits, shift, (u64*)d_out, on_stream((hipStream_t)stream)); });
}
int zk_stark_zh_inv_dev(uint32_t nbits, uint32_t extend_bits, uint64_t* d_out, void* stream) {
    return guard([&] { ZK_REQUIRE(extend_bits <= 16, "zh_inv: extend_bits > 16"); zh_inv_dev(nbits, extend_bits, (u64*)d_out, on_stream((hipStream_t)stream)); });
}
int zk_stark_xdivxsub_dev(const uint64_t* d_xi, uint64_t mulw, uint32_t nbits_ext, uint64_t* d_out, void* stream) {
    return guard([&] { ZK_REQUIRE(nbits_ext <= 32, "xdivxsub: nbits_ext > 32"); xdivxsub_dev((const u64*)d_xi, mulw, nbits_ext, (u64*)d_out, on_stream((hipStream_t)stream)); });
}
int zk_stark_lev_dev(const uint64_t* d_xi, uint32_t nbits, int prime, uint64_t* d_out, uint64_t* d_tmp, uint64_t* d_tmp2, void* stream) {
    return guard([&] { lev_dev((const u64*)d_xi, nbits, prime != 0, 49, (u64*)d_out, (u64*)d_tmp, (u64*)d_tmp2, on_stream((hipStream_t)stream)); });
}
int zk_stark_evals_dev(const zk_eval_desc* descs, uint32_t n_ev, uint32_t nbits, uint32_t ext, const uint64_t* d_LEv,
                       const uint64_t* d_LpEv, uint64_t* d_out, void* stream) {
    return guard([&] {
        static_assert(sizeof(zk_eval_desc) == sizeof(EvalDescHost), "eval descriptor layout");
        evals_dev((const EvalDescHost*)descs, n_ev, nbits, ext, (const u64*)d_LEv, (const u64*)d_LpEv, (u64*)d_out, on_stream((hipStream_t)stream));
    });
}
int zk_stark_qsplit_dev(const uint64_t* d_qq1, uint32_t nbits, uint32_t q_dim, uint32_t q_deg, uint64_t* d_qq2, void* stream) {
    return guard([&] { qsplit_dev((const u64*)d_qq1, nbits, q_dim, q_deg, (u64*)d_qq2, on_stream((hipStream_t)stream)); });
}

// ---- the curves (curve.h): one function per contract, taking the curve, the group and the sizes from the table; the exported names are
// stamped below as one-line calls ----
static int msm_host(CurveId id, Group g, const void* bases, const void* scalars, uint64_t n, void* out, int* is_infinity) {
    return guard([&] {
        ZK_REQUIRE(out && is_infinity, "msm: null output");
        ZK_REQUIRE(n == 0 || (bases && scalars), "msm: null input");
        const size_t pb = curve(id).point_bytes(g);
        if (n == 0) { memset(out, 0, pb); *is_infinity = 1; return; }  // empty sum
        DevBuf db, ds, dout;
        db.reserve(n * pb); ds.reserve(n * 32); dout.reserve(pb + 4);
        ZK_HIP(hipMemcpy(db.p, bases, n * pb, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(ds.p, scalars, n * 32, hipMemcpyHostToDevice));
        curve(id).group(g).msm_dev(db.p, ds.p, n, dout.p, nullptr);
        std::vector<uint32_t> h(pb / 4 + 1);                           // the point and the flag word
        ZK_HIP(hipStreamSynchronize(nullptr));
        ZK_HIP(hipMemcpy(h.data(), dout.p, pb + 4, hipMemcpyDeviceToHost));
        memcpy(out, h.data(), pb);
        *is_infinity = (int)h[pb / 4];
    });
}
static int msm_device(CurveId id, Group g, const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, void* stream) {
    return guard([&] { curve(id).group(g).msm_dev(d_bases, d_scalars, n, d_out, on_stream((hipStream_t)stream)); });
}
static int mul_generator(CurveId id, Group g, bool full_width, const uint64_t* d_k, uint64_t n, void* d_bases, void* stream) {
    return guard([&] {
        const GroupOps& o = curve(id).group(g);
        if (full_width) ZK_REQUIRE((d_k && d_bases) || n == 0, "mul_generator: null argument");
        (full_width ? o.mul_generator_fr_dev : o.mul_generator_dev)((const u64*)d_k, n, d_bases, on_stream((hipStream_t)stream));
    });
}
static int msm_table_build(CurveId id, Group g, const void* d_bases, uint64_t table_n, void* d_table, void* stream) {
    return guard([&] { ZK_REQUIRE(d_bases && d_table, "msm table: null argument"); curve(id).group(g).fixed_prepare_dev(d_bases, table_n, d_table, on_stream((hipStream_t)stream)); });
}
static int msm_table(CurveId id, Group g, const void* d_table, uint64_t table_n, uint64_t offset, const void* d_scalars, uint64_t n, void* d_out, void* stream) {
    return guard([&] { ZK_REQUIRE(d_table && d_scalars && d_out, "msm table: null argument"); curve(id).group(g).fixed_dev(d_table, table_n, offset, d_scalars, n, d_out, on_stream((hipStream_t)stream)); });
}
static int fr_ntt_device(CurveId id, uint64_t* d, uint32_t log_n, int inverse, int coset, void* stream) {
    return guard([&] { ZK_REQUIRE(d, "fr ntt: null data"); curve(id).groth16().fr_ntt_dev((u64*)d, (int)log_n, inverse != 0, coset != 0, on_stream((hipStream_t)stream)); });
}
static int fr_ntt_host(CurveId id, uint64_t* data, uint32_t log_n, int inverse, int coset) {
    return guard([&] {
        ZK_REQUIRE(data, "fr ntt: null data");
        ZK_REQUIRE(log_n <= 32, "fr ntt: domain too large");
        const size_t bytes = ((size_t)32) << log_n;
        DevBuf d; d.reserve(bytes);
        ZK_HIP(hipMemcpy(d.p, data, bytes, hipMemcpyHostToDevice));
        curve(id).groth16().fr_ntt_dev((u64*)d.p, (int)log_n, inverse != 0, coset != 0, nullptr);
        ZK_HIP(hipStreamSynchronize(nullptr));
        ZK_HIP(hipMemcpy(data, d.p, bytes, hipMemcpyDeviceToHost));
    });
}
static int fr_quotient(CurveId id, uint64_t* a, const uint64_t* b, const uint64_t* c, uint32_t log_n, void* stream) {
    return guard([&] { ZK_REQUIRE(a && b && c, "fr quotient: null data"); curve(id).groth16().fr_quotient_dev((u64*)a, (const u64*)b, (const u64*)c, (int)log_n, on_stream((hipStream_t)stream)); });
}
static int fq_convert(CurveId id, void* d, uint64_t n, int to_mont, void* stream) {
    return guard([&] {
        ZK_REQUIRE(d || n == 0, "fq convert: null data");
        const MsmOps& o = curve(id).msm();
        (to_mont ? o.fq_canon_to_mont_dev : o.fq_mont_to_canon_dev)(d, n, on_stream((hipStream_t)stream));
    });
}
static int pairing_device(CurveId id, const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream) {
    return guard([&] {
        ZK_REQUIRE(n == 0 || (d_g1 && d_g2 && d_gt), "pairing: null argument");
        pairing_dev(curve(id), d_g1, d_g2, n, d_gt, with_final_exp, on_stream((hipStream_t)stream));
    });
}
static int pairing_host(CurveId id, const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp) {
    return guard([&] {
        ZK_REQUIRE(n == 0 || (g1 && g2 && gt_out), "pairing: null argument");
        if (n == 0) return;
        const Curve& cv = curve(id);
        DevBuf d1, d2, dg;
        d1.reserve(n * cv.point_bytes(G1)); d2.reserve(n * cv.point_bytes(G2)); dg.reserve(n * cv.gt_bytes());
        h2d_sync(d1.p, g1, n * cv.point_bytes(G1)); h2d_sync(d2.p, g2, n * cv.point_bytes(G2));
        pairing_dev(cv, d1.p, d2.p, n, dg.p, with_final_exp, cur_stream());
        d2h_sync(gt_out, dg.p, n * cv.gt_bytes());
    });
}
static int pairing_product_device(CurveId id, const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream) {
    return guard([&] {
        ZK_REQUIRE(d_gt && (n == 0 || (d_g1 && d_g2)), "pairing product: null argument");
        pairing_product_dev(curve(id), d_g1, d_g2, n, d_gt, with_final_exp, on_stream((hipStream_t)stream));
    });
}
static int pairing_product_host(CurveId id, const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp) {
    return guard([&] {
        ZK_REQUIRE(gt_out && (n == 0 || (g1 && g2)), "pairing product: null argument");
        const Curve& cv = curve(id);
        DevBuf d1, d2, dg;
        d1.reserve(n * cv.point_bytes(G1) + 4); d2.reserve(n * cv.point_bytes(G2) + 4); dg.reserve(cv.gt_bytes());
        if (n) { h2d_sync(d1.p, g1, n * cv.point_bytes(G1)); h2d_sync(d2.p, g2, n * cv.point_bytes(G2)); }
        pairing_product_dev(cv, d1.p, d2.p, n, dg.p, with_final_exp, cur_stream());
        d2h_sync(gt_out, dg.p, cv.gt_bytes());
    });
}
static int points_check_device(CurveId id, int group, const void* d_points, uint64_t n, int plain, uint64_t* d_out, void* stream) {
    return guard([&] {
        ZK_REQUIRE(group == 1 || group == 2, "points check: group must be 1 or 2");
        ZK_REQUIRE(d_out && (d_points || n == 0), "points check: null argument");
        const Group g = group == 1 ? G1 : G2;
        curve(id).pairing().points_check[g](d_points, curve(id).point_words(g), n, plain != 0, 0, (u64*)d_out, on_stream((hipStream_t)stream));
    });
}
static int points_check_host(CurveId id, int group, const void* points, uint64_t n, int plain, uint64_t* out) {
    return guard([&] {
        ZK_REQUIRE(group == 1 || group == 2, "points check: group must be 1 or 2");
        ZK_REQUIRE(out && (points || n == 0), "points check: null argument");
        const Curve& cv = curve(id);
        const Group g = group == 1 ? G1 : G2;
        DevBuf d, r;
        d.reserve(n * cv.point_bytes(g) + 4); r.reserve(64);
        if (n) h2d_sync(d.p, points, n * cv.point_bytes(g));
        cv.pairing().points_check[g](d.p, cv.point_words(g), n, plain != 0, 0, r.u(), cur_stream());
        d2h_sync(out, r.p, 64);
    });
}
#define ZK_GROUP_API(GN, NAME, ID, G)                                                                                                         \
    int zk_msm_##GN##_##NAME(const void* bases, const void* scalars, uint64_t n, void* out, int* is_infinity) { return msm_host(ID, G, bases, scalars, n, out, is_infinity); } \
    int zk_msm_##GN##_##NAME##_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, void* stream) { return msm_device(ID, G, d_bases, d_scalars, n, d_out, stream); } \
    int zk_##GN##_##NAME##_mul_generator_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream) { return mul_generator(ID, G, false, d_k, n, d_bases, stream); } \
    int zk_##GN##_##NAME##_mul_generator_fr_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream) { return mul_generator(ID, G, true, d_k, n, d_bases, stream); } \
    size_t zk_msm_##GN##_##NAME##_table_bytes(uint64_t table_n) { return curve(ID).group(G).fixed_table_bytes(table_n); }                     \
    int zk_msm_##GN##_##NAME##_table_build_dev(const void* d_bases, uint64_t table_n, void* d_table, void* stream) { return msm_table_build(ID, G, d_bases, table_n, d_table, stream); } \
    int zk_msm_##GN##_##NAME##_table_dev(const void* d_table, uint64_t table_n, uint64_t offset, const void* d_scalars, uint64_t n, void* d_out, void* stream) { \
        return msm_table(ID, G, d_table, table_n, offset, d_scalars, n, d_out, stream);                                                       \
    }
#define ZK_CURVE_API(NAME, ID)                                                                                                                \
    ZK_GROUP_API(g1, NAME, ID, G1)                                                                                                            \
    ZK_GROUP_API(g2, NAME, ID, G2)                                                                                                            \
    int zk_fr_##NAME##_ntt_dev(uint64_t* d, uint32_t log_n, int inverse, int coset, void* stream) { return fr_ntt_device(ID, d, log_n, inverse, coset, stream); } \
    int zk_fr_##NAME##_ntt(uint64_t* data, uint32_t log_n, int inverse, int coset) { return fr_ntt_host(ID, data, log_n, inverse, coset); }   \
    int zk_fr_##NAME##_quotient_dev(uint64_t* a, const uint64_t* b, const uint64_t* c, uint32_t log_n, void* stream) { return fr_quotient(ID, a, b, c, log_n, stream); } \
    int zk_fq_##NAME##_convert_dev(void* d, uint64_t n, int to_mont, void* stream) { return fq_convert(ID, d, n, to_mont, stream); }          \
    int zk_pairing_##NAME##_dev(const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream) { return pairing_device(ID, d_g1, d_g2, n, d_gt, with_final_exp, stream); } \
    int zk_pairing_##NAME(const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp) { return pairing_host(ID, g1, g2, n, gt_out, with_final_exp); } \
    int zk_pairing_product_##NAME##_dev(const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream) { return pairing_product_device(ID, d_g1, d_g2, n, d_gt, with_final_exp, stream); } \
    int zk_pairing_product_##NAME(const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp) { return pairing_product_host(ID, g1, g2, n, gt_out, with_final_exp); } \
    int zk_points_check_##NAME##_dev(int group, const void* d_points, uint64_t n, int plain, uint64_t* d_out, void* stream) { return points_check_device(ID, group, d_points, n, plain, d_out, stream); } \
    int zk_points_check_##NAME(int group, const void* points, uint64_t n, int plain, uint64_t* out) { return points_check_host(ID, group, points, n, plain, out); }
ZK_CURVE_API(bn254, CURVE_BN254)
ZK_CURVE_API(bls12_381, CURVE_BLS12_381)
#undef ZK_CURVE_API
#undef ZK_GROUP_API

// ---- scalar-field hashing (verificationHashType "BN128" / "BLS12381"): two name families over one implementation (commit.hip) ----
// one permutation / one row from host buffers, on the null stream
static void fr_poseidon(const FrField& F, const uint64_t* inp, uint32_t n_in, const uint64_t* init_state, uint32_t n_out, uint64_t* out) {
    ZK_REQUIRE(inp && init_state && out, "poseidon: null buffer");
    ZK_REQUIRE(n_in >= 1 && n_in <= 16, "Wrong inputs length");
    on_stream(nullptr);
    DevBuf d_in, d_init, d_out;
    d_in.reserve(n_in * 32); d_init.reserve(32); d_out.reserve(17 * 32);
    ZK_HIP(hipMemcpy(d_in.p, inp, n_in * 32, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(d_init.p, init_state, 32, hipMemcpyHostToDevice));
    F.poseidon_dev(d_in.u(), 1, n_in, d_init.u(), n_out, d_out.u(), nullptr);
    ZK_HIP(hipStreamSynchronize(nullptr));
    ZK_HIP(hipMemcpy(out, d_out.p, n_out * 32, hipMemcpyDeviceToHost));
}
static void fr_linearhash(const FrField& F, const uint64_t* v, size_t n, uint64_t* out) {
    ZK_REQUIRE(out && (v || n == 0), "linearhash: null buffer");
    on_stream(nullptr);
    DevBuf d_v, d_o; d_v.reserve(n * 8 + 8); d_o.reserve(32);
    if (n) ZK_HIP(hipMemcpy(d_v.p, v, n * 8, hipMemcpyHostToDevice));
    ZK_HIP(hipMemset(d_o.p, 0, 32));
    F.linearhash_rows_dev(d_v.u(), (uint32_t)n, 1, d_o.u(), nullptr);
    ZK_HIP(hipStreamSynchronize(nullptr));
    ZK_HIP(hipMemcpy(out, d_o.p, 32, hipMemcpyDeviceToHost));
}
#define ZK_FRHASH_CAPI(P, F)                                                                                            \
    int zk_##P##_load_constants(const char* path) { return guard([&] { ZK_REQUIRE(path, "null path"); F.load(path); }); } \
    int zk_##P##_poseidon_selfcheck(const char* path) {                  /* host arithmetic only: no CallScope, no device */ \
        try {                                                                                                           \
            if (!path) { set_error("null path"); return -1; }                                                           \
            const std::string why = F.selfcheck(path);                                                                  \
            if (why.empty()) return 0;                                                                                  \
            set_error(why);                                                                                             \
        } catch (const std::exception& e) { set_error(e.what()); }                                                      \
        return -1;                                                                                                      \
    }                                                                                                                   \
    int zk_##P##_poseidon(const uint64_t* inp, uint32_t n_in, const uint64_t init_state[4], uint32_t n_out, uint64_t* out) { \
        return guard([&] { fr_poseidon(F, inp, n_in, init_state, n_out, out); });                                       \
    }                                                                                                                   \
    int zk_##P##_poseidon_dev(const uint64_t* d_inp, uint64_t n, uint32_t n_in, const uint64_t* d_init_state, uint32_t n_out, \
                              uint64_t* d_out, void* stream) {                                                          \
        return guard([&] { F.poseidon_dev((const u64*)d_inp, n, n_in, (const u64*)d_init_state, n_out, (u64*)d_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                   \
    int zk_##P##_linearhash(const uint64_t* v, size_t n, uint64_t out[4]) { return guard([&] { fr_linearhash(F, v, n, out); }); } \
    uint64_t zk_##P##_merkle_n_nodes(uint64_t height) { return height ? F.n_nodes(height) : 0; }                          \
    static zk_##P##_merkle_t* P##_merkelize(const uint64_t* buff, bool on_device, uint32_t width, uint64_t height, void* stream) { \
        std::unique_ptr<zk_##P##_merkle> t;                                                                             \
        if (guard([&] {                                                                                                 \
                ZK_REQUIRE(height >= 1, "merkelize: height must be >= 1");                                              \
                ZK_REQUIRE(buff || width == 0, "merkelize: null buffer");                                               \
                t.reset(new zk_##P##_merkle);                                                                           \
                if (on_device) t->build_dev((const u64*)buff, width, height, (hipStream_t)stream); else t->build_host((const u64*)buff, width, height); \
            }) != 0) return nullptr;                                                                                    \
        return t.release();                                                                                             \
    }                                                                                                                   \
    zk_##P##_merkle_t* zk_##P##_merkelize(const uint64_t* buff, uint32_t width, uint64_t height) { return P##_merkelize(buff, false, width, height, nullptr); } \
    zk_##P##_merkle_t* zk_##P##_merkelize_dev(const uint64_t* d_buff, uint32_t width, uint64_t height, void* stream) { return P##_merkelize(d_buff, true, width, height, stream); } \
    int zk_##P##_merkle_root(const zk_##P##_merkle_t* t, uint64_t out[4]) { return guard([&] { ZK_REQUIRE(t && out, "null argument"); t->root((u64*)out); }); } \
    int zk_##P##_merkle_nodes(const zk_##P##_merkle_t* t, uint64_t* out) { return guard([&] { ZK_REQUIRE(t && out, "null argument"); t->nodes_host((u64*)out); }); } \
    uint32_t zk_##P##_merkle_depth(const zk_##P##_merkle_t* t) { return t ? t->depth : 0; }                               \
    int zk_##P##_merkle_group_proof(const zk_##P##_merkle_t* t, uint64_t idx, uint64_t* row_out, uint64_t* path_out) {    \
        return guard([&] { ZK_REQUIRE(t && row_out && path_out, "null argument"); t->group_proof(idx, (u64*)row_out, (u64*)path_out); }); \
    }                                                                                                                   \
    int zk_##P##_merkle_group_proofs(const zk_##P##_merkle_t* t, const uint64_t* idx, uint32_t n, uint64_t* rows_out,     \
                                     uint64_t* paths_out) {                                                              \
        return guard([&] { ZK_REQUIRE(t && (n == 0 || (idx && rows_out && paths_out)), "null argument"); t->group_proofs((const u64*)idx, n, (u64*)rows_out, (u64*)paths_out); }); \
    }                                                                                                                   \
    int zk_##P##_merkle_free(zk_##P##_merkle_t* t) { return guard([&] { delete t; }); }                                   \
    zk_##P##_transcript_t* zk_##P##_transcript_new(void) {                                                               \
        zk_##P##_transcript* t = nullptr;                                                                               \
        if (guard([&] { t = new zk_##P##_transcript; }) != 0) return nullptr;                                            \
        return t;                                                                                                       \
    }                                                                                                                   \
    int zk_##P##_transcript_put(zk_##P##_transcript_t* t, const uint64_t* e, size_t n) {   /* transcript_bn128.rs:90-101: a Goldilocks value or a digest */ \
        return guard([&] {                                                                                              \
            ZK_REQUIRE(t && e, "null argument");                                                                        \
            if (n == 1) t->put_words((const u64*)e, 1); else if (n == 4) t->put_digest((const u64*)e);                  \
            else throw Error("Invalid elements as inputs to transcript");                                               \
        });                                                                                                             \
    }                                                                                                                   \
    int zk_##P##_transcript_get_fields1(zk_##P##_transcript_t* t, uint64_t* out) { return guard([&] { ZK_REQUIRE(t && out, "null argument"); t->get((u64*)out, 1); }); } \
    int zk_##P##_transcript_get_field(zk_##P##_transcript_t* t, uint64_t out[3]) { return guard([&] { ZK_REQUIRE(t && out, "null argument"); t->get((u64*)out, 3); }); } \
    int zk_##P##_transcript_get_permutations(zk_##P##_transcript_t* t, uint32_t n, uint32_t nbits, uint64_t* out) {       \
        return guard([&] { ZK_REQUIRE(t && out, "bad argument"); t->get_permutations(n, nbits, (u64*)out); });          \
    }                                                                                                                   \
    int zk_##P##_transcript_free(zk_##P##_transcript_t* t) { return guard([&] { delete t; }); }
ZK_FRHASH_CAPI(bn128, (*fr_field(HASH_BN128)))
ZK_FRHASH_CAPI(bls12381, (*fr_field(HASH_BLS12381)))
#undef ZK_FRHASH_CAPI

int zk_stark_get_pol_dev(const uint64_t* d_buf, uint64_t width, uint64_t offset, uint32_t dim, uint64_t n, uint64_t* d_out3, void* stream) {
    return guard([&] { pol_get_dev((const u64*)d_buf, width, offset, dim, n, (u64*)d_out3, on_stream((hipStream_t)stream)); });
}
int zk_stark_set_pol_dev(uint64_t* d_buf, uint64_t width, uint64_t offset, uint32_t dim, uint64_t n, const uint64_t* d_in3, void* stream) {
    return guard([&] { pol_set_dev((u64*)d_buf, width, offset, dim, n, (const u64*)d_in3, on_stream((hipStream_t)stream)); });
}
int zk_stark_calculate_h1h2_dev(const uint64_t* d_f3, const uint64_t* d_t3, uint64_t n, uint64_t* d_h1_3, uint64_t* d_h2_3, void* stream) {
    return guard([&] {
        ZK_REQUIRE(d_f3 && d_t3 && d_h1_3 && d_h2_3 && n >= 1, "calculate_H1H2: null or empty argument");
        ZK_REQUIRE(n <= (1ull << 28), "calculate_H1H2: more than 2^28 rows");
        hipStream_t st = on_stream((hipStream_t)stream);
        DevBuf work; work.reserve(h1h2_work_words(n) * 8);
        u64* d_missing = nullptr;
        calculate_h1h2_dev((const u64*)d_f3, (const u64*)d_t3, n, (u64*)d_h1_3, (u64*)d_h2_3, work.u(), &d_missing, st);
        u64 missing = 0;
        ZK_HIP(hipStreamSynchronize(st));
        ZK_HIP(hipMemcpy(&missing, d_missing, 8, hipMemcpyDeviceToHost));
        if (missing != ~0ull) {                                          // stark_gen.rs:636-638, the first f that the table lacks
            u64 e = 0;
            ZK_HIP(hipMemcpy(&e, d_f3 + 3 * missing, 8, hipMemcpyDeviceToHost));
            throw Error("Number not included: " + std::to_string(e));
        }
    });
}
int zk_stark_calculate_z_dev(const uint64_t* d_num3, const uint64_t* d_den3, uint64_t n, uint64_t* d_z3, void* stream) {
    return guard([&] {
        ZK_REQUIRE(n >= 1, "calculate_Z: empty polynomial");
        DevBuf work; work.reserve((n + n / 1024 + 8) * 24);
        u64 h[3];
        calculate_z_dev((const u64*)d_num3, (const u64*)d_den3, n, (u64*)d_z3, work.u(), work.u() + 3 * (n + n / 1024 + 4), on_stream((hipStream_t)stream));
        ZK_HIP(hipStreamSynchronize(on_stream((hipStream_t)stream)));
        ZK_HIP(hipMemcpy(h, work.u() + 3 * (n + n / 1024 + 4), 24, hipMemcpyDeviceToHost));
        ZK_REQUIRE(h[0] == 1 && h[1] == 0 && h[2] == 0, "calculate_Z: z does not close (grand product != 1)");
    });
}

// ---- compressor12 exec (compressor12.hip) ----------------------------------------------------------------------
struct zk_c12_exec { C12Exec* impl; };
zk_c12_exec_t* zk_c12_exec_new(const char* exec_json, size_t len, uint64_t n_witness) {
    zk_c12_exec_t* out = nullptr;
    if (guard([&] { C12Exec* e = c12_exec_new(exec_json, len, n_witness); out = new zk_c12_exec{e}; }) != 0) return nullptr;
    return out;
}
int zk_c12_exec_dev(const zk_c12_exec_t* e, const uint64_t* d_witness, uint64_t n_witness, uint64_t n_rows, uint64_t* d_cm, void* stream) {
    return guard([&] { ZK_REQUIRE(e && e->impl, "compressor12: null handle"); c12_exec_dev(e->impl, (const u64*)d_witness, n_witness, n_rows, (u64*)d_cm, on_stream((hipStream_t)stream)); });
}
uint64_t zk_c12_exec_depth(const zk_c12_exec_t* e) { return e && e->impl ? c12_exec_levels(e->impl) : 0; }
int zk_c12_exec_free(zk_c12_exec_t* e) {
    return guard([&] { if (e) { c12_exec_free(e->impl); delete e; } });
}

// ---- compressor12 setup (c12_setup.hip) ------------------------------------------------------------------------
struct zk_c12_setup { C12Setup* impl; };
static char* c12_dup(const std::string& s) {
    char* out = (char*)malloc(s.size() + 1);
    ZK_REQUIRE(out, "out of memory");
    memcpy(out, s.c_str(), s.size() + 1);
    return out;
}
zk_c12_setup_t* zk_c12_setup_new(const void* r1cs, size_t len, uint32_t force_n_bits) {
    zk_c12_setup_t* out = nullptr;
    if (guard([&] { C12Setup* s = c12_setup_new(r1cs, len, force_n_bits); out = new zk_c12_setup{s}; }) != 0) return nullptr;
    return out;
}
static uint64_t c12_info(const zk_c12_setup_t* s, int i) { uint64_t v[6] = {}; if (s && s->impl) c12_setup_info(s->impl, v); return v[i]; }
uint32_t zk_c12_setup_n_bits(const zk_c12_setup_t* s) { return (uint32_t)c12_info(s, 0); }
uint64_t zk_c12_setup_n_publics(const zk_c12_setup_t* s) { return c12_info(s, 1); }
uint64_t zk_c12_setup_n_used(const zk_c12_setup_t* s) { return c12_info(s, 2); }
uint64_t zk_c12_setup_n_const(const zk_c12_setup_t* s) { return c12_info(s, 3); }
uint64_t zk_c12_setup_n_gates(const zk_c12_setup_t* s) { return c12_info(s, 4); }
uint64_t zk_c12_setup_n_adds(const zk_c12_setup_t* s) { return c12_info(s, 5); }
int zk_c12_setup_gates(const zk_c12_setup_t* s, uint64_t* out) {
    return guard([&] { ZK_REQUIRE(s && s->impl && out, "compressor12 setup: null argument"); c12_setup_gates(s->impl, (u64*)out); });
}
char* zk_c12_setup_pil(const zk_c12_setup_t* s) {
    char* out = nullptr;
    if (guard([&] { ZK_REQUIRE(s && s->impl, "compressor12 setup: null handle"); out = c12_dup(c12_setup_pil(s->impl)); }) != 0) return nullptr;
    return out;
}
char* zk_c12_setup_exec(const zk_c12_setup_t* s) {
    char* out = nullptr;
    if (guard([&] { ZK_REQUIRE(s && s->impl, "compressor12 setup: null handle"); out = c12_dup(c12_setup_exec(s->impl)); }) != 0) return nullptr;
    return out;
}
int zk_c12_setup_consts_dev(const zk_c12_setup_t* s, uint64_t* d_out, void* stream) {
    return guard([&] { ZK_REQUIRE(s && s->impl, "compressor12 setup: null handle"); c12_setup_consts_dev(s->impl, (u64*)d_out, on_stream((hipStream_t)stream)); });
}
int zk_c12_setup_consts(const zk_c12_setup_t* s, uint64_t* out) {
    return guard([&] {
        ZK_REQUIRE(s && s->impl && out, "compressor12 setup: null argument");
        uint64_t v[6]; c12_setup_info(s->impl, v);
        const size_t bytes = ((size_t)1 << v[0]) * v[3] * 8;
        DevBuf d; d.reserve(bytes);
        c12_setup_consts_dev(s->impl, d.u(), cur_stream());
        d2h_sync(out, d.p, bytes);
    });
}
int zk_c12_setup_free(zk_c12_setup_t* s) {
    return guard([&] { if (s) { c12_setup_free(s->impl); delete s; } });
}
int zk_c12_sigma_dev(const uint32_t* d_s_map, uint64_t n_used, uint32_t n_bits, uint32_t n_const, uint32_t col0, uint64_t* d_out, void* stream) {
    return guard([&] { c12_sigma_dev((const u32*)d_s_map, n_used, n_bits, n_const, col0, (u64*)d_out, on_stream((hipStream_t)stream)); });
}

// ---- Groth16 (groth16.hip) ------------------------------------------------------------------------------------
zk_groth16_setup_t* zk_groth16_setup_new(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len) {
    zk_groth16_setup_t* out = nullptr;
    if (guard([&] { out = groth16_setup_new(curve, r1cs, r1cs_len, params, params_len); }) != 0) return nullptr;
    return out;
}
char* zk_groth16_key_check(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const char* vk_json,
                           const uint8_t* seed, uint32_t max_findings) {
    char* out = nullptr;
    if (guard([&] { out = c12_dup(groth16_key_check(curve, r1cs, r1cs_len, params, params_len, vk_json, seed, max_findings)); }) != 0) return nullptr;
    return out;
}
int zk_groth16_setup_info(const zk_groth16_setup_t* s, uint32_t* n_wires, uint32_t* n_inputs, uint32_t* domain_log) {
    return guard([&] {
        ZK_REQUIRE(s, "groth16: null setup");
        if (n_wires) *n_wires = s->num_wires();
        if (n_inputs) *n_inputs = s->num_inputs();
        if (domain_log) *domain_log = s->domain_log();
    });
}
static char* groth16_prove_any(zk_groth16_setup_t* g, const void* witness, bool on_device, uint64_t n_wires, const uint64_t* r, const uint64_t* s_, void* proof, uint64_t* d_h) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(g, "groth16: null setup");
            ZK_REQUIRE(witness && r && s_, "groth16: null argument");
            ZK_REQUIRE(n_wires == g->num_wires(), "groth16: the witness has " + std::to_string(n_wires) + " values, the circuit has " + std::to_string(g->num_wires()) + " wires");
            auto lt = [&](const u32* v) { return g->curve->fr_canonical(v); };
            ZK_REQUIRE(lt((const u32*)r) && lt((const u32*)s_), "groth16: r and s must be canonical field elements");
            if (!on_device) {   // Fr::from_repr (reader.rs:131-134) rejects non-canonical values
                const u32* w = (const u32*)witness;
                for (uint64_t i = 0; i < n_wires; ++i) ZK_REQUIRE(lt(w + 8 * i), "groth16: witness value " + std::to_string(i) + " is not a canonical field element");
            }
            std::string js;
            g->prove(witness, on_device, (const u64*)r, (const u64*)s_, (u32*)proof, &js, (u64*)d_h);
            out = (char*)malloc(js.size() + 1);
            ZK_REQUIRE(out, "out of memory");
            memcpy(out, js.c_str(), js.size() + 1);
        }) != 0) return nullptr;
    return out;
}
char* zk_groth16_prove(zk_groth16_setup_t* s, const void* witness, uint64_t n_wires, const uint64_t r[4], const uint64_t s_[4], void* proof) {
    return groth16_prove_any(s, witness, false, n_wires, r, s_, proof, nullptr);
}
char* zk_groth16_prove_dev(zk_groth16_setup_t* s, const void* d_witness, uint64_t n_wires, const uint64_t r[4], const uint64_t s_[4], void* proof, uint64_t* d_h) {
    return groth16_prove_any(s, d_witness, true, n_wires, r, s_, proof, d_h);
}
int zk_groth16_wtns_payload(const void* wtns, size_t len, const char* curve, uint64_t* offset, uint64_t* n_values) {
    return guard([&] { ZK_REQUIRE(wtns && offset && n_values, "wtns: null argument"); groth16_wtns_payload(wtns, len, curve, offset, n_values); });
}
int zk_groth16_setup_free(zk_groth16_setup_t* s) {
    return guard([&] { delete s; });
}

// ---- Groth16 key generation (fixedbase_impl.hip.h, groth16_keygen_impl.hip.h) ------------------------------------
zk_groth16_keygen_t* zk_groth16_keygen_new(const char* curve, const void* r1cs, size_t r1cs_len, const uint64_t* trapdoor) {
    zk_groth16_keygen_t* out = nullptr;
    if (guard([&] { out = groth16_keygen_new(curve, r1cs, r1cs_len, trapdoor); }) != 0) return nullptr;
    return out;
}
size_t zk_groth16_keygen_params_size(const zk_groth16_keygen_t* k) { return k ? k->params.size() : 0; }
int zk_groth16_keygen_params(const zk_groth16_keygen_t* k, void* out, size_t cap) {
    return guard([&] {
        ZK_REQUIRE(k && out, "groth16 keygen: null argument");
        ZK_REQUIRE(cap >= k->params.size(), "groth16 keygen: the buffer holds " + std::to_string(cap) + " bytes, the key has " + std::to_string(k->params.size()));
        memcpy(out, k->params.data(), k->params.size());
    });
}
char* zk_groth16_keygen_vk_json(const zk_groth16_keygen_t* k, int to_hex) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(k, "groth16 keygen: null handle");
            const std::string js = groth16_keygen_vk_json(*k, to_hex != 0);
            out = (char*)malloc(js.size() + 1);
            ZK_REQUIRE(out, "out of memory");
            memcpy(out, js.c_str(), js.size() + 1);
        }) != 0) return nullptr;
    return out;
}
int zk_groth16_keygen_timing(const zk_groth16_keygen_t* k, double ms[5]) {
    return guard([&] { ZK_REQUIRE(k && ms, "groth16 keygen: null argument"); for (int i = 0; i < 5; ++i) ms[i] = k->ms[i]; });
}
int zk_groth16_keygen_free(zk_groth16_keygen_t* k) {
    return guard([&] { delete k; });
}

// ---- a key from a powers-of-tau file, contributions to it (groth16_srs.hip.h, ecntt.hip) ----------------------------------------
static char* dup_report(const std::string& js) {
    char* out = (char*)malloc(js.size() + 1);
    ZK_REQUIRE(out, "out of memory");
    memcpy(out, js.c_str(), js.size() + 1);
    return out;
}
zk_srs_t* zk_srs_open(const char* curve, const char* path) {
    zk_srs_t* out = nullptr;
    if (guard([&] { out = srs_open(curve, path); }) != 0) return nullptr;
    return out;
}
int zk_srs_info(const zk_srs_t* s, uint32_t* power, uint32_t* ceremony_power) {
    return guard([&] {
        ZK_REQUIRE(s, "ptau: null handle");
        if (power) *power = s->power;
        if (ceremony_power) *ceremony_power = s->ceremony_power;
    });
}
int zk_srs_free(zk_srs_t* s) {
    return guard([&] { delete s; });
}
char* zk_srs_check(const zk_srs_t* s, const uint8_t* seed, uint32_t max_findings) {
    char* out = nullptr;
    if (guard([&] { ZK_REQUIRE(s, "ptau: null handle"); out = dup_report(srs_check(*s, seed, max_findings)); }) != 0) return nullptr;
    return out;
}
int zk_srs_new(const char* curve, uint32_t power, const char* path) {
    return guard([&] { srs_new(curve, power, path); });
}
int zk_srs_contribute(const zk_srs_t* s, const char* out_path, const uint64_t* secrets, const uint8_t* beacon_seed, uint32_t beacon_iter_log) {
    return guard([&] { ZK_REQUIRE(s, "ptau: null handle"); srs_contribute(*s, out_path, secrets, beacon_seed, beacon_iter_log); });
}
char* zk_srs_verify(const zk_srs_t* s, const uint8_t* seed, uint32_t max_findings) {
    char* out = nullptr;
    if (guard([&] { ZK_REQUIRE(s, "ptau: null handle"); out = dup_report(srs_verify(*s, seed, max_findings)); }) != 0) return nullptr;
    return out;
}
int zk_srs_transcript_count(const zk_srs_t* s, int64_t* count) {
    return guard([&] { ZK_REQUIRE(s && count, "ptau: null argument"); *count = srs_transcript_count(*s); });
}
zk_groth16_keygen_t* zk_groth16_keygen_from_srs(const char* curve, const void* r1cs, size_t r1cs_len, const zk_srs_t* srs) {
    zk_groth16_keygen_t* out = nullptr;
    if (guard([&] { out = groth16_keygen_from_srs(curve, r1cs, r1cs_len, srs); }) != 0) return nullptr;
    return out;
}
int zk_groth16_params_contribute(const char* curve, const void* params, size_t len, const uint64_t* delta, void* out) {
    return guard([&] { groth16_params_contribute(curve, params, len, delta, out); });
}
char* zk_groth16_contribution_check(const char* curve, const void* old_params, size_t old_len, const void* new_params, size_t new_len, const uint8_t* seed,
                                    uint32_t max_findings) {
    char* out = nullptr;
    if (guard([&] { out = dup_report(groth16_contribution_check(curve, old_params, old_len, new_params, new_len, seed, max_findings)); }) != 0) return nullptr;
    return out;
}
size_t zk_groth16_key_transcript_size(const char* curve, uint32_t count) {
    size_t out = 0;
    if (guard([&] { out = groth16_key_transcript_size(curve, count); }) != 0) return 0;
    return out;
}
int zk_groth16_params_contribute_pok(const char* curve, const void* params, size_t len, const uint64_t* delta, const void* transcript, size_t t_len, void* out_params,
                                     void* out_transcript) {
    return guard([&] { groth16_params_contribute_pok(curve, params, len, delta, transcript, t_len, out_params, out_transcript); });
}
char* zk_groth16_key_transcript_check(const char* curve, const void* initial, size_t initial_len, const void* final_key, size_t final_len, const void* transcript,
                                      size_t t_len, const uint8_t* seed, uint32_t max_findings) {
    char* out = nullptr;
    if (guard([&] { out = dup_report(groth16_key_transcript_check(curve, initial, initial_len, final_key, final_len, transcript, t_len, seed, max_findings)); }) != 0) return nullptr;
    return out;
}
char* zk_groth16_key_check_srs(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const zk_srs_t* srs, const uint8_t* seed,
                                uint32_t max_findings) {
    char* out = nullptr;
    if (guard([&] { out = dup_report(groth16_key_check_srs(curve, r1cs, r1cs_len, params, params_len, srs, seed, max_findings)); }) != 0) return nullptr;
    return out;
}
static int group_ntt_device(CurveId id, Group g, void* d_points, uint32_t log_n, int inverse, void* stream) {
    return guard([&] { group_ntt_dev(curve(id), g, d_points, (int)log_n, inverse != 0, on_stream((hipStream_t)stream)); });
}
static int mul_scalar_device(CurveId id, Group g, const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream) {
    return guard([&] {
        ZK_REQUIRE(n == 0 || (d_points && d_k && d_out), "mul_scalar: null argument");
        curve(id).ec().g[g].mul_scalar(d_points, n, (const u32*)d_k, d_out, on_stream((hipStream_t)stream));
    });
}
static int mul_scalars_device(CurveId id, Group g, const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream) {
    return guard([&] {
        ZK_REQUIRE(n == 0 || (d_points && d_k && d_out), "mul_scalars: null argument");
        curve(id).ec().g[g].mul_scalars(d_points, curve(id).point_words(g), n, (const u32*)d_k, d_out, on_stream((hipStream_t)stream));
    });
}
static int mul_scalars_glv_device(CurveId id, const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream) {
    return guard([&] {
        ZK_REQUIRE(n == 0 || (d_points && d_k && d_out), "mul_scalars_glv: null argument");
        curve(id).ec().g[G1].mul_scalars_glv(d_points, curve(id).point_words(G1), n, (const u32*)d_k, d_out, on_stream((hipStream_t)stream));
    });
}
int zk_g1_bn254_mul_scalars_glv_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream) { return mul_scalars_glv_device(CURVE_BN254, d_points, n, d_k, d_out, stream); }
int zk_g1_bls12_381_mul_scalars_glv_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream) { return mul_scalars_glv_device(CURVE_BLS12_381, d_points, n, d_k, d_out, stream); }
#define ZK_EC_API(GN, NAME, ID, G)                                                                                                            \
    int zk_##GN##_##NAME##_ntt_dev(void* d_points, uint32_t log_n, int inverse, void* stream) { return group_ntt_device(ID, G, d_points, log_n, inverse, stream); } \
    int zk_##GN##_##NAME##_mul_scalar_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream) { return mul_scalar_device(ID, G, d_points, n, d_k, d_out, stream); } \
    int zk_##GN##_##NAME##_mul_scalars_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream) { return mul_scalars_device(ID, G, d_points, n, d_k, d_out, stream); }
ZK_EC_API(g1, bn254, CURVE_BN254, G1)
ZK_EC_API(g2, bn254, CURVE_BN254, G2)
ZK_EC_API(g1, bls12_381, CURVE_BLS12_381, G1)
ZK_EC_API(g2, bls12_381, CURVE_BLS12_381, G2)
#undef ZK_EC_API

// ---- pairings and Groth16 verification (pairing.hip) ----
zk_groth16_vk_t* zk_groth16_vk_new(const char* curve, const char* vk_json) {
    zk_groth16_vk_t* h = nullptr;
    if (guard([&] { h = groth16_vk_new(curve, vk_json); }) != 0) return nullptr;
    return h;
}
int zk_groth16_vk_info(const zk_groth16_vk_t* vk, uint32_t* n_public, uint32_t* proof_bytes, uint32_t* gt_bytes) {
    return guard([&] { ZK_REQUIRE(vk, "groth16 verify: null key"); groth16_vk_info(vk, n_public, proof_bytes, gt_bytes); });
}
int zk_groth16_vk_free(zk_groth16_vk_t* vk) {
    return guard([&] { delete vk; });
}
int zk_groth16_verify_batch(const zk_groth16_vk_t* vk, const void* proofs, const void* publics, uint64_t n, int* verdicts) {
    return guard([&] { ZK_REQUIRE(vk, "groth16 verify: null key"); groth16_verify_batch(vk, proofs, publics, n, verdicts); });
}
int zk_groth16_verify_batch_dev(const zk_groth16_vk_t* vk, const void* d_proofs, const void* d_publics, uint64_t n, int* d_verdicts, void* stream) {
    return guard([&] {
        ZK_REQUIRE(vk, "groth16 verify: null key");
        groth16_verify_batch_dev(vk, d_proofs, d_publics, n, d_verdicts, on_stream((hipStream_t)stream));
    });
}
int zk_groth16_verify_json(const zk_groth16_vk_t* vk, const char* proof_json, const char* public_input_json) {
    int verdict = ZK_VERDICT_ERROR;
    if (guard([&] { ZK_REQUIRE(vk, "groth16 verify: null key"); verdict = groth16_verify_json(vk, proof_json, public_input_json); }) != 0)
        return ZK_VERDICT_ERROR;
    return verdict;
}
int zk_groth16_verify_aggregate(const zk_groth16_vk_t* vk, const void* proofs, const void* publics, uint64_t n, const uint8_t* seed, int* verdict, uint64_t* first_bad) {
    return guard([&] {
        ZK_REQUIRE(vk && verdict, "groth16 verify: null argument");
        *verdict = ZK_VERDICT_ERROR;
        groth16_verify_aggregate(vk, proofs, publics, n, seed, first_bad != nullptr, verdict, first_bad);
    });
}
int zk_groth16_verify_aggregate_dev(const zk_groth16_vk_t* vk, const void* d_proofs, const void* d_publics, uint64_t n, const uint8_t* seed, int* verdict,
                                    uint64_t* first_bad, void* stream) {
    return guard([&] {
        ZK_REQUIRE(vk && verdict, "groth16 verify: null argument");
        *verdict = ZK_VERDICT_ERROR;
        groth16_verify_aggregate_dev(vk, d_proofs, d_publics, n, seed, first_bad != nullptr, verdict, first_bad, on_stream((hipStream_t)stream));
    });
}
// ---- KZG commitments over a powers-of-tau file (kzg.hip) ----
uint64_t zk_kzg_tile_elems(void) { return KZG_TILE; }
uint64_t zk_kzg_aggregate_span(void) { return KZG_SPAN; }
#define ZK_KZG_API(NAME, ID)                                                                                                                  \
    int zk_kzg_##NAME##_divide_dev(const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_q, uint64_t* d_y, void* stream) {     \
        return guard([&] { kzg_divide_dev(curve(ID), d_coeffs, n, z, d_q, d_y, on_stream((hipStream_t)stream)); });                           \
    }                                                                                                                                         \
    int zk_kzg_##NAME##_lincomb_dev(const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, const uint64_t* gamma, uint64_t* d_out, void* stream) { \
        return guard([&] { kzg_lincomb_dev(curve(ID), d_polys, n, k, gamma, d_out, on_stream((hipStream_t)stream)); });                       \
    }
ZK_KZG_API(bn254, CURVE_BN254)
ZK_KZG_API(bls12_381, CURVE_BLS12_381)
#undef ZK_KZG_API
zk_kzg_t* zk_kzg_new(const zk_srs_t* srs, uint64_t max_coeffs) {
    zk_kzg_t* out = nullptr;
    if (guard([&] { out = kzg_new(srs, max_coeffs); }) != 0) return nullptr;
    return out;
}
int zk_kzg_free(zk_kzg_t* k) {
    return guard([&] { delete k; });
}
int zk_kzg_info(const zk_kzg_t* k, const char** curve, uint64_t* max_coeffs, uint32_t* power, uint32_t* point_bytes, uint32_t* opening_bytes) {
    return guard([&] {
        ZK_REQUIRE(k, "kzg: null handle");
        if (curve) *curve = k->curve->name;
        if (max_coeffs) *max_coeffs = k->max_coeffs;
        if (power) *power = k->power;
        if (point_bytes) *point_bytes = (uint32_t)k->curve->point_bytes(G1);
        if (opening_bytes) *opening_bytes = (uint32_t)(2 * k->curve->point_bytes(G1) + 64);
    });
}
int zk_kzg_commit_dev(zk_kzg_t* k, const uint64_t* d_coeffs, uint64_t n, void* d_out, void* stream) {
    return guard([&] { ZK_REQUIRE(k, "kzg: null handle"); kzg_commit_dev(*k, d_coeffs, n, d_out, on_stream((hipStream_t)stream)); });
}
int zk_kzg_commit_evals_dev(zk_kzg_t* k, const uint64_t* d_evals, uint32_t log_n, void* d_out, void* stream) {
    return guard([&] { ZK_REQUIRE(k, "kzg: null handle"); kzg_commit_evals_dev(*k, d_evals, log_n, d_out, on_stream((hipStream_t)stream)); });
}
int zk_kzg_eval_dev(zk_kzg_t* k, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_y_out, void* stream) {
    return guard([&] { ZK_REQUIRE(k, "kzg: null handle"); kzg_divide_dev(*k->curve, d_coeffs, n, z, nullptr, d_y_out, on_stream((hipStream_t)stream)); });
}
int zk_kzg_open_dev(zk_kzg_t* k, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_y_out, void* d_w_out, void* stream) {
    return guard([&] { ZK_REQUIRE(k, "kzg: null handle"); kzg_open_dev(*k, d_coeffs, n, z, d_y_out, d_w_out, on_stream((hipStream_t)stream)); });
}
int zk_kzg_open_many_dev(zk_kzg_t* k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* z, const uint64_t* gamma,
                         uint64_t* d_ys_out, void* d_w_out, void* stream) {
    return guard([&] { ZK_REQUIRE(k, "kzg: null handle"); kzg_open_many_dev(*k, d_polys, n, n_polys, z, gamma, d_ys_out, d_w_out, on_stream((hipStream_t)stream)); });
}
int zk_kzg_fold_commitments(zk_kzg_t* k, const void* commitments, uint32_t n, const uint64_t* gamma, void* out) {
    return guard([&] { ZK_REQUIRE(k, "kzg: null handle"); kzg_fold_commitments(*k, commitments, n, gamma, out); });
}
int zk_kzg_verify(zk_kzg_t* k, const void* openings, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad) {
    return guard([&] {
        ZK_REQUIRE(k && verdict, "kzg verify: null argument");
        *verdict = ZK_VERDICT_ERROR;
        kzg_verify(*k, openings, m, seed, first_bad != nullptr, verdict, first_bad);
    });
}
int zk_kzg_verify_dev(zk_kzg_t* k, const void* d_openings, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad, void* stream) {
    return guard([&] {
        ZK_REQUIRE(k && verdict, "kzg verify: null argument");
        *verdict = ZK_VERDICT_ERROR;
        kzg_verify_dev(*k, d_openings, m, seed, first_bad != nullptr, verdict, first_bad, on_stream((hipStream_t)stream));
    });
}
// ---- KZG: several polynomials at several points in one two-point proof (kzg.hip) ----
#define ZK_KZG_MULTI_API(NAME, ID)                                                                                                            \
    int zk_kzg_##NAME##_divide_acc_dev(const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, const uint64_t* w, uint64_t* d_acc_inout, uint64_t* d_y, \
                                       void* stream) {                                                                                        \
        return guard([&] { kzg_divide_acc_dev(curve(ID), d_coeffs, n, z, w, d_acc_inout, d_y, on_stream((hipStream_t)stream)); });            \
    }                                                                                                                                         \
    int zk_kzg_##NAME##_interleave_dev(const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, uint64_t* d_out, void* stream) {        \
        return guard([&] { kzg_interleave_dev(curve(ID), d_polys, n, k, d_out, on_stream((hipStream_t)stream)); });                           \
    }
ZK_KZG_MULTI_API(bn254, CURVE_BN254)
ZK_KZG_MULTI_API(bls12_381, CURVE_BLS12_381)
#undef ZK_KZG_MULTI_API
zk_kzg_multi_t* zk_kzg_multi_begin(zk_kzg_t* k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* points,
                                   const uint32_t* set_sizes, uint64_t* d_values_out, void* stream) {
    zk_kzg_multi_t* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(k, "kzg: null handle");
            out = kzg_multi_begin(*k, d_polys, n, n_polys, points, set_sizes, d_values_out, on_stream((hipStream_t)stream));
        }) != 0)
        return nullptr;
    return out;
}
int zk_kzg_multi_quotient(zk_kzg_multi_t* m, const uint64_t* gamma, void* d_w1_out, void* stream) {
    return guard([&] { ZK_REQUIRE(m, "kzg multi: null handle"); kzg_multi_quotient(*m, gamma, d_w1_out, on_stream((hipStream_t)stream)); });
}
int zk_kzg_multi_finish(zk_kzg_multi_t* m, const uint64_t* z, void* d_w2_out, void* stream) {
    return guard([&] { ZK_REQUIRE(m, "kzg multi: null handle"); kzg_multi_finish(*m, z, d_w2_out, on_stream((hipStream_t)stream)); });
}
int zk_kzg_multi_free(zk_kzg_multi_t* m) {
    return guard([&] { delete m; });
}
int zk_kzg_multi_verify(zk_kzg_t* k, const void* proofs, uint64_t bytes, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad) {
    return guard([&] {
        ZK_REQUIRE(k && verdict, "kzg multi verify: null argument");
        *verdict = ZK_VERDICT_ERROR;
        kzg_multi_verify(*k, proofs, bytes, m, seed, first_bad != nullptr, verdict, first_bad, cur_stream());
    });
}
int zk_kzg_multi_verify_dev(zk_kzg_t* k, const void* d_proofs, uint64_t bytes, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad, void* stream) {
    return guard([&] {
        ZK_REQUIRE(k && verdict && (d_proofs || !bytes), "kzg multi verify: null argument");
        *verdict = ZK_VERDICT_ERROR;
        hipStream_t st = on_stream((hipStream_t)stream);
        std::vector<uint8_t> host(bytes);                                   // the scalars of a proof are derived on the host: the sets are tiny
        if (bytes) { ZK_HIP(hipMemcpyAsync(host.data(), d_proofs, bytes, hipMemcpyDeviceToHost, st)); ZK_HIP(hipStreamSynchronize(st)); }
        kzg_multi_verify(*k, host.data(), bytes, m, seed, first_bad != nullptr, verdict, first_bad, st);
    });
}
// ---- polynomial arithmetic over the scalar field (frpoly_impl.hip.h through groth16.hip) ----
uint64_t zk_frpoly_tile_elems(void) { return FRPOLY_TILE; }
uint64_t zk_frpoly_span(void) { return FRPOLY_SPAN; }
#define ZK_FRPOLY_API(NAME, ID)                                                                                                               \
    int zk_fr_##NAME##_prefix_product_dev(const uint64_t* d_in, uint64_t n, int inclusive, uint64_t* d_out, uint64_t* total_out, void* stream) { \
        return guard([&] { curve(ID).frpoly().prefix_product_dev((const u64*)d_in, n, inclusive != 0, (u64*)d_out, (u64*)total_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_batch_inverse_dev(const uint64_t* d_in, uint64_t n, uint64_t* d_out, uint64_t* n_zero, uint64_t* first_zero, void* stream) { \
        return guard([&] { curve(ID).frpoly().batch_inverse_dev((const u64*)d_in, n, (u64*)d_out, (u64*)n_zero, (u64*)first_zero, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_pointwise_dev(int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, uint64_t n, void* stream) {           \
        return guard([&] { curve(ID).frpoly().pointwise_dev(op, (const u64*)d_a, (const u64*)d_b, (u64*)d_out, n, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_powers_dev(const uint64_t* base, const uint64_t* scale, uint64_t n, uint64_t* d_out, void* stream) {                   \
        return guard([&] { curve(ID).frpoly().powers_dev((const u64*)base, (const u64*)scale, n, (u64*)d_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_terms_dev(const uint64_t* const* d_cols, const uint64_t* const* d_labels, uint32_t k, uint64_t n, const uint64_t* beta, \
                                 const uint64_t* gamma, uint64_t* d_out, void* stream) {                                                      \
        return guard([&] {                                                                                                                    \
            curve(ID).frpoly().terms_dev((const u64* const*)d_cols, (const u64* const*)d_labels, k, n, (const u64*)beta, (const u64*)gamma, (u64*)d_out, on_stream((hipStream_t)stream)); \
        });                                                                                                                                   \
    }                                                                                                                                         \
    int zk_fr_##NAME##_grand_product_dev(const uint64_t* d_num, const uint64_t* d_den, uint64_t n, uint64_t* d_z, uint64_t* last_out, void* stream) { \
        return guard([&] { curve(ID).frpoly().grand_product_dev((const u64*)d_num, (const u64*)d_den, n, (u64*)d_z, (u64*)last_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_poly_mul_dev(const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* d_out, void* stream) {      \
        return guard([&] { curve(ID).frpoly().poly_mul_dev((const u64*)d_a, na, (const u64*)d_b, nb, (u64*)d_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_divmod_zh_dev(const uint64_t* d_p, uint64_t n_p, uint32_t log_n, uint64_t* d_q, uint64_t* d_rem, uint64_t* rem_nonzero, void* stream) { \
        return guard([&] { curve(ID).frpoly().divmod_zh_dev((const u64*)d_p, n_p, log_n, (u64*)d_q, (u64*)d_rem, (u64*)rem_nonzero, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_divide_zh_coset_dev(uint64_t* d_evals, uint32_t log_m, uint32_t log_n, void* stream) {                                 \
        return guard([&] { curve(ID).frpoly().divide_zh_coset_dev((u64*)d_evals, log_m, log_n, on_stream((hipStream_t)stream)); });           \
    }                                                                                                                                         \
    int zk_fr_##NAME##_prefix_sum_dev(const uint64_t* d_in, uint64_t n, int inclusive, uint64_t* d_out, uint64_t* total_out, void* stream) {  \
        return guard([&] { curve(ID).frpoly().prefix_sum_dev((const u64*)d_in, n, inclusive != 0, (u64*)d_out, (u64*)total_out, on_stream((hipStream_t)stream)); }); \
    }
ZK_FRPOLY_API(bn254, CURVE_BN254)
ZK_FRPOLY_API(bls12_381, CURVE_BLS12_381)
#undef ZK_FRPOLY_API
// ---- the device side of the PLONK prover (plonk_impl.hip.h through groth16.hip) ----
#define ZK_PLONK_API(NAME, ID)                                                                                                                \
    int zk_plonk_##NAME##_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, \
                                       const uint64_t* k1, const uint64_t* k2, uint64_t* d_out, void* stream) {                               \
        return guard([&] {                                                                                                                    \
            curve(ID).plonk().quotient_dev((const u64* const*)d_cols, log_n, (const u64*)alpha, (const u64*)beta, (const u64*)gamma, (const u64*)k1, (const u64*)k2, (u64*)d_out, \
                                           on_stream((hipStream_t)stream));                                                                   \
        });                                                                                                                                   \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_gate_check_dev(const uint64_t* const* d_cols, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* stream) {      \
        return guard([&] { curve(ID).plonk().gate_check_dev((const u64* const*)d_cols, n, (u64*)n_bad, (u64*)first_bad, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_next_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, \
                                            const uint64_t* k1, const uint64_t* k2, uint64_t* d_out, void* stream) {                          \
        return guard([&] {                                                                                                                    \
            curve(ID).plonk().next_quotient_dev((const u64* const*)d_cols, log_n, (const u64*)alpha, (const u64*)beta, (const u64*)gamma, (const u64*)k1, (const u64*)k2, (u64*)d_out, \
                                                on_stream((hipStream_t)stream));                                                              \
        });                                                                                                                                   \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_next_gate_check_dev(const uint64_t* const* d_cols, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* stream) { \
        return guard([&] { curve(ID).plonk().next_gate_check_dev((const u64* const*)d_cols, n, (u64*)n_bad, (u64*)first_bad, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_fr_##NAME##_gather_dev(const uint64_t* d_src, uint64_t n_src, const uint32_t* d_idx, uint64_t n, uint64_t* d_out, void* stream) {   \
        return guard([&] { curve(ID).plonk().gather_dev((const u64*)d_src, n_src, d_idx, n, (u64*)d_out, on_stream((hipStream_t)stream)); }); \
    }
ZK_PLONK_API(bn254, CURVE_BN254)
ZK_PLONK_API(bls12_381, CURVE_BLS12_381)
#undef ZK_PLONK_API
// ---- the device side of the fflonk prover (fflonk_impl.hip.h through groth16.hip) ----
#define ZK_FFLONK_API(NAME, ID)                                                                                                               \
    int zk_fflonk_##NAME##_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1, \
                                         const uint64_t* k2, uint64_t* d_out0, uint64_t* d_out1, uint64_t* d_out2, void* stream) {            \
        return guard([&] {                                                                                                                    \
            curve(ID).fflonk().quotients_dev((const u64* const*)d_cols, log_n, (const u64*)beta, (const u64*)gamma, (const u64*)k1, (const u64*)k2, (u64*)d_out0, (u64*)d_out1, \
                                             (u64*)d_out2, on_stream((hipStream_t)stream));                                                   \
        });                                                                                                                                   \
    }
ZK_FFLONK_API(bn254, CURVE_BN254)
ZK_FFLONK_API(bls12_381, CURVE_BLS12_381)
#undef ZK_FFLONK_API
// ---- the device side of PLONK's lookup argument (plonk_lookup_impl.hip.h and plonk_lookup_tagged_impl.hip.h through groth16.hip) ----
static const zk_plonk_lookup_table_t& plonk_lookup_table_of(const zk_plonk_lookup_table_t* h, CurveId id) {
    ZK_REQUIRE(h, "plonk lookup: null table");
    ZK_REQUIRE(h->curve == &curve(id), "plonk lookup: the table is over another field");
    return *h;
}
#define ZK_PLONK_LOOKUP_API(NAME, ID)                                                                                                         \
    zk_plonk_lookup_table_t* zk_plonk_##NAME##_lookup_table_new(const uint64_t* d_t1, const uint64_t* d_t2, const uint64_t* d_t3, uint64_t T, void* stream) { \
        zk_plonk_lookup_table_t* out = nullptr;                                                                                               \
        guard([&] { out = curve(ID).plonk_lookup().table_new((const u64*)d_t1, (const u64*)d_t2, (const u64*)d_t3, T, on_stream((hipStream_t)stream)); }); \
        return out;                                                                                                                           \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_lookup_table_free(zk_plonk_lookup_table_t* table) { return guard([&] { delete table; }); }                          \
    int zk_plonk_##NAME##_lookup_count_dev(const zk_plonk_lookup_table_t* table, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, const uint64_t* d_qK, uint64_t n, \
                                           uint64_t* d_m_out, uint64_t* n_bad, uint64_t* first_bad, void* stream) {                           \
        return guard([&] {                                                                                                                    \
            curve(ID).plonk_lookup().count_dev(plonk_lookup_table_of(table, ID), (const u64*)d_a, (const u64*)d_b, (const u64*)d_c, (const u64*)d_qK, n, (u64*)d_m_out, (u64*)n_bad, \
                                               (u64*)first_bad, on_stream((hipStream_t)stream));                                              \
        });                                                                                                                                   \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_lookup_terms_dev(const uint64_t* const* d_cols, uint64_t n, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out, void* stream) { \
        return guard([&] { curve(ID).plonk_lookup().terms_dev((const u64* const*)d_cols, n, (const u64*)eta, (const u64*)delta, (u64*)d_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_lookup_summands_dev(const uint64_t* d_inv, const uint64_t* d_qK, const uint64_t* d_m, uint64_t n, uint64_t* d_out, void* stream) { \
        return guard([&] { curve(ID).plonk_lookup().summands_dev((const u64*)d_inv, (const u64*)d_qK, (const u64*)d_m, n, (u64*)d_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_lookup_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* eta, const uint64_t* delta, uint64_t* d_acc, \
                                              void* stream) {                                                                                 \
        return guard([&] {                                                                                                                    \
            curve(ID).plonk_lookup().quotient_dev((const u64* const*)d_cols, log_n, (const u64*)alpha, (const u64*)eta, (const u64*)delta, (u64*)d_acc, on_stream((hipStream_t)stream)); \
        });                                                                                                                                   \
    }
#define ZK_PLONK_LOOKUP_TAGGED_API(NAME, ID)                                                                                                  \
    zk_plonk_lookup_table_t* zk_plonk_##NAME##_lookup_tagged_table_new(const uint64_t* d_t0, const uint64_t* d_t1, const uint64_t* d_t2, const uint64_t* d_t3, uint64_t T, \
                                                                       void* stream) {                                                        \
        zk_plonk_lookup_table_t* out = nullptr;                                                                                               \
        guard([&] { out = curve(ID).plonk_lookup().tagged_table_new((const u64*)d_t0, (const u64*)d_t1, (const u64*)d_t2, (const u64*)d_t3, T, on_stream((hipStream_t)stream)); }); \
        return out;                                                                                                                           \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_lookup_tagged_count_dev(const zk_plonk_lookup_table_t* table, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, const uint64_t* d_qK, \
                                                  uint64_t n, uint64_t* d_m_out, uint64_t* n_bad, uint64_t* first_bad, void* stream) {        \
        return guard([&] {                                                                                                                    \
            curve(ID).plonk_lookup().tagged_count_dev(plonk_lookup_table_of(table, ID), (const u64*)d_a, (const u64*)d_b, (const u64*)d_c, (const u64*)d_qK, n, (u64*)d_m_out, \
                                                      (u64*)n_bad, (u64*)first_bad, on_stream((hipStream_t)stream));                          \
        });                                                                                                                                   \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_lookup_tagged_terms_dev(const uint64_t* const* d_cols, uint64_t n, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out, void* stream) { \
        return guard([&] { curve(ID).plonk_lookup().tagged_terms_dev((const u64* const*)d_cols, n, (const u64*)eta, (const u64*)delta, (u64*)d_out, on_stream((hipStream_t)stream)); }); \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_lookup_tagged_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* eta, const uint64_t* delta, \
                                                     uint64_t* d_acc, void* stream) {                                                         \
        return guard([&] {                                                                                                                    \
            curve(ID).plonk_lookup().tagged_quotient_dev((const u64* const*)d_cols, log_n, (const u64*)alpha, (const u64*)eta, (const u64*)delta, (u64*)d_acc, \
                                                         on_stream((hipStream_t)stream));                                                     \
        });                                                                                                                                   \
    }
ZK_PLONK_LOOKUP_API(bn254, CURVE_BN254)
ZK_PLONK_LOOKUP_API(bls12_381, CURVE_BLS12_381)
#undef ZK_PLONK_LOOKUP_API
ZK_PLONK_LOOKUP_TAGGED_API(bn254, CURVE_BN254)
ZK_PLONK_LOOKUP_TAGGED_API(bls12_381, CURVE_BLS12_381)
#undef ZK_PLONK_LOOKUP_TAGGED_API
// ---- the device side of the fflonk prover with lookups (fflonk_lookup_impl.hip.h and fflonk_lookup_tagged_impl.hip.h through groth16.hip) ----
#define ZK_FFLONK_LOOKUP_API(NAME, ID)                                                                                                        \
    int zk_fflonk_##NAME##_lookup_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1, \
                                                const uint64_t* k2, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out0, uint64_t* d_out1, uint64_t* d_out2, \
                                                uint64_t* d_out3, void* stream) {                                                             \
        return guard([&] {                                                                                                                    \
            curve(ID).fflonk_lookup().quotients_dev((const u64* const*)d_cols, log_n, (const u64*)beta, (const u64*)gamma, (const u64*)k1, (const u64*)k2, (const u64*)eta, \
                                                    (const u64*)delta, (u64*)d_out0, (u64*)d_out1, (u64*)d_out2, (u64*)d_out3, on_stream((hipStream_t)stream)); \
        });                                                                                                                                   \
    }                                                                                                                                         \
    int zk_fflonk_##NAME##_lookup_tagged_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1, \
                                                       const uint64_t* k2, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out0, uint64_t* d_out1,          \
                                                       uint64_t* d_out2, uint64_t* d_out3, void* stream) {                                    \
        return guard([&] {                                                                                                                    \
            curve(ID).fflonk_lookup().tagged_quotients_dev((const u64* const*)d_cols, log_n, (const u64*)beta, (const u64*)gamma, (const u64*)k1, (const u64*)k2,    \
                                                           (const u64*)eta, (const u64*)delta, (u64*)d_out0, (u64*)d_out1, (u64*)d_out2, (u64*)d_out3,             \
                                                           on_stream((hipStream_t)stream));                                                   \
        });                                                                                                                                   \
    }
ZK_FFLONK_LOOKUP_API(bn254, CURVE_BN254)
ZK_FFLONK_LOOKUP_API(bls12_381, CURVE_BLS12_381)
#undef ZK_FFLONK_LOOKUP_API
// ---- the R1CS import of the PLONK prover (plonk_r1cs_impl.hip.h through groth16.hip); new, info, tables and free touch no device ----
uint64_t zk_plonk_r1cs_wave_min_terms(void) { return PLONK_R1CS_WAVE_MIN_TERMS; }
static const zk_plonk_r1cs_t& plonk_r1cs_of(const zk_plonk_r1cs_t* h, CurveId id) {
    ZK_REQUIRE(h, "plonk r1cs: null handle");
    ZK_REQUIRE(h->curve == &curve(id), "plonk r1cs: the handle is over another field");
    return *h;
}
static void plonk_r1cs_info(const zk_plonk_r1cs_t& h, uint64_t* out) {
    ZK_REQUIRE(out, "plonk r1cs: null argument");
    const uint64_t v[ZK_PLONK_R1CS_INFO_WORDS] = {h.n_wires, h.n_public, h.n_constraints, h.origin.size(), h.n_vars - h.n_wires, h.seg_first.size(), h.max_terms, h.seg_wire.size()};
    std::memcpy(out, v, sizeof v);
}
static void plonk_r1cs_tables(const zk_plonk_r1cs_t& h, uint64_t* sel, uint32_t* a, uint32_t* b, uint32_t* c, uint32_t* origin, uint32_t* seg_first, uint64_t* seg_ptr, uint32_t* seg_wire,
                              uint64_t* seg_coef) {
    const size_t m = h.origin.size(), ns = h.seg_first.size(), nt = h.seg_wire.size();
    ZK_REQUIRE((sel && a && b && c && origin) || !m, "plonk r1cs: null gate table");
    ZK_REQUIRE(seg_ptr && ((seg_first || !ns) && ((seg_wire && seg_coef) || !nt)), "plonk r1cs: null segment table");
    uint32_t* wires[3] = {a, b, c};
    if (m) {
        for (int s = 0; s < 5; ++s) std::memcpy(sel + (size_t)s * m * 4, h.sel[s].data(), m * 32);
        for (int w = 0; w < 3; ++w) std::memcpy(wires[w], h.wire[w].data(), m * 4);
        std::memcpy(origin, h.origin.data(), m * 4);
    }
    std::memcpy(seg_ptr, h.seg_ptr.data(), (ns + 1) * 8);
    if (ns) std::memcpy(seg_first, h.seg_first.data(), ns * 4);
    if (nt) { std::memcpy(seg_wire, h.seg_wire.data(), nt * 4); std::memcpy(seg_coef, h.seg_coef.data(), nt * 32); }
}
// q_N of a handle compiled under the chain rule (plonk_next_impl.hip.h): n_gates x 4 canonical words
static void plonk_r1cs_qn(const zk_plonk_r1cs_t& h, uint64_t* qn) {
    ZK_REQUIRE(h.store_step == 2, "plonk r1cs: the handle was not compiled under the chain rule");
    ZK_REQUIRE(qn || h.sel_n.empty(), "plonk r1cs: null gate table");
    if (!h.sel_n.empty()) std::memcpy(qn, h.sel_n.data(), h.sel_n.size() * 8);
}
#define ZK_PLONK_R1CS_API(NAME, ID)                                                                                                           \
    zk_plonk_r1cs_t* zk_plonk_##NAME##_r1cs_new(const void* r1cs, size_t len) {                                                               \
        zk_plonk_r1cs_t* out = nullptr;                                                                                                       \
        guard([&] { out = curve(ID).plonk().r1cs_new(r1cs, len); });                                                                          \
        return out;                                                                                                                           \
    }                                                                                                                                         \
    zk_plonk_r1cs_t* zk_plonk_##NAME##_next_r1cs_new(const void* r1cs, size_t len) {                                                          \
        zk_plonk_r1cs_t* out = nullptr;                                                                                                       \
        guard([&] { out = curve(ID).plonk().next_r1cs_new(r1cs, len); });                                                                     \
        return out;                                                                                                                           \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_next_r1cs_qn(const zk_plonk_r1cs_t* h, uint64_t* qn) { return guard([&] { plonk_r1cs_qn(plonk_r1cs_of(h, ID), qn); }); } \
    int zk_plonk_##NAME##_r1cs_info(const zk_plonk_r1cs_t* h, uint64_t* out) { return guard([&] { plonk_r1cs_info(plonk_r1cs_of(h, ID), out); }); } \
    int zk_plonk_##NAME##_r1cs_tables(const zk_plonk_r1cs_t* h, uint64_t* sel, uint32_t* a, uint32_t* b, uint32_t* c, uint32_t* origin, uint32_t* seg_first, uint64_t* seg_ptr,  \
                                      uint32_t* seg_wire, uint64_t* seg_coef) {                                                               \
        return guard([&] { plonk_r1cs_tables(plonk_r1cs_of(h, ID), sel, a, b, c, origin, seg_first, seg_ptr, seg_wire, seg_coef); });         \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_r1cs_extend_dev(zk_plonk_r1cs_t* h, uint64_t* d_w, void* stream) {                                                  \
        return guard([&] {                                                                                                                    \
            const PlonkOps& ops = curve(ID).plonk();                                                                                          \
            (plonk_r1cs_of(h, ID).store_step == 2 ? ops.next_r1cs_extend_dev : ops.r1cs_extend_dev)(*h, (u64*)d_w, on_stream((hipStream_t)stream)); \
        });                                                                                                                                   \
    }                                                                                                                                         \
    int zk_plonk_##NAME##_r1cs_free(zk_plonk_r1cs_t* h) { return guard([&] { delete h; }); }
ZK_PLONK_R1CS_API(bn254, CURVE_BN254)
ZK_PLONK_R1CS_API(bls12_381, CURVE_BLS12_381)
#undef ZK_PLONK_R1CS_API
int zk_groth16_verify_aggregate_timing(double* ms) {
    return guard([&] { ZK_REQUIRE(ms, "groth16 verify: null argument"); groth16_verify_aggregate_timing(ms); });
}
int zk_groth16_proof_words(const zk_groth16_vk_t* vk, const char* proof_json, const char* public_input_json, void* proof_out, void* public_out) {
    int verdict = ZK_VERDICT_ERROR;
    if (guard([&] { ZK_REQUIRE(vk, "groth16 verify: null key"); verdict = groth16_proof_words(vk, proof_json, public_input_json, proof_out, public_out); }) != 0)
        return ZK_VERDICT_ERROR;
    return verdict;
}
const char* zk_groth16_verdict_name(int verdict) {
    switch (verdict) {
        case ZK_VERDICT_ACCEPTED: return "accepted";
        case ZK_VERDICT_REJECTED: return "the verification equation does not hold";
        case ZK_VERDICT_INPUT_NOT_CANONICAL: return "a public input is not below the group order";
        case ZK_VERDICT_INPUT_COUNT: return "wrong number of public inputs";
        case ZK_VERDICT_NOT_ON_CURVE: return "a proof point is not on its curve";
        case ZK_VERDICT_NOT_IN_SUBGROUP: return "a proof point is outside the subgroup of order r";
        default: return "error";
    }
}

// ---- pil_verify (pil_check.hip) ----------------------------------------------------------------------------------
struct zk_pil_check { PilCheck* impl; };
zk_pil_check_t* zk_pil_check_new(const char* pil_json) {
    zk_pil_check_t* h = nullptr;
    if (guard([&] { ZK_REQUIRE(pil_json, "zk_pil_check_new: null argument"); PilCheck* c = pil_check_new(pil_json); h = new zk_pil_check{c}; }) != 0) return nullptr;
    return h;
}
const char* zk_pil_check_listing(const zk_pil_check_t* c) { return c && c->impl ? pil_check_listing(c->impl) : nullptr; }
char* zk_pil_check_run_dev(zk_pil_check_t* c, const uint64_t* d_const_pols, const uint64_t* d_cm_pols, uint64_t n_rows, void* stream) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(c && c->impl, "pil_verify: null handle");
            out = c12_dup(pil_check_run_dev(c->impl, (const u64*)d_const_pols, (const u64*)d_cm_pols, n_rows, on_stream((hipStream_t)stream)));
        }) != 0) return nullptr;
    return out;
}
char* zk_pil_check_run(zk_pil_check_t* c, const uint64_t* const_pols, const uint64_t* cm_pols, uint64_t n_rows) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(c && c->impl, "pil_verify: null handle");
            ZK_REQUIRE(n_rows == pil_check_rows(c->impl), "pil_verify: the trace has " + std::to_string(n_rows) + " rows, the PIL's polDeg is " + std::to_string(pil_check_rows(c->impl)));
            uint32_t n_const = 0, n_cm = 0;
            pil_check_widths(c->impl, &n_const, &n_cm);
            ZK_REQUIRE((const_pols || !n_const) && (cm_pols || !n_cm), "pil_verify: null trace");
            DevBuf d_const, d_cm;
            d_const.reserve(std::max<size_t>(8, (size_t)n_rows * n_const * 8)); d_cm.reserve(std::max<size_t>(8, (size_t)n_rows * n_cm * 8));
            h2d_sync(d_const.p, const_pols, (size_t)n_rows * n_const * 8); h2d_sync(d_cm.p, cm_pols, (size_t)n_rows * n_cm * 8);
            out = c12_dup(pil_check_run_dev(c->impl, d_const.u(), d_cm.u(), n_rows, cur_stream()));
        }) != 0) return nullptr;
    return out;
}
int zk_pil_check_free(zk_pil_check_t* c) {
    return guard([&] { if (c) { pil_check_free(c->impl); delete c; } });
}

// ---- wtns_check (r1cs_check.hip) ---------------------------------------------------------------------------------
struct zk_r1cs_check { R1csCheck* impl; };
zk_r1cs_check_t* zk_r1cs_check_new(const char* field, const void* r1cs, size_t len) {
    zk_r1cs_check_t* h = nullptr;
    if (guard([&] { R1csCheck* c = r1cs_check_new(field, r1cs, len); h = new zk_r1cs_check{c}; }) != 0) return nullptr;
    return h;
}
int zk_r1cs_check_info(const zk_r1cs_check_t* c, uint32_t* n_wires, uint64_t* n_constraints, uint64_t* n_custom_uses, uint32_t* n_public) {
    return guard([&] { ZK_REQUIRE(c && c->impl, "r1cs check: null handle"); r1cs_check_info(c->impl, n_wires, n_constraints, n_custom_uses, n_public); });
}
static char* r1cs_check_run_any(zk_r1cs_check_t* c, const void* witness, bool on_device, uint64_t n_values, uint32_t max_findings) {
    char* out = nullptr;
    if (guard([&] {
            ZK_REQUIRE(c && c->impl, "r1cs check: null handle");
            ZK_REQUIRE(witness, "r1cs check: null witness");
            uint32_t n_wires = 0;
            r1cs_check_info(c->impl, &n_wires, nullptr, nullptr, nullptr);
            ZK_REQUIRE(n_values == n_wires, "r1cs check: the witness has " + std::to_string(n_values) + " values, the circuit has " + std::to_string(n_wires) + " wires");
            if (on_device) { out = c12_dup(r1cs_check_run_dev(c->impl, witness, max_findings, cur_stream())); return; }
            const size_t vb = r1cs_check_value_bytes(c->impl);
            for (uint64_t i = 0; i < n_values; ++i)
                ZK_REQUIRE(r1cs_check_value_canonical(c->impl, (const uint8_t*)witness + i * vb), "groth16: witness value " + std::to_string(i) + " is not a canonical field element");
            DevBuf d_wit;
            d_wit.reserve((size_t)n_values * vb);
            h2d_sync(d_wit.p, witness, (size_t)n_values * vb);
            out = c12_dup(r1cs_check_run_dev(c->impl, d_wit.p, max_findings, cur_stream()));
        }) != 0) return nullptr;
    return out;
}
char* zk_r1cs_check_run(zk_r1cs_check_t* c, const void* witness, uint64_t n_values, uint32_t max_findings) {
    return r1cs_check_run_any(c, witness, false, n_values, max_findings);
}
char* zk_r1cs_check_run_dev(zk_r1cs_check_t* c, const void* d_witness, uint64_t n_values, uint32_t max_findings) {
    return r1cs_check_run_any(c, d_witness, true, n_values, max_findings);
}
int zk_r1cs_check_free(zk_r1cs_check_t* c) {
    return guard([&] { if (c) { r1cs_check_free(c->impl); delete c; } });
}

}  // extern "C"
