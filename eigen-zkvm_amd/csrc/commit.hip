// The Merkle trees and transcripts of the three verificationHashTypes (commit.h): the field table of the two scalar fields with
// its host arithmetic, the gather kernels of the openings, and the two implementations of Tree and Transcript.
#include "commit.h"
#include <algorithm>
#include <cstring>

namespace zk {
namespace {

// one opening by one block: the row, then thread 0 walks up the tree and copies the sibling of every level
__device__ __forceinline__ void gather_proof(const u64* __restrict__ elements, const u64* __restrict__ nodes, u32 width,
                                             u64 height, u64 idx, u64* __restrict__ out /* width + depth*4 */) {
    const u32 t = threadIdx.x;
    for (u32 i = t; i < width; i += blockDim.x) out[i] = elements[idx * width + i];
    if (t == 0) {  // merklehash.rs:64-76 merkle_gen_merkle_proof
        u64 n = height, off = 0, id = idx; u32 d = 0;
        while (n > 1) {
            const u64* sib = nodes + 4 * (off + (id ^ 1));
            for (int k = 0; k < 4; ++k) out[width + 4 * d + k] = sib[k];
            u64 next = (n - 1) / 2 + 1;
            off += next * 2; n = next; id >>= 1; ++d;
        }
    }
}
__global__ void gather_proof_kernel(const u64* __restrict__ elements, const u64* __restrict__ nodes, u32 width,
                                    u64 height, u64 idx, u64* __restrict__ out) {
    gather_proof(elements, nodes, width, height, idx, out);
}
// the same for n queries at once: block q serves idx[q], out + q * (width + 4 * depth)
__global__ void gather_proofs_kernel(const u64* __restrict__ elements, const u64* __restrict__ nodes, u32 width, u64 height,
                                     u32 depth, const u64* __restrict__ idxs, u64* __restrict__ outs, u64 mask) {
    const u64 idx = idxs[blockIdx.x] & mask;             // mask: the query index reduced to a later FRI step's domain (fri.rs:166-168)
    gather_proof(elements, nodes, width, height, idx, outs + (u64)blockIdx.x * (width + 4 * depth));
}
// every tree of a proof in ONE launch: block (q, j) serves query q of tree j (a small proof opened its seven or eight trees in as many
// launches of ~5 us each); lane d copies the sibling of level d
struct GatherMulti { const u64* elements[16]; const u64* nodes[16]; u64* out[16]; u64 height[16], mask[16]; u32 width[16], depth[16]; };
__global__ void gather_proofs_multi_kernel(const GatherMulti G, const u64* __restrict__ idxs) {
    const u32 t = threadIdx.x, j = blockIdx.y;
    const u32 width = G.width[j], depth = G.depth[j];
    const u64 idx = idxs[blockIdx.x] & G.mask[j];
    const u64* __restrict__ elements = G.elements[j];
    const u64* __restrict__ nodes = G.nodes[j];
    u64* __restrict__ out = G.out[j] + (u64)blockIdx.x * (width + 4 * depth);
    for (u32 i = t; i < width; i += blockDim.x) out[i] = elements[idx * width + i];
    for (u32 d = t; d < depth; d += blockDim.x) {
        u64 n = G.height[j], off = 0;
        for (u32 k = 0; k < d; ++k) { const u64 next = (n - 1) / 2 + 1; off += next * 2; n = next; }
        const u64* sib = nodes + 4 * (off + ((idx >> d) ^ 1));
        for (int k = 0; k < 4; ++k) out[width + 4 * d + k] = sib[k];
    }
}
// arity-16 trees of the scalar-field hashes (merklehash_bn128.rs:86-106): block q -> row + depth groups of 16 digests
__global__ void fr_gather_proofs_kernel(const u64* __restrict__ elements, const u64* __restrict__ nodes, u32 width, u64 height,
                                        u32 depth, const u64* __restrict__ idxs, u64* __restrict__ outs) {
    const u32 t = threadIdx.x;
    const u64 idx = idxs[blockIdx.x];
    u64* __restrict__ out = outs + (u64)blockIdx.x * (width + 64 * depth);
    for (u32 i = t; i < width; i += blockDim.x) out[i] = elements[idx * width + i];
    u64 n = height, off = 0, id = idx; u32 d = 0;
    while (n > 1) {
        const u64 si = id & ~(u64)15;
        if (t < 64) out[width + 64 * d + t] = nodes[4 * (off + si) + t];
        const u64 next = (n - 1) / 16 + 1;
        off += next * 16; n = next; id >>= 4; ++d;
    }
}

uint32_t tree_depth(uint64_t height, uint32_t arity) {
    uint32_t d = 0;
    for (uint64_t n = height; n > 1; n = (n - 1) / arity + 1) ++d;
    return d;
}
// n openings of `per` words each, as the gather kernels lay them out, into the caller's rows and paths
void split_openings(const u64* h, uint32_t n, size_t per, uint32_t width, u64* rows_out, u64* paths_out) {
    for (uint32_t q = 0; q < n; ++q) {
        memcpy(rows_out + (size_t)q * width, h + q * per, (size_t)width * 8);
        if (per > width) memcpy(paths_out + (size_t)q * (per - width), h + q * per + width, (per - width) * 8);
    }
}

const FrField FR_BN128 = {"bn128",
    {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL},
    {1997599621687373223ULL, 6052339484930628067ULL, 10108755138030829701ULL, 150537098327114917ULL}, 0xc2e1f593efffffffULL, 0,
    bn128_load_constants, bn128_tables_selfcheck, bn128_poseidon_dev, bn128_merkle_n_nodes, bn128_linearhash_rows_dev, bn128_merkelize_dev};
const FrField FR_BLS12381 = {"bls12381",
    {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL},
    {14526898881837571181ULL, 3129137299524312099ULL, 419701826671360399ULL, 524908885293268753ULL}, 0xfffffffeffffffffULL, 1,
    bls12381_load_constants, bls12381_tables_selfcheck, bls12381_poseidon_dev, bls12381_merkle_n_nodes, bls12381_linearhash_rows_dev, bls12381_merkelize_dev};

}  // namespace

// ---- the hash types and the scalar fields' host arithmetic ----------------------------------------
HashType hash_type_of(const std::string& s) {
    ZK_REQUIRE(s == "GL" || s == "BN128" || s == "BLS12381", "verificationHashType must be GL, BN128 or BLS12381");
    return s == "GL" ? HASH_GL : s == "BN128" ? HASH_BN128 : HASH_BLS12381;
}
const FrField* fr_field(HashType h) { return h == HASH_BN128 ? &FR_BN128 : h == HASH_BLS12381 ? &FR_BLS12381 : nullptr; }

void FrField::mont_mul(const u64 a[4], const u64 b[4], u64 r[4]) const {   // CIOS
    typedef unsigned __int128 u128;
    u64 t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        u128 c = 0;
        for (int j = 0; j < 4; ++j) { c += (u128)a[j] * b[i] + t[j]; t[j] = (u64)c; c >>= 64; }
        c += t[4]; t[4] = (u64)c; t[5] = (u64)(c >> 64);
        const u64 m = t[0] * INV;
        c = ((u128)m * R[0] + t[0]) >> 64;
        for (int j = 1; j < 4; ++j) { c += (u128)m * R[j] + t[j]; t[j - 1] = (u64)c; c >>= 64; }
        c += t[4]; t[3] = (u64)c; t[4] = t[5] + (u64)(c >> 64);
    }
    for (;;) {
        bool ge = t[4] != 0;
        if (!ge) { ge = true; for (int i = 3; i >= 0; --i) { if (t[i] > R[i]) break; if (t[i] < R[i]) { ge = false; break; } } }
        if (!ge) break;
        u128 br = 0;
        for (int i = 0; i < 4; ++i) { u128 d = (u128)t[i] - R[i] - br; t[i] = (u64)d; br = (d >> 64) & 1; }
        t[4] -= (u64)br;
    }
    memcpy(r, t, 32);
}
std::string FrField::to_dec(const u64 raw[4]) const {     // helper::fr_to_biguint: the canonical value, by repeated division by 10^18
    typedef unsigned __int128 u128;
    u64 v[4];
    canonical(raw, v);
    std::string out;
    while (v[0] | v[1] | v[2] | v[3]) {
        u128 rem = 0;
        for (int i = 3; i >= 0; --i) { u128 cur = (rem << 64) | v[i]; v[i] = (u64)(cur / 1000000000000000000ULL); rem = cur % 1000000000000000000ULL; }
        std::string chunk = std::to_string((u64)rem);
        if (v[0] | v[1] | v[2] | v[3]) chunk = std::string(18 - chunk.size(), '0') + chunk;
        out = chunk + out;
    }
    return out.empty() ? "0" : out;
}
bool FrField::from_dec(const std::string& dec, u64 raw[4]) const {
    if (dec.empty() || dec.size() > 78) return false;
    u64 v[4] = {0, 0, 0, 0};
    for (char c : dec) {
        if (c < '0' || c > '9') return false;
        unsigned __int128 carry = (unsigned)(c - '0');
        for (int i = 0; i < 4; ++i) { carry += (unsigned __int128)v[i] * 10; v[i] = (u64)carry; carry >>= 64; }
        if (carry) return false;
    }
    for (int i = 3; i >= 0; --i) { if (v[i] < R[i]) break; if (v[i] > R[i] || i == 0) return false; }
    to_mont(v, raw);
    return true;
}

// ---- trees ------------------------------------------------------------------------------------------
void Tree::build_dev(const u64* d_rows, uint32_t w, uint64_t h, hipStream_t st) {
    KeepStream keep;
    d_elements = d_rows; width = w; height = h; stream = on_stream(st);
    merkelize(st);
}
void Tree::build_host(const u64* rows, uint32_t w, uint64_t h) {
    KeepStream keep;
    on_stream(nullptr);
    const size_t bytes = (size_t)w * h * sizeof(u64);
    owned_elements.reserve(bytes ? bytes : 8);
    if (bytes) ZK_HIP(hipMemcpy(owned_elements.p, rows, bytes, hipMemcpyHostToDevice));
    d_elements = owned_elements.u(); width = w; height = h; stream = nullptr;
    merkelize(nullptr);
    ZK_HIP(hipStreamSynchronize(nullptr));
}
std::unique_ptr<Tree> build_tree(HashType h, const u64* d_rows, uint32_t w, uint64_t height, hipStream_t st) {
    std::unique_ptr<Tree> t(h == HASH_GL ? (Tree*)new zk_merkle : new FrTree(h));
    t->build_dev(d_rows, w, height, st);
    return t;
}

void GlTree::merkelize(hipStream_t st) {
    n_nodes = merkle_n_nodes(height); depth = tree_depth(height, 2);
    nodes.reserve(n_nodes * 32);
    proof.reserve(((size_t)width + 4 * (size_t)depth + 4) * sizeof(u64));
    merkelize_dev(d_elements, width, height, nodes.u(), st);
}
void GlTree::root(u64 out[4]) const {
    ZK_HIP(hipStreamSynchronize(stream));
    ZK_HIP(hipMemcpy(out, root_dev(), 32, hipMemcpyDeviceToHost));
}
void GlTree::nodes_host(u64* out) const {
    ZK_HIP(hipStreamSynchronize(stream));
    ZK_HIP(hipMemcpy(out, nodes.p, n_nodes * 32, hipMemcpyDeviceToHost));
}
void GlTree::elements_host(u64* out) const {
    ZK_HIP(hipStreamSynchronize(stream));
    ZK_HIP(hipMemcpy(out, d_elements, (size_t)height * width * 8, hipMemcpyDeviceToHost));
}
void GlTree::group_proof(u64 idx, u64* row_out, u64* path_out) const {
    ZK_REQUIRE(idx < height, "MerkleTreeError: access invalid node");  // merklehash.rs:431-433
    hipLaunchKernelGGL(gather_proof_kernel, dim3(1), dim3(64), 0, stream, d_elements, nodes.u(), width, height, idx, proof.u());
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(stream));
    ZK_HIP(hipMemcpy(row_out, proof.p, width * sizeof(u64), hipMemcpyDeviceToHost));
    if (depth) ZK_HIP(hipMemcpy(path_out, proof.u() + width, (size_t)depth * 32, hipMemcpyDeviceToHost));
}
void GlTree::group_proofs(const u64* idx, uint32_t n, u64* rows_out, u64* paths_out) const {
    if (n == 0) return;
    for (uint32_t q = 0; q < n; ++q) ZK_REQUIRE(idx[q] < height, "MerkleTreeError: access invalid node");
    const size_t per = (size_t)width + 4 * (size_t)depth;
    KeepStream keep;
    on_stream(stream);
    DevBuf d_idx, d_out; d_idx.reserve(n * 8); d_out.reserve(std::max<size_t>(1, per * n) * 8);
    ZK_HIP(hipMemcpyAsync(d_idx.p, idx, n * 8, hipMemcpyHostToDevice, stream));
    open_async(d_idx.u(), ~0ull, n, d_out.u(), stream);
    std::vector<u64> h(std::max<size_t>(1, per * n));
    ZK_HIP(hipMemcpyAsync(h.data(), d_out.p, per * n * 8, hipMemcpyDeviceToHost, stream));
    ZK_HIP(hipStreamSynchronize(stream));
    split_openings(h.data(), n, per, width, rows_out, paths_out);
}
void GlTree::open_async(const u64* d_idx, u64 mask, uint32_t n, u64* d_out, hipStream_t st) const {
    if (n == 0) return;
    ZK_REQUIRE(mask == ~0ull || mask < height, "MerkleTreeError: access invalid node");   // ~0: the caller has range-checked the indices
    hipLaunchKernelGGL(gather_proofs_kernel, dim3(n), dim3(64), 0, st, d_elements, nodes.u(), width, height, depth, d_idx, d_out, mask);
    ZK_HIP(hipGetLastError());
}
void GlTree::open_multi_async(const GlTree* const* trees, const u64* masks, u64* const* d_outs, uint32_t n_trees, const u64* d_idx, uint32_t n, hipStream_t st) {
    if (n == 0 || n_trees == 0) return;
    for (uint32_t j0 = 0; j0 < n_trees; j0 += 16) {
        GatherMulti G; memset(&G, 0, sizeof G);
        const uint32_t m = std::min<uint32_t>(16, n_trees - j0);
        for (uint32_t j = 0; j < m; ++j) {
            const GlTree* t = trees[j0 + j];
            ZK_REQUIRE(masks[j0 + j] < t->height, "MerkleTreeError: access invalid node");
            G.elements[j] = t->d_elements; G.nodes[j] = t->nodes.u(); G.out[j] = d_outs[j0 + j];
            G.height[j] = t->height; G.mask[j] = masks[j0 + j]; G.width[j] = t->width; G.depth[j] = t->depth;
        }
        hipLaunchKernelGGL(gather_proofs_multi_kernel, dim3(n, m), dim3(64), 0, st, G, d_idx);
        ZK_HIP(hipGetLastError());
    }
}

// A scalar-field tree is read after a wait for the whole device, not for `stream`: its openings read the caller's rows, whose producer
// may have run on any stream, and are gathered on the null stream, which a non-blocking stream does not order itself against.  A wait
// for `stream` alone would not give the same ordering.
void FrTree::merkelize(hipStream_t st) {
    n_nodes = F.n_nodes(height); depth = tree_depth(height, 16);
    nodes.reserve(n_nodes * 32);
    F.merkelize_dev(d_elements, width, height, nodes.u(), st);
}
void FrTree::root(u64 out[4]) const {
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, nodes.u() + 4 * (n_nodes - 1), 32, hipMemcpyDeviceToHost));
}
void FrTree::nodes_host(u64* out) const {
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, nodes.p, n_nodes * 32, hipMemcpyDeviceToHost));
}
void FrTree::group_proof(u64 idx, u64* row_out, u64* path_out) const {   // get_group_proof (merklehash_bn128.rs:246-254)
    ZK_REQUIRE(idx < height, "MerkleTreeError: access invalid node");
    ZK_HIP(hipDeviceSynchronize());
    if (width) ZK_HIP(hipMemcpy(row_out, d_elements + idx * width, width * 8, hipMemcpyDeviceToHost));
    uint64_t n = height, off = 0, id = idx; uint32_t d = 0;
    while (n > 1) {   // merklehash_bn128.rs:86-106
        const uint64_t si = id & ~(uint64_t)15;
        ZK_HIP(hipMemcpy(path_out + (size_t)d * 64, nodes.u() + 4 * (off + si), 16 * 32, hipMemcpyDeviceToHost));
        const uint64_t next = (n - 1) / 16 + 1;
        off += next * 16; n = next; id >>= 4; ++d;
    }
}
void FrTree::group_proofs(const u64* idx, uint32_t n, u64* rows_out, u64* paths_out) const {
    if (n == 0) return;
    for (uint32_t q = 0; q < n; ++q) ZK_REQUIRE(idx[q] < height, "MerkleTreeError: access invalid node");
    ZK_HIP(hipDeviceSynchronize());
    KeepStream keep;
    on_stream(nullptr);
    const size_t per = (size_t)width + 64 * (size_t)depth;
    DevBuf d_idx, d_out; d_idx.reserve(n * 8); d_out.reserve(std::max<size_t>(1, per * n) * 8);
    ZK_HIP(hipMemcpy(d_idx.p, idx, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(fr_gather_proofs_kernel, dim3(n), dim3(64), 0, nullptr, d_elements, nodes.u(), width, height, depth, d_idx.u(), d_out.u());
    ZK_HIP(hipGetLastError());
    std::vector<u64> h(std::max<size_t>(1, per * n));
    ZK_HIP(hipMemcpy(h.data(), d_out.p, per * n * 8, hipMemcpyDeviceToHost));
    split_openings(h.data(), n, per, width, rows_out, paths_out);
}

// ---- transcripts -------------------------------------------------------------------------------------
std::unique_ptr<Transcript> new_transcript(HashType h) {
    if (h == HASH_GL) return std::unique_ptr<Transcript>(new zk_transcript);
    return std::unique_ptr<Transcript>(new FrTranscript(h));
}
GlTranscript::GlTranscript() : stream(cur_stream()) {                      // the caller's (a prover's own stream, or the null stream)
    state.reserve(transcript_state_bytes());
    io.reserve(4096 * sizeof(u64));
    transcript_init_dev(state.p, stream);
}
// the sponge state lives on one stream at a time: work moves to `st` after whatever was issued on the previous stream
hipStream_t GlTranscript::move_to(hipStream_t st) {
    if (stream != st) { ZK_HIP(hipStreamSynchronize(stream)); stream = st; }
    return st;
}
void GlTranscript::put_dev(const u64* d_src, size_t n, hipStream_t st) { KeepStream keep; transcript_put_dev(state.p, d_src, n, on_stream(move_to(st))); }
void GlTranscript::get_dev(u64* d_out, uint32_t n_words, hipStream_t st) { KeepStream keep; transcript_get_dev(state.p, d_out, n_words, on_stream(move_to(st))); }
void GlTranscript::put_get_async(const u64* d_src, uint64_t n_put, u64* d_dst, uint32_t n_get, uint32_t bits, hipStream_t st) {
    transcript_put_get_dev(state.p, d_src, n_put, d_dst, n_get, bits, move_to(st));
}
void GlTranscript::put_words(const u64* w, size_t n) {
    if (n == 0) return;
    KeepStream keep;
    on_stream(stream);
    io.reserve(n * sizeof(u64));
    ZK_HIP(hipStreamSynchronize(stream));                                 // io may still be read by an earlier put
    ZK_HIP(hipMemcpy(io.p, w, n * sizeof(u64), hipMemcpyHostToDevice));
    transcript_put_dev(state.p, io.u(), n, stream);
    ZK_HIP(hipStreamSynchronize(stream));
}
void GlTranscript::get(u64* out, uint32_t n_words) {
    KeepStream keep;
    transcript_get_dev(state.p, io.u(), n_words, on_stream(stream));
    ZK_HIP(hipStreamSynchronize(stream));
    ZK_HIP(hipMemcpy(out, io.p, n_words * sizeof(u64), hipMemcpyDeviceToHost));
}
void GlTranscript::get_permutations(uint32_t n, uint32_t nbits, u64* out) {   // transcript.rs:73-102
    KeepStream keep;
    on_stream(stream);
    io.reserve((size_t)n * sizeof(u64) + 64);
    transcript_permutations_dev(state.p, n, nbits, io.u(), stream);
    ZK_HIP(hipStreamSynchronize(stream));
    ZK_HIP(hipMemcpy(out, io.p, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost));
}

void FrTranscript::update() {   // transcript_bn128.rs:22-31
    pending.resize(64, 0);
    on_stream(nullptr);                         // the scalar-field sponges work on the null stream, whoever calls (the public methods put the caller's back)
    d_in.reserve(64 * 8); d_init.reserve(32); d_out.reserve(17 * 32);
    ZK_HIP(hipMemcpy(d_in.p, pending.data(), 64 * 8, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(d_init.p, state, 32, hipMemcpyHostToDevice));
    F.poseidon_dev(d_in.u(), 1, 16, d_init.u(), 17, d_out.u(), nullptr);
    out.resize(68);
    ZK_HIP(hipStreamSynchronize(nullptr));
    ZK_HIP(hipMemcpy(out.data(), d_out.p, 17 * 32, hipMemcpyDeviceToHost));
    out_pos = 0; n_out = 17; n_out3 = 0; out3_pos = 0; pending.clear();
    memcpy(state, out.data(), 32);
}
void FrTranscript::add1(const u64 raw[4]) {   // :32-40
    n_out = 0; out_pos = 0;
    pending.insert(pending.end(), raw, raw + 4);
    if (pending.size() == 64) update();
}
void FrTranscript::get253(u64 canon[4]) {   // :42-48, canonical value of the popped element
    if (out_pos >= n_out) update();
    F.canonical(out.data() + 4 * out_pos, canon);
    ++out_pos;
}
void FrTranscript::put_words(const u64* w, size_t n) {   // :90-101, a Goldilocks value is one element
    KeepStream keep;
    for (size_t i = 0; i < n; ++i) {
        const u64 x[4] = {w[i], 0, 0, 0}; u64 m[4];
        F.to_mont(x, m);
        add1(m);
    }
}
void FrTranscript::get(u64* o, uint32_t n_words) {   // get_fields1 (:71-88), n_words times
    KeepStream keep;
    for (uint32_t k = 0; k < n_words;) {
        if (out3_pos < n_out3) { o[k++] = out3[out3_pos++]; continue; }
        if (out_pos < n_out) {
            u64 c[4];
            get253(c);
            for (int i = 0; i < 3; ++i) out3[i] = c[i] % GL_P;   // biguint_to_be (helper.rs:61-65)
            out3_pos = 0; n_out3 = 3;
            continue;
        }
        update();
    }
}
void FrTranscript::get_permutations(uint32_t n, uint32_t nbits, u64* o) {   // :103-131
    ZK_REQUIRE(n >= 1 && nbits >= 1 && nbits <= 63, "bad argument");
    KeepStream keep;
    const uint32_t total = n * nbits, nf = (total - 1) / 253 + 1;
    std::vector<u64> f(4 * (size_t)nf);
    for (uint32_t i = 0; i < nf; ++i) get253(f.data() + 4 * i);
    uint32_t cf = 0, cb = 0;
    for (uint32_t i = 0; i < n; ++i) {
        u64 a = 0;
        for (uint32_t j = 0; j < nbits; ++j) {
            if ((f[4 * cf + cb / 64] >> (cb % 64)) & 1) a += (u64)1 << j;
            if (++cb == 253) { cb = 0; ++cf; }
        }
        o[i] = a;
    }
}

}  // namespace zk
