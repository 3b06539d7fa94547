// Commitments (commit.hip): the Merkle trees and Fiat-Shamir transcripts of the three verificationHashTypes behind one interface.
// The C ABI (capi.hip), the prover (stark_prover.hip) and the verifier (stark_verify.hip) all work on these types; the opaque
// handles of include/zkgpu.h ARE these types (bottom of this file).  Methods throw zk::Error.  A method that moves the calling
// thread to another stream (the scalar-field code works on the null stream, whoever calls) puts the thread's stream back.
#pragma once
#include "zk_internal.h"
#include <memory>

namespace zk {

enum HashType { HASH_GL, HASH_BN128, HASH_BLS12381 };
HashType hash_type_of(const std::string& verification_hash_type);   // "GL" | "BN128" | "BLS12381", anything else throws

// One scalar field: the device entry points of frhash.hip / frhash_bls12381.hip and the host-side arithmetic on its elements.
// An element (a digest, ElementDigest<4, Fr>) is the 4 raw limbs of its Montgomery form, R = 2^256.
struct FrField {
    const char* name;
    u64 R[4], R2[4], INV;          // modulus, 2^512 mod r, -r^-1 mod 2^64
    uint32_t hash_word;            // Poseidon::hash is this word of the permutation (poseidon_bn128_opt.rs:80-83, poseidon_bls12381_opt.rs:94-103)
    void (*load)(const char*);
    std::string (*selfcheck)(const char*);
    void (*poseidon_dev)(const u64*, uint64_t, uint32_t, const u64*, uint32_t, u64*, hipStream_t);
    uint64_t (*n_nodes)(uint64_t);
    void (*linearhash_rows_dev)(const u64*, uint32_t, uint64_t, u64*, hipStream_t);
    void (*merkelize_dev)(const u64*, uint32_t, uint64_t, u64*, hipStream_t);
    void mont_mul(const u64 a[4], const u64 b[4], u64 r[4]) const;         // a b / 2^256 mod r, canonical (< r)
    void to_mont(const u64 v[4], u64 raw[4]) const { mont_mul(v, R2, raw); }
    void canonical(const u64 raw[4], u64 v[4]) const { const u64 one[4] = {1, 0, 0, 0}; mont_mul(raw, one, v); }
    std::string to_dec(const u64 raw[4]) const;                            // how a digest travels in zkin JSON (digest.rs:91-94)
    bool from_dec(const std::string& dec, u64 raw[4]) const;               // false: not a canonical value below the modulus
};
const FrField* fr_field(HashType h);                                       // nullptr for HASH_GL

struct KeepStream {   // the calling thread's current stream, put back at the end of the scope
    hipStream_t saved = cur_stream();
    KeepStream() = default; KeepStream(const KeepStream&) = delete; KeepStream& operator=(const KeepStream&) = delete;
    ~KeepStream() { on_stream(saved); }
};

// ---- Merkle trees over a row-major [height][width] matrix of Goldilocks words ----
struct GlTree;
struct Tree {
    const u64* d_elements = nullptr;   // the rows, in device memory: borrowed (build_dev) or owned_elements (build_host)
    DevBuf owned_elements, nodes;      // nodes: n_nodes digests of 4 words, the root last
    uint32_t width = 0, depth = 0;
    uint64_t height = 0, n_nodes = 0;
    hipStream_t stream = nullptr;      // the stream the tree was built on
    Tree() = default; Tree(const Tree&) = delete; Tree& operator=(const Tree&) = delete;
    virtual ~Tree() {}
    void build_dev(const u64* d_rows, uint32_t w, uint64_t h, hipStream_t st);   // asynchronous on st; the rows stay the caller's
    void build_host(const u64* rows, uint32_t w, uint64_t h);                    // null stream; built when it returns
    virtual uint32_t level_words() const = 0;                       // words of one path level: a sibling digest (4), or the 16 digests of a group (64)
    virtual const GlTree* gl() const { return nullptr; }            // the trees whose openings can stay in device memory
    virtual void root(u64 out[4]) const = 0;                        // to host memory, as the three below
    virtual void nodes_host(u64* out) const = 0;
    virtual void group_proof(u64 idx, u64* row_out, u64* path_out) const = 0;    // row_out[width], path_out[depth][level_words]
    virtual void group_proofs(const u64* idx, uint32_t n, u64* rows_out, u64* paths_out) const = 0;   // n of them, one round trip
protected:
    virtual void merkelize(hipStream_t st) = 0;                     // sizes n_nodes / depth / nodes and queues the hashing
};
struct GlTree : Tree {                 // MerkleTreeGL (merklehash.rs): binary, Poseidon over Goldilocks
    DevBuf proof;                      // staging of group_proof
    uint32_t level_words() const override { return 4; }
    const GlTree* gl() const override { return this; }
    const u64* root_dev() const { return nodes.u() + 4 * (n_nodes - 1); }   // last node (merklehash.rs:455-457)
    void root(u64 out[4]) const override;
    void nodes_host(u64* out) const override;
    void elements_host(u64* out) const;
    void group_proof(u64 idx, u64* row_out, u64* path_out) const override;
    void group_proofs(const u64* idx, uint32_t n, u64* rows_out, u64* paths_out) const override;
    // openings at n device-resident indices d_idx[q] & mask (mask + 1 = a power of two <= height: the query index reduced to a later
    // FRI step's domain, fri.rs:166-168) into device memory, n x (width + 4 depth) words, on st: no host round trip
    void open_async(const u64* d_idx, u64 mask, uint32_t n, u64* d_out, hipStream_t st) const;
    // the same for several trees in one launch per 16 of them: tree j at d_idx[q] & masks[j] into d_outs[j]
    static void open_multi_async(const GlTree* const* trees, const u64* masks, u64* const* d_outs, uint32_t n_trees, const u64* d_idx, uint32_t n, hipStream_t st);
protected:
    void merkelize(hipStream_t st) override;
};
struct FrTree : Tree {                 // MerkleTreeBN128 / MerkleTreeBLS12381 (merklehash_bn128.rs): arity 16 over a scalar field
    const FrField& F;
    explicit FrTree(HashType h) : F(*fr_field(h)) {}
    uint32_t level_words() const override { return 64; }
    void root(u64 out[4]) const override;
    void nodes_host(u64* out) const override;
    void group_proof(u64 idx, u64* row_out, u64* path_out) const override;
    void group_proofs(const u64* idx, uint32_t n, u64* rows_out, u64* paths_out) const override;
protected:
    void merkelize(hipStream_t st) override;
};
// the tree of hash type h over device rows, as build_dev (a GL tree is made as a zk_merkle: zk_stark_tree() hands it out as one)
std::unique_ptr<Tree> build_tree(HashType h, const u64* d_rows, uint32_t w, uint64_t height, hipStream_t st);

// ---- transcripts (transcript.rs, transcript_bn128.rs) ----
struct GlTranscript;
struct Transcript {
    Transcript() = default; Transcript(const Transcript&) = delete; Transcript& operator=(const Transcript&) = delete;
    virtual ~Transcript() {}
    virtual GlTranscript* gl() { return nullptr; }                  // the sponge that lives in device memory
    virtual void put_words(const u64* w, size_t n) = 0;             // n Goldilocks words of host memory, one transcript element each
    virtual void put_digest(const u64 d[4]) = 0;                    // a root: four elements of the GL sponge, ONE of a scalar-field sponge
    virtual void get(u64* out, uint32_t n_words) = 0;               // get_field is 3 words, get_fields1 is 1
    virtual void get_permutations(uint32_t n, uint32_t nbits, u64* out) = 0;
};
struct GlTranscript : Transcript {     // TranscriptGL, the state in device memory (poseidon.hip)
    DevBuf state, io;                  // io: staging of the host-word calls
    hipStream_t stream;                // where the state was last worked on: the host-word calls continue (and wait) there
    GlTranscript();                    // on the calling thread's current stream
    GlTranscript* gl() override { return this; }
    void put_words(const u64* w, size_t n) override;
    void put_digest(const u64 d[4]) override { put_words(d, 4); }
    void get(u64* out, uint32_t n_words) override;
    void get_permutations(uint32_t n, uint32_t nbits, u64* out) override;
    // device pointers, asynchronous on st (the state moves there after whatever was queued on its previous stream)
    void put_dev(const u64* d_src, size_t n, hipStream_t st);
    void get_dev(u64* d_out, uint32_t n_words, hipStream_t st);
    // put d_src[0..n_put) and squeeze n_get words (bits == 0) or n_get indices of `bits` bits, one launch
    void put_get_async(const u64* d_src, uint64_t n_put, u64* d_dst, uint32_t n_get, uint32_t bits, hipStream_t st);
private:
    hipStream_t move_to(hipStream_t st);
};
struct FrTranscript : Transcript {     // transcript_bn128.rs:14-20: sponge bookkeeping on the host, permutations on the device (null stream)
    const FrField& F;
    explicit FrTranscript(HashType h) : F(*fr_field(h)) {}
    void put_words(const u64* w, size_t n) override;
    void put_digest(const u64 d[4]) override { KeepStream keep; add1(d); }
    void get(u64* out, uint32_t n_words) override;
    void get_permutations(uint32_t n, uint32_t nbits, u64* out) override;
private:
    u64 state[4] = {0, 0, 0, 0};
    std::vector<u64> pending, out;     // raw limbs, 4 per element: absorbed and not yet permuted; the 17 squeezed elements
    size_t out_pos = 0, n_out = 0;
    u64 out3[3] = {0, 0, 0}; size_t out3_pos = 0, n_out3 = 0;
    DevBuf d_in, d_init, d_out;
    void update();
    void add1(const u64 raw[4]);
    void get253(u64 canon[4]);
};
std::unique_ptr<Transcript> new_transcript(HashType h);

}  // namespace zk

// the opaque handles of include/zkgpu.h
struct zk_merkle : zk::GlTree {};
struct zk_transcript : zk::GlTranscript {};
struct zk_bn128_merkle : zk::FrTree { zk_bn128_merkle() : FrTree(zk::HASH_BN128) {} };
struct zk_bn128_transcript : zk::FrTranscript { zk_bn128_transcript() : FrTranscript(zk::HASH_BN128) {} };
struct zk_bls12381_merkle : zk::FrTree { zk_bls12381_merkle() : FrTree(zk::HASH_BLS12381) {} };
struct zk_bls12381_transcript : zk::FrTranscript { zk_bls12381_transcript() : FrTranscript(zk::HASH_BLS12381) {} };
