/* libzkgpu -- C ABI of the MI355X (gfx950) prover backend for eigen-zkvm's starky hot path.
 *
 * Each entry point stands behind one Rust seam of the reference (there is no FFI on this path in
 * the reference; the seams are traits / free functions -- SURVEY.md section 8b).  The binding a
 * maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - field elements: canonical Goldilocks u64 (value < p = 2^64 - 2^32 + 1), little-endian, the
 *     same words the reference reads/writes in .cm/.const files (polsarray.rs:137-217) and
 *     obtains from Fr::as_int() (fields/src/field_gl.rs:542-544).
 *   - matrices: row-major [rows][cols], like the reference's buffers (polsarray.rs:219-227).
 *   - status: 0 = ok, nonzero = error; zk_last_error() returns the message for the calling
 *     thread (reference: anyhow::Result / panic).  Pointer-returning calls return NULL on error.
 *   - `*_dev` variants take DEVICE pointers (HBM-resident data) and a hipStream_t passed as
 *     void*; they enqueue work and return without synchronising.  The plain variants take HOST
 *     pointers, copy in/out and synchronise (drop-in for the reference's Vec<FGL> arguments).
 *   - a process drives one GPU, the one zk_init names: every host thread that calls into the library afterwards is
 *     bound to it on its first call (HIP's current device is per thread and a new thread starts on device 0).
 *     Without zk_init the threads stay on whatever device the caller gave them.  Handles are not re-entrant.
 */
#ifndef ZKGPU_H
#define ZKGPU_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ---------------------------------------------------------------------------- */
int zk_init(int device);            /* select the GPU this process, all its threads, proves on  */
const char* zk_last_error(void);    /* message of the last failing call on this thread        */
int zk_device_count(void);          /* number of visible GPUs, <= 0 when none                  */
uint64_t zk_gl_modulus(void);       /* 0xFFFFFFFF00000001 (fields/src/field_gl.rs:12)          */
uint64_t zk_gl_root_of_unity(uint32_t k); /* MG.0[k] (starky/src/constant.rs:54-68), k <= 32   */

/* device memory helpers for callers that keep traces resident in HBM.  Blocks are cached by size
 * (a prover re-allocates the same multi-GB sections for every proof); zk_dev_trim returns the cache. */
void* zk_dev_alloc(size_t bytes);
int zk_dev_free(void* d_ptr);
int zk_dev_trim(void);
int zk_dev_upload(void* d_dst, const void* h_src, size_t bytes);
int zk_dev_download(void* h_dst, const void* d_src, size_t bytes);
int zk_dev_sync(void);
/* A non-blocking HIP stream of the library's own making (any hipStream_t of the caller's serves as well) -- for hosts
 * without a HIP binding of their own: one per concurrent prover thread.  zk_stream_free waits for the stream first;
 * call it from the thread that used the stream. */
void* zk_stream_new(void);
int zk_stream_sync(void* stream);
int zk_stream_free(void* stream);
int zk_dev_memset(void* d_ptr, int value, size_t bytes);
/* Synthetic field elements for benchmarks and size tests, generated where they are used: word i = splitmix64(seed + i), minus p
 * when that is >= p (the reference's benches fill their inputs with random field elements the same way, the files under starky/benches). */
int zk_dev_fill_splitmix(uint64_t* d, uint64_t n_words, uint64_t seed, void* stream);

/* ---- NTT / LDE ---------------------------------------------------------------------------
 * replaces fft_p::fft / fft_p::ifft (starky/src/fft_p.rs:242-253):
 *   (buffsrc:&Vec<F>, n_pols, nbits, buffdst:&mut Vec<F>)  -- natural order in and out,
 *   forward root MG.0[nbits]; inverse includes the 1/N factor.  dst must not alias src.      */
int zk_gl_ntt(const uint64_t* src, uint64_t* dst, uint32_t n_pols, uint32_t nbits, int inverse);
/* replaces fft_p::interpolate (fft_p.rs:255-261): LDE on the coset 49*<w_ext>;
 * src [1<<nbits][n_pols] -> dst [1<<nbits_ext][n_pols]; n_pols == 0 is a no-op (:262-264).   */
int zk_gl_lde(const uint64_t* src, uint32_t n_pols, uint32_t nbits, uint64_t* dst, uint32_t nbits_ext);
/* Streams.  Every `*_dev` entry point takes the HIP stream to issue on (NULL = the default stream).  Scratch memory
 * comes from a caching allocator inside the library; it orders the reuse of a block behind the work of every stream
 * the library has been handed so far, so calls on different streams (and from different host threads) may be mixed.
 * Handles (trees, transcripts, setups) are not re-entrant: one call at a time per handle.                            */
/* device-resident forms.  d_tmp: scratch of (1<<nbits)*n_pols words (ntt) or
 * (1<<nbits_ext)*n_pols words (lde); may be NULL when zk_gl_ntt_passes(nbits) == 1 (ntt only). */
int zk_gl_ntt_dev(const uint64_t* d_src, uint64_t* d_dst, uint64_t* d_tmp, uint32_t n_pols,
                  uint32_t nbits, int inverse, void* stream);
int zk_gl_lde_dev(const uint64_t* d_src, uint32_t n_pols, uint32_t nbits, uint64_t* d_dst,
                  uint64_t* d_tmp, uint32_t nbits_ext, void* stream);
int zk_gl_ntt_passes(uint32_t nbits); /* HBM passes a 2^nbits transform takes (bytes = 16*passes*N*n_pols) */

/* ---- Poseidon / LinearHash ---------------------------------------------------------------
 * replaces Poseidon::hash(inp, init_state, out) (starky/src/poseidon_opt.rs:76-200):
 * in[8] || cap[4] -> first n_out (1..12) state words.                                        */
int zk_gl_poseidon(const uint64_t in[8], const uint64_t cap[4], uint64_t* out, uint32_t n_out);
/* Host-only self check (NO GPU needed): the tables behind the kernels' matrix-pipe products -- the pre-sparse matrix P and the dense products
 * of the lazy partial-round blocks (poseidon_opt.rs:121-163) as balanced base-256 digit rows -- against their coefficients, and the
 * matrix-pipe arithmetic replayed step by step on the host against 128-bit arithmetic.  0 = fine, -1 = zk_last_error() says what is wrong. */
int zk_gl_poseidon_selfcheck(void);
/* replaces LinearHash::hash(flatvals, 0) (starky/src/linearhash.rs:79-110)                   */
int zk_gl_linearhash(const uint64_t* v, size_t n, uint64_t out[4]);
/* one digest per row of a device-resident [height][width] matrix -> d_digests[height][4]     */
int zk_gl_linearhash_rows_dev(const uint64_t* d_rows, uint32_t width, uint64_t height,
                              uint64_t* d_digests, void* stream);

/* ---- Merkle tree (trait MerkleTree, starky/src/traits.rs:24-55; MerkleTreeGL,
 *      starky/src/merklehash.rs:293-346, :430-457) ------------------------------------------ */
typedef struct zk_merkle zk_merkle_t;
uint64_t zk_merkle_n_nodes(uint64_t height);                       /* merklehash.rs:47-61      */
/* merkelize(buff, width, height): the tree copies `buff` to the device and owns it, as the
 * reference tree takes ownership of the Vec (merklehash.rs:326-329).                          */
zk_merkle_t* zk_gl_merkelize(const uint64_t* buff, uint32_t width, uint64_t height);
/* device-resident form: the tree BORROWS d_buff (must outlive the tree) and hashes on `stream` */
zk_merkle_t* zk_gl_merkelize_dev(const uint64_t* d_buff, uint32_t width, uint64_t height, void* stream);
int zk_merkle_root(const zk_merkle_t* t, uint64_t out[4]);          /* merklehash.rs:455-457    */
int zk_merkle_nodes(const zk_merkle_t* t, uint64_t* out);           /* all n_nodes*4 words      */
int zk_merkle_elements(const zk_merkle_t* t, uint64_t* out);        /* the committed rows, height*width words: what
                                                                       MerkleTree::to_extend reads back (merklehash.rs:260-265) */
uint32_t zk_merkle_depth(const zk_merkle_t* t);                     /* siblings per proof       */
/* get_group_proof(idx) (merklehash.rs:430-438): row_out[width], path_out[depth*4];
 * idx >= height is an error, as the reference bails.                                          */
int zk_merkle_group_proof(const zk_merkle_t* t, uint64_t idx, uint64_t* row_out, uint64_t* path_out);
/* n openings in one round trip (one launch, one copy): rows_out[n][width], paths_out[n][depth][4].  A proof opens every tree at
 * every query index (fri.rs:160-181); asked one by one, the launch + wait + copy of each opening is most of a small proof.    */
int zk_merkle_group_proofs(const zk_merkle_t* t, const uint64_t* idx, uint32_t n, uint64_t* rows_out, uint64_t* paths_out);
const uint64_t* zk_merkle_elements_dev(const zk_merkle_t* t);       /* device pointer of rows   */
const uint64_t* zk_merkle_nodes_dev(const zk_merkle_t* t);          /* device pointer of nodes  */
int zk_merkle_free(zk_merkle_t* t);

/* ---- Transcript (trait Transcript, starky/src/traits.rs:57-63; TranscriptGL,
 *      starky/src/transcript.rs:8-103).  The sponge state lives on the device: absorbing a root,
 *      the evals or the last FRI polynomial and drawing a challenge need no host round trip.     */
typedef struct zk_transcript zk_transcript_t;
zk_transcript_t* zk_transcript_new(void);                                        /* T::new()            */
int zk_transcript_put(zk_transcript_t* t, const uint64_t* src, size_t n);        /* put(), host words   */
int zk_transcript_put_dev(zk_transcript_t* t, const uint64_t* d_src, size_t n, void* stream);
int zk_transcript_get_field(zk_transcript_t* t, uint64_t out[3]);                /* get_field() -> host */
int zk_transcript_get_field_dev(zk_transcript_t* t, uint64_t* d_out3, void* stream);
int zk_transcript_get_fields1(zk_transcript_t* t, uint64_t* out);                /* get_fields1()       */
int zk_transcript_get_permutations(zk_transcript_t* t, uint32_t n, uint32_t nbits, uint64_t* out);
int zk_transcript_free(zk_transcript_t* t);

/* ---- FRI (starky/src/fri.rs:84-184) ----------------------------------------------------------
 * one folding step (fri.rs:101-126): d_pol [1<<pol_bits][3] -> d_out [1<<step_bits][3];
 * d_special_x = the step's challenge (3 device words); shift_inv = (49^-1)^(2^(nBitsExt-pol_bits)).
 * pol_bits - step_bits <= 11 (the reference folds any number of bits, fri.rs:112-126; its largest step is the 10 bits of
 * final.starkStruct.*.json, 2^17 -> 2^7).  step_bits == pol_bits copies (step 0 of the reference).                   */
int zk_fri_fold_dev(const uint64_t* d_pol, uint32_t pol_bits, uint32_t step_bits,
                    const uint64_t* d_special_x, uint64_t shift_inv, uint64_t* d_out, void* stream);
/* get_transposed_buffer (fri.rs:299-317): [n] F3G -> [1<<tbits][n>>tbits][3] words */
int zk_fri_transpose_dev(const uint64_t* d_pol, uint64_t n, uint32_t tbits, uint64_t* d_out, void* stream);

/* ---- stark_gen glue (starky/src/stark_gen.rs) --------------------------------------------------
 * x_n / x_2ns tables (:231-247): out[k] = shift * MG.0[nbits]^k                                    */
int zk_stark_x_table_dev(uint32_t nbits, uint64_t shift, uint64_t* d_out, void* stream);
/* build_Zh_Inv (:575-592): out[j] = 1/(49^(2^nbits) * MG.0[ext]^j - 1), j < 2^ext                 */
int zk_stark_zh_inv_dev(uint32_t nbits, uint32_t extend_bits, uint64_t* d_out, void* stream);
/* xDivXSubXi / xDivXSubWXi (:481-522): out[k] = x/(x - xi*mulw), x = 49*MG.0[nbits_ext]^k, [Next][3];
 * mulw = 1 for xi, MG.0[nBits] for w*xi                                                            */
int zk_stark_xdivxsub_dev(const uint64_t* d_xi, uint64_t mulw, uint32_t nbits_ext, uint64_t* d_out, void* stream);
/* LEv / LpEv (:416-430): iNTT_N of ((xi[*w])/49)^i -> [N][3]; d_tmp, d_tmp2: N*3 words each        */
int zk_stark_lev_dev(const uint64_t* d_xi, uint32_t nbits, int prime, uint64_t* d_out, uint64_t* d_tmp,
                     uint64_t* d_tmp2, void* stream);
/* evals (:432-466): out[e] = sum_k cell_e[(k<<ext)*width + offset] * L_e[k]; L_e = LpEv if prime   */
typedef struct { const uint64_t* d_buf; uint64_t width; uint64_t offset; uint32_t dim; uint32_t prime; } zk_eval_desc;
int zk_stark_evals_dev(const zk_eval_desc* descs, uint32_t n_ev, uint32_t nbits, uint32_t ext,
                       const uint64_t* d_LEv, const uint64_t* d_LpEv, uint64_t* d_out, void* stream);
/* Q split (:375-391): qq2[i][p*q_dim+k] = qq1[p*N+i][k] * (49^-N)^p ; qq2 is [Next][q_dim*q_deg]
 * and must be zero-filled by the caller beyond row N                                               */
int zk_stark_qsplit_dev(const uint64_t* d_qq1, uint32_t nbits, uint32_t q_dim, uint32_t q_deg,
                        uint64_t* d_qq2, void* stream);

/* get_pol / set_pol (:594-622, :683-707): column `offset` (1 or 3 words wide) of a [n][width] section
 * <-> a dense [n][3] polynomial (dim-1 columns are zero padded)                                    */
int zk_stark_get_pol_dev(const uint64_t* d_buf, uint64_t width, uint64_t offset, uint32_t dim, uint64_t n,
                         uint64_t* d_out3, void* stream);
int zk_stark_set_pol_dev(uint64_t* d_buf, uint64_t width, uint64_t offset, uint32_t dim, uint64_t n,
                         const uint64_t* d_in3, void* stream);
/* calculate_H1H2 (:624-651) over [n][3] operands: the sorted merge of the looked-up values f and the table t, split into its even
 * (h1) and odd (h2) entries.  A hash table over t on the device instead of the reference's HashMap + stable sort on the host;
 * synchronises and fails with "Number not included: <value>" for the first f the table lacks (:636-638). */
int zk_stark_calculate_h1h2_dev(const uint64_t* d_f3, const uint64_t* d_t3, uint64_t n, uint64_t* d_h1_3, uint64_t* d_h2_3, void* stream);
/* calculate_Z (:653-666): z[0] = 1, z[i] = z[i-1]*num[i-1]/den[i-1] over [n][3] operands; synchronises
 * and fails ("z does not close") when z[n-1]*num[n-1]/den[n-1] != 1, as the reference asserts (:663-664) */
int zk_stark_calculate_z_dev(const uint64_t* d_num3, const uint64_t* d_den3, uint64_t n, uint64_t* d_z3, void* stream);

/* ---- G1 multi-scalar multiplication (groth16 final wrap) ---------------------------------------
 * stands behind Groth16::prove (groth16/src/groth16.rs:88-96) -> bellman_ce::create_random_proof ->
 * multiexp, the seam bellperson occupies under `--features cuda` (groth16.rs:45-57).  Layout as
 * bellman keeps it: bases n x 64 B affine (x || y), Fq in Montgomery form (R = 2^256), little-endian
 * limbs; scalars n x 32 B canonical little-endian (FrRepr); out 64 B affine Montgomery, *is_infinity
 * set when the sum is the point at infinity.  `_dev` takes device pointers (d_out: 68 bytes) and, as
 * every `_dev` entry point, returns once the work is queued on `stream`.                              */
int zk_msm_g1_bn254(const void* bases, const void* scalars, uint64_t n, void* out, int* is_infinity);
int zk_msm_g1_bn254_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, void* stream);
/* the same on BLS12-381 G1 (zkit --curve BLS12381; pairing_ce bls12_381): Fq = 12 x 32-bit limbs, Montgomery
 * R = 2^384, bases n x 96 B, scalars n x 32 B canonical (255 bits), out 96 B; d_out of `_dev`: 100 bytes.  */
int zk_msm_g1_bls12_381(const void* bases, const void* scalars, uint64_t n, void* out, int* is_infinity);
int zk_msm_g1_bls12_381_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, void* stream);
int zk_g1_bls12_381_mul_generator_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);
/* G2 (the B-query of a Groth16 proving key): the same entry points over the sextic twist, coordinates in
 * Fq2 = Fq[u]/(u^2 + 1).  A point is x.c0 || x.c1 || y.c0 || y.c1 (pairing_ce's G2Affine), each Fq as above:
 * 128 B (BN254) / 192 B (BLS12-381); `_dev` output = the point followed by a 4-byte infinity flag.              */
int zk_msm_g2_bn254(const void* bases, const void* scalars, uint64_t n, void* out, int* is_infinity);
int zk_msm_g2_bn254_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, void* stream);
int zk_g2_bn254_mul_generator_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);
int zk_msm_g2_bls12_381(const void* bases, const void* scalars, uint64_t n, void* out, int* is_infinity);
int zk_msm_g2_bls12_381_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, void* stream);
int zk_g2_bls12_381_mul_generator_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);
/* synthetic CRS for benches and tests: d_bases[i] = [d_k[i]] G, G = (1, 2), k_i a non-zero 64-bit integer
 * (what generate_random_parameters, groth16.rs:39,82, does with secret exponents).                     */
int zk_g1_bn254_mul_generator_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);

/* ---- BN128-field hashing: verificationHashType "BN128", the final STARK of every aggregation --------------
 * (test/stark_aggregation.sh:199-210).  A digest is an ElementDigest<4, Fr> (starky/src/digest.rs:45-65): the
 * four RAW limbs of an Fr of BN254's scalar field, i.e. its Montgomery form a*2^256 mod r -- every uint64_t[4]
 * below carries that format, exactly what MTNodeType::from_scalar / as_scalar exchange.
 * zk_bn128_load_constants reads the Poseidon parameter tables (t = 2..17; data/poseidon_bn128_constants.bin,
 * written by tools/gen_poseidon_bn128_constants.py from poseidon_bn128_constants_opt.rs) once per device.      */
int zk_bn128_load_constants(const char* path);
/* Host-only check (no GPU) of the matrix-pipe tables the dense layers of the one-lane kernels run on (csrc/fr_mfma.hip.h): built from
 * the constants file, emulated the device's way on random and extreme vectors, compared with plain modular arithmetic.  0, or -1 with
 * zk_last_error() naming the first difference.                                                                                      */
int zk_bn128_poseidon_selfcheck(const char* path);
/* Poseidon::hash_ex(inp, init_state, out) (poseidon_bn128_opt.rs:80-86, 98-224): n_in = 1..16 inputs, t = n_in + 1,
 * first n_out (<= t) state words.  Wrong lengths are errors, as the reference bails (:99-105).                   */
int zk_bn128_poseidon(const uint64_t* inp, uint32_t n_in, const uint64_t init_state[4], uint32_t n_out, uint64_t* out);
/* batch form on device memory: inp [n][n_in][4], one shared init_state, out [n][n_out][4]                        */
int zk_bn128_poseidon_dev(const uint64_t* d_inp, uint64_t n, uint32_t n_in, const uint64_t* d_init_state, uint32_t n_out,
                          uint64_t* d_out, void* stream);
/* LinearHashBN128::hash_element_array (linearhash_bn128.rs:105-131): n Goldilocks words -> digest               */
int zk_bn128_linearhash(const uint64_t* v, size_t n, uint64_t out[4]);
/* MerkleTreeBN128 (merklehash_bn128.rs): arity 16; same ownership rules as zk_gl_merkelize(_dev)                */
typedef struct zk_bn128_merkle zk_bn128_merkle_t;
uint64_t zk_bn128_merkle_n_nodes(uint64_t height);                        /* :26-39                     */
zk_bn128_merkle_t* zk_bn128_merkelize(const uint64_t* buff, uint32_t width, uint64_t height);           /* :196-239 */
zk_bn128_merkle_t* zk_bn128_merkelize_dev(const uint64_t* d_buff, uint32_t width, uint64_t height, void* stream);
int zk_bn128_merkle_root(const zk_bn128_merkle_t* t, uint64_t out[4]);   /* :275-277                    */
int zk_bn128_merkle_nodes(const zk_bn128_merkle_t* t, uint64_t* out);    /* all n_nodes*4 words         */
uint32_t zk_bn128_merkle_depth(const zk_bn128_merkle_t* t);
/* get_group_proof (:246-254): row_out[width], path_out[depth][16][4]; idx >= height is an error          */
int zk_bn128_merkle_group_proof(const zk_bn128_merkle_t* t, uint64_t idx, uint64_t* row_out, uint64_t* path_out);
/* n openings at once: rows_out[n][width], paths_out[n][depth][16][4] */
int zk_bn128_merkle_group_proofs(const zk_bn128_merkle_t* t, const uint64_t* idx, uint32_t n, uint64_t* rows_out, uint64_t* paths_out);
int zk_bn128_merkle_free(zk_bn128_merkle_t* t);
/* TranscriptBN128 (transcript_bn128.rs:14-132): put takes one Goldilocks word (n = 1) or one digest (n = 4)       */
typedef struct zk_bn128_transcript zk_bn128_transcript_t;
zk_bn128_transcript_t* zk_bn128_transcript_new(void);
int zk_bn128_transcript_put(zk_bn128_transcript_t* t, const uint64_t* e, size_t n);
int zk_bn128_transcript_get_fields1(zk_bn128_transcript_t* t, uint64_t* out);
int zk_bn128_transcript_get_field(zk_bn128_transcript_t* t, uint64_t out[3]);
int zk_bn128_transcript_get_permutations(zk_bn128_transcript_t* t, uint32_t n, uint32_t nbits, uint64_t* out);
int zk_bn128_transcript_free(zk_bn128_transcript_t* t);

/* ---- the same over the BLS12-381 scalar field: verificationHashType "BLS12381" (`--curve BLS12381`).  Twins of the
 * BN128 entry points above, behind poseidon_bls12381_opt.rs (hash() returns state[1], :94-103), linearhash_bls12381.rs,
 * merklehash_bls12381.rs, transcript_bls12381.rs; tables in data/poseidon_bls12381_constants.bin.                     */
typedef struct zk_bls12381_merkle zk_bls12381_merkle_t;
typedef struct zk_bls12381_transcript zk_bls12381_transcript_t;
int zk_bls12381_load_constants(const char* path);
int zk_bls12381_poseidon_selfcheck(const char* path);
int zk_bls12381_poseidon(const uint64_t* inp, uint32_t n_in, const uint64_t init_state[4], uint32_t n_out, uint64_t* out);
int zk_bls12381_poseidon_dev(const uint64_t* d_inp, uint64_t n, uint32_t n_in, const uint64_t* d_init_state, uint32_t n_out,
                          uint64_t* d_out, void* stream);
int zk_bls12381_linearhash(const uint64_t* v, size_t n, uint64_t out[4]);
uint64_t zk_bls12381_merkle_n_nodes(uint64_t height);
zk_bls12381_merkle_t* zk_bls12381_merkelize(const uint64_t* buff, uint32_t width, uint64_t height);
zk_bls12381_merkle_t* zk_bls12381_merkelize_dev(const uint64_t* d_buff, uint32_t width, uint64_t height, void* stream);
int zk_bls12381_merkle_root(const zk_bls12381_merkle_t* t, uint64_t out[4]);
int zk_bls12381_merkle_nodes(const zk_bls12381_merkle_t* t, uint64_t* out);
uint32_t zk_bls12381_merkle_depth(const zk_bls12381_merkle_t* t);
int zk_bls12381_merkle_group_proof(const zk_bls12381_merkle_t* t, uint64_t idx, uint64_t* row_out, uint64_t* path_out);
int zk_bls12381_merkle_group_proofs(const zk_bls12381_merkle_t* t, const uint64_t* idx, uint32_t n, uint64_t* rows_out, uint64_t* paths_out);
int zk_bls12381_merkle_free(zk_bls12381_merkle_t* t);
zk_bls12381_transcript_t* zk_bls12381_transcript_new(void);
int zk_bls12381_transcript_put(zk_bls12381_transcript_t* t, const uint64_t* e, size_t n);
int zk_bls12381_transcript_get_fields1(zk_bls12381_transcript_t* t, uint64_t* out);
int zk_bls12381_transcript_get_field(zk_bls12381_transcript_t* t, uint64_t out[3]);
int zk_bls12381_transcript_get_permutations(zk_bls12381_transcript_t* t, uint32_t n, uint32_t nbits, uint64_t* out);
int zk_bls12381_transcript_free(zk_bls12381_transcript_t* t);


/* ---- whole prover (starky/src/prove.rs:95-160: StarkSetup::new + StarkProof::stark_gen + FRI::prove) ------
 * zk_stark_setup_new stands behind StarkSetup::new (stark_setup.rs:27-66): it takes the reference's
 * serialised code-generator output, {"starkinfo": StarkInfo, "program": Program} (serde field names,
 * starkinfo.rs:27-95), the StarkStruct JSON (verificationHashType "GL", or "BN128" after
 * zk_bn128_load_constants: MerkleTreeBN128 + TranscriptBN128, prove.rs:47-61) and the constant
 * polynomials ([2^nBits][n_constants] words, the .const file, polsarray.rs:137-217); it extends and
 * merkelizes the constants on the device and compiles the step programs for gfx950.
 * zk_stark_gen stands behind StarkProof::stark_gen (stark_gen.rs:193-202) + FRI::prove (fri.rs:84-89):
 * cm_pols = the committed trace ([2^nBits][n_cm1] words, the .cm file).  Returns the proof as the
 * zkin JSON the reference's serialiser writes (serializer.rs:146-261), malloc'ed: release it with
 * zk_string_free.  NULL on error (zk_last_error), e.g. "z does not close" (stark_gen.rs:663-664).
 * A setup is bound to the device current at creation and is not re-entrant.                         */
/* The code generator: stands behind StarkInfo::new (starky/src/starkinfo.rs:160-272; called from StarkSetup::new,
 * stark_setup.rs:45-52).  pil_json = the compiled PIL (types.rs:134-155, what pilcom writes), stark_struct_json = the
 * StarkStruct.  Returns the JSON zk_stark_setup_new takes, {"starkinfo": StarkInfo, "program": Program} in the reference's
 * serde names, malloc'ed (zk_string_free); NULL on error, e.g. "stark_deg != pil_deg", "Global.L1 must be defined".
 * Host only.  A caller that has the Rust front end passes its own serde output instead and never needs this. */
char* zk_starkinfo_generate(const char* pil_json, const char* stark_struct_json);
typedef struct zk_stark_setup zk_stark_setup_t;
zk_stark_setup_t* zk_stark_setup_new(const char* starkinfo_program_json, const char* stark_struct_json,
                                     const uint64_t* const_pols, uint64_t n_words);
int zk_stark_setup_const_root(const zk_stark_setup_t* s, uint64_t out[4]);   /* StarkSetup.const_root */
/* stark_gen's `prover_addr` argument (stark_gen.rs:201): echoed as "proverAddr" by non-GL proofs (serializer.rs:255-262) */
int zk_stark_setup_set_prover_addr(zk_stark_setup_t* s, const char* prover_addr);
/* stark_verify (starky/src/stark_verify.rs:20-136, fri.rs:187-297) on a proof in the prover's own output format, the zkin
 * JSON of serializer.rs:146-261, for all three hash types: 1 = accepted, 0 = rejected (zk_last_error() names the failed
 * check: "Q != C * P", "FRIVerifierFailed: ...", a fold mismatch, the last polynomial's degree), -1 = malformed input.
 * The sponge, the LinearHash of every opened row and every Merkle path run in the library's kernels; the two short
 * verifier programs and the FRI groups' inverse transforms are scalar host work.  This is a verifier for UNTRUSTED zkin, stricter
 * than the reference where the reference is loose: scalar-field (16-ary) Merkle paths are walked level by level -- the node at position
 * idx & 15 of every level must be the value carried up, starting from the row's digest -- whereas merklehash_bn128.rs:108-128 binds only
 * the last level to the root (rows unbound); finalPol must hold exactly 2^steps.last values and every path must have the depth its tree
 * implies.  Honest proofs pass either way.  zk_stark_verify_set_reference_compat(1) switches the CALLING THREAD to the reference's lenient path
 * check (for parity tests against a verifier that follows the reference to the letter); it returns the previous setting.
 *   zk_stark_verify       against a prover's setup (its StarkInfo / Program / StarkStruct and the root of its constants)
 *   zk_stark_verify_with  without one: the same JSON texts zk_stark_setup_new takes + const_root (GL words, or the raw
 *                         Montgomery limbs zk_stark_setup_const_root returns for BN128 / BLS12381)
 * zk_stark_setup_set_self_check(s, 1): every later zk_stark_gen* of the setup verifies its proof before returning it and
 * fails (NULL, "the proof does not verify: ...") otherwise -- the `assert!(stark_verify(..))` of prove.rs:124-132.        */
int zk_stark_verify(const zk_stark_setup_t* s, const char* zkin_json);
int zk_stark_verify_with(const char* starkinfo_program_json, const char* stark_struct_json, const uint64_t const_root[4],
                         const char* zkin_json);
int zk_stark_verify_set_reference_compat(int on);
int zk_stark_setup_set_self_check(zk_stark_setup_t* s, int on);
/* Where the time went, as JSON text owned by the setup (valid until the next call on it / its release).
 * zk_stark_setup_timing: StarkSetup::new (stark_setup.rs:26-66, one `#[time_profiler("stark_setup")]` span there) split into
 *   json_parse_ms, const_lde_merkle_ms, programs_ms (+ how many step programs hipRTC compiled and how many came from the
 *   code-object cache: $ZK_JIT_CACHE, default ~/.cache/zkgpu, "off" disables; `hiprtc_processes`: how many of the compilations ran
 *   in a helper process -- a setup compiles its step programs side by side, one `zkgpu_jitc` (next to libzkgpu.so; $ZK_JITC names
 *   another, "off" disables) per program, because hipRTC compiles serially inside one process; a code object is sha256-checked when it
 *   comes back from disk, and a cache directory that is not the user's own or is writable by others is not used);
 *   "eval_mode": "jit" | "bytecode" and "bytecode_programs": how many of the setup's programs are interpreter bytecode: in bytecode
 *   mode the five steps (a step without code is an empty program) and every public calculator, otherwise 0 (then nothing was compiled:
 *   hiprtc_compiled and the cache counters stay 0).
 * zk_stark_last_timing: the stages of the last proof of this setup in HIP-event milliseconds, named after the reference's
 *   spans (stark_gen.rs:192,624,709,734,785; fri.rs:83): extend, merkelize, calculate_exps_parallel, calculate_H1H2,
 *   calculate_Z, fri_prove, ...  Collected only when the environment has ZK_STARK_TIMING=1 (also logged to stderr); "" otherwise. */
const char* zk_stark_setup_timing(const zk_stark_setup_t* s);
const char* zk_stark_last_timing(const zk_stark_setup_t* s);
char* zk_stark_gen(zk_stark_setup_t* s, const uint64_t* cm_pols, uint64_t n_words);
/* same with the trace already resident in HBM (borrowed, not modified), e.g. written there by a device-side
 * witness generator or uploaded while the previous proof was running                                     */
char* zk_stark_gen_dev(zk_stark_setup_t* s, const uint64_t* d_cm_pols, uint64_t n_words);
/* The same on a stream of the caller's.  Proofs of DIFFERENT setups may run at the same time from different host threads,
 * each on its own (non-blocking) stream: small proofs are bound by the latency of their launch chain, not by the device
 * (test/stark_aggregation.sh:70-73 runs its recursion tasks as parallel processes for the same reason).  One setup serves
 * one proof at a time. */
char* zk_stark_gen_dev_on(zk_stark_setup_t* s, const uint64_t* d_cm_pols, uint64_t n_words, void* stream);

/* ---- the staged prover: stark_gen cut at the reference's own seams ----
 * For a caller that keeps its own stark_gen.rs and swaps in the device for the heavy calls it makes:
 *   calculate_exps_parallel(ctx, starkinfo, segment, domain, step)   stark_gen.rs:786-792   -> zk_stark_eval
 *   extend_and_merkelize(ctx, stage) + transcript.put(root)          stark_gen.rs:709-750   -> zk_stark_commit_stage
 *   transcript.get_field() into ctx.challenges[i]                    stark_gen.rs:285-294   -> zk_stark_challenge (or zk_stark_set_challenge)
 *   calculate_H1H2 / calculate_Z over every argument of the PIL      stark_gen.rs:300-353   -> zk_stark_calculate_h1h2 / _z
 *   the evaluations at xi, w xi + their absorption                   stark_gen.rs:416-472   -> zk_stark_evals
 *   FRI::prove(transcript, pol, query_pol)                           fri.rs:84-184          -> zk_stark_fri_prove, or zk_fri_prove_dev alone
 * A context (one proof in progress) belongs to one setup and one stream; its sections stay in HBM between the calls.  The calls are
 * accepted in the reference's order only (an out-of-order call fails with a message naming what comes first):
 *   new -> commit 1 -> challenge 0, 1 -> eval 2PREV -> calculate_h1h2 -> commit 2 -> challenge 2, 3 -> eval 3PREV -> calculate_z ->
 *   eval 3 -> commit 3 -> challenge 4 -> eval 42NS -> commit 4 -> challenge 7 -> evals -> challenge 5, 6 -> eval 52NS -> fri_prove -> finish.
 * zk_stark_gen* is exactly this sequence; a proof driven through the stages is byte-equal to zk_stark_gen's (tests/cabi/zkgpu_cabi_test.c).
 *   zk_stark_new            the trace in host memory (cm_pols) or in HBM (d_cm_pols), the other NULL; sections allocated, publics computed and absorbed.
 *                           d_cm_pols is BORROWED for the life of the context: every later stage reads it; it must stay allocated and unchanged
 *                           until zk_stark_free (a host trace is copied, the caller may release it when zk_stark_new returns)
 *   zk_stark_commit_stage   stage 1..3: LDE + Merkle tree of cm<stage>; stage 4: Q split (inverse NTT, split, NTT) + tree 4; the root is absorbed by the
 *                           context's transcript and copied to root[4] when non-NULL (GL words, or the raw Montgomery limbs of a scalar-field digest)
 *   zk_stark_challenge      challenge i <- the context's transcript (copied to out[3] when non-NULL); i: 0 u, 1 defVal, 2 gamma, 3 beta, 4 vc, 5 v1, 6 v2, 7 xi
 *   zk_stark_set_challenge  challenge i <- v: for a caller whose own sponge does Fiat-Shamir; such a caller also runs FRI through zk_fri_prove_dev
 *                           with its own transcript (zk_stark_fri_pol_dev, zk_stark_tree give it the polynomial and the query trees)
 *   zk_stark_evals          -> number of evaluations; 3 words each into evals_out (host, may be NULL)
 *   zk_stark_finish         the openings, the one read-back, the zkin JSON (malloc'ed: zk_string_free); honours zk_stark_setup_set_self_check
 *   zk_fri_prove_dev        FRI::prove on any device polynomial of 2^nbits_ext extension values (3 words each) with the caller's TranscriptGL and the
 *                           GL trees its queries open: -> JSON {"ys", "s<k>_root", "s<k>_vals", "s<k>_siblings", "s0_vals<j>", "s0_siblings<j>", "finalPol"}
 *                           (query trees numbered from 1; serializer.rs:189-252's layout), malloc'ed                                              */
typedef struct zk_stark_ctx zk_stark_ctx_t;
enum { ZK_STEP_2PREV = 0, ZK_STEP_3PREV = 1, ZK_STEP_3 = 2, ZK_STEP_42NS = 3, ZK_STEP_52NS = 4 };
zk_stark_ctx_t* zk_stark_new(zk_stark_setup_t* s, const uint64_t* cm_pols, const uint64_t* d_cm_pols, uint64_t n_words, void* stream);
int zk_stark_commit_stage(zk_stark_ctx_t* c, int stage, uint64_t root[4]);
int zk_stark_challenge(zk_stark_ctx_t* c, int i, uint64_t out[3]);
int zk_stark_set_challenge(zk_stark_ctx_t* c, int i, const uint64_t v[3]);
int zk_stark_eval(zk_stark_ctx_t* c, int step);
int zk_stark_calculate_h1h2(zk_stark_ctx_t* c);
int zk_stark_calculate_z(zk_stark_ctx_t* c);
int zk_stark_evals(zk_stark_ctx_t* c, uint64_t* evals_out, uint64_t cap_words);
int zk_stark_fri_prove(zk_stark_ctx_t* c);
char* zk_stark_finish(zk_stark_ctx_t* c);
const uint64_t* zk_stark_fri_pol_dev(const zk_stark_ctx_t* c);            /* f_2ns after step 52NS: FRI's input, 3 << nBitsExt words in HBM */
const zk_merkle_t* zk_stark_tree(const zk_stark_ctx_t* c, int j);         /* 1..4 once committed, 5 = the constants' tree; NULL for scalar-field hashing */
int zk_stark_free(zk_stark_ctx_t* c);
char* zk_fri_prove_dev(zk_transcript_t* transcript, const uint64_t* d_pol, uint32_t nbits_ext, const uint32_t* steps, uint32_t n_steps,
                       uint32_t n_queries, const zk_merkle_t* const* query_trees, uint32_t n_query_trees, void* stream);
void zk_string_free(char* s);
int zk_stark_setup_free(zk_stark_setup_t* s);

/* Window tables for bases that do not change between calls (a Groth16 proving key): the table holds 2^(16 w) P_i for the
 * 16 windows of every base (16 x the size of the internal point form; *_table_bytes says how much), built once on the
 * device; a sum over the points [offset, offset + n) of a table built for table_n bases then needs no doublings.
 * table_n < 2^24.  Same operand formats and the same (bit-identical) result as zk_msm_*_dev.                        */
size_t zk_msm_g1_bn254_table_bytes(uint64_t table_n);
int zk_msm_g1_bn254_table_build_dev(const void* d_bases, uint64_t table_n, void* d_table, void* stream);
int zk_msm_g1_bn254_table_dev(const void* d_table, uint64_t table_n, uint64_t offset, const void* d_scalars, uint64_t n, void* d_out, void* stream);
size_t zk_msm_g2_bn254_table_bytes(uint64_t table_n);
int zk_msm_g2_bn254_table_build_dev(const void* d_bases, uint64_t table_n, void* d_table, void* stream);
int zk_msm_g2_bn254_table_dev(const void* d_table, uint64_t table_n, uint64_t offset, const void* d_scalars, uint64_t n, void* d_out, void* stream);
size_t zk_msm_g1_bls12_381_table_bytes(uint64_t table_n);
int zk_msm_g1_bls12_381_table_build_dev(const void* d_bases, uint64_t table_n, void* d_table, void* stream);
int zk_msm_g1_bls12_381_table_dev(const void* d_table, uint64_t table_n, uint64_t offset, const void* d_scalars, uint64_t n, void* d_out, void* stream);
size_t zk_msm_g2_bls12_381_table_bytes(uint64_t table_n);
int zk_msm_g2_bls12_381_table_build_dev(const void* d_bases, uint64_t table_n, void* d_table, void* stream);
int zk_msm_g2_bls12_381_table_dev(const void* d_table, uint64_t table_n, uint64_t offset, const void* d_scalars, uint64_t n, void* d_out, void* stream);

/* ---- Groth16 around the multi-scalar sums (`zkit groth16_prove`, groth16/src/api.rs:144-205) ----
 * The reference hands the whole proof to bellman_ce::groth16::create_random_proof (groth16/src/groth16.rs:88-96;
 * third-party).  These entry points keep everything after witness generation on the device.
 *
 * zk_fr_*_ntt stand behind bellman's EvaluationDomain::{fft, ifft, coset_fft, icoset_fft}: 2^log_n elements of
 * the curve's scalar field (4 x u64 Montgomery R = 2^256, i.e. the raw limbs of an Fr), natural order in and
 * out, in place; omega = Fr::root_of_unity()^(2^(S - log_n)), coset generator Fr::multiplicative_generator() = 7.
 * zk_fr_*_quotient stand behind create_proof's `h` block: from the per-row evaluations a, b, c (2^log_n each)
 * to the coefficients of (A B - C)/(X^n - 1), written over a (bellman then drops the last one).              */
int zk_fr_bn254_ntt(uint64_t* data, uint32_t log_n, int inverse, int coset);
int zk_fr_bn254_ntt_dev(uint64_t* d_data, uint32_t log_n, int inverse, int coset, void* stream);
int zk_fr_bls12_381_ntt(uint64_t* data, uint32_t log_n, int inverse, int coset);
int zk_fr_bls12_381_ntt_dev(uint64_t* d_data, uint32_t log_n, int inverse, int coset, void* stream);
int zk_fr_bn254_quotient_dev(uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, uint32_t log_n, void* stream);
int zk_fr_bls12_381_quotient_dev(uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, uint32_t log_n, void* stream);
/* zk_groth16_setup_new stands behind api.rs:161-171 (read_pk_from_file + create_circuit_from_file): `curve` is the
 * reference's curve_type string ("BN128" | "BLS12381"), `r1cs` the bytes of the circom .r1cs file
 * (algebraic/src/r1cs_file.rs), `params` the bytes of the proving key as bellman's Parameters::write lays it out
 * (unchecked read: points are not tested for curve membership, as with checked = false).  The circuit is the one
 * algebraic/src/circom_circuit.rs:94-160 synthesises; a key whose query sizes do not match it is an error.
 * zk_groth16_prove: `witness` = n_wires x 32 B little-endian canonical values (the body of a .wtns file, see
 * zk_groth16_wtns_payload; reader.rs:86-137), r and s = the two blinding scalars create_random_proof draws from its
 * rng (canonical, < the field modulus), `proof` (optional) receives A || B || C as affine Montgomery coordinates
 * (BN254: 64 + 128 + 64 B; BLS12-381: 96 + 192 + 96 B; G2 as x.c0 || x.c1 || y.c0 || y.c1).  Returns proof.json
 * as json_utils.rs:305-315 renders it (malloc'ed; zk_string_free), NULL on error.  A setup is bound to the device
 * current at its creation, keeps the key resident there (as window tables, 16 x the key, when it has fewer than 2^24
 * G1 bases) and is not re-entrant: one zk_groth16_prove at a time per setup.                                      */
/* base-field elements in place on the device: to_mont = 1: canonical integers (what key files and proof.json carry,
 * Fq::from_repr) -> Montgomery limbs (what the multi-scalar sums take); to_mont = 0: the inverse (Fq::into_repr).
 * n_elems elements of 32 B (BN254) / 48 B (BLS12-381), little-endian words.                                    */
int zk_fq_bn254_convert_dev(void* d_elems, uint64_t n_elems, int to_mont, void* stream);
int zk_fq_bls12_381_convert_dev(void* d_elems, uint64_t n_elems, int to_mont, void* stream);
typedef struct zk_groth16_setup zk_groth16_setup_t;
zk_groth16_setup_t* zk_groth16_setup_new(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len);
int zk_groth16_setup_info(const zk_groth16_setup_t* s, uint32_t* n_wires, uint32_t* n_inputs, uint32_t* domain_log);
char* zk_groth16_prove(zk_groth16_setup_t* s, const void* witness, uint64_t n_wires, const uint64_t r[4], const uint64_t s_[4], void* proof);
/* same with the witness already in HBM (its values are taken as canonical: the host-side range check of zk_groth16_prove is
 * not repeated); d_h (optional) receives the quotient's 2^domain_log - 1 canonical coefficients */
char* zk_groth16_prove_dev(zk_groth16_setup_t* s, const void* d_witness, uint64_t n_wires, const uint64_t r[4], const uint64_t s_[4], void* proof, uint64_t* d_h);
int zk_groth16_wtns_payload(const void* wtns, size_t len, const char* curve, uint64_t* offset, uint64_t* n_values);
int zk_groth16_setup_free(zk_groth16_setup_t* s);

/* ---- Groth16 key generation (`zkit groth16_setup`, groth16/src/api.rs:42-66 -> Groth16::circuit_specific_setup,
 * groth16.rs:77-86 -> bellman's generate_random_parameters) ----------------------------------------------------
 * zk_*_mul_generator_fr_dev: d_bases[i] = [d_k[i]] G for n full-width scalars (4 x u64 canonical little-endian, below
 * the scalar field's modulus), G the generator of G1 / G2; the output layout of zk_*_mul_generator_dev (affine,
 * Montgomery), a zero scalar gives the all-zero encoding.  One window table of G per device, no doublings, one field
 * inversion per workgroup.
 * zk_groth16_keygen_new evaluates the QAP of the circuit zk_groth16_setup_new would synthesise at tau on the device and
 * forms the key's points with the kernel above.  trapdoor = tau, alpha, beta, gamma, delta (5 x 4 u64 canonical; values
 * of 2^256 range are reduced), or NULL to draw them from the operating system -- then nothing of them survives the call.
 * Errors (NULL, zk_last_error): a zero component, tau^m = 1 for the domain size m, an unknown curve, and every .r1cs
 * fault zk_groth16_setup_new reports.  _params writes bellman's Parameters::write layout (what zk_groth16_setup_new
 * reads) when cap >= _params_size, and nothing otherwise; _vk_json renders verification_key.json as
 * json_utils.rs:285-303 does (decimal coordinates, or fixed-width 0x strings with to_hex; malloc'ed, zk_string_free). */
int zk_g1_bn254_mul_generator_fr_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);
int zk_g2_bn254_mul_generator_fr_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);
int zk_g1_bls12_381_mul_generator_fr_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);
int zk_g2_bls12_381_mul_generator_fr_dev(const uint64_t* d_k, uint64_t n, void* d_bases, void* stream);
typedef struct zk_groth16_keygen zk_groth16_keygen_t;
zk_groth16_keygen_t* zk_groth16_keygen_new(const char* curve, const void* r1cs, size_t r1cs_len, const uint64_t* trapdoor);
size_t zk_groth16_keygen_params_size(const zk_groth16_keygen_t* k);
int zk_groth16_keygen_params(const zk_groth16_keygen_t* k, void* out, size_t cap);
char* zk_groth16_keygen_vk_json(const zk_groth16_keygen_t* k, int to_hex);
/* Diagnostic, not part of what `zkit groth16_setup` offers: where zk_groth16_keygen_new spent its time, in milliseconds of the host clock --
 * the transform, the column sums, the G1 points, the G2 points, serialisation.  The five stream synchronisations that separate the phases
 * are made on every call; each phase is milliseconds to seconds of device work, and the call ends in a copy to the host anyway. */
int zk_groth16_keygen_timing(const zk_groth16_keygen_t* k, double ms[5]);
int zk_groth16_keygen_free(zk_groth16_keygen_t* k);

/* ---- a Groth16 key from a powers-of-tau file, and contributions to it (csrc/groth16_srs.hip.h, csrc/ecntt.hip) ------------
 * The key of zk_groth16_keygen_new is only as good as the promise that its trapdoor was forgotten.  These entry points make the key
 * zk_groth16_keygen_new would make for (tau, alpha, beta, gamma = 1, delta = 1) from a ceremony's file, in which tau, alpha and beta
 * exist only as points, and then let anybody multiply delta by a secret of their own.
 * zk_srs_open reads a snarkjs .ptau container on the host (no GPU): magic "ptau", version 1, sections 1 (n8, the base field's modulus,
 * power, ceremonyPower), 2 tauG1 (2 * 2^power - 1 points), 3 tauG2, 4 alphaTauG1, 5 betaTauG1 (2^power each), 6 betaG2 (one); other
 * sections are ignored.  Points are uncompressed affine, little-endian Montgomery -- the layout of the multi-scalar sums.  curve: BN128 |
 * BLS12381.  Errors (NULL, zk_last_error): wrong magic or version, a modulus that is not the curve's, a missing or wrong-sized section,
 * a truncated file.  The layout is restated from snarkjs's writer; the reader has only met files tools/make_test_ptau.py wrote.
 * zk_srs_check -> a JSON report (malloc'ed, zk_string_free) in the style of zk_groth16_key_check: every point's class; tauG1[0] = G1 and
 * tauG2[0] = G2 ("not_generator"); each section a geometric sequence in tau, by one random linear combination and two pairings per section
 * ("not_powers"); betaG2 against betaTauG1[0] ("beta_mismatch").  seed: 32 bytes, tests only; NULL = the operating system's randomness.
 * zk_<g1|g2>_<curve>_ntt_dev: bellman's EvaluationDomain::{fft, ifft} on 2^log_n points in place -- natural order in and out, infinity
 * allowed, the omega of zk_fr_<curve>_ntt, 1 / n in the inverse.  zk_<g1|g2>_<curve>_mul_scalar_dev: d_out[i] = [k] d_points[i] for one
 * scalar k (4 x u64 canonical, below r) on the device; d_out may be d_points.  zk_<g1|g2>_<curve>_mul_scalars_dev: d_out[i] =
 * [d_k[i]] d_points[i], one scalar of 4 x u64 per point; the walk starts at each scalar's top set bit, so scalars of 128 bits cost half of
 * full-width ones; a zero scalar or the all-zero point gives the all-zero encoding; d_out may be d_points.
 * zk_g1_<curve>_mul_scalars_glv_dev: the same contract and the same bytes for points of the subgroup of order r, through the curve's
 * endomorphism: each scalar is split into two halves below 2^128 and one joint walk serves both, about half the point operations of the
 * walk above for full-width scalars and no gain for scalars of 128 bits or fewer.  G1 only: G2 has no such split here.
 * A ceremony.  zk_srs_new (host only, no device) writes the file of tau = alpha = beta = 1 -- every point its group's generator -- with an
 * empty transcript.  zk_srs_contribute writes to out_path the file for (tau t, alpha a, beta b): tauG1[i] t^i, tauG2[i] t^i, alphaTauG1[i] a t^i,
 * betaTauG1[i] b t^i, betaG2 b, the old transcript and one new record.  secrets: 3 x 4 u64 canonical and non-zero (t, a, b), or NULL to draw
 * them from the operating system; they and the proofs' nonces are overwritten on the host and on the device before the call returns.
 * beacon_seed (32 bytes, then secrets must be NULL): a contribution whose factors anyone can recompute -- d = SHA-256 iterated
 * 2^beacon_iter_log times over the seed, factor j = SHA-256(d | u8 j) as a little-endian integer cut to 253 bits.  The work goes section by
 * section in chunks of 2^20 points through one device buffer, each chunk straight into the file.  The transcript is section 64 of the
 * container -- a layout of this project (csrc/ceremony_host.h), not snarkjs's contribution section; zk_srs_open walks over it, so a
 * contributed file serves zk_groth16_keygen_from_srs and zk_groth16_key_check_srs as it is.  Each record holds the three images after
 * the contribution (tauG1[1], alphaTauG1[0], betaTauG1[0]), a Schnorr proof of knowledge of each factor over the previous record's image
 * (G1 for the first) and a hash chained over all records before it.  zk_srs_transcript_count (host only): the records of the file's
 * transcript, -1 without one.  zk_srs_verify -> a JSON report (malloc'ed, zk_string_free): zk_srs_check's whole report under "file", and
 * the findings "no_transcript", "chain_hash" {contribution}, "pok_invalid" {contribution, which: tau | alpha | beta} (the proof's equation,
 * or an image that is infinity or no point of the group), "beacon_mismatch" (a beacon record's images are not its recomputed factors'),
 * "image_mismatch" (the last record's images are not the file's, byte for byte).  The transcript proves that somebody knew every factor
 * from G1 to the last images; "file" proves that every section is the powers of that tau with those alpha and beta.
 * zk_groth16_keygen_from_srs returns what zk_groth16_keygen_new returns (_params_size, _params, _vk_json, _timing and _free serve both;
 * _timing here: G1 transforms, G1 column sums, uploads and the h differences, G2 transform and sums, serialisation).  It fails before any
 * device work when the file's power is below the circuit's domain; a larger file is fine.
 * zk_groth16_params_contribute: out (len bytes) = the key with delta_g1, delta_g2 multiplied by delta and every point of l and h by
 * 1 / delta.  delta: 4 x u64 canonical, non-zero, or NULL to draw it from the operating system; it is overwritten on the host and on the
 * device before the call returns.  zk_groth16_contribution_check -> a JSON report: sections that must be byte-equal ("changed", "size"),
 * the classes of the new delta, l and h points, delta_g1 against delta_g2 ("delta_mismatch"), and l, h scaled by exactly the ratio of the
 * two deltas ("not_scaled").
 * zk_groth16_contribution_check holds for ANY ratio of the two deltas that its presenter knows -- the delta = 1 key scaled by a known k passes
 * as the successor of any key -- so a chain of contributions carries proofs of knowledge in a transcript beside the key (bellman's layout
 * has no room for one): "zkgk", u32 version = 1, u32 n8, u32 count, SHA-256 of the initial key; per contribution SHA-256 of the new key,
 * delta_g1 after, R, z (32 B canonical little-endian) and a chain hash; points in the key's encoding; the proof is Schnorr's over base
 * delta_g1 before and image delta_g1 after (csrc/groth16_ceremony.hip.h has the hashes).  zk_groth16_params_contribute_pok is
 * zk_groth16_params_contribute plus the appended record: t_len = 0 starts a transcript with this key as the initial one, otherwise the
 * transcript must end at this key; out_transcript takes zk_groth16_key_transcript_size(curve, count + 1) bytes; out_params may be params.
 * zk_groth16_key_transcript_check -> a JSON report (malloc'ed, zk_string_free): "initial_key_mismatch" (the transcript starts at another
 * key), "chain_hash" {contribution}, "pok_invalid" {contribution}, "final_key_mismatch" (the last delta_g1, or the last key hash, is not
 * the final key's), and zk_groth16_contribution_check(initial, final) under "keys" -- that check holds for any ratio, so the intermediate
 * keys are not needed.  Whether the initial key is a delta = 1 key of its circuit stays zk_groth16_key_check_srs's question.
 * zk_groth16_key_check_srs -> a JSON report (malloc'ed, zk_string_free): is this key a key for this circuit over this file?  What
 * zk_groth16_key_check cannot see: every query (a, b_g1, b_g2, ic, l, h) against the circuit's polynomials at the file's tau, each by one
 * random linear combination over the wires (weights of 128 bits; a wrong section survives with probability 2^-128) -- multi-scalar sums
 * against the file's sections as they stand, no group transform; ic and l are paired against the key's own gamma_g2 and delta_g2, h against
 * delta_g2, so any gamma and any chain of contributions to delta pass.  Findings: {"kind":"query_mismatch","section":..,"first_index":k,
 * "wire":j} (the first entry of the section that is wrong, by bisection; no "wire" for h) and {"kind":"vk_mismatch","field":"alpha_g1" |
 * "beta_g1" | "beta_g2"} (word for word against alphaTauG1[0], betaTauG1[0], betaG2).  A section of the wrong length or with a point
 * that is off its curve, outside the subgroup or out of range is not compared and is listed under "skipped"; run zk_groth16_key_check for
 * those findings and zk_srs_check for the file's.  Errors (NULL, zk_last_error): the readers' texts, a file of a power below the circuit's
 * domain, a file opened for another curve.  seed: 32 bytes, tests only; NULL = the operating system's randomness.  With
 * ZK_KEY_CHECK_TIMING set the report carries "timing_ms" {parse, row_sums, transforms, sums, pairings}. */
typedef struct zk_srs zk_srs_t;
zk_srs_t* zk_srs_open(const char* curve, const char* path);
int zk_srs_info(const zk_srs_t* s, uint32_t* power, uint32_t* ceremony_power);
char* zk_srs_check(const zk_srs_t* s, const uint8_t* seed, uint32_t max_findings);
int zk_srs_free(zk_srs_t* s);
int zk_srs_new(const char* curve, uint32_t power, const char* path);
int zk_srs_contribute(const zk_srs_t* s, const char* out_path, const uint64_t* secrets, const uint8_t* beacon_seed, uint32_t beacon_iter_log);
char* zk_srs_verify(const zk_srs_t* s, const uint8_t* seed, uint32_t max_findings);
int zk_srs_transcript_count(const zk_srs_t* s, int64_t* count);
int zk_g1_bn254_ntt_dev(void* d_points, uint32_t log_n, int inverse, void* stream);
int zk_g2_bn254_ntt_dev(void* d_points, uint32_t log_n, int inverse, void* stream);
int zk_g1_bls12_381_ntt_dev(void* d_points, uint32_t log_n, int inverse, void* stream);
int zk_g2_bls12_381_ntt_dev(void* d_points, uint32_t log_n, int inverse, void* stream);
int zk_g1_bn254_mul_scalar_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g2_bn254_mul_scalar_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g1_bls12_381_mul_scalar_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g2_bls12_381_mul_scalar_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g1_bn254_mul_scalars_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g2_bn254_mul_scalars_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g1_bls12_381_mul_scalars_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g2_bls12_381_mul_scalars_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g1_bn254_mul_scalars_glv_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
int zk_g1_bls12_381_mul_scalars_glv_dev(const void* d_points, uint64_t n, const uint64_t* d_k, void* d_out, void* stream);
zk_groth16_keygen_t* zk_groth16_keygen_from_srs(const char* curve, const void* r1cs, size_t r1cs_len, const zk_srs_t* srs);
int zk_groth16_params_contribute(const char* curve, const void* params, size_t len, const uint64_t* delta, void* out);
size_t zk_groth16_key_transcript_size(const char* curve, uint32_t count);
int zk_groth16_params_contribute_pok(const char* curve, const void* params, size_t len, const uint64_t* delta, const void* transcript, size_t t_len, void* out_params,
                                     void* out_transcript);
char* zk_groth16_key_transcript_check(const char* curve, const void* initial, size_t initial_len, const void* final_key, size_t final_len, const void* transcript,
                                      size_t t_len, const uint8_t* seed, uint32_t max_findings);
char* zk_groth16_contribution_check(const char* curve, const void* old_params, size_t old_len, const void* new_params, size_t new_len, const uint8_t* seed,
                                    uint32_t max_findings);
char* zk_groth16_key_check_srs(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const zk_srs_t* srs, const uint8_t* seed,
                                uint32_t max_findings);

/* ---- pairings and Groth16 verification (`zkit groth16_verify`, zkit/src/main.rs:221-230, groth16/src/api.rs:302-341 ->
 * bellman's prepare_verifying_key + verify_proof) --------------------------------------------------------------------
 * zk_pairing_*: n pairs (g1[i], g2[i]) in the point layout of the multi-scalar sums (affine, Montgomery; the all-zero
 * encoding is the point at infinity and gives 1) -> n values of GT, each 12 canonical little-endian Fq (32 B / 48 B):
 * c0, c1 of the Fq2 coefficient of w^0, then of w^1 .. w^5, in Fq12 = Fq2[w]/(w^6 - xi), Fq2 = Fq[u]/(u^2 + 1), xi = 9 + u
 * (BN254) / 1 + u (BLS12-381).  with_final_exp = 0 stops after the Miller loop (a value defined up to factors the final
 * exponentiation removes).  The optimal ate pairing as pairing_ce computes it (BLS12-381: conjugated for the negative
 * curve parameter).  Points are taken as they are: no curve or subgroup check here.
 * zk_groth16_vk_new parses verification_key.json as zk_groth16_keygen_vk_json writes it and json_utils.rs reads it
 * (decimal or 0x strings), checks every point of it (curve, subgroup) and keeps on the device e(alpha, beta), the line
 * tables of -gamma and -delta and the IC points; NULL on error (zk_last_error).  The handle owns them: zk_groth16_vk_free.
 * zk_groth16_verify_batch: n proofs, each A || B || C exactly as zk_groth16_prove writes its `proof` argument, and
 * n x n_public x 32 B canonical public inputs (n_public = len(IC) - 1, zk_groth16_vk_info) -> n verdicts.  One verdict per
 * proof; the checks are stricter than the reference's, which reads points unchecked (json_utils.rs:163-198): proof points
 * must be on their curve and in the subgroup of order r ([r]P = O), inputs must be below r.
 * zk_groth16_verify_json: the file-level form, proof.json and public_input.json -> the verdict, or ZK_VERDICT_ERROR
 * (zk_last_error) when a file cannot be read as what it should be.
 * zk_pairing_product_*: prod_i e(g1[i], g2[i]) as ONE value of GT in the layout above (n = 0: one), through single-pair
 * Miller loops, a product reduction in a fixed order and one final exponentiation.
 * zk_groth16_verify_aggregate: the same n proofs and inputs as zk_groth16_verify_batch, ONE answer: *verdict =
 * ZK_VERDICT_ACCEPTED when every proof is well formed and
 *     prod_i e([rho_i]A_i, B_i) . e(sum_i rho_i X_i, -gamma) . e(sum_i rho_i C_i, -delta) . e([sum_i rho_i]alpha, -beta) = 1
 * for secret weights rho_i of 128 bits (X_i = IC_0 + sum_j pub_ij IC_j): one short scalar product and one single-pair Miller
 * loop per proof, one final exponentiation per batch.  A batch that holds a wrong proof is accepted with probability about
 * 2^-128 over the weights.  seed: 32 bytes from which the weights are derived, FOR TESTS ONLY; NULL -- the only value to use
 * anywhere else -- draws them from the operating system, and a caller who can predict them can make wrong proofs cancel.
 * On refusal with first_bad != NULL the per-proof path runs: *first_bad = the index of the first proof it does not accept
 * and *verdict = that proof's code; with first_bad == NULL nothing is located and *verdict = ZK_VERDICT_REJECTED.  Accepted
 * batches leave *first_bad = n.  n = 0 is accepted.  The well-formedness rules and their codes are the per-proof path's.
 * zk_groth16_verify_aggregate_timing: ms[6] = host milliseconds of the calling thread's last aggregate call spent in the
 * checks, the scalar products, lines and Miller loops, the product, the sums, the tail -- measured (with a stream
 * synchronisation after every phase) only while the environment holds ZK_VERIFY_AGG_TIMING.
 * zk_groth16_proof_words: proof.json and public_input.json through the library's readers -> the words
 * zk_groth16_verify_batch takes (proof_out: proof_bytes; public_out: n_public x 32 B); returns ZK_VERDICT_ACCEPTED, or
 * ZK_VERDICT_INPUT_COUNT / ZK_VERDICT_INPUT_NOT_CANONICAL as zk_groth16_verify_json would, or ZK_VERDICT_ERROR.        */
enum {
    ZK_VERDICT_ACCEPTED = 1,
    ZK_VERDICT_REJECTED = 0,              /* well-formed, the equation does not hold */
    ZK_VERDICT_INPUT_NOT_CANONICAL = -1,  /* a public input >= r */
    ZK_VERDICT_INPUT_COUNT = -2,          /* number of public inputs != len(IC) - 1 */
    ZK_VERDICT_NOT_ON_CURVE = -3,         /* A, B or C not on its curve */
    ZK_VERDICT_NOT_IN_SUBGROUP = -4,      /* on the curve, not of order r */
    ZK_VERDICT_ERROR = -100               /* the call itself failed */
};
int zk_pairing_bn254(const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp);
int zk_pairing_bn254_dev(const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream);
int zk_pairing_bls12_381(const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp);
int zk_pairing_bls12_381_dev(const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream);
typedef struct zk_groth16_vk zk_groth16_vk_t;
zk_groth16_vk_t* zk_groth16_vk_new(const char* curve, const char* vk_json);
int zk_groth16_vk_info(const zk_groth16_vk_t* vk, uint32_t* n_public, uint32_t* proof_bytes, uint32_t* gt_bytes);
int zk_groth16_vk_free(zk_groth16_vk_t* vk);
int zk_groth16_verify_batch(const zk_groth16_vk_t* vk, const void* proofs, const void* publics, uint64_t n, int* verdicts);
int zk_groth16_verify_batch_dev(const zk_groth16_vk_t* vk, const void* d_proofs, const void* d_publics, uint64_t n, int* d_verdicts, void* stream);
int zk_groth16_verify_json(const zk_groth16_vk_t* vk, const char* proof_json, const char* public_input_json);
int zk_pairing_product_bn254(const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp);
int zk_pairing_product_bn254_dev(const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream);
int zk_pairing_product_bls12_381(const void* g1, const void* g2, uint64_t n, void* gt_out, int with_final_exp);
int zk_pairing_product_bls12_381_dev(const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, void* stream);
int zk_groth16_verify_aggregate(const zk_groth16_vk_t* vk, const void* proofs, const void* publics, uint64_t n, const uint8_t* seed, int* verdict, uint64_t* first_bad);
int zk_groth16_verify_aggregate_dev(const zk_groth16_vk_t* vk, const void* d_proofs, const void* d_publics, uint64_t n, const uint8_t* seed, int* verdict,
                                    uint64_t* first_bad, void* stream);
int zk_groth16_verify_aggregate_timing(double* ms);
int zk_groth16_proof_words(const zk_groth16_vk_t* vk, const char* proof_json, const char* public_input_json, void* proof_out, void* public_out);
const char* zk_groth16_verdict_name(int verdict);

/* ---- compressor12 exec (recursion/src/compressor12/compressor12_exec.rs:17-103) ----------------
 * The step between a recursive circuit's circom witness and the committed trace of its STARK: the PlonkAdd sums
 * appended to the witness (:60-66) and the s_map gather into the 12 columns of Compressor.a (:72-94).
 * zk_c12_exec_new takes the text of the .exec file (a JSON array of u64, compressor12_setup.rs:51-83) and the length of
 * the circuit's witness; zk_c12_exec_dev writes the [n_rows][12] matrix (the .cm file's content; rows beyond
 * s_map_column_len are zero) from a witness of one u64 per wire, both in HBM -- ready for zk_stark_gen_dev.            */
typedef struct zk_c12_exec zk_c12_exec_t;
zk_c12_exec_t* zk_c12_exec_new(const char* exec_json, size_t len, uint64_t n_witness);
int zk_c12_exec_dev(const zk_c12_exec_t* e, const uint64_t* d_witness, uint64_t n_witness, uint64_t n_rows, uint64_t* d_cm, void* stream);
uint64_t zk_c12_exec_depth(const zk_c12_exec_t* e);   /* launches of the addition phase (longest chain of dependent sums) */
int zk_c12_exec_free(zk_c12_exec_t* e);

/* ---- compressor12 setup (`zkit compressor12_setup`, zkit/src/main.rs:140-151; recursion/src/compressor12/plonk_setup.rs) ----
 * From the R1CS of a recursive circuit over Goldilocks (8-byte field; custom gates Poseidon12, CMulAdd, FFT4, EvPol4) to what
 * zk_c12_exec_new and the following proof consume: the compressor's .pil text, its .exec text and its constant matrix.
 * zk_c12_setup_new reads the file and does the host part (R1CS -> PLONK gates and additions in the reference's order, the
 * packing of gates into rows); force_n_bits = 0 takes the smallest power of two that holds the rows.  NULL on error
 * (zk_last_error), e.g. "Invalid magic number", "Different prime", "Invalid custom gate X", "wire id does not fit 32 bits".
 * zk_c12_setup_consts_dev writes the [2^n_bits][n_const] row-major matrix into caller HBM: the S columns, their wiring and
 * the fill are kernels (the layout of the .const file, polsarray.rs:184-); zk_c12_setup_consts the same to host memory.
 * zk_c12_setup_gates: n_gates x (sl, sr, so, qm, ql, qr, qo, qc).  The two texts are malloc'ed: zk_string_free.
 * zk_c12_sigma_dev is the wiring on its own: d_s_map is any [n_used][12] map of 32-bit wire ids (0 = no wire; row i,
 * column c at 12 i + c, the .exec order) in HBM; it writes S[c][i] = w^i k^c with the copy constraints applied into columns
 * [col0, col0 + 12) of the [2^n_bits][n_const] matrix d_out and touches no other column.                                      */
typedef struct zk_c12_setup zk_c12_setup_t;
zk_c12_setup_t* zk_c12_setup_new(const void* r1cs, size_t len, uint32_t force_n_bits);
uint32_t zk_c12_setup_n_bits(const zk_c12_setup_t* s);
uint64_t zk_c12_setup_n_publics(const zk_c12_setup_t* s);
uint64_t zk_c12_setup_n_used(const zk_c12_setup_t* s);
uint64_t zk_c12_setup_n_const(const zk_c12_setup_t* s);
uint64_t zk_c12_setup_n_gates(const zk_c12_setup_t* s);
uint64_t zk_c12_setup_n_adds(const zk_c12_setup_t* s);
int zk_c12_setup_gates(const zk_c12_setup_t* s, uint64_t* out);
char* zk_c12_setup_pil(const zk_c12_setup_t* s);
char* zk_c12_setup_exec(const zk_c12_setup_t* s);
int zk_c12_setup_consts_dev(const zk_c12_setup_t* s, uint64_t* d_out, void* stream);
int zk_c12_setup_consts(const zk_c12_setup_t* s, uint64_t* out);
int zk_c12_setup_free(zk_c12_setup_t* s);
int zk_c12_sigma_dev(const uint32_t* d_s_map, uint64_t n_used, uint32_t n_bits, uint32_t n_const, uint32_t col0, uint64_t* d_out, void* stream);

/* ---- constraint evaluation (starky/src/interpreter.rs:91-225, stark_gen.rs:752-963) ------------
 * A step's program is the reference's Segment.first (Vec<Section{op,dest,src}>,
 * starkinfo_codegen.rs:76-89) with every Node resolved to an address exactly as
 * interpreter.rs get_ref/set_ref/eval_map do (:286-524): section cells become
 * (buffer slot, column offset, row stride, prime); tmp/number/public/challenge/eval/x/Zi/xDivXSub*
 * keep their meaning.  zk_program_compile translates it to a gfx950 kernel (hipRTC) once;
 * zk_program_run_dev evaluates it for every row i of the domain, reading rows (i + next*prime) % N.
 * Value widths (the F3G dim) are inferred from the operands: dim-1 op dim-1 -> 1, anything with a
 * dim-3 operand -> 3 (f3g.rs:323-449); a dim-3 result written to a section cell occupies 3 words,
 * a dim-1 result 1 word (interpreter.rs:149-159).
 *
 * Two evaluators stand behind the same zk_program_t (zk_program_kind says which):
 *   ZK_EVAL_JIT       zk_program_compile: the program becomes HIP text, compiled by hipRTC (seconds per step program of a
 *                     large PIL, once per text: the code-object cache).  The fastest evaluation; the default.
 *   ZK_EVAL_BYTECODE  zk_program_assemble: the program becomes bytecode for ONE interpreter kernel that is part of
 *                     libzkgpu.so.  Nothing is compiled at run time: no hipRTC, no helper process, no cache; the values are the
 *                     same canonical words.  zk_program_source returns its listing: one line per instruction, then a
 *                     summary line "; slots: <words> (lds <words>, arena <words>) ...".  Temporaries live in slots numbered by
 *                     liveness (per-wave LDS first, a pooled arena in HBM past the LDS budget: no program is too large).
 *                     It executes in program order, so a read that partially overlaps an earlier write of the same row,
 *                     which zk_program_compile rejects (it hoists reads), is accepted; every other rejection is shared.
 * zk_eval_set_mode chooses, for the calling thread, what the NEXT zk_stark_setup_new builds its step and public programs
 * with (the setup keeps its mode for life); it returns the previous mode (-1 and no change for an unknown mode).  A thread
 * starts with $ZK_EVAL = "jit" | "bytecode" (default jit).                                               */
enum { ZK_EVAL_JIT = 0, ZK_EVAL_BYTECODE = 1 };
enum { ZK_OP_ADD = 0, ZK_OP_SUB = 1, ZK_OP_MUL = 2, ZK_OP_COPY = 3 };
enum { ZK_OPND_TMP = 0, ZK_OPND_MEM = 1, ZK_OPND_NUMBER = 2, ZK_OPND_PUBLIC = 3, ZK_OPND_CHALLENGE = 4,
       ZK_OPND_EVAL = 5, ZK_OPND_X = 6, ZK_OPND_ZI = 7, ZK_OPND_XDIVXSUBXI = 8, ZK_OPND_XDIVXSUBWXI = 9 };
typedef struct {
    uint8_t kind;     /* ZK_OPND_*                                                            */
    uint8_t dim;      /* MEM: width of the cell (1 or 3); ignored for the other kinds          */
    uint8_t prime;    /* MEM: read row (i + next) % N                                          */
    uint8_t buf;      /* MEM: slot in zk_eval_ctx.bufs                                         */
    uint32_t id;      /* TMP: id; MEM: column offset; PUBLIC/CHALLENGE/EVAL: index             */
    uint32_t stride;  /* MEM: words per row of the section                                     */
    uint32_t _pad;
    uint64_t value;   /* NUMBER: canonical value                                               */
} zk_operand;
typedef struct { uint32_t op; uint32_t _pad; zk_operand dest; zk_operand src[2]; } zk_instr;
typedef struct {
    uint64_t* bufs[16];            /* device base pointers of the sections the program touches  */
    const uint64_t* publics;       /* [n_publics]                                               */
    const uint64_t* challenges;    /* [8][3]  (constant.rs:39-50)                               */
    const uint64_t* evals;         /* [n_evals][3]                                              */
    const uint64_t* x;             /* x_n or x_2ns, [N]                                         */
    const uint64_t* zi;            /* ZHInv table, [zi_mask + 1]                                */
    uint64_t zi_mask;
    const uint64_t* xdivxsubxi;    /* [N][3]                                                    */
    const uint64_t* xdivxsubwxi;   /* [N][3]                                                    */
} zk_eval_ctx;
typedef struct zk_program zk_program_t;
zk_program_t* zk_program_compile(const zk_instr* code, uint32_t n_instr);    /* needs no GPU */
zk_program_t* zk_program_assemble(const zk_instr* code, uint32_t n_instr);   /* needs no GPU, no hipRTC */
int zk_program_kind(const zk_program_t* p);                                   /* ZK_EVAL_* */
int zk_eval_set_mode(int mode);
const char* zk_program_source(const zk_program_t* p);                         /* generated HIP text / bytecode listing */
/* what the code-object cache of the step kernels did so far in this process: out = {compiled by hipRTC, taken from
 * $ZK_JIT_CACHE (default ~/.cache/zkgpu; "off" disables), taken from memory} */
void zk_jit_cache_stats(uint64_t out[3]);
int zk_program_run_dev(zk_program_t* p, const zk_eval_ctx* ctx, uint32_t nbits_domain, uint64_t next, void* stream);
/* The same for rows row0 .. row0 + count - 1 only (the domain is still 2^nbits_domain rows: primed reads wrap around it).
 * calculate_exp_at_point (stark_gen.rs:558-572) is this with count = 1: a public calculator is evaluated at its one row. */
int zk_program_run_rows_dev(zk_program_t* p, const zk_eval_ctx* ctx, uint32_t nbits_domain, uint64_t next, uint64_t row0, uint64_t count,
                            void* stream);
int zk_program_free(zk_program_t* p);

/* ---- pil_verify: a trace against its PIL, row by row (csrc/pil_check.hip) ------------------------------------------
 * The check the reference runs between building a trace and proving it (starkjs/src/pil_verifier.js:46, pilcom's
 * verifyPil): the PIL's own constraints -- expressions, polIdentities, plookupIdentities, permutationIdentities,
 * connectionIdentities, publics -- on domain n, before any of the prover's rewriting; no starkStruct, no setup, no
 * challenges.  N is the common polDeg of the PIL's references, `next` reads row (i + 1) mod N.
 * zk_pil_check_new parses the compiled PIL (.pil.json text), generates the check programs and assembles them for the
 * bytecode interpreter (always: $ZK_EVAL does not matter, nothing is compiled at run time); it needs no GPU.
 * zk_pil_check_listing: the assembled programs, one line per instruction ("check1 idK <- value" closes polynomial
 * identity K), owned by the handle.
 * zk_pil_check_run / _run_dev: the report, JSON text (malloc'ed: zk_string_free):
 *   {"n": N, "publics": ["..."], "checked": {"polIdentities": a, "plookupIdentities": b, "permutationIdentities": c,
 *    "connectionIdentities": d}, "findings": [...]}
 * Rows, counts and field words are decimal strings.  Every finding has "kind", "index" (of the identity in its list),
 * "fileName" and "line"; polynomial identities come first, then plookups, permutations, connections, each in PIL order:
 *   identity          n_rows, first_row, value            rows where the expression is not 0, the smallest, the value there
 *   selector          identity ("plookup" | "permutation"), side ("f" | "t"), n_rows, first_row, value: a selector outside
 *                     {0, 1}; listed in front of its identity's own finding (for the set checks a row is selected when the
 *                     selector is not 0)
 *   plookup           n_rows, first_row, values           selected f rows whose tuple no selected t row holds
 *   permutation       n_f_unmatched, n_t_unmatched, first_f_row, first_t_row, f_values, t_values (null on a side nothing
 *                     is unmatched on): with c = #t rows - #f rows per distinct tuple, the sum of |c| over c < 0 and of c
 *                     over c > 0, the smallest selected row of each side whose tuple has such a c
 *   connection_value  n_cells, col, row, value            S words that name no cell k_j w^i; first by col * N + row
 *   connection        n_cells, col, row, partner_col, partner_row, value, partner_value: wired cells that differ
 * The run borrows device-resident inputs ([N][nConstants] and [N][nCommitments], row-major).  NULL + zk_last_error on
 * error: n_rows != polDeg, an expression id out of range, a set identity whose sides differ in length, a polDeg that
 * is not a power of two. */
typedef struct zk_pil_check zk_pil_check_t;
zk_pil_check_t* zk_pil_check_new(const char* pil_json);                      /* needs no GPU */
const char* zk_pil_check_listing(const zk_pil_check_t* c);
char* zk_pil_check_run(zk_pil_check_t* c, const uint64_t* const_pols, const uint64_t* cm_pols, uint64_t n_rows);
char* zk_pil_check_run_dev(zk_pil_check_t* c, const uint64_t* d_const_pols, const uint64_t* d_cm_pols, uint64_t n_rows, void* stream);
int zk_pil_check_free(zk_pil_check_t* c);

/* ---- wtns_check: a witness against its R1CS (csrc/r1cs_check.hip) ----------------------------------------------------
 * What `snarkjs wtns check` answers, on the device and for the three fields of this pipeline; neither the reference nor
 * bellman checks a witness (the prover divides (A w)(B w) - C w by Z and drops the remainder).  No proving key is needed.
 * field: "BN128" | "BLS12381" (the scalar fields, 32-byte values) | "GL" (Goldilocks, 8-byte values, the compressor's circuits).
 * Checked: every constraint of the file's section 2 as written and in file order -- the rows the Groth16 circuit leaves
 * unenforced included, bellman's appended `input * 0 = 0` rows not --, w[0] = 1, and over "GL" every use of the custom gates
 * CMulAdd, Poseidon12, FFT4, EvPol4 (sections 4 and 5, resolved by template name as zk_c12_setup_new resolves them).
 * zk_r1cs_check_new reads the file with the readers of zk_groth16_setup_new / zk_c12_setup_new (same error texts) and puts the
 * three matrices on the device in CSR form.  zk_r1cs_check_info: n_public = public outputs + public inputs (wire 0 not counted).
 * zk_r1cs_check_run: `witness` = n_values values, little-endian canonical, 32 B or 8 B each; _run_dev: the same already in HBM
 * (taken as canonical, as zk_groth16_prove_dev takes its witness).  The report, JSON text (malloc'ed: zk_string_free):
 *   {"field": "GL", "n_wires": n, "n_constraints": m,
 *    "checked":   {"constraint": m, "cmuladd": a, "poseidon12": b, "fft4": c, "evpol4": d},
 *    "n_failing": {"one_wire": 0 | 1, "constraint": ., "cmuladd": ., "poseidon12": ., "fft4": ., "evpol4": .},
 *    "findings": [
 *      {"kind": "one_wire", "value": "2"},
 *      {"kind": "constraint", "index": 17, "a": "..", "b": "..", "c": "..",            the three row sums; a b != c
 *       "wires": {"a": [[wire, "coefficient"], ..], "b": [..], "c": [..]}},           the row as the reader keeps it: by ascending wire
 *      {"kind": "poseidon12", "use": u, "row": j, "column": i, "wire": w, "expected": "..", "value": ".."},
 *      {"kind": "cmuladd" | "fft4" | "evpol4", "use": u, "position": k, "wire": w, "expected": "..", "value": ".."}]}
 * Field values are decimal strings.  Kinds come in the order above; within a kind the findings ascend by index and there are at
 * most max_findings of them; the n_failing counts are exact whatever max_findings is.  "use" counts the uses of section 5 in file
 * order.  A gate finding names the first output that differs from what the use's inputs force: "position" counts the outputs
 * (CMulAdd s[9 + k], FFT4 s[12 + k], EvPol4 s[18 + k]); Poseidon12 checks each of the 30 transitions from the witness' own
 * row j and names (j, column) of the first wrong cell of row j + 1.  "wire" is the signal at that output.
 * NULL + zk_last_error on error: n_values != n_wires, a host value that is not below the modulus (zk_groth16_prove's message),
 * an unknown field, every fault of the readers, custom gates in a 32-byte-field file.  A handle is bound to the device
 * current at its creation and is not re-entrant: one run at a time per handle. */
typedef struct zk_r1cs_check zk_r1cs_check_t;
zk_r1cs_check_t* zk_r1cs_check_new(const char* field, const void* r1cs, size_t len);
int zk_r1cs_check_info(const zk_r1cs_check_t* c, uint32_t* n_wires, uint64_t* n_constraints, uint64_t* n_custom_uses, uint32_t* n_public);
char* zk_r1cs_check_run(zk_r1cs_check_t* c, const void* witness, uint64_t n_values, uint32_t max_findings);
char* zk_r1cs_check_run_dev(zk_r1cs_check_t* c, const void* d_witness, uint64_t n_values, uint32_t max_findings);
int zk_r1cs_check_free(zk_r1cs_check_t* c);

/* ---- groth16_key_check: a Groth16 proving key against its circuit (csrc/groth16.hip, csrc/key_check_impl.hip.h) ----------
 *
 * zk_groth16_setup_new reads a key as the reference does (read_pk_from_file(path, checked = false)): no point is looked at.
 * zk_groth16_key_check reads the same two files with the same readers (same error texts when a file cannot be parsed: NULL and
 * zk_last_error) and returns a report as JSON text (zk_string_free):
 *   {"curve", "n_wires", "n_public", "domain_log", "sections": {"ic", "h", "l", "a", "b_g1", "b_g2": lengths},
 *    "checked": {"g1_points", "g2_points", "pairs"}, "skipped": [{"check", "section", "reason"}],
 *    "counts": {kind: number of findings, exact}, "findings": [...at most max_findings per kind; kind by kind in the order below, and within a
 *    kind in the order of the sections...]}
 *   size              {"section", "have", "want"}: a section's length against the circuit's (ic = public wires + 1, l = the rest,
 *                     h = 2^domain_log - 1, a / b_g1 / b_g2 = what bellman's density trackers count); the key of another circuit stops here
 *   infinity, coordinate_range, not_on_curve, not_in_subgroup
 *                     {"section", "n_points", "first_index"} per section: alpha_g1 beta_g1 beta_g2 gamma_g2 delta_g1 delta_g2 (one
 *                     point each), ic, h, l, a, b_g1, b_g2.  A point has the first class that applies.  Infinity is a finding in every
 *                     section, as bellman's Parameters::read refuses it there.
 *   g1_g2_mismatch    {"section": "beta" | "delta" | "b", "first_index"}: e(P1, G2) != e(G1, P2).  b: one random linear combination
 *                     of 128-bit factors over both queries (a wrong pair passes with probability 2^-128), then the smallest failing
 *                     prefix by bisection.  Skipped (and listed under "skipped") when a section holds an invalid point or the lengths differ.
 *   vk_mismatch       {"field"}: a field of verification_key.json (vk_json, may be NULL) against the key's embedded copy
 * seed: 32 bytes from which the factors are expanded on the device.  FOR TESTS ONLY: pass NULL anywhere else, and the factors come from
 * the operating system (getrandom); a caller who can predict them can make a wrong pair pass.
 * NOT checked: h, l, ic and a against the circuit's polynomials.  That needs tau in G2 or the trapdoor; "no findings" means well formed
 * and self-consistent, and the functional test remains a proof that verifies.
 *
 * zk_points_check_*: the per-point part on its own.  group: 1 = G1, 2 = G2; points: n affine points in the layout of the
 * multi-scalar sums (Montgomery; all zero = infinity), as zk_pairing_* take them; plain != 0: [r]P = O bit by bit instead of the
 * endomorphism tests (same answer; the comparator).  out: 4 x 2 words -- for ZK_POINT_INFINITY .. ZK_POINT_NOT_IN_SUBGROUP the
 * exact number of points of the class and the smallest index of one (all ones when there is none). */
enum { ZK_POINT_INFINITY = 0, ZK_POINT_COORDINATE_RANGE = 1, ZK_POINT_NOT_ON_CURVE = 2, ZK_POINT_NOT_IN_SUBGROUP = 3, ZK_POINT_CLASSES = 4 };
char* zk_groth16_key_check(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const char* vk_json,
                           const uint8_t* seed, uint32_t max_findings);
int zk_points_check_bn254(int group, const void* points, uint64_t n, int plain, uint64_t* out);
int zk_points_check_bn254_dev(int group, const void* d_points, uint64_t n, int plain, uint64_t* d_out, void* stream);
int zk_points_check_bls12_381(int group, const void* points, uint64_t n, int plain, uint64_t* out);
int zk_points_check_bls12_381_dev(int group, const void* d_points, uint64_t n, int plain, uint64_t* d_out, void* stream);

/* ---- KZG commitments over a powers-of-tau file: commit, open, verify (csrc/kzg.hip, csrc/kzg_impl.hip.h) ----------
 * The family of snarkjs `ffs` / `fff` / `ffv` (test/snark_verifier.sh:67-106: PLONK, fflonk) stands on two operations over the tauG1
 * section of a .ptau file: C = [p(tau)] G1, and for a point z the value y = p(z) with the witness W = [q(tau)] G1, q = (p - y) / (X - z).
 * Commitments are in G1 and are NOT hiding: no blinding term is added, C is a function of p alone.
 * Polynomials are coefficient vectors, lowest degree first, in the layout zk_fr_<curve>_ntt_dev keeps (4 x u64 Montgomery R = 2^256 per
 * coefficient).  A point z and a value y are 32 B canonical little-endian, below r.  A commitment or witness on the device is the point
 * in the layout of the sums followed by the 4-byte infinity word (zk_msm_*_dev's d_out); on the host the all-zero encoding is infinity.
 * zk_kzg_<curve>_divide_dev needs no file: d_q[j] = sum_{i > j} d_coeffs[i] z^(i - j - 1) for j < n - 1 (same layout as d_coeffs; may be
 *   NULL: evaluation only, nothing but y is written) and d_y = p(z) (32 B canonical, device).  z is read from HOST memory before the call
 *   returns.  A tiled scan of affine maps (z^len, value): zk_kzg_tile_elems() coefficients per workgroup, the tile aggregates combined by
 *   one workgroup that walks them zk_kzg_aggregate_span() at a time.  No inverse of z (z = 0 is fine), no atomics, bit-exact.
 * zk_kzg_<curve>_lincomb_dev: d_out[j] = sum_i gamma^i p_i[j] for j < max n_i; d_polys, n: HOST arrays of k device pointers / lengths;
 *   shorter polynomials count as zero-padded; gamma 32 B canonical on the host.
 * zk_kzg_new uploads tauG1[0, max_coeffs) of the file once (max_coeffs = 0: all 2^(power + 1) - 1; more than the file has is an error
 *   raised before any device work), keeps G2 and -tauG2[1], and builds window tables for the sums when there are fewer than 2^24 points
 *   (the policy of zk_groth16_setup_new).  The file is trusted as zk_groth16_keygen_from_srs trusts it: run zk_srs_check first.
 * zk_kzg_commit_dev: n <= max_coeffs; n = 0 and the zero polynomial give infinity.  zk_kzg_commit_evals_dev: the commitment to the
 *   polynomial of degree < 2^log_n whose values on the domain of zk_fr_<curve>_ntt are d_evals (same layout), through the Lagrange basis
 *   iNTT(tauG1[0, 2^log_n)) in the group, made on first use of a log_n and cached in the handle; 2^log_n <= max_coeffs, log_n <= power.
 * zk_kzg_open_dev: d_y_out (32 B canonical, device) and d_w_out = [q(tau)] G1; n <= 1 gives W = infinity.
 * zk_kzg_open_many_dev: d_ys_out = the k values p_i(z) and one witness for f = sum_i gamma^i p_i.  The verifier folds: C = sum gamma^i C_i
 *   (zk_kzg_fold_commitments: host points in, one host point out; an all-zero point is infinity), y = sum gamma^i y_i.
 * zk_kzg_verify: m openings, each C || z || y || W (point_bytes + 32 + 32 + point_bytes, host; _dev: device).  With weights rho_j
 *   (m = 1: rho = 1; m > 1: secret, 128 bits) L = sum rho_j C_j - [sum rho_j y_j] G1 + sum [rho_j z_j] W_j, R = sum rho_j W_j, and the
 *   batch is accepted when e(L, G2) e(R, -tau G2) = 1: two Miller loops and one final exponentiation whatever m is.  A batch that holds a
 *   wrong opening is accepted with probability about 2^-128 over the weights.  seed: as in zk_groth16_verify_aggregate -- 32 bytes, FOR
 *   TESTS ONLY, NULL anywhere else.  Verdicts are the ZK_VERDICT_* codes: C and W must be on the curve (a coordinate >= q counts as off
 *   it) and in the subgroup, infinity is legal for both, z and y must be below r (ZK_VERDICT_INPUT_NOT_CANONICAL).  On refusal with
 *   first_bad != NULL the openings are checked one by one: *first_bad = the first one not accepted, *verdict = its code; with first_bad ==
 *   NULL *verdict = ZK_VERDICT_REJECTED.  Accepted batches leave *first_bad = m.  m = 0 is accepted.  Both forms synchronise.
 * A handle is bound to the device current at its creation and is not re-entrant: one call at a time per handle, from any thread or stream
 *   (the Lagrange basis of a log_n is made, and waited for, inside the first zk_kzg_commit_evals_dev that asks for it).
 * Not built: hiding commitments, commitments in G2.  Openings at several points: the next section.                                   */
typedef struct zk_kzg zk_kzg_t;
uint64_t zk_kzg_tile_elems(void);
uint64_t zk_kzg_aggregate_span(void);
int zk_kzg_bn254_divide_dev(const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_q, uint64_t* d_y, void* stream);
int zk_kzg_bls12_381_divide_dev(const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_q, uint64_t* d_y, void* stream);
int zk_kzg_bn254_lincomb_dev(const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, const uint64_t* gamma, uint64_t* d_out, void* stream);
int zk_kzg_bls12_381_lincomb_dev(const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, const uint64_t* gamma, uint64_t* d_out, void* stream);
zk_kzg_t* zk_kzg_new(const zk_srs_t* srs, uint64_t max_coeffs);
int zk_kzg_free(zk_kzg_t* k);
int zk_kzg_info(const zk_kzg_t* k, const char** curve, uint64_t* max_coeffs, uint32_t* power, uint32_t* point_bytes, uint32_t* opening_bytes);
int zk_kzg_commit_dev(zk_kzg_t* k, const uint64_t* d_coeffs, uint64_t n, void* d_out, void* stream);
int zk_kzg_commit_evals_dev(zk_kzg_t* k, const uint64_t* d_evals, uint32_t log_n, void* d_out, void* stream);
int zk_kzg_eval_dev(zk_kzg_t* k, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_y_out, void* stream);
int zk_kzg_open_dev(zk_kzg_t* k, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_y_out, void* d_w_out, void* stream);
int zk_kzg_open_many_dev(zk_kzg_t* k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* z, const uint64_t* gamma,
                         uint64_t* d_ys_out, void* d_w_out, void* stream);
int zk_kzg_fold_commitments(zk_kzg_t* k, const void* commitments, uint32_t n, const uint64_t* gamma, void* out);
int zk_kzg_verify(zk_kzg_t* k, const void* openings, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad);
int zk_kzg_verify_dev(zk_kzg_t* k, const void* d_openings, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad, void* stream);

/* ---- KZG: several polynomials at several points in one two-point proof (csrc/kzg.hip) ---------------------------------
 * The opening of Boneh, Drake, Fisch, Gabizon 2020 section 4 ("Shplonk"), which is the whole commitment scheme of snarkjs `ffs` / `fff` /
 * `ffv` (fflonk; test/snark_verifier.sh:81-105): polynomials f_0 .. f_(k-1) with commitments C_i, each opened on its own set S_i of
 * 1 .. ZK_KZG_MULTI_MAX_POINTS distinct points; T is the union of the sets.  With r_i the interpolant of the values on S_i and Z_S the
 * vanishing polynomial of S:
 *   W1 = [q(tau)] G1,              q = sum_i gamma^i (f_i - r_i) / Z_(S_i)
 *   W2 = [(L / (X - z))(tau)] G1,  L = sum_i w_i (f_i - r_i(z)) - Z_T(z) q,  w_i = gamma^i Z_(T \ S_i)(z),  for a z outside T
 *   verifier: F = sum_i w_i C_i - [sum_i w_i r_i(z)] G1 - Z_T(z) W1 and e(F + z W2, G2) e(-W2, tau G2) = 1
 * The quotient by Z_S is never formed as such: (f - r_S) / Z_S = sum_(s in S) a_s (f - f(s)) / (X - s) with a_s = 1 / prod_(s' != s) (s - s'),
 * so every term is the single-point division of the section above, added into a running sum by its last phase.
 * Building blocks (no file):
 * zk_kzg_<curve>_divide_acc_dev: d_acc_inout[j] += w q_j for j < n - 1, q = (p - p(z)) / (X - z), and d_y = p(z) (32 B canonical, device).
 *   d_acc_inout is in the layout of d_coeffs and holds at least n - 1 elements; elements from n - 1 on are not touched.  z, w: 32 B canonical
 *   on the host, read before the call returns.  n <= 1 writes d_y alone.
 * zk_kzg_<curve>_interleave_dev: d_out[j k + i] = p_i[j] for j < max n_i, zero where p_i is shorter: sum_i p_i(X^k) X^i, fflonk's
 *   combination.  d_polys, n: HOST arrays of k device pointers / lengths (k <= 65536); d_out holds k max n_i elements and overlaps no input.
 * The prover is staged because z is a challenge that depends on W1 (the style of zk_stark_new .. finish):
 * zk_kzg_multi_begin: d_polys, n: HOST arrays of k device pointers / lengths; the polynomials stay where they are, unchanged, until
 *   zk_kzg_multi_finish has returned.  points: the sets one after another, 32 B canonical each, HOST; set_sizes: k counts.  d_values_out
 *   (device, may be NULL) receives f_i(s) in the order of `points`, 32 B canonical each.  Returns NULL -- before any device work -- for k = 0,
 *   an empty set, a set of more than ZK_KZG_MULTI_MAX_POINTS points, a point >= r, a point repeated within a set, a polynomial longer than
 *   the handle's max_coeffs.  The powers table of every point is kept for the next stage.
 * zk_kzg_multi_quotient: gamma 32 B canonical, HOST; d_w1_out = W1 (a sum's result slot).  A polynomial with n_i <= |S_i| is its own
 *   interpolant and adds nothing; q = 0 gives infinity.  q stays in the handle.
 * zk_kzg_multi_finish: z 32 B canonical, HOST; refused when z is in T.  d_w2_out = W2.  Before it returns it checks on the host, from the
 *   evaluations the divisions leave, that L(z) = sum w_i f_i(z) - Z_T(z) q(z) - sum w_i r_i(z) is zero, and fails with an internal-error
 *   text when it is not.  The stages run once each, in this order, and synchronise; a handle is used by one call at a time, and the zk_kzg_t
 *   it was made from outlives it.
 * zk_kzg_multi_verify: m proofs, one after another in `bytes` bytes (HOST; _dev: device memory, copied first).  One proof is
 *     u64 k | k x C_i (point_bytes) | k x u64 |S_i| | P x point (32 B) | P x value (32 B) | gamma (32 B) | z (32 B) | W1 | W2
 *   with P = sum |S_i|, points and values set by set, integers little-endian, scalars canonical, points as zk_kzg_verify takes them (all
 *   zero: infinity, legal for C_i, W1 and W2).  The host derives w_i, sum w_i r_i(z) and Z_T(z); one small sum per proof gives F_j; the
 *   openings (F_j, z_j, 0, W2_j) go through the batched check of zk_kzg_verify (rho = 1 for m = 1, 128-bit weights otherwise; seed FOR
 *   TESTS ONLY).  Verdicts: k = 0, a set size outside 1 .. ZK_KZG_MULTI_MAX_POINTS, a point repeated within a set and z in T give
 *   ZK_VERDICT_INPUT_COUNT; a point, value, gamma or z >= r gives ZK_VERDICT_INPUT_NOT_CANONICAL; then the points' classes as in
 *   zk_kzg_verify; then ZK_VERDICT_REJECTED.  first_bad as in zk_kzg_verify: the proofs one by one, the first not accepted.  A buffer that
 *   ends inside a proof, or after the m-th, is an error of the call.                                                                      */
#define ZK_KZG_MULTI_MAX_POINTS 16
typedef struct zk_kzg_multi zk_kzg_multi_t;
int zk_kzg_bn254_divide_acc_dev(const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, const uint64_t* w, uint64_t* d_acc_inout, uint64_t* d_y, void* stream);
int zk_kzg_bls12_381_divide_acc_dev(const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, const uint64_t* w, uint64_t* d_acc_inout, uint64_t* d_y, void* stream);
int zk_kzg_bn254_interleave_dev(const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, uint64_t* d_out, void* stream);
int zk_kzg_bls12_381_interleave_dev(const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, uint64_t* d_out, void* stream);
zk_kzg_multi_t* zk_kzg_multi_begin(zk_kzg_t* k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* points,
                                   const uint32_t* set_sizes, uint64_t* d_values_out, void* stream);
int zk_kzg_multi_quotient(zk_kzg_multi_t* m, const uint64_t* gamma, void* d_w1_out, void* stream);
int zk_kzg_multi_finish(zk_kzg_multi_t* m, const uint64_t* z, void* d_w2_out, void* stream);
int zk_kzg_multi_free(zk_kzg_multi_t* m);
int zk_kzg_multi_verify(zk_kzg_t* k, const void* proofs, uint64_t bytes, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad);
int zk_kzg_multi_verify_dev(zk_kzg_t* k, const void* d_proofs, uint64_t bytes, uint64_t m, const uint8_t* seed, int* verdict, uint64_t* first_bad, void* stream);

/* ---- Polynomial arithmetic over the scalar field (csrc/frpoly_impl.hip.h) ----------------------------------------------
 * What a PLONK-family prover, a lookup argument or a batched opening is made of, and nothing of a protocol: no transcript, no soundness
 * claim.  <curve> is bn254 or bls12_381.  A vector is n x 4 u64 Montgomery words (R = 2^256), element-major, on the device and 16-byte
 * aligned: the layout of zk_fr_<curve>_ntt_dev and zk_kzg_<curve>_divide_dev; input words may be anything those leave.  EVERY OUTPUT
 * VECTOR HOLDS THE CANONICAL REPRESENTATIVE (< r): results are bit-exact and the same on every run.  A scalar argument (base, scale, beta,
 * gamma) is 4 canonical u64 words on the HOST; one that is not below r is refused before any device work.  A host result (total_out,
 * last_out) is 4 canonical words of the plain integer, not Montgomery; a call that fills a host result waits for the stream.
 * zk_fr_<curve>_prefix_product_dev: out[i] = prod_{j < i} in[j] (inclusive = 0, so out[0] = 1) or prod_{j <= i} in[j]; total_out = prod in.
 *   d_out == NULL: the total alone.  n = 0: total 1.  d_out may be d_in.  A zero element is an ordinary value.  A tiled scan:
 *   zk_frpoly_tile_elems() elements per workgroup, the tile aggregates combined by one workgroup that walks them zk_frpoly_span() at a time.
 * zk_fr_<curve>_prefix_sum_dev: out[i] = sum_{j < i} in[j] (inclusive = 0, so out[0] = 0) or sum_{j <= i} in[j]; total_out = sum in.  The
 *   same tiles and the same argument rules under addition: d_out == NULL the total alone, n = 0 total 0, d_out may be d_in.
 * zk_fr_<curve>_batch_inverse_dev: out[i] = 1 / in[i]; a zero stays zero and does not disturb its neighbours.  n_zero, first_zero (HOST,
 *   either may be NULL): how many zeros, the index of the first (UINT64_MAX when none).  d_out may be d_in.  One inversion per tile.
 * zk_fr_<curve>_pointwise_dev: out[i] = a[i] op b[i], op one of ZK_FR_MUL, ZK_FR_ADD, ZK_FR_SUB; d_out may be either operand.
 * zk_fr_<curve>_powers_dev: out[i] = scale base^i; base = 0 gives scale, 0, 0, ...
 * zk_fr_<curve>_terms_dev: out[i] = prod_{c < k} (cols_c[i] + beta labels_c[i] + gamma), 1 <= k <= 16; d_cols, d_labels: HOST arrays of k
 *   device pointers; d_labels == NULL drops the beta term.
 * zk_fr_<curve>_grand_product_dev: z_0 = 1, z_(i+1) = z_i num_i / den_i; d_z receives z_0 .. z_(n-1), last_out z_n: "the two products
 *   agree" is last_out == 1, which the caller compares.  A zero denominator is refused with its first row named and d_z untouched.  d_z may
 *   be d_num.
 * zk_fr_<curve>_poly_mul_dev: the na + nb - 1 coefficients of a b (na, nb >= 1; leading zeros kept) by two forward transforms of the next
 *   power of two, a pointwise product and one inverse transform; a length beyond the field's 2-adicity is refused.  d_out overlaps no input.
 * zk_fr_<curve>_divmod_zh_dev: p = q (X^N - 1) + rem for N = 2^log_n, exactly: rem (N elements, zero-padded when n_p < N) and q
 *   (max(n_p - N, 0) elements); d_q or d_rem may be NULL, d_q overlaps no input.  rem_nonzero (HOST): the number of non-zero remainder
 *   coefficients -- zero exactly when X^N - 1 divides p.  Additions only.  ceil(n_p / N) > ZK_FRPOLY_MAX_RATIO is refused.
 * zk_fr_<curve>_divide_zh_coset_dev: d_evals holds values on the coset 7 H_m in the order zk_fr_<curve>_ntt_dev(.., coset = 1) leaves them,
 *   m = 2^log_m >= N = 2^log_n; element i is multiplied in place by 1 / (7^N w_m^(iN) - 1), the m / N distinct factors made on the device.
 * Not built: the prover that stands on this (gate constraints, transcript, blinding).                                                    */
#define ZK_FR_MUL 0
#define ZK_FR_ADD 1
#define ZK_FR_SUB 2
#define ZK_FRPOLY_MAX_RATIO 4096
uint64_t zk_frpoly_tile_elems(void);
uint64_t zk_frpoly_span(void);
int zk_fr_bn254_prefix_product_dev(const uint64_t* d_in, uint64_t n, int inclusive, uint64_t* d_out, uint64_t* total_out, void* stream);
int zk_fr_bls12_381_prefix_product_dev(const uint64_t* d_in, uint64_t n, int inclusive, uint64_t* d_out, uint64_t* total_out, void* stream);
int zk_fr_bn254_prefix_sum_dev(const uint64_t* d_in, uint64_t n, int inclusive, uint64_t* d_out, uint64_t* total_out, void* stream);
int zk_fr_bls12_381_prefix_sum_dev(const uint64_t* d_in, uint64_t n, int inclusive, uint64_t* d_out, uint64_t* total_out, void* stream);
int zk_fr_bn254_batch_inverse_dev(const uint64_t* d_in, uint64_t n, uint64_t* d_out, uint64_t* n_zero, uint64_t* first_zero, void* stream);
int zk_fr_bls12_381_batch_inverse_dev(const uint64_t* d_in, uint64_t n, uint64_t* d_out, uint64_t* n_zero, uint64_t* first_zero, void* stream);
int zk_fr_bn254_pointwise_dev(int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, uint64_t n, void* stream);
int zk_fr_bls12_381_pointwise_dev(int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, uint64_t n, void* stream);
int zk_fr_bn254_powers_dev(const uint64_t* base, const uint64_t* scale, uint64_t n, uint64_t* d_out, void* stream);
int zk_fr_bls12_381_powers_dev(const uint64_t* base, const uint64_t* scale, uint64_t n, uint64_t* d_out, void* stream);
int zk_fr_bn254_terms_dev(const uint64_t* const* d_cols, const uint64_t* const* d_labels, uint32_t k, uint64_t n, const uint64_t* beta, const uint64_t* gamma,
                          uint64_t* d_out, void* stream);
int zk_fr_bls12_381_terms_dev(const uint64_t* const* d_cols, const uint64_t* const* d_labels, uint32_t k, uint64_t n, const uint64_t* beta, const uint64_t* gamma,
                              uint64_t* d_out, void* stream);
int zk_fr_bn254_grand_product_dev(const uint64_t* d_num, const uint64_t* d_den, uint64_t n, uint64_t* d_z, uint64_t* last_out, void* stream);
int zk_fr_bls12_381_grand_product_dev(const uint64_t* d_num, const uint64_t* d_den, uint64_t n, uint64_t* d_z, uint64_t* last_out, void* stream);
int zk_fr_bn254_poly_mul_dev(const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* d_out, void* stream);
int zk_fr_bls12_381_poly_mul_dev(const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* d_out, void* stream);
int zk_fr_bn254_divmod_zh_dev(const uint64_t* d_p, uint64_t n_p, uint32_t log_n, uint64_t* d_q, uint64_t* d_rem, uint64_t* rem_nonzero, void* stream);
int zk_fr_bls12_381_divmod_zh_dev(const uint64_t* d_p, uint64_t n_p, uint32_t log_n, uint64_t* d_q, uint64_t* d_rem, uint64_t* rem_nonzero, void* stream);
int zk_fr_bn254_divide_zh_coset_dev(uint64_t* d_evals, uint32_t log_m, uint32_t log_n, void* stream);
int zk_fr_bls12_381_divide_zh_coset_dev(uint64_t* d_evals, uint32_t log_m, uint32_t log_n, void* stream);

/* ---- The device side of the PLONK prover (csrc/plonk_impl.hip.h) ---------------------------------------------------------
 * The three kernels the prover of eigen_zkvm_amd/plonk.py adds to the layer above; the protocol itself (rounds, transcript, keys, files) is
 * Python over these calls, as Kzg.open_multi is over zk_kzg_multi_*.  Vectors, scalars and <curve> as for the polynomial layer: n x 4 u64
 * Montgomery words on the device, 16-byte aligned, input words anything below 2^256; scalars 4 canonical u64 words on the HOST, refused before
 * any device work when not below r; every output vector canonical.
 * zk_plonk_<curve>_quotient_dev: the numerator of the quotient on the coset 7 H_m, m = 4n = 4 2^log_n, in the order
 *   zk_fr_<curve>_ntt_dev(.., coset = 1) leaves it.  d_cols: a HOST array of ZK_PLONK_QUOTIENT_COLS (15) device pointers to m elements each,
 *   in this order: a, b, c, Z, q_L, q_R, q_O, q_M, q_C, S_sigma1, S_sigma2, S_sigma3, PI, L_1, X.  out[i] =
 *     a b q_M + a q_L + b q_R + c q_O + q_C + PI
 *     + alpha ((a + beta X + gamma)(b + beta k1 X + gamma)(c + beta k2 X + gamma) Z
 *              - (a + beta S_sigma1 + gamma)(b + beta S_sigma2 + gamma)(c + beta S_sigma3 + gamma) Z[(i + 4) mod m])
 *     + alpha^2 L_1 (Z - 1)
 *   at element i of every column.  d_out (m elements) overlaps no column.  log_n + 2 beyond the field's 2-adicity is refused.  One lane per
 *   element, one launch; the division by Z_H is zk_fr_<curve>_divide_zh_coset_dev(d_out, log_n + 2, log_n).
 * zk_plonk_<curve>_gate_check_dev: the gate equation row by row over n rows.  d_cols: a HOST array of ZK_PLONK_GATE_COLS (9) device pointers
 *   in the order a, b, c, q_L, q_R, q_O, q_M, q_C, PI (the wire VALUES, the selectors' values on H).  n_bad (HOST): the number of rows with
 *   q_L a + q_R b + q_O c + q_M a b + q_C + PI != 0, exact; first_bad (HOST): the first of them, UINT64_MAX when none.  Waits for the stream.
 * zk_fr_<curve>_gather_dev: out[i] = src[idx[i]] for i < n; d_idx: n uint32 on the device; d_out overlaps no source element.  An index that is
 *   not below n_src reads nothing and leaves zero; the call then fails with their number and the first position.  Waits for the stream.
 * Not built: a linearisation polynomial, the split of the quotient, a one-call C prover.  Lookups: the section after fflonk's.  A custom gate:
 * the next-row term, the last section of this header.                                                                                       */
#define ZK_PLONK_QUOTIENT_COLS 15
#define ZK_PLONK_GATE_COLS 9
int zk_plonk_bn254_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                const uint64_t* k1, const uint64_t* k2, uint64_t* d_out, void* stream);
int zk_plonk_bls12_381_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                    const uint64_t* k1, const uint64_t* k2, uint64_t* d_out, void* stream);
int zk_plonk_bn254_gate_check_dev(const uint64_t* const* d_cols, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* stream);
int zk_plonk_bls12_381_gate_check_dev(const uint64_t* const* d_cols, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* stream);
int zk_fr_bn254_gather_dev(const uint64_t* d_src, uint64_t n_src, const uint32_t* d_idx, uint64_t n, uint64_t* d_out, void* stream);
int zk_fr_bls12_381_gather_dev(const uint64_t* d_src, uint64_t n_src, const uint32_t* d_idx, uint64_t n, uint64_t* d_out, void* stream);

/* ---- The device side of the fflonk prover (csrc/fflonk_impl.hip.h) --------------------------------------------------------
 * The one kernel the prover of eigen_zkvm_amd/fflonk.py adds: fflonk commits to the three quotients of the identity apart, so their numerators
 * leave one launch apart where zk_plonk_<curve>_quotient_dev folds them with alpha.  Vectors, scalars, <curve> and d_cols (the same
 * ZK_PLONK_QUOTIENT_COLS columns in the same order, on the coset 7 H_m, m = 4n = 4 2^log_n) as above.  At element i of every column
 *   d_out0[i] = a b q_M + a q_L + b q_R + c q_O + q_C + PI
 *   d_out1[i] = L_1 (Z - 1)
 *   d_out2[i] = (a + beta X + gamma)(b + beta k1 X + gamma)(c + beta k2 X + gamma) Z
 *               - (a + beta S_sigma1 + gamma)(b + beta S_sigma2 + gamma)(c + beta S_sigma3 + gamma) Z[(i + 4) mod m]
 * every one canonical.  An output may be NULL (not all three): that part is not computed and the columns it alone reads are not read, though
 * every column pointer must still be valid -- T0 is committed before beta and gamma exist, so the prover takes d_out0 in round 1 and the other
 * two in round 2.  An output (m elements each) overlaps no column and no other output; a scalar that is not below r and log_n + 2 beyond
 * the field's 2-adicity are refused before any device work.  One lane per element, one launch; each output is then divided by Z_H with
 * zk_fr_<curve>_divide_zh_coset_dev(d_out, log_n + 2, log_n).                                                                              */
int zk_fflonk_bn254_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1,
                                  const uint64_t* k2, uint64_t* d_out0, uint64_t* d_out1, uint64_t* d_out2, void* stream);
int zk_fflonk_bls12_381_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1,
                                      const uint64_t* k2, uint64_t* d_out0, uint64_t* d_out1, uint64_t* d_out2, void* stream);

/* ---- The device side of PLONK's lookup argument (csrc/plonk_lookup_impl.hip.h) -------------------------------------------
 * What the prover of eigen_zkvm_amd/plonk_lookup.py adds: the log-derivative argument.  A row of the gate table with q_K = 1 claims that
 * (a, b, c) is a row (t1, t2, t3) of a table; with f = a + eta b + eta^2 c, t = t1 + eta t2 + eta^2 t3 and m_j the number of selected rows
 * that equal table row j, the claim holds exactly when sum_i q_K,i / (delta + f_i) = sum_j m_j / (delta + t_j) for random eta, delta.
 * Vectors, scalars and <curve> as for the polynomial layer; every output vector canonical; results are integers of the field, the same on
 * every run.  The running sum is zk_fr_<curve>_prefix_sum_dev, the inverses are zk_fr_<curve>_batch_inverse_dev.
 * zk_plonk_<curve>_lookup_table_new: the T >= 1 rows (d_t1[j], d_t2[j], d_t3[j]) as an open-addressing hash table on the device; NULL +
 *   zk_last_error() on failure; T > ZK_PLONK_LOOKUP_MAX_ROWS is refused.  The key of a row is the CANONICAL value of its three elements: the
 *   encodings v and v + r are one key.  The hash is FNV-1a over the 24 u32 words of the canonical Montgomery representatives of t1, t2, t3
 *   (h = 0x811c9dc5; h = (h ^ word) * 0x01000193), then h ^= h >> 16; the slot is h & (slots - 1), slots the smallest power of two >= 2T;
 *   a collision walks to the next slot and wraps.  A slot is claimed by atomicCAS and keeps the SMALLEST row index of its key (atomicMin).
 *   The columns are read during the call's launches only; the handle is read-only afterwards and is freed by ..._lookup_table_free.
 * zk_plonk_<curve>_lookup_count_dev: one lane per row i < n.  A row whose q_K is not zero looks (a_i, b_i, c_i) up and adds 1 to the counter
 *   of the table row it finds (the smallest index of that key); d_m_out[j] (n elements, T <= n) receives the count of table row j as a field
 *   element, 0 from T on.  n_bad (HOST): the selected rows that are no row of the table, exact; first_bad (HOST): the first of them,
 *   UINT64_MAX when none.  The lanes of a wave that hit one counter are combined before the global atomic.  Waits for the stream.
 * zk_plonk_<curve>_lookup_terms_dev: d_cols: a HOST array of ZK_PLONK_LOOKUP_TERMS_COLS (6) device pointers to n elements each: a, b, c, t1,
 *   t2, t3.  d_out[i] = delta + a + eta b + eta^2 c and d_out[n + i] = delta + t1 + eta t2 + eta^2 t3 at row i: 2n elements, overlapping no
 *   column.
 * zk_plonk_<curve>_lookup_summands_dev: d_out[i] = q_K[i] inv[i] - m[i] inv[n + i]; d_inv holds 2n elements (the inverses of the terms);
 *   d_out (n elements) overlaps no input.
 * zk_plonk_<curve>_lookup_quotient_dev: on the coset 7 H_m, m = 4n = 4 2^log_n.  d_cols: a HOST array of ZK_PLONK_LOOKUP_QUOTIENT_COLS (9)
 *   device pointers to m elements each: a, b, c, q_K, t1, t2, t3, M, Phi.  With f and t as above at element i,
 *     d_acc[i] = d_acc[i] + alpha^3 ((Phi[(i + 4) mod m] - Phi[i]) (delta + f)(delta + t) - q_K (delta + t) + M (delta + f))
 *   in place, canonical on the way out; d_acc overlaps no column.  It runs after zk_plonk_<curve>_quotient_dev on that call's output and
 *   before the division by Z_H.  One lane per element, one launch.
 * Not built: tables of more or fewer than three columns, several tables in one circuit, lookups under fflonk, a one-call C prover.  (That is
 * these five calls; several tables in one circuit are the tagged calls that follow.)
 *
 * TAGGED lookups (csrc/plonk_lookup_tagged_impl.hip.h): several tables in one circuit.  Table row j is (T0_j, t1_j, t2_j,
 * t3_j), T0_j = k in 1 .. ZK_PLONK_LOOKUP_MAX_TABLES the number of its table; a gate row with q_K = k != 0 claims that (a, b, c) is a row of
 * table k.  f = a + eta b + eta^2 c + eta^3 q_K, t = t1 + eta t2 + eta^2 t3 + eta^3 T0, m_j = T0_j x (the selected rows whose (q_K, a, b, c)
 * equals (T0_j, t1_j, t2_j, t3_j)); the sum and the identity keep their form.  The summand and the running sum are the calls above.
 * zk_plonk_<curve>_lookup_tagged_table_new: as ..._lookup_table_new over four columns, d_t0 the tags as field elements.  A key is the 32 words
 *   of the canonical Montgomery representatives of T0, t1, t2, t3 in that order, hashed and stored as there: the same (t1, t2, t3) under two
 *   tags are two keys.  A tag outside 1 .. ZK_PLONK_LOOKUP_MAX_TABLES is refused, with the first such row and their count.  Waits for the
 *   stream.  The handle is freed by ..._lookup_table_free; ..._lookup_count_dev refuses it, as ..._lookup_tagged_count_dev refuses a plain one.
 * zk_plonk_<curve>_lookup_tagged_count_dev: as ..._lookup_count_dev, the key of a selected row being (q_K, a, b, c): a tuple that sits only in
 *   another table than the one q_K names is a miss.  d_m_out[j] = T0_j x the count of table row j, an integer below 2^46, as a field element.
 * zk_plonk_<curve>_lookup_tagged_terms_dev: d_cols: ZK_PLONK_LOOKUP_TAGGED_TERMS_COLS (8) pointers: a, b, c, q_K, t1, t2, t3, T0.
 *   d_out[i] = delta + a + eta b + eta^2 c + eta^3 q_K and d_out[n + i] = delta + t1 + eta t2 + eta^2 t3 + eta^3 T0 at row i.
 * zk_plonk_<curve>_lookup_tagged_quotient_dev: d_cols: ZK_PLONK_LOOKUP_TAGGED_QUOTIENT_COLS (10) pointers: a, b, c, q_K, t1, t2, t3, T0, M,
 *   Phi; d_acc as for ..._lookup_quotient_dev with the f and t of the tagged argument.
 * Not built for the tagged calls: tables of more than three columns.  Under fflonk: zk_fflonk_<curve>_lookup_tagged_quotients_dev below.    */
#define ZK_PLONK_LOOKUP_TERMS_COLS 6
#define ZK_PLONK_LOOKUP_QUOTIENT_COLS 9
#define ZK_PLONK_LOOKUP_MAX_ROWS 1073741824
#define ZK_PLONK_LOOKUP_TAGGED_TERMS_COLS 8
#define ZK_PLONK_LOOKUP_TAGGED_QUOTIENT_COLS 10
#define ZK_PLONK_LOOKUP_MAX_TABLES 65535
typedef struct zk_plonk_lookup_table zk_plonk_lookup_table_t;
zk_plonk_lookup_table_t* zk_plonk_bn254_lookup_table_new(const uint64_t* d_t1, const uint64_t* d_t2, const uint64_t* d_t3, uint64_t T, void* stream);
zk_plonk_lookup_table_t* zk_plonk_bls12_381_lookup_table_new(const uint64_t* d_t1, const uint64_t* d_t2, const uint64_t* d_t3, uint64_t T, void* stream);
int zk_plonk_bn254_lookup_table_free(zk_plonk_lookup_table_t* table);
int zk_plonk_bls12_381_lookup_table_free(zk_plonk_lookup_table_t* table);
int zk_plonk_bn254_lookup_count_dev(const zk_plonk_lookup_table_t* table, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, const uint64_t* d_qK, uint64_t n,
                                    uint64_t* d_m_out, uint64_t* n_bad, uint64_t* first_bad, void* stream);
int zk_plonk_bls12_381_lookup_count_dev(const zk_plonk_lookup_table_t* table, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, const uint64_t* d_qK, uint64_t n,
                                        uint64_t* d_m_out, uint64_t* n_bad, uint64_t* first_bad, void* stream);
int zk_plonk_bn254_lookup_terms_dev(const uint64_t* const* d_cols, uint64_t n, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out, void* stream);
int zk_plonk_bls12_381_lookup_terms_dev(const uint64_t* const* d_cols, uint64_t n, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out, void* stream);
int zk_plonk_bn254_lookup_summands_dev(const uint64_t* d_inv, const uint64_t* d_qK, const uint64_t* d_m, uint64_t n, uint64_t* d_out, void* stream);
int zk_plonk_bls12_381_lookup_summands_dev(const uint64_t* d_inv, const uint64_t* d_qK, const uint64_t* d_m, uint64_t n, uint64_t* d_out, void* stream);
int zk_plonk_bn254_lookup_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* eta, const uint64_t* delta, uint64_t* d_acc,
                                       void* stream);
int zk_plonk_bls12_381_lookup_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* eta, const uint64_t* delta, uint64_t* d_acc,
                                           void* stream);
zk_plonk_lookup_table_t* zk_plonk_bn254_lookup_tagged_table_new(const uint64_t* d_t0, const uint64_t* d_t1, const uint64_t* d_t2, const uint64_t* d_t3, uint64_t T, void* stream);
zk_plonk_lookup_table_t* zk_plonk_bls12_381_lookup_tagged_table_new(const uint64_t* d_t0, const uint64_t* d_t1, const uint64_t* d_t2, const uint64_t* d_t3, uint64_t T, void* stream);
int zk_plonk_bn254_lookup_tagged_count_dev(const zk_plonk_lookup_table_t* table, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, const uint64_t* d_qK, uint64_t n,
                                           uint64_t* d_m_out, uint64_t* n_bad, uint64_t* first_bad, void* stream);
int zk_plonk_bls12_381_lookup_tagged_count_dev(const zk_plonk_lookup_table_t* table, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, const uint64_t* d_qK, uint64_t n,
                                               uint64_t* d_m_out, uint64_t* n_bad, uint64_t* first_bad, void* stream);
int zk_plonk_bn254_lookup_tagged_terms_dev(const uint64_t* const* d_cols, uint64_t n, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out, void* stream);
int zk_plonk_bls12_381_lookup_tagged_terms_dev(const uint64_t* const* d_cols, uint64_t n, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out, void* stream);
int zk_plonk_bn254_lookup_tagged_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* eta, const uint64_t* delta, uint64_t* d_acc,
                                              void* stream);
int zk_plonk_bls12_381_lookup_tagged_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* eta, const uint64_t* delta,
                                                  uint64_t* d_acc, void* stream);

/* ---- The device side of the fflonk prover with lookups (csrc/fflonk_lookup_impl.hip.h) -----------------------------------
 * The one kernel the prover of eigen_zkvm_amd/fflonk_lookup.py adds -- that module is where the log-derivative argument lives under fflonk:
 * the lookup term is a fourth quotient there, so its numerator leaves the launch beside the three of zk_fflonk_<curve>_quotients_dev, with
 * a, b, c read once for all four.  Vectors, scalars and <curve> as above.  d_cols: a HOST array of ZK_FFLONK_LOOKUP_QUOTIENT_COLS (21) device
 * pointers to m = 4n = 4 2^log_n elements each, on the coset 7 H_m: the ZK_PLONK_QUOTIENT_COLS columns in their order, then q_K, t1, t2, t3,
 * M, Phi.  At element i of every column, with f = a + eta b + eta^2 c and t = t1 + eta t2 + eta^2 t3,
 *   d_out0[i], d_out1[i], d_out2[i] = exactly zk_fflonk_<curve>_quotients_dev's
 *   d_out3[i] = (Phi[(i + 4) mod m] - Phi[i]) (delta + f)(delta + t) - q_K (delta + t) + M (delta + f)
 * every one canonical.  An output may be NULL (not all four): that part is not computed and the columns it alone reads are not read, though
 * every column pointer must still be valid.  An output (m elements each) overlaps no column and no other output; a scalar that is not below r
 * and log_n + 2 beyond the field's 2-adicity are refused before any device work.  One lane per element, one launch; each output is then
 * divided by Z_H with zk_fr_<curve>_divide_zh_coset_dev(d_out, log_n + 2, log_n).
 * Not built: a one-call C prover, tables of another width.  Several tables in one circuit: the tagged call below.                       */
#define ZK_FFLONK_LOOKUP_QUOTIENT_COLS 21
int zk_fflonk_bn254_lookup_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1,
                                         const uint64_t* k2, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out0, uint64_t* d_out1, uint64_t* d_out2,
                                         uint64_t* d_out3, void* stream);
int zk_fflonk_bls12_381_lookup_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1,
                                             const uint64_t* k2, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out0, uint64_t* d_out1, uint64_t* d_out2,
                                             uint64_t* d_out3, void* stream);

/* ---- The device side of the fflonk prover with tagged lookups (csrc/fflonk_lookup_tagged_impl.hip.h) ---------------------
 * The one kernel the prover of eigen_zkvm_amd/fflonk_lookup_tagged.py adds: zk_fflonk_<curve>_lookup_quotients_dev with the tag column of
 * several tables in the lookup term.  d_cols: a HOST array of ZK_FFLONK_LOOKUP_TAGGED_QUOTIENT_COLS (22) device pointers to
 * m = 4n = 4 2^log_n elements each, on the coset 7 H_m: the ZK_FFLONK_LOOKUP_QUOTIENT_COLS columns in their order, then Tg, the table's tag
 * column (the T0 of the zk_plonk_<curve>_lookup_tagged_* calls).  At element i of every column, with f = a + eta b + eta^2 c + eta^3 q_K and
 * t = t1 + eta t2 + eta^2 t3 + eta^3 Tg,
 *   d_out0[i], d_out1[i], d_out2[i] = exactly zk_fflonk_<curve>_quotients_dev's
 *   d_out3[i] = (Phi[(i + 4) mod m] - Phi[i]) (delta + f)(delta + t) - q_K (delta + t) + M (delta + f)
 * every one canonical; d_out3 is what zk_plonk_<curve>_lookup_tagged_quotient_dev adds to a zero accumulator under alpha = 1.  Null outputs,
 * overlaps, scalars and log_n as for zk_fflonk_<curve>_lookup_quotients_dev.  One lane per element, one launch.
 * Not built: a one-call C prover, tables wider than three.                                                                                */
#define ZK_FFLONK_LOOKUP_TAGGED_QUOTIENT_COLS 22
int zk_fflonk_bn254_lookup_tagged_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1,
                                                const uint64_t* k2, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out0, uint64_t* d_out1,
                                                uint64_t* d_out2, uint64_t* d_out3, void* stream);
int zk_fflonk_bls12_381_lookup_tagged_quotients_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* beta, const uint64_t* gamma, const uint64_t* k1,
                                                    const uint64_t* k2, const uint64_t* eta, const uint64_t* delta, uint64_t* d_out0, uint64_t* d_out1,
                                                    uint64_t* d_out2, uint64_t* d_out3, void* stream);

/* ---- The R1CS import of the PLONK prover (csrc/plonk_r1cs_impl.hip.h) -----------------------------------------------------
 * A circom .r1cs over the curve's scalar field compiled to the gate table the prover takes, and the values of the auxiliary variables that
 * table adds, computed on the device from the witness at every proof.
 * The rule.  Wire w is variable w; auxiliaries follow from n_wires in emission order; wire 0 (the constant 1) is never a gate operand with a
 * non-zero selector; the publics are wires 1 .. n_pub_out + n_pub_in.  A side is normalised: equal wires added, zeros dropped, wire 0 taken
 * out as the constant k, the signals by ascending wire.  reduce(sig, keep): at most `keep` signals stay as they are; otherwise the first
 * m = len - keep + 1 signals (s_i, c_i) fold into auxiliaries x_1 .. x_(m-1), x_j = sum_{i <= j+1} c_i w[s_i] -- a PREFIX of the side's sum
 * over original wires -- by gate 1 (qL, qR, qO, qM, qC) = (c_1, c_2, -1, 0, 0) on (s_1, s_2, x_1) and gates j >= 2 (1, c_(j+1), -1, 0, 0)
 * on (x_(j-1), s_(j+1), x_j), leaving [(x_(m-1), 1)] and the untouched signals; one SEGMENT (first auxiliary, the m terms) per fold.
 * Constraint A B = C in file order, constants kA, kB, kC.  Linear (A or B without a signal): L = kA B_sig - C_sig (kB A_sig - C_sig when it
 * is B), normalised again, k0 = kA kB - kC; nothing left: no gate when k0 = 0, a refusal otherwise; else reduce(L, 3) and one gate
 * (c_1, c_2, c_3, 0, k0) on (s_1, s_2, s_3), missing operands variable 0 with coefficient 0.  Product: reduce(A, 1), reduce(B, 1),
 * reduce(C, 1) leaving (sA, fA), (sB, fB), (sC, fC) ((0, 0) when C has no signal), then qM = fA fB, qL = fA kB, qR = kA fB, qO = -fC,
 * qC = kA kB - kC on (sA, sB, sC).  origin[g] is the constraint of gate g.
 * zk_plonk_<curve>_r1cs_new: reads the file and applies the rule ON THE HOST; no device is touched.  NULL + zk_last_error() for a malformed
 *   file, a file over another field, a wire index that is not below n_wires, a table that needs a variable id of more than 32 bits, and a
 *   constraint 0 = k with k not zero (named by its index).
 * zk_plonk_<curve>_r1cs_info: out[ZK_PLONK_R1CS_INFO_WORDS] = n_wires, n_public, n_constraints, n_gates, n_aux, n_segments,
 *   max_segment_terms, n_segment_terms.  n_vars = n_wires + n_aux.
 * zk_plonk_<curve>_r1cs_tables: copies out, to HOST arrays of the sizes info gives: sel = q_L, q_R, q_O, q_M, q_C one after another, each
 *   n_gates x 4 canonical u64 words; a, b, c, origin: n_gates uint32 each; seg_first: n_segments uint32 (the first auxiliary of each);
 *   seg_ptr: n_segments + 1 offsets into the terms; seg_wire: n_segment_terms uint32; seg_coef: n_segment_terms x 4 canonical words.
 *   Term t >= 1 of segment s defines variable seg_first[s] + t - 1.
 * zk_plonk_<curve>_r1cs_extend_dev: d_w holds n_vars x 4 u64 words on the device, 16-byte aligned; elements 0 .. n_wires - 1 are the witness
 *   as Montgomery words (what zk_fr_<curve>_gather_dev reads); the call fills elements n_wires .. n_vars - 1 in the same form, canonical, and
 *   writes nothing below n_wires.  The segment table goes to the device on the first call and stays with the handle (one call at a time).
 *   One lane per segment of fewer than zk_plonk_r1cs_wave_min_terms() terms, one wave per longer segment.  Asynchronous on the stream.
 * Not built: folding a chain's last step into the product gate, Goldilocks circuits, a proving-key file.  A gate that reads the next row and
 * the import rule that uses it: the next section.                                                                                          */
#define ZK_PLONK_R1CS_INFO_WORDS 8
typedef struct zk_plonk_r1cs zk_plonk_r1cs_t;
uint64_t zk_plonk_r1cs_wave_min_terms(void);
zk_plonk_r1cs_t* zk_plonk_bn254_r1cs_new(const void* r1cs, size_t len);
zk_plonk_r1cs_t* zk_plonk_bls12_381_r1cs_new(const void* r1cs, size_t len);
int zk_plonk_bn254_r1cs_info(const zk_plonk_r1cs_t* h, uint64_t* out);
int zk_plonk_bls12_381_r1cs_info(const zk_plonk_r1cs_t* h, uint64_t* out);
int zk_plonk_bn254_r1cs_tables(const zk_plonk_r1cs_t* h, uint64_t* sel, uint32_t* a, uint32_t* b, uint32_t* c, uint32_t* origin, uint32_t* seg_first, uint64_t* seg_ptr,
                               uint32_t* seg_wire, uint64_t* seg_coef);
int zk_plonk_bls12_381_r1cs_tables(const zk_plonk_r1cs_t* h, uint64_t* sel, uint32_t* a, uint32_t* b, uint32_t* c, uint32_t* origin, uint32_t* seg_first, uint64_t* seg_ptr,
                                   uint32_t* seg_wire, uint64_t* seg_coef);
int zk_plonk_bn254_r1cs_extend_dev(zk_plonk_r1cs_t* h, uint64_t* d_w, void* stream);
int zk_plonk_bls12_381_r1cs_extend_dev(zk_plonk_r1cs_t* h, uint64_t* d_w, void* stream);
int zk_plonk_bn254_r1cs_free(zk_plonk_r1cs_t* h);
int zk_plonk_bls12_381_r1cs_free(zk_plonk_r1cs_t* h);

/* ---- PLONK with a next-row term (csrc/plonk_next_impl.hip.h) -------------------------------------------------------------
 * The device side of eigen_zkvm_amd/plonk_next.py: row i of the gate table satisfies
 *   q_L a + q_R b + q_O c + q_M a b + q_C + q_N c[(i + 1) mod n] + PI = 0,
 * the next row cyclic on H.  Vectors, scalars and <curve> as for zk_plonk_<curve>_quotient_dev.
 * zk_plonk_<curve>_next_quotient_dev: d_cols: a HOST array of ZK_PLONK_NEXT_QUOTIENT_COLS (16) device pointers to m = 4n elements each: the
 *   ZK_PLONK_QUOTIENT_COLS columns in their order, then q_N.  out[i] = what zk_plonk_<curve>_quotient_dev gives + q_N[i] c[(i + 4) mod m]: on
 *   the coset of 4n points c(wX) is c four elements on.  With q_N = 0 everywhere the output is that call's, word for word.  The same refusals;
 *   one lane per element, one launch.
 * zk_plonk_<curve>_next_gate_check_dev: d_cols: ZK_PLONK_NEXT_GATE_COLS (10) pointers to n elements: the ZK_PLONK_GATE_COLS columns in their
 *   order, then q_N.  n_bad: the rows i < n that fail the equation above, exact; first_bad: the first, UINT64_MAX when none.  Row n - 1 reads
 *   c[0].  Waits for the stream.
 * The chain rule: the R1CS import of the section above with a second way to fold.  Normalisation, the numbering of wires and auxiliaries,
 * origin, the linear and the product case, the refusals and folds of two signals (one gate (c_1, c_2, -1, 0, 0) on (s_1, s_2, x_1)) are that
 * section's.  A fold of m >= 3 signals (s_i, c_i) is chain(sig): k = ceil(m / 2) rows; row j = 1 .. k has (a, b) = (s_(2j-1), s_(2j)),
 * (q_L, q_R) = (c_(2j-1), c_(2j)) -- for odd m the last row has b = variable 0 and q_R = 0 --, q_O = 0 in row 1 and 1 after it, c = x_(j-1)
 * for j >= 2, q_N = -1 (that is r - 1), q_M = q_C = 0; k auxiliaries x_j = sum_{i <= min(2j, m)} c_i w[s_i], x_k the fold's value.  Row j
 * constrains the c of the row after it, so x_k must stand in c of the row emitted NEXT: row 1 of the next chain takes it (its c is free,
 * q_O = 0); the closing product gate has it when x_k is its C side; otherwise a row of its own follows, every selector zero and a = b =
 * variable 0, c = x_k.  Product constraint: the folds of two signals first, in the order A, B, C; then the chains in the order A, B, C;
 * then the landing row when the last chain is not C's; then the gate of the section above on (sA, sB, sC).  Linear constraint with L of at
 * most three signals: that section's one gate.  With m >= 4 signals: one chain CLOSED on itself: rows as above, but the last row has q_N = 0
 * and q_C = k0, there are k - 1 auxiliaries and nothing lands.  Every row outside a chain has q_N = 0; the last gate of a table never has
 * q_N != 0.  Segments: one per fold; a chain's holds its m terms, a closed chain's the first 2 (k - 1).  Term t >= 1 (from 0) of a segment
 * of m terms defines an auxiliary when t is odd or t = m - 1: variable seg_first[s] + t / 2 (rounded down).
 * zk_plonk_<curve>_next_r1cs_new: as zk_plonk_<curve>_r1cs_new under the chain rule.  The handle is read by zk_plonk_<curve>_r1cs_info (the
 *   same eight words), _r1cs_tables and _r1cs_free, and zk_plonk_<curve>_r1cs_extend_dev extends a witness by it: the same lane and wave
 *   kernels with a store step of 2, chosen by the handle.
 * zk_plonk_<curve>_next_r1cs_qn: qn: n_gates x 4 canonical u64 words on the HOST, q_N of every gate; refused for a handle of _r1cs_new.
 * Not built: the term in the fflonk and lookup provers, other custom gates, a linearisation polynomial, a one-call C prover, Rust
 * declarations.                                                                                                                              */
#define ZK_PLONK_NEXT_QUOTIENT_COLS 16
#define ZK_PLONK_NEXT_GATE_COLS 10
int zk_plonk_bn254_next_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                     const uint64_t* k1, const uint64_t* k2, uint64_t* d_out, void* stream);
int zk_plonk_bls12_381_next_quotient_dev(const uint64_t* const* d_cols, uint32_t log_n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                         const uint64_t* k1, const uint64_t* k2, uint64_t* d_out, void* stream);
int zk_plonk_bn254_next_gate_check_dev(const uint64_t* const* d_cols, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* stream);
int zk_plonk_bls12_381_next_gate_check_dev(const uint64_t* const* d_cols, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* stream);
zk_plonk_r1cs_t* zk_plonk_bn254_next_r1cs_new(const void* r1cs, size_t len);
zk_plonk_r1cs_t* zk_plonk_bls12_381_next_r1cs_new(const void* r1cs, size_t len);
int zk_plonk_bn254_next_r1cs_qn(const zk_plonk_r1cs_t* h, uint64_t* qn);
int zk_plonk_bls12_381_next_r1cs_qn(const zk_plonk_r1cs_t* h, uint64_t* qn);

#ifdef __cplusplus
}
#endif
#endif /* ZKGPU_H */
