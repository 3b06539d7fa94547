// The pairing curves (BN254, BLS12-381) as one table: what msm.hip, groth16.hip, pairing.hip and the C ABI (capi.hip) need of a curve, as
// data plus entry points.  To the curves what commit.h is to the hash types; no other unit sees it.  Each of the three units fills the
// slice of what it compiles (msm_ops, groth16_ops, pairing_ops below); identity, sizes and the scalar modulus live here, and curve_of()
// is the one place where a name becomes a curve.  The Groth16 handles of include/zkgpu.h ARE the library's objects (bottom of this file).
#pragma once
#include "zk_internal.h"

struct zk_groth16_setup;
struct zk_groth16_keygen;
struct zk_groth16_vk;
struct zk_srs;
struct zk_kzg;
struct zk_kzg_multi;
struct zk_plonk_r1cs;
struct zk_plonk_lookup_table;

namespace zk {

using Groth16Setup = ::zk_groth16_setup;
using Groth16Key = ::zk_groth16_keygen;
using Groth16Vk = ::zk_groth16_vk;
using Srs = ::zk_srs;
using Kzg = ::zk_kzg;
using KzgMulti = ::zk_kzg_multi;
using PlonkR1cs = ::zk_plonk_r1cs;
using PlonkLookupTable = ::zk_plonk_lookup_table;
namespace g16 { struct Circuit; struct Params; }
// what miller_kernel takes (pairing_impl.hip.h): up to three pairs per item -- G1 points, line tables and infinity words with their strides
struct MillerArgs {
    const u32* g1[3]; u64 g1_stride[3];
    const u32* lines[3]; u64 lines_stride[3];
    const u32* inf[3]; u64 inf_stride[3];
    int np;
};
struct Curve;

enum CurveId { CURVE_BN254, CURVE_BLS12_381 };
enum Group { G1, G2 };

// ---- msm.hip: the sums of one group.  Points affine (x, y), Fq in Montgomery form, little-endian limbs (G2: x.c0 || x.c1 || y.c0 || y.c1);
// scalars 32 B canonical; a result is one point and a flag word (1 = infinity)
struct GroupOps {
    void (*msm_dev)(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, hipStream_t st);
    void (*mul_generator_dev)(const u64* d_k, uint64_t n, void* d_bases, hipStream_t st);      // P_i = [k_i]G, k_i != 0, one u64 each
    // P_i = [k_i]G for n full-width scalars (4 x u64 canonical, < r; zero gives the all-zero encoding): a window table of the generator,
    // no doublings, one inversion per workgroup (fixedbase_impl.hip.h)
    void (*mul_generator_fr_dev)(const u64* d_k, uint64_t n, void* d_bases, hipStream_t st);
    // window tables for fixed bases (msm_impl.hip.h): table[w * n + i] = 2^(16 w) P_i; a sum over points [off, off + n) of it
    size_t (*fixed_table_bytes)(uint64_t n);
    void (*fixed_prepare_dev)(const void* d_bases, uint64_t n, void* d_table, hipStream_t st);
    void (*fixed_dev)(const void* d_table, uint64_t table_n, uint64_t off, const void* d_scalars, uint64_t n, void* d_out, hipStream_t st);
    void (*generator_words)(u32* out);                                     // host: the generator as one affine point in the layout of the sums
};
struct MsmOps {
    GroupOps g[2];                                                          // by Group
    void (*fq_canon_to_mont_dev)(void* d, uint64_t n, hipStream_t st);      // n base-field elements in place: canonical integers <-> Montgomery
    void (*fq_mont_to_canon_dev)(void* d, uint64_t n, hipStream_t st);
};
// ---- groth16.hip: the scalar field's transforms and the prover / key generation built on them
struct KcMatrix { const u64* ptr; const u32* cols; const u32* coef; u64 n_rows; };   // one matrix by rows on the device; coef as kc_coef_dev leaves it
struct Groth16Ops {
    // bellman's EvaluationDomain::{fft, ifft, coset_fft, icoset_fft} on 2^logn Fr elements (4 x u64 Montgomery), in place
    void (*fr_ntt_dev)(u64* d_data, int logn, bool inverse, bool coset, hipStream_t st);
    // a <- coefficients of (A B - C) / (X^n - 1) from the row evaluations a, b, c (prover.rs create_proof's h block)
    void (*fr_quotient_dev)(u64* d_a, const u64* d_b, const u64* d_c, int logn, hipStream_t st);
    Groth16Setup* (*setup_new)(const Curve& cv, const g16::Circuit& C, const g16::Params& pk);
    void (*keygen_run)(const Curve& cv, const g16::Circuit& C, const u32* td, std::vector<uint8_t>& out, double* ms);
    // verify_sums_impl.hip.h: rho (n x 8 words) and inputs (n x n_pub x 8 canonical words) -> s_0 = sum rho_i, s_j = sum rho_i pub_ij mod r as
    // (n_pub + 1) x 8 canonical words, then n_pub + 1 words: per column the number of inputs that are not below r
    void (*verify_sums_dev)(const void* d_rho, const void* d_pub, uint64_t n, uint32_t n_pub, void* d_out, hipStream_t st);
    // key_check_srs_impl.hip.h: n coefficients of 8 canonical words -> the 9 words a term the row sums read; and for one matrix and the weights
    // rho (8 words each, 128 bits) the coefficient vectors iNTT(M rho) over the public wires below bound, over the others below bound, and
    // (d_sum, may be null) over both: 2^logm x 8 canonical words each.  ms (may be null): += milliseconds of the row sums, of the transforms
    void (*kc_coef_dev)(const u32* d_canon, u64 n, u32* d_fe, hipStream_t st);
    void (*kc_coeffs_dev)(const KcMatrix& M, const u32* d_rho, u32 ni, u32 bound, int logm, u32* d_pub, u32* d_aux, u32* d_sum, double* ms, hipStream_t st);
    // ceremony_impl.hip.h: out_i = s t^(i0 + i), i < n, as 8 canonical words each; d_tab: 30 x 8 words Montgomery (fr_host.h): s, then t^(2^j), j < 29
    void (*powers_dev)(const u32* d_tab, u64 i0, u64 n, u32* d_out, hipStream_t st);
    // n Fr elements (4 x u64 Montgomery, the transforms' layout) -> the canonical scalars the sums take (8 words each): the prover's two
    // layout kernels back to back (frntt_impl.hip.h)
    void (*fr_to_canon_dev)(const u64* d_mont, u64 n, u32* d_canon, hipStream_t st);
};
// ---- kzg.hip: the polynomial side of a KZG opening over the scalar field (kzg_impl.hip.h)
struct KzgOps {
    // y = p(z) (8 canonical words, device) and, when d_q is not null, q_j = sum_{i > j} c_i z^(i - j - 1), j < n - 1: Montgomery words as the
    // coefficients are, or with q_canon the canonical scalars of the sums.  z: 8 canonical words on the host, below r
    // d_table: the block table_dev made for the same z (table_bytes() bytes: the square chain of z and z^0 .. z^(T-1)), or null to make one for this call
    void (*divide_dev)(const u64* d_coeffs, u64 n, const u32* z, const void* d_table, u64* d_q, bool q_canon, u32* d_y, hipStream_t st);
    size_t (*table_bytes)();
    void (*table_dev)(const u32* z, void* d_table, hipStream_t st);
    // out_j = sum_i gamma^i p_i[j], j < n_max; d_polys / d_lens: k pointers and lengths in device memory
    void (*lincomb_dev)(const u64* const* d_polys, const u64* d_lens, u32 k, u64 n_max, const u32* gamma, u64* d_out, hipStream_t st);
    // m openings `stride` words apart, z at word z_off and y behind it: d_rz_j = rho_j z_j mod r, d_y_j = y_j packed (8 canonical words each),
    // d_flag_j = 1 when z_j is not below r
    void (*weights_dev)(const u32* d_open, u64 stride, u64 z_off, u64 m, const u32* d_rho, u32* d_rz, u32* d_y, u32* d_flag, hipStream_t st);
    // divide_dev's phases 1 and 2, then d_out[j] = d_acc[j] + w q_j for j < n - 1 (Montgomery words; d_out may be d_acc); w: 8 canonical words, host
    void (*divide_acc_dev)(const u64* d_coeffs, u64 n, const u32* z, const void* d_table, const u32* w, const u64* d_acc, u64* d_out, u32* d_y, hipStream_t st);
    // d_out[j k + i] = p_i[j], j < n_max, zero where p_i is shorter; d_polys / d_lens as for lincomb_dev
    void (*interleave_dev)(const u64* const* d_polys, const u64* d_lens, u32 k, u64 n_max, u64* d_out, hipStream_t st);
};
const KzgOps& kzg_ops(CurveId id);
constexpr uint64_t KZG_TILE = 2048, KZG_SPAN = 512;   // coefficients per workgroup; tile aggregates per step of the combining workgroup
// ---- groth16.hip: polynomial arithmetic over the scalar field (frpoly_impl.hip.h).  Vectors: n x 4 u64 Montgomery words on the
// device, the transforms' layout; scalars and host results: 4 canonical u64 words on the host.  What include/zkgpu.h states for
// zk_fr_<curve>_<name>_dev holds for each of these
struct FrPolyOps {
    void (*prefix_product_dev)(const u64* d_in, u64 n, bool inclusive, u64* d_out, u64* total_out, hipStream_t st);
    void (*batch_inverse_dev)(const u64* d_in, u64 n, u64* d_out, u64* n_zero, u64* first_zero, hipStream_t st);
    void (*pointwise_dev)(int op, const u64* d_a, const u64* d_b, u64* d_out, u64 n, hipStream_t st);
    void (*powers_dev)(const u64* base, const u64* scale, u64 n, u64* d_out, hipStream_t st);
    void (*terms_dev)(const u64* const* d_cols, const u64* const* d_labels, u32 k, u64 n, const u64* beta, const u64* gamma, u64* d_out, hipStream_t st);
    void (*grand_product_dev)(const u64* d_num, const u64* d_den, u64 n, u64* d_z, u64* last_out, hipStream_t st);
    void (*poly_mul_dev)(const u64* d_a, u64 na, const u64* d_b, u64 nb, u64* d_out, hipStream_t st);
    void (*divmod_zh_dev)(const u64* d_p, u64 n_p, u32 log_n, u64* d_q, u64* d_rem, u64* rem_nonzero, hipStream_t st);
    void (*divide_zh_coset_dev)(u64* d_evals, u32 log_m, u32 log_n, hipStream_t st);
    void (*prefix_sum_dev)(const u64* d_in, u64 n, bool inclusive, u64* d_out, u64* total_out, hipStream_t st);   // plonk_lookup_impl.hip.h: the same tiles under addition
};
const FrPolyOps& frpoly_ops(CurveId id);
constexpr uint64_t FRPOLY_TILE = 2048, FRPOLY_SPAN = 512;   // elements per workgroup of the running product; tile aggregates per step of the combining workgroup
// ---- groth16.hip: the device side of the PLONK prover (plonk_impl.hip.h).  Vectors and scalars as for FrPolyOps; what
// include/zkgpu.h states for zk_plonk_<curve>_quotient_dev, zk_plonk_<curve>_gate_check_dev and zk_fr_<curve>_gather_dev holds for these
struct PlonkOps {
    void (*quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, u64* d_out, hipStream_t st);
    void (*gate_check_dev)(const u64* const* d_cols, u64 n, u64* n_bad, u64* first_bad, hipStream_t st);
    void (*gather_dev)(const u64* d_src, u64 n_src, const u32* d_idx, u64 n, u64* d_out, hipStream_t st);
    // plonk_r1cs_impl.hip.h: an .r1cs compiled to a gate table on the host (no device is touched); the auxiliary variables
    // of a witness on the device
    PlonkR1cs* (*r1cs_new)(const void* r1cs, size_t len);
    void (*r1cs_extend_dev)(PlonkR1cs& h, u64* d_w, hipStream_t st);
    // plonk_next_impl.hip.h: the gate with the term q_N c(wX): one more column behind the others', and the import's chain rule
    // (a handle of next_r1cs_new is extended by next_r1cs_extend_dev: two terms a stored prefix)
    void (*next_quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, u64* d_out, hipStream_t st);
    void (*next_gate_check_dev)(const u64* const* d_cols, u64 n, u64* n_bad, u64* first_bad, hipStream_t st);
    PlonkR1cs* (*next_r1cs_new)(const void* r1cs, size_t len);
    void (*next_r1cs_extend_dev)(PlonkR1cs& h, u64* d_w, hipStream_t st);
};
const PlonkOps& plonk_ops(CurveId id);
// ---- groth16.hip: the device side of the fflonk prover (fflonk_impl.hip.h): the three numerators of the identity apart, in
// one launch.  What include/zkgpu.h states for zk_fflonk_<curve>_quotients_dev holds for it
struct FflonkOps {
    void (*quotients_dev)(const u64* const* d_cols, u32 log_n, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, u64* d_out0, u64* d_out1, u64* d_out2, hipStream_t st);
};
const FflonkOps& fflonk_ops(CurveId id);
// ---- groth16.hip: the device side of PLONK's lookup argument (plonk_lookup_impl.hip.h).  Vectors and scalars as for FrPolyOps;
// what include/zkgpu.h states for zk_plonk_<curve>_lookup_* holds for these
struct PlonkLookupOps {
    PlonkLookupTable* (*table_new)(const u64* d_t1, const u64* d_t2, const u64* d_t3, u64 T, hipStream_t st);
    void (*count_dev)(const PlonkLookupTable& h, const u64* d_a, const u64* d_b, const u64* d_c, const u64* d_qk, u64 n, u64* d_m_out, u64* n_bad, u64* first_bad, hipStream_t st);
    void (*terms_dev)(const u64* const* d_cols, u64 n, const u64* eta, const u64* delta, u64* d_out, hipStream_t st);
    void (*summands_dev)(const u64* d_inv, const u64* d_qk, const u64* d_m, u64 n, u64* d_out, hipStream_t st);
    void (*quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* eta, const u64* delta, u64* d_acc, hipStream_t st);
    // the tagged argument (plonk_lookup_tagged_impl.hip.h): several tables, a fourth column T0 / q_K; zk_plonk_<curve>_lookup_tagged_*
    PlonkLookupTable* (*tagged_table_new)(const u64* d_t0, const u64* d_t1, const u64* d_t2, const u64* d_t3, u64 T, hipStream_t st);
    void (*tagged_count_dev)(const PlonkLookupTable& h, const u64* d_a, const u64* d_b, const u64* d_c, const u64* d_qk, u64 n, u64* d_m_out, u64* n_bad, u64* first_bad, hipStream_t st);
    void (*tagged_terms_dev)(const u64* const* d_cols, u64 n, const u64* eta, const u64* delta, u64* d_out, hipStream_t st);
    void (*tagged_quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* eta, const u64* delta, u64* d_acc, hipStream_t st);
};
const PlonkLookupOps& plonk_lookup_ops(CurveId id);
// ---- groth16.hip: the device side of the fflonk prover with lookups (fflonk_lookup_impl.hip.h): the four numerators of the
// identity apart, in one launch.  What include/zkgpu.h states for zk_fflonk_<curve>_lookup_quotients_dev holds for it
struct FflonkLookupOps {
    void (*quotients_dev)(const u64* const* d_cols, u32 log_n, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, const u64* eta, const u64* delta, u64* d_out0, u64* d_out1,
                          u64* d_out2, u64* d_out3, hipStream_t st);
    // the tagged form (fflonk_lookup_tagged_impl.hip.h): one more column, Tg; zk_fflonk_<curve>_lookup_tagged_quotients_dev
    void (*tagged_quotients_dev)(const u64* const* d_cols, u32 log_n, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, const u64* eta, const u64* delta, u64* d_out0,
                                 u64* d_out1, u64* d_out2, u64* d_out3, hipStream_t st);
};
const FflonkLookupOps& fflonk_lookup_ops(CurveId id);
constexpr uint64_t PLONK_R1CS_WAVE_MIN_TERMS = 64;   // a segment of this many terms or more is walked by a whole wave (plonk_r1cs_impl.hip.h)
// ---- pairing.hip: the steps of the optimal ate pairing and of Groth16 verification (pairing_impl.hip.h)
struct PairingOps {
    const char* q_hex;                                                      // the base field's modulus
    void (*g1_check)(const void*, u64, u64, int*, u64, hipStream_t);
    void (*g16_acc)(const void*, u32, const void*, u64, void*, int*, hipStream_t);
    void (*g2_check)(const void*, u64, u64, int*, u64, hipStream_t);
    size_t (*lines_bytes)(u64);
    void (*g2_lines)(const void*, u64, u64, void*, void*, hipStream_t);
    size_t (*f12_bytes)(u64);
    size_t (*tab_bytes)(u64);
    void (*miller)(const MillerArgs&, u64, void*, hipStream_t);
    void (*final_exp)(const void*, u64, void*, void*, int, hipStream_t);
    void (*verdict)(const void*, const void*, u64, const int*, int*, hipStream_t);
    // the product of n Miller values (f12_bytes(1) each) as one: input, n, scratch of f12_prod_scratch(n) bytes, output; a fixed order
    size_t (*f12_prod_scratch)(u64);
    void (*f12_prod)(const void*, u64, void*, void*, hipStream_t);
    // by Group (key_check_impl.hip.h): points, stride in words, n, plain, canon -> 4 x (count, first index) for infinity, coordinate_range,
    // not_on_curve, not_in_subgroup
    void (*points_check[2])(const void*, u64, u64, int, int, u64*, hipStream_t);
};
// ---- ecntt.hip: transforms, column sums and scalar products whose elements are points (ecntt_impl.hip.h).  Points as for the sums; scalars and
// coefficients 8 canonical words
struct EcCsc { const u64* ptr; const u32* rows; const u32* coef; const u32* base; };   // one matrix by columns and the points its rows select
struct EcGroupOps {
    void (*ntt)(void* d_points, int logn, const u32* d_tw, const u32* d_scale, hipStream_t st);
    void (*mul_scalar)(const void* d_points, u64 n, const u32* d_k, void* d_out, hipStream_t st);          // out_i = [k] P_i, one k
    // out_i = [k_i] P_i, one k per point; the points stride_words apart (a proof's A), the results packed; a walk from each scalar's top set bit
    void (*mul_scalars)(const void* d_points, u64 stride_words, u64 n, const u32* d_k, void* d_out, hipStream_t st);
    // the same through the endomorphism split of G1 (one joint walk over two 128-bit halves; points of the subgroup of order r); null for G2
    void (*mul_scalars_glv)(const void* d_points, u64 stride_words, u64 n, const u32* d_k, void* d_out, hipStream_t st);
    void (*diff)(const void* d_a, const void* d_b, u64 n, void* d_out, hipStream_t st);                    // out_i = a_i - b_i
    // out_j = sum over the sets and the terms of column j of coef * base[row], j < n_wires; r: the scalar modulus
    void (*column_sums)(const EcCsc* sets, int n_sets, const u32* r, u32 n_wires, void* d_out, hipStream_t st);
};
struct EcOps { EcGroupOps g[2]; };
const MsmOps& msm_ops(CurveId id);
const EcOps& ec_ops(CurveId id);
const Groth16Ops& groth16_ops(CurveId id);
const PairingOps& pairing_ops(CurveId id);

struct Curve {
    CurveId id;
    const char* name;        // the reference's curve_type (groth16/src/api.rs:148-204), also what proof.json and the key's JSON carry
    const char* abi_name;    // as the symbols of include/zkgpu.h spell it
    uint32_t fq_words;       // u32 words per base-field element
    u32 r[8];                // the scalar field's modulus
    size_t point_words(Group g) const { return (g == G1 ? 2 : 4) * (size_t)fq_words; }   // affine; a sum's result is this and a flag word
    size_t point_bytes(Group g) const { return 4 * point_words(g); }
    size_t proof_words() const { return 2 * point_words(G1) + point_words(G2); }         // A || B || C
    size_t gt_bytes() const { return 48 * (size_t)fq_words; }                            // 12 canonical Fq
    int r_bits() const { return 256 - __builtin_clz(r[7]); }
    bool fr_canonical(const u32* v) const {                                              // 8 words, below r
        for (int i = 7; i >= 0; --i) { if (v[i] < r[i]) return true; if (v[i] > r[i]) return false; }
        return false;
    }
    const MsmOps& msm() const { return msm_ops(id); }
    const GroupOps& group(Group g) const { return msm_ops(id).g[g]; }
    const Groth16Ops& groth16() const { return groth16_ops(id); }
    const PairingOps& pairing() const { return pairing_ops(id); }
    const EcOps& ec() const { return ec_ops(id); }
    const KzgOps& kzg() const { return kzg_ops(id); }
    const FrPolyOps& frpoly() const { return frpoly_ops(id); }
    const PlonkOps& plonk() const { return plonk_ops(id); }
    const FflonkOps& fflonk() const { return fflonk_ops(id); }
    const PlonkLookupOps& plonk_lookup() const { return plonk_lookup_ops(id); }
    const FflonkLookupOps& fflonk_lookup() const { return fflonk_lookup_ops(id); }
};
inline const Curve CURVES[2] = {
    {CURVE_BN254, "BN128", "bn254", 8, {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
    {CURVE_BLS12_381, "BLS12381", "bls12_381", 12, {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}},
};
inline const Curve& curve(CurveId id) { return CURVES[id]; }
// Which names an entry point takes, and how it words its refusal: the Groth16 prover and key generation know the reference's names only,
// the pairing side also the ABI's and refuses a null name apart
enum CurveNames { GROTH16_NAMES, PAIRING_NAMES };
inline const Curve& curve_of(const char* name, CurveNames rule) {
    ZK_REQUIRE(name || rule == GROTH16_NAMES, "pairing: null curve");
    const std::string c = name ? name : "";
    for (const Curve& cv : CURVES)
        if (c == cv.name || (rule == PAIRING_NAMES && c == cv.abi_name)) return cv;
    throw Error(rule == GROTH16_NAMES ? "groth16: unknown curve \"" + c + "\" (BN128 | BLS12381)" : "pairing: unknown curve '" + c + "' (BN128 | BLS12381)");
}

// ---- Groth16 around the multi-scalar sums (groth16.hip) ----
void groth16_wtns_payload(const void* wtns, size_t len, const char* curve, uint64_t* offset, uint64_t* n);
// Key generation (groth16_keygen_impl.hip.h; `zkit groth16_setup`, groth16/src/api.rs:42-66): the finished key as bellman's
// Parameters::write lays it out.  trapdoor: 5 x 4 u64 (tau, alpha, beta, gamma, delta), or null to draw them from the OS.
Groth16Setup* groth16_setup_new(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len);
Groth16Key* groth16_keygen_new(const char* curve, const void* r1cs, size_t r1cs_len, const uint64_t* trapdoor);
std::string groth16_keygen_vk_json(const Groth16Key& k, bool to_hex);   // json_utils.rs:285-303 serialize_vk
// A key from a powers-of-tau file instead of a trapdoor (groth16.hip; the group work is ecntt.hip's).  srs_open is host only.
void group_ntt_dev(const Curve& cv, Group g, void* d_points, int logn, bool inverse, hipStream_t st);
Srs* srs_open(const char* curve, const char* path);
std::string srs_check(const Srs& srs, const uint8_t* seed, uint32_t max_findings);
Groth16Key* groth16_keygen_from_srs(const char* curve, const void* r1cs, size_t r1cs_len, const Srs* srs);
// A powers-of-tau ceremony (groth16_ceremony.hip.h).  srs_new and srs_transcript_count are host only.
void srs_new(const char* curve, uint32_t power, const char* path);
// secrets: 3 x 4 canonical words (tau, alpha, beta factors), or null to draw them; beacon_seed: 32 bytes for a beacon (then no secrets), or null
void srs_contribute(const Srs& srs, const char* out_path, const uint64_t* secrets, const uint8_t* beacon_seed, uint32_t beacon_iter_log);
std::string srs_verify(const Srs& srs, const uint8_t* seed, uint32_t max_findings);
int64_t srs_transcript_count(const Srs& srs);                              // records of the file's transcript, -1 without one
// delta: 4 canonical words, non-zero and below r, or null to draw it from the OS; out: len bytes
void groth16_params_contribute(const char* curve, const void* params, size_t len, const uint64_t* delta, void* out);
std::string groth16_contribution_check(const char* curve, const void* old_params, size_t old_len, const void* new_params, size_t new_len,
                                       const uint8_t* seed, uint32_t max_findings);
// contributions with proofs of knowledge and their transcript (groth16_ceremony.hip.h): groth16_params_contribute plus one
// record appended to the transcript (t_len = 0 starts one at this key); out_transcript: groth16_key_transcript_size(count + 1) bytes
size_t groth16_key_transcript_size(const char* curve, uint32_t count);
void groth16_params_contribute_pok(const char* curve, const void* params, size_t len, const uint64_t* delta, const void* transcript, size_t t_len,
                                   void* out_params, void* out_transcript);
std::string groth16_key_transcript_check(const char* curve, const void* initial, size_t initial_len, const void* final_key, size_t final_len,
                                         const void* transcript, size_t t_len, const uint8_t* seed, uint32_t max_findings);
// groth16_key_check_srs (key_check_srs.hip.h): every query of the key and alpha, beta against the circuit's polynomials at the tau
// of a powers-of-tau file -> the report as JSON text.  seed as for groth16_key_check.
std::string groth16_key_check_srs(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const Srs* srs,
                                  const uint8_t* seed, uint32_t max_findings);
// groth16_key_check (groth16.hip): the report as JSON text.  seed: 32 bytes for the random linear combination, for tests only -- null (the operating
// system's randomness) anywhere else.
std::string groth16_key_check(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const char* vk_json,
                              const uint8_t* seed, uint32_t max_findings);

// n weights of 128 bits as 32 B canonical scalars: ChaCha20 of the seed on the device (kc_rho_kernel).  seed: 32 bytes, tests only; null = the
// operating system's randomness.  Synchronises the stream.
void groth16_rho_dev(const uint8_t* seed, uint64_t n, DevBuf& d_rho, hipStream_t st, const char* who);

// ---- pairing.hip: the optimal ate pairing and Groth16 verification ----
// one point of a verification_key.json or a proof ({"x", "y"}; G2: [c0, c1] pairs) -> 2 or 4 x fq_words canonical 32-bit words; pairing_ce's
// zero (0, 1) becomes the all-zero encoding; negate: y -> q - y.  Throws on what is no number or does not fit the field's width.
struct JVal;
void groth16_json_g1(const Curve& cv, const JVal& v, uint32_t* w);
void groth16_json_g2(const Curve& cv, const JVal& v, uint32_t* w, bool negate);
void pairing_dev(const Curve& cv, const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, hipStream_t st);
Groth16Vk* groth16_vk_new(const char* curve, const char* vk_json);
void groth16_vk_info(const Groth16Vk* vk, uint32_t* n_public, uint32_t* proof_bytes, uint32_t* gt_bytes);
void groth16_verify_batch_dev(const Groth16Vk* vk, const void* d_proofs, const void* d_publics, uint64_t n, int* d_verdicts, hipStream_t st);
void groth16_verify_batch(const Groth16Vk* vk, const void* proofs, const void* publics, uint64_t n, int* verdicts);
int groth16_verify_json(const Groth16Vk* vk, const char* proof_json, const char* public_json);
// prod_i e(g1_i, g2_i) as ONE value of GT (the layout of pairing_dev): line tables, single-pair Miller loops, the product reduction, one final
// exponentiation; n = 0 gives one.  In chunks, so that the tables of a large n are never allocated at once.
void pairing_product_dev(const Curve& cv, const void* d_g1, const void* d_g2, uint64_t n, void* d_gt, int with_final_exp, hipStream_t st);
// n proofs in one randomised check: accepted exactly when every proof is, except with probability about 2^-128 over the
// weights.  seed: 32 bytes for the weights, for tests only -- null (the operating system's randomness) anywhere else.  locate: on refusal run
// the per-proof path and report the first proof it does not accept (*first_bad, *verdict = its code); without it *verdict is REJECTED and
// *first_bad is left at n.  Synchronises the stream.
void groth16_verify_aggregate_dev(const Groth16Vk* vk, const void* d_proofs, const void* d_publics, uint64_t n, const uint8_t* seed, bool locate,
                                  int* verdict, uint64_t* first_bad, hipStream_t st);
void groth16_verify_aggregate(const Groth16Vk* vk, const void* proofs, const void* publics, uint64_t n, const uint8_t* seed, bool locate,
                              int* verdict, uint64_t* first_bad);
// proof.json and public_input.json -> the words groth16_verify_batch takes: proof_out A || B || C (Montgomery), public_out n_public x 8
// canonical words.  -> 1, or the verdict the file-level form gives without looking at a point (INPUT_COUNT, INPUT_NOT_CANONICAL)
int groth16_proof_words(const Groth16Vk* vk, const char* proof_json, const char* public_json, void* proof_out, void* public_out);
// phases of the last aggregate call on this thread, host milliseconds around stream synchronisations, when ZK_VERIFY_AGG_TIMING is set:
// checks, scalar products, lines and Miller loops, product, sums, tail
void groth16_verify_aggregate_timing(double ms[6]);

// ---- kzg.hip: KZG commitments over a powers-of-tau file.  Polynomials: coefficients in the transforms' layout; z, gamma: 8
// canonical words on the host; results as include/zkgpu.h states them
Kzg* kzg_new(const Srs* srs, uint64_t max_coeffs);
void kzg_divide_dev(const Curve& cv, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_q, uint64_t* d_y, hipStream_t st);
void kzg_lincomb_dev(const Curve& cv, const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, const uint64_t* gamma, uint64_t* d_out, hipStream_t st);
void kzg_commit_dev(Kzg& k, const uint64_t* d_coeffs, uint64_t n, void* d_out, hipStream_t st);
void kzg_commit_evals_dev(Kzg& k, const uint64_t* d_evals, uint32_t log_n, void* d_out, hipStream_t st);
void kzg_open_dev(Kzg& k, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, uint64_t* d_y_out, void* d_w_out, hipStream_t st);
void kzg_open_many_dev(Kzg& k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* z, const uint64_t* gamma, uint64_t* d_ys_out, void* d_w_out,
                       hipStream_t st);
void kzg_fold_commitments(Kzg& k, const void* commitments, uint32_t n, const uint64_t* gamma, void* out);
void kzg_verify_dev(Kzg& k, const void* d_openings, uint64_t m, const uint8_t* seed, bool locate, int* verdict, uint64_t* first_bad, hipStream_t st);
void kzg_verify(Kzg& k, const void* openings, uint64_t m, const uint8_t* seed, bool locate, int* verdict, uint64_t* first_bad);
// several polynomials at several points in one two-point proof; w as z
void kzg_divide_acc_dev(const Curve& cv, const uint64_t* d_coeffs, uint64_t n, const uint64_t* z, const uint64_t* w, uint64_t* d_acc, uint64_t* d_y, hipStream_t st);
void kzg_interleave_dev(const Curve& cv, const uint64_t* const* d_polys, const uint64_t* n, uint32_t k, uint64_t* d_out, hipStream_t st);
KzgMulti* kzg_multi_begin(Kzg& k, const uint64_t* const* d_polys, const uint64_t* n, uint32_t n_polys, const uint64_t* points, const uint32_t* set_sizes,
                          uint64_t* d_values_out, hipStream_t st);
void kzg_multi_quotient(KzgMulti& m, const uint64_t* gamma, void* d_w1_out, hipStream_t st);
void kzg_multi_finish(KzgMulti& m, const uint64_t* z, void* d_w2_out, hipStream_t st);
void kzg_multi_verify(Kzg& k, const void* proofs, uint64_t bytes, uint64_t m, const uint8_t* seed, bool locate, int* verdict, uint64_t* first_bad, hipStream_t st);

}  // namespace zk

// the opaque handles of include/zkgpu.h
struct zk_groth16_setup {    // a proving key and its circuit, resident on the device (groth16_impl.hip.h implements it per scalar field)
    const zk::Curve* curve = nullptr;
    virtual ~zk_groth16_setup() {}
    // witness: n_wires x 32 B canonical (host or device); proof_out: A || B || C affine Montgomery words; d_h_out:
    // optional device buffer for the quotient's (2^domain_log - 1) x 32 B canonical coefficients
    virtual void prove(const void* witness, bool on_device, const u64 r[4], const u64 s[4], u32* proof_out, std::string* json, u64* d_h_out) = 0;
    virtual uint32_t num_wires() const = 0;
    virtual uint32_t num_inputs() const = 0;
    virtual uint32_t domain_log() const = 0;
};
struct zk_groth16_keygen {   // a finished key
    const zk::Curve* curve = nullptr;
    std::vector<uint8_t> params;
    double ms[5] = {};       // transform, column sums, G1 points, G2 points, serialisation
};
struct zk_srs {              // a powers-of-tau file, read and measured; the sections stay in the file's bytes
    const zk::Curve* curve = nullptr;
    uint32_t power = 0, ceremony_power = 0;
    std::vector<uint8_t> file;
    size_t off[7] = {};      // by section id (2 tauG1, 3 tauG2, 4 alphaTauG1, 5 betaTauG1, 6 betaG2): where the payload starts
};
struct zk_kzg {              // the G1 powers of a file on the device, and what verification pairs against (kzg.hip)
    const zk::Curve* curve = nullptr;
    uint32_t power = 0;
    uint64_t max_coeffs = 0;
    void *d_tau = nullptr, *d_table = nullptr;       // tauG1[0, max_coeffs) as the sums take it; its window tables, when built
    void *d_gen1 = nullptr, *d_g2 = nullptr;         // G1; G2 || -tauG2[1]
    void* d_lagrange[32] = {};                       // by log_n: iNTT(tauG1[0, 2^log_n)), made and waited for on first use; like every handle, one call at a time
    zk_kzg() = default; zk_kzg(const zk_kzg&) = delete; zk_kzg& operator=(const zk_kzg&) = delete;
    ~zk_kzg() { for (void* p : {d_tau, d_table, d_gen1, d_g2}) if (p) zk::pool_free(p); for (void* p : d_lagrange) if (p) zk::pool_free(p); }
};
struct zk_kzg_multi {        // an opening at several points between its stages (kzg.hip)
    zk_kzg* k = nullptr;
    std::vector<const uint64_t*> polys;              // the caller's, on the device, until finish
    std::vector<uint64_t> n;
    std::vector<uint32_t> sizes;                     // |S_i|
    std::vector<uint64_t> points, values, gamma;     // 4 canonical words each: the sets one after another, f_i(s) in the same order
    std::vector<uint32_t> table_of;                  // per point: its block of d_tables (one per distinct point, table_bytes() each)
    void *d_tables = nullptr, *d_q = nullptr;        // q: nq coefficients, Montgomery words
    uint64_t nq = 0;
    int stage = 0;                                   // 1 after begin, 2 after quotient, 3 after finish
    zk_kzg_multi() = default; zk_kzg_multi(const zk_kzg_multi&) = delete; zk_kzg_multi& operator=(const zk_kzg_multi&) = delete;
    ~zk_kzg_multi() { for (void* p : {d_tables, d_q}) if (p) zk::pool_free(p); }
};
struct zk_plonk_r1cs {       // an .r1cs as the PLONK prover takes it (plonk_r1cs_impl.hip.h): host tables, the segments on the device from the first extension on
    const zk::Curve* curve = nullptr;
    uint32_t n_wires = 0, n_public = 0;
    uint64_t n_constraints = 0, n_vars = 0, max_terms = 0;
    std::vector<uint64_t> sel[5];                    // qL, qR, qO, qM, qC: 4 canonical words per gate
    std::vector<uint32_t> wire[3], origin;           // a, b, c: variable ids; the constraint of every gate
    std::vector<uint64_t> sel_n;                     // the chain rule (plonk_next_impl.hip.h): q_N, 4 canonical words per gate; empty otherwise
    uint32_t store_step = 1;                         // 1: every term after the first defines an auxiliary; 2 (the chain rule): every second one and the last
    std::vector<uint32_t> seg_first;                 // per segment: its first auxiliary
    std::vector<uint64_t> seg_ptr;                   // n_segments + 1 offsets into the terms
    std::vector<uint32_t> seg_wire;                  // per term: the original wire
    std::vector<uint64_t> seg_coef;                  // per term: 4 canonical words
    // the device's copy: offsets, first auxiliaries, wires, the coefficients in internal form (9 words a term), and the segments by kernel
    zk::DevBuf d_ptr, d_first, d_wire, d_coef, d_short, d_long;
    uint64_t n_short = 0, n_long = 0;
    bool on_device = false;
    zk_plonk_r1cs() = default; zk_plonk_r1cs(const zk_plonk_r1cs&) = delete; zk_plonk_r1cs& operator=(const zk_plonk_r1cs&) = delete;
};
struct zk_plonk_lookup_table {   // the rows of a lookup table as a hash table on the device (plonk_lookup_impl.hip.h); read-only once built
    const zk::Curve* curve = nullptr;
    uint64_t n_rows = 0, n_slots = 0;                // n_slots: the smallest power of two >= 2 n_rows
    zk::DevBuf d_keys, d_slots;                      // per row: the 24 canonical Montgomery words of its key; per slot: a row or 0xffffffff
    bool tagged = false;                             // a tagged table (plonk_lookup_tagged_impl.hip.h): keys of 32 words, the tag first
    zk::DevBuf d_tags;                               // tagged: per row, its tag 1 .. 65535 as a u32
    zk_plonk_lookup_table() = default; zk_plonk_lookup_table(const zk_plonk_lookup_table&) = delete; zk_plonk_lookup_table& operator=(const zk_plonk_lookup_table&) = delete;
};
struct zk_groth16_vk {       // a verification key, checked and prepared
    const zk::Curve* curve = nullptr;
    uint32_t n_ic = 0;
    void *d_ic = nullptr, *d_lines = nullptr, *d_inf = nullptr, *d_ab = nullptr;   // IC (Montgomery), the lines of -gamma, -delta and -beta, e(alpha, beta)
    void* d_alpha = nullptr;                                                       // alpha (Montgomery), for the aggregate check
    bool ic_has_infinity = false;                                                  // an IC point at infinity: the sums cannot take it
    zk_groth16_vk() = default; zk_groth16_vk(const zk_groth16_vk&) = delete; zk_groth16_vk& operator=(const zk_groth16_vk&) = delete;
    ~zk_groth16_vk() { for (void* p : {d_ic, d_lines, d_inf, d_ab, d_alpha}) if (p) zk::pool_free(p); }
};
