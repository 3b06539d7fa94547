// The device side of the fflonk prover over the scalar field on gfx950, generic over the field: the THREE numerators of the
// identity on the coset as one kernel.  PLONK's pk_quotient_kernel folds them together with alpha; fflonk commits to the three quotients
// separately (T0 inside C1, T1 and T2 inside C2), so they leave the kernel apart.  The protocol itself (rounds, transcript, files) is
// eigen_zkvm_amd/fflonk.py.  Included by groth16.hip after plonk_impl.hip.h, in the same namespace: it uses that file's columns and constants
// (PkCols, PkConsts, pk_setup_kernel with alpha = 0), its loads (pk_plain, pk_internal), pk_times_k and pk_gate_macs, and its host checks
// (pk_scalar, pk_columns, pk_apart).  No include guard on purpose.
//
// Vectors, forms (plain P(v) = v R < 6r, internal I(v) = v R', fe_mul(I(u), P(v)) = P(u v)) and the order of d_cols are plonk_impl.hip.h's.
//
// zk_fflonk_<curve>_quotients_dev, per lane (ff_quotients_kernel); "=" is the value, "<" the bound against fe29_impl.hip.h's A B <= 68:
// Only the rows that differ from plonk_impl.hip.h's table stand here; A, B, C, AB, zm1 and the rows Bx .. D of the permutation difference are
// that table's (the same twelve lines of code in both kernels: shared through one inlined function they compile to other code, and
// pk_quotient_kernel came out 4 % slower, profiles/r26/plonk_arith.md), with A, B, C made ONCE for all three outputs.
//   W0         = A P(q_L) + B P(q_R) + C P(q_O) + AB P(q_M) with ONE reduction (fe_wide_mac, 4 pairs <= FE_WIDE_MAX)
//                4 x (2 x 6) = 48                                                                                             < 2r, plain
//   out0       = W0 + P(q_C) + P(PI): < 14r, reduced once in fp_put_plain                                                     canonical
//   L          = I(L_1) by fe_from_std: 6                                                                                     < 2r
//   out1       = fe_mul(L, zm1) = P(L_1 (Z - 1)): 2 x 8 = 16; reduced once in fp_put_plain                                    < 2r -> canonical
//   out2       = D = P1 - P2 + 2r: < 4r, reduced once in fp_put_plain                                                         canonical
// (6r is 2^256 against BN254's r; the true factor is 5.3 there and 2.3 for BLS12-381, so the 48 of W0 is 43 and 19 in fact.)
// Products: 3 + 1 + 2 + 1 + 3 + 3 + 3 = 16, four multiply-accumulates with one reduction, three reductions on the way out; 2 more when a
// k_j is large.  Each output is stored as soon as it is made, so that only A, B, C, G and P(Z) live across the three parts.
// No LDS, no atomics: a lane reads 16 elements (Z twice) and writes 3.
//
// An output may be NULL: that part is then not computed and its own columns are not read (the same for every lane, so no divergence).  The
// prover needs it: T0 is committed inside C1 BEFORE beta and gamma exist, so round 1 asks for out0 alone and round 2 for out1 and out2; a
// caller that has every column at once takes all three from one launch.

struct FfOuts { u32* o[3]; };

// out0_i, out1_i, out2_i = the gate numerator with PI, L_1 (Z - 1) and the permutation difference at point i of the coset 7 H_m, m = 4n;
// Z(wX) is element (i + 4) mod m.  One lane per element.  A null output is skipped: without out0 the selectors, q_C and PI are not read;
// without out1 L_1 is not; without out2 X and the S_sigma_j are not, and without both Z is not.
__global__ __launch_bounds__(FP_BLOCK) void ff_quotients_kernel(const PkCols cs, const PkConsts* __restrict__ pc, const FfOuts out, u64 m) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u64 iw = (i + 4) & (m - 1);
    const fe A = pk_internal(cs.c[PK_A], i), B = pk_internal(cs.c[PK_B], i), C = pk_internal(cs.c[PK_C], i);
    if (out.o[0]) {
        fe_wide acc;
        fe_wide_zero(acc);
        pk_gate_macs<PK_QL, PK_QR, PK_QO, PK_QM>(acc, cs, i, A, B, C);
        const fe W0 = fe_wide_reduce(acc);
        fp_put_plain(out.o[0], i, fe_add(fe_add(W0, pk_plain(cs.c[PK_QC], i)), pk_plain(cs.c[PK_PI], i)));
    }
    if (!out.o[1] && !out.o[2]) return;
    const fe Zp = pk_plain(cs.c[PK_Z], i);
    if (out.o[1]) fp_put_plain(out.o[1], i, fe_mul(pk_internal(cs.c[PK_L1], i), fe_sub<2>(Zp, fp_const_cout())));
    if (!out.o[2]) return;
    const fe G = pc->G, BI = pc->BI;
    const fe Bx = fe_mul(pk_plain(cs.c[PK_X], i), BI);
    const fe f1 = fe_add(fe_add(A, Bx), G);
    const fe f2 = fe_add(fe_add(B, pk_times_k(Bx, pc->k1_small, pc->K1)), G);
    const fe f3 = fe_add(fe_add(C, pk_times_k(Bx, pc->k2_small, pc->K2)), G);
    const fe P1 = fe_mul(fe_mul(fe_mul(f1, f2), f3), Zp);
    const fe g1 = fe_add(fe_add(A, fe_mul(pk_plain(cs.c[PK_S1], i), BI)), G);
    const fe g2 = fe_add(fe_add(B, fe_mul(pk_plain(cs.c[PK_S2], i), BI)), G);
    const fe g3 = fe_add(fe_add(C, fe_mul(pk_plain(cs.c[PK_S3], i), BI)), G);
    const fe P2 = fe_mul(fe_mul(fe_mul(g1, g2), g3), pk_plain(cs.c[PK_Z], iw));
    fp_put_plain(out.o[2], i, fe_sub<2>(P1, P2));
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
void FRN_FN(ff_quotients_dev)(const u64* const* d_cols, u32 log_n, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, u64* d_out0, u64* d_out1, u64* d_out2, hipStream_t st) {
    const FpWords b = pk_scalar("fflonk", beta, "beta"), g = pk_scalar("fflonk", gamma, "gamma"), w1 = pk_scalar("fflonk", k1, "k1"), w2 = pk_scalar("fflonk", k2, "k2");
    if (log_n + 2 > (u32)FRN_S) throw std::runtime_error("fflonk: the coset of 2^" + std::to_string(log_n + 2) + " points for n = 2^" + std::to_string(log_n) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(d_cols, "fflonk: null argument");
    ZK_REQUIRE(d_out0 || d_out1 || d_out2, "fflonk: quotients: every output is null");
    const u64 m = 4ull << log_n;
    u64* const outs[3] = {d_out0, d_out1, d_out2};
    const PkCols cs = pk_columns("fflonk: quotients", d_cols);
    FfOuts os{};
    for (int j = 0; j < 3; ++j) {
        os.o[j] = (u32*)outs[j];
        if (!outs[j]) continue;
        fp_aligned({outs[j]});
        for (int c = 0; c < PK_NCOL; ++c) ZK_REQUIRE(pk_apart(outs[j], cs.c[c], m), "fflonk: quotients: output " + std::to_string(j) + " overlaps column " + std::to_string(c));
        for (int j2 = 0; j2 < j; ++j2)
            ZK_REQUIRE(!outs[j2] || pk_apart(outs[j], outs[j2], m), "fflonk: quotients: output " + std::to_string(j) + " overlaps output " + std::to_string(j2));
    }
    FpWords zero{};
    DevBuf pc;
    pc.reserve(sizeof(PkConsts));
    hipLaunchKernelGGL(pk_setup_kernel, dim3(1), dim3(64), 0, st, zero, b, g, w1, w2, (PkConsts*)pc.p);
    hipLaunchKernelGGL(ff_quotients_kernel, dim3(fp_blocks(m)), dim3(FP_BLOCK), 0, st, cs, (const PkConsts*)pc.p, os, m);
    ZK_HIP(hipGetLastError());
}
