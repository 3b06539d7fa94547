// The device side of the fflonk prover with TAGGED lookups over the scalar field on gfx950, generic over the field: the four
// numerators of fflonk_lookup_impl.hip.h with the tag column of plonk_lookup_tagged_impl.hip.h in the lookup
// argument's L, as one kernel.  The protocol itself (rounds, transcript, files) is eigen_zkvm_amd/fflonk_lookup_tagged.py.  Included by
// groth16.hip after fflonk_lookup_impl.hip.h and plonk_lookup_tagged_impl.hip.h, in the same namespace: it uses plonk_impl.hip.h's constants
// and loads (PkConsts, pk_setup_kernel with alpha = 0, pk_plain, pk_internal, pk_times_k, pk_gate_macs), plonk_lookup_tagged_impl.hip.h's
// plt_term over PltConsts (plt_setup_kernel with alpha = 0: E1, E2, E3, DP), and the host checks pk_scalar / pk_apart.  flt_quotients_kernel
// is a sibling of fl_quotients_kernel, not a template of it: no existing kernel is touched, so no existing register count can move.  No
// include guard on purpose.
//
// Vectors and forms (plain P(v) = v R < 6r, internal I(v) = v R', fe_mul(I(u), P(v)) = P(u v), fe_mul(I(u), I(v)) = I(u v)) are
// plonk_impl.hip.h's.  d_cols: fflonk_lookup_impl.hip.h's twenty-one columns in their order, then Tg, the tag column of the table (the T0 of
// DESIGN.md 3.26; fflonk's T0 is a quotient, so here the column is Tg).
//
// zk_fflonk_<curve>_lookup_tagged_quotients_dev, per lane (flt_quotients_kernel); "=" is the value, "<" the bound against fe29_impl.hip.h's
// A B <= 68.  A, B, C, W0, out0, zm1, out1, Bx .. D and out2 are fl_quotients_kernel's rows, the same lines of code.  The lookup part:
//   E1, E2, E3 = I(eta), I(eta^2), I(eta^3); DP = P(delta) canonical  (plt_setup_kernel, alpha = 0)                           < 2r each, < r
//   DI         = I(delta) = fe_canon(fe_mul(P'(delta), RR2)): 1 x 1 (flt_setup_kernel)                                        < r
//   E3Q        = fe_mul(E3, CIN) = eta^3 R'^2 / R, so that fe_mul(P(v), E3Q) = I(eta^3 v): 2 x 1 (flt_setup_kernel)            < 2r
//   QK         = P(q_K), loaded ONCE                                                                                          < 6r
//   Tp         = P(delta + t) = P(t1) + fe_mul(P(t2), E1) + fe_mul(P(t3), E2) + fe_mul(P(Tg), E3) + DP (plt_term):
//                products 6 x 2 = 12 each; the sum 6r + 2r + 2r + 2r + r                                                       < 13r
//   TI         = fe_mul(Tp, CIN) = I(delta + t): 13 x 1                                                                       < 2r
//   V          = A I(1) + B E1 + C E2 + QK E3Q with ONE reduction = I(a + eta b + eta^2 c + eta^3 q_K), I(1) = R' mod r < r:
//                2 x 1 + 2 x 2 + 2 x 2 + 6 x 2 = 22 (4 pairs <= FE_WIDE_MAX).  q_K reaches internal form through the CONSTANT E3Q:
//                no product of its own per lane, only one more multiply-accumulate under the reduction V had already                < 2r
//   X1         = V + DI = I(delta + f)                                                                                         < 3r
//   X2         = fe_mul(X1, TI) = I((delta + f)(delta + t)): 3 x 2 = 6                                                         < 2r
//   D3         = P(Phi(wX)) - P(Phi) + 8r  (fe_sub<8>, P(Phi) < 6r <= 8r)                                                      < 14r
//   NQ         = 8r - QK  (fe_sub<8> of zero)                                                                                  <= 8r
//   W3         = X2 D3 + TI NQ + X1 P(M) with ONE reduction (3 pairs <= FE_WIDE_MAX): 2 x 14 + 2 x 8 + 3 x 6 = 62              < 2r, plain
//   out3       = W3, reduced once in fp_put_plain: 2                                                                          canonical
// Against fl_quotients_kernel a lane loads one more column (Tg) and makes one more product (P(Tg) E3) and one more multiply-accumulate
// (QK E3Q).  Each output is stored as soon as it is made, and the lookup part runs between out0 and out1, while only A, B, C live: Z, G and
// BI are loaded after it.  No LDS, no atomics: with every output a lane reads 24 elements (Z and Phi twice) and writes 4.
//
// An output may be NULL: that part is then not computed and its own columns are not read (the same for every lane, so no divergence).

constexpr int FLT_NCOL = FL_NCOL + 1;
enum { FLT_TG = FL_NCOL };                                      // the order of d_cols after fflonk_lookup_impl.hip.h's
static_assert(FLT_NCOL == ZK_FFLONK_LOOKUP_TAGGED_QUOTIENT_COLS, "include/zkgpu.h states the number of columns");

struct FltCols { const u32* c[FLT_NCOL]; };
struct FltConsts { PkConsts pk; PltConsts pl; fe DI, E3Q; };

// delta: 8 canonical words -> I(delta), canonical; E3Q from pl.E3, which plt_setup_kernel wrote before this launch on the same stream; pk and
// pl are pk_setup_kernel's and plt_setup_kernel's
__global__ void flt_setup_kernel(const FpWords delta, FltConsts* __restrict__ fc) {
    if (threadIdx.x || blockIdx.x) return;
    fc->DI = fe_canon(fe_mul(fp_split(delta.w), fp_const_rr2()));
    fc->E3Q = fe_mul(fc->pl.E3, fp_const_cin());
}

// out0_i .. out2_i as fl_quotients_kernel; out3_i = the numerator L of the tagged lookup argument at point i of the coset 7 H_m, m = 4n; Z(wX)
// and Phi(wX) are element (i + 4) mod m.  One lane per element.  A null output is skipped: without out0 the selectors, q_C and PI are not read;
// without out3 q_K, t1, t2, t3, Tg, M and Phi are not; without out1 L_1 is not; without out2 X and the S_sigma_j are not, and without both Z
// is not.
__global__ __launch_bounds__(FP_BLOCK) void flt_quotients_kernel(const FltCols cs, const FltConsts* __restrict__ fc, const FlOuts out, u64 m) {
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
    if (out.o[3]) {
        const PltConsts* lc = &fc->pl;
        const fe QK = pk_plain(cs.c[FL_QK], i);
        fe_wide acc;
        fe_wide_zero(acc);
        fe_wide_mac(acc, A, fe_one());
        fe_wide_mac(acc, B, lc->E1);
        fe_wide_mac(acc, C, lc->E2);
        fe_wide_mac(acc, QK, fc->E3Q);
        const fe X1 = fe_add(fe_wide_reduce(acc), fc->DI);
        const fe TI = fe_mul(plt_term(cs.c[FL_T1], cs.c[FL_T2], cs.c[FL_T3], cs.c[FLT_TG], i, lc), fp_const_cin());
        fe_wide_zero(acc);
        fe_wide_mac(acc, fe_mul(X1, TI), fe_sub<8>(pk_plain(cs.c[FL_PHI], iw), pk_plain(cs.c[FL_PHI], i)));
        fe_wide_mac(acc, TI, fe_sub<8>(fe_zero(), QK));
        fe_wide_mac(acc, X1, pk_plain(cs.c[FL_M], i));
        fp_put_plain(out.o[3], i, fe_wide_reduce(acc));
    }
    if (!out.o[1] && !out.o[2]) return;
    const PkConsts* pc = &fc->pk;
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
void FRN_FN(flt_quotients_dev)(const u64* const* d_cols, u32 log_n, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, const u64* eta, const u64* delta, u64* d_out0,
                               u64* d_out1, u64* d_out2, u64* d_out3, hipStream_t st) {
    const std::string who = "fflonk lookup tagged";
    const FpWords b = pk_scalar(who, beta, "beta"), g = pk_scalar(who, gamma, "gamma"), w1 = pk_scalar(who, k1, "k1"), w2 = pk_scalar(who, k2, "k2");
    const FpWords e = pk_scalar(who, eta, "eta"), d = pk_scalar(who, delta, "delta");
    if (log_n + 2 > (u32)FRN_S) throw std::runtime_error(who + ": the coset of 2^" + std::to_string(log_n + 2) + " points for n = 2^" + std::to_string(log_n) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(d_cols, who + ": null argument");
    ZK_REQUIRE(d_out0 || d_out1 || d_out2 || d_out3, who + ": quotients: every output is null");
    const u64 m = 4ull << log_n;
    u64* const outs[4] = {d_out0, d_out1, d_out2, d_out3};
    FltCols cs{};
    for (int c = 0; c < FLT_NCOL; ++c) {
        cs.c[c] = (const u32*)d_cols[c];
        ZK_REQUIRE(cs.c[c], who + ": quotients: column " + std::to_string(c) + " is null");
        fp_aligned({cs.c[c]});
    }
    FlOuts os{};
    for (int j = 0; j < 4; ++j) {
        os.o[j] = (u32*)outs[j];
        if (!outs[j]) continue;
        fp_aligned({outs[j]});
        for (int c = 0; c < FLT_NCOL; ++c) ZK_REQUIRE(pk_apart(outs[j], cs.c[c], m), who + ": quotients: output " + std::to_string(j) + " overlaps column " + std::to_string(c));
        for (int j2 = 0; j2 < j; ++j2)
            ZK_REQUIRE(!outs[j2] || pk_apart(outs[j], outs[j2], m), who + ": quotients: output " + std::to_string(j) + " overlaps output " + std::to_string(j2));
    }
    FpWords zero{};
    DevBuf fc;
    fc.reserve(sizeof(FltConsts));
    FltConsts* k = (FltConsts*)fc.p;
    hipLaunchKernelGGL(pk_setup_kernel, dim3(1), dim3(64), 0, st, zero, b, g, w1, w2, &k->pk);
    hipLaunchKernelGGL(plt_setup_kernel, dim3(1), dim3(64), 0, st, e, d, zero, &k->pl);
    hipLaunchKernelGGL(flt_setup_kernel, dim3(1), dim3(64), 0, st, d, k);
    hipLaunchKernelGGL(flt_quotients_kernel, dim3(fp_blocks(m)), dim3(FP_BLOCK), 0, st, cs, (const FltConsts*)k, os, m);
    ZK_HIP(hipGetLastError());
}
