// The device side of the PLONK prover with a next-row term, generic over the scalar field: the gate of row i reads the
// c-wire of row i + 1 through a sixth selector, q_L a + q_R b + q_O c + q_M a b + q_C + q_N c' + PI = 0 with c' = c_(i + 1 mod n).  Three
// things: the numerator of the quotient on the coset, the row-by-row check of that gate, and the R1CS import's CHAIN rule with the extension
// of a witness by it.  The protocol is eigen_zkvm_amd/plonk_next.py.  Included by groth16.hip after plonk_r1cs_impl.hip.h, in the same
// namespace: it uses plonk_impl.hip.h's forms and loads (pk_plain, pk_internal, pk_times_k, pk_gate_macs: all inlined, so the kernels of that
// file are compiled as before), its constants (PkConsts, pk_setup_kernel) and host checks, and plonk_r1cs_impl.hip.h's compiler (PrCompiler)
// and term product (pr_term, pr_store).  The kernels here are copies that stand apart: pk_quotient_kernel, pk_gate_kernel and the two
// extension kernels are not templates of these and their code does not change.  No include guard on purpose.
//
// Vectors and forms are plonk_impl.hip.h's: plain P(v) = v R mod r as the integer the words are (< 2^256 <= 6r), internal I(v) = v R'
// (< 2r), fe_mul(I(u), P(v)) = P(u v) < 2r.
//
// pn_quotient_kernel.  Rows A .. W of plonk_impl.hip.h's table hold as they stand, the same lines of code: W, the sum of six pairs under ONE
// reduction, is at exactly 68 = 4 x (2 x 6) + 4 x 1 + 2 x 8 against fe29_impl.hip.h's A B <= 68, and fe_wide_mac takes FE_WIDE_MAX = 6 pairs:
// the 64-bit columns hold (6 + 1) x 9 products of 2^58.  A seventh pair fits neither bound, so the new product has a reduction of its own:
//   Cn         = I(c[(i + 4) mod m]) by fe_from_std                                  P < 6r times CIN < r: 6                  < 2r
//   N          = fe_mul(Cn, P(q_N)) = P(q_N c')                                      2 x 6 = 12                               < 2r, plain
//   out        = W + N + P(q_C) + P(PI): < 2r + 2r + 6r + 6r = 16r, times R' mod r (< r) in fp_put_plain: 16                  canonical
// (fp_put_plain takes < 68r.  The limbs: every addend has limbs < 2^29 below the top one and fe_add carries after each sum; the top limb of
// a value < 16r < 2^260 is < 2^28.)  Products: the parent's 15 and 6 pairs, and 2 more (Cn, N): one more column read at i and one at i + 4.
// With the fields' true factors (2^256 = 5.3r for BN254, 2.3r for BLS12-381) out is < 14.6r and < 8.6r.
// pn_gate_kernel is the first four pairs of W (48) plus N plus q_C + PI over the rows of H, c' = c[(i + 1) mod n]: the same < 16r,
// renormalised and compared with 0 and r.
constexpr int PN_NCOL = PK_NCOL + 1, PN_GATE_NCOL = PK_GATE_NCOL + 1;
constexpr int PN_QN = PK_NCOL, PNG_QN = PK_GATE_NCOL;                          // q_N follows plonk_impl.hip.h's columns in both orders

struct PnCols { const u32* c[PN_NCOL]; };
struct PnGateCols { const u32* c[PN_GATE_NCOL]; };

// out_i = the bracket of round 3 at point i of the coset 7 H_m, m = 4n; Z(wX) and c(wX) are element (i + 4) mod m.  One lane per element.
__global__ __launch_bounds__(FP_BLOCK) void pn_quotient_kernel(const PnCols cs, const PkConsts* __restrict__ pc, u32* __restrict__ out, u64 m) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const u64 iw = (i + 4) & (m - 1);
    const fe A = pk_internal(cs.c[PK_A], i), B = pk_internal(cs.c[PK_B], i), C = pk_internal(cs.c[PK_C], i);
    const fe G = pc->G, BI = pc->BI;
    const fe Zp = pk_plain(cs.c[PK_Z], i);
    fe D;
    {
        const fe Bx = fe_mul(pk_plain(cs.c[PK_X], i), BI);
        const fe f1 = fe_add(fe_add(A, Bx), G);
        const fe f2 = fe_add(fe_add(B, pk_times_k(Bx, pc->k1_small, pc->K1)), G);
        const fe f3 = fe_add(fe_add(C, pk_times_k(Bx, pc->k2_small, pc->K2)), G);
        const fe P1 = fe_mul(fe_mul(fe_mul(f1, f2), f3), Zp);
        const fe g1 = fe_add(fe_add(A, fe_mul(pk_plain(cs.c[PK_S1], i), BI)), G);
        const fe g2 = fe_add(fe_add(B, fe_mul(pk_plain(cs.c[PK_S2], i), BI)), G);
        const fe g3 = fe_add(fe_add(C, fe_mul(pk_plain(cs.c[PK_S3], i), BI)), G);
        const fe P2 = fe_mul(fe_mul(fe_mul(g1, g2), g3), pk_plain(cs.c[PK_Z], iw));
        D = fe_sub<2>(P1, P2);
    }
    fe_wide acc;
    fe_wide_zero(acc);
    pk_gate_macs<PK_QL, PK_QR, PK_QO, PK_QM>(acc, cs, i, A, B, C);
    fe_wide_mac(acc, D, pc->AI);
    fe_wide_mac(acc, fe_mul(pk_plain(cs.c[PK_L1], i), pc->A2), fe_sub<2>(Zp, fp_const_cout()));
    const fe W = fe_wide_reduce(acc);
    // the next-row term after the wide sum is reduced: only W is live while its two products run
    const fe N = fe_mul(pk_internal(cs.c[PK_C], iw), pk_plain(cs.c[PN_QN], i));
    fp_put_plain(out, i, fe_add(fe_add(fe_add(W, N), pk_plain(cs.c[PK_QC], i)), pk_plain(cs.c[PK_PI], i)));
}

// row i of H: q_L a + q_R b + q_O c + q_M a b + q_C + q_N c[(i + 1) mod n] + PI = 0?  stat[0] += the rows that fail, stat[1] = min(stat[1],
// the first of them): counted as pk_gate_kernel counts, in LDS, one atomic add and one atomic min per workgroup that has a failure
__global__ __launch_bounds__(FP_BLOCK) void pn_gate_kernel(const PnGateCols cs, u64 n, unsigned long long* __restrict__ stat) {
    __shared__ unsigned long long zs[2];
    const int t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * FP_BLOCK + t;
    if (t == 0) { zs[0] = 0; zs[1] = ~0ull; }
    __syncthreads();
    if (i < n) {
        const u64 in = i + 1 < n ? i + 1 : 0;
        const fe A = pk_internal(cs.c[PG_A], i), B = pk_internal(cs.c[PG_B], i), C = pk_internal(cs.c[PG_C], i);
        fe_wide acc;
        fe_wide_zero(acc);
        pk_gate_macs<PG_QL, PG_QR, PG_QO, PG_QM>(acc, cs, i, A, B, C);
        const fe W = fe_wide_reduce(acc);
        const fe N = fe_mul(pk_internal(cs.c[PG_C], in), pk_plain(cs.c[PNG_QN], i));
        const fe s = fe_renorm(fe_add(fe_add(fe_add(W, N), pk_plain(cs.c[PG_QC], i)), pk_plain(cs.c[PG_PI], i)));
        if (!fe_is_zero_m(s)) {
            atomicAdd(&zs[0], 1ull);
            atomicMin(&zs[1], (unsigned long long)i);
        }
    }
    __syncthreads();
    if (t == 0 && zs[0]) {
        atomicAdd(&stat[0], zs[0]);
        atomicMin(&stat[1], zs[1]);
    }
}

// ---- the extension of a witness under the chain rule: plonk_r1cs_impl.hip.h's two kernels with a store step of 2 --------------------------
// Term t >= 1 of a segment of m terms defines an auxiliary when it completes an even prefix (t odd) or is the last (t = m - 1): variable
// first + t / 2.  Forms and bounds are that file's, line for line: the sums are the same, only fewer of them are stored.
__device__ __forceinline__ bool pn_stores(u64 t, u64 m) { return (t & 1) || t + 1 == m; }

__global__ __launch_bounds__(FP_BLOCK) void pn_r1cs_extend_kernel(const u32* __restrict__ ids, u64 n, const u64* __restrict__ ptr, const u32* __restrict__ first,
                                                                 const u32* __restrict__ cols, const u32* __restrict__ coef, u32* w) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 s = ids[i];
    const u64 k0 = ptr[s], k1 = ptr[s + 1], x0 = first[s];
    fe acc = pr_term(coef, cols, w, k0);
    for (u64 k = k0 + 1; k < k1; ++k) {
        acc = fe_renorm(fe_add(acc, pr_term(coef, cols, w, k)));
        if (pn_stores(k - k0, k1 - k0)) pr_store(w, x0 + ((k - k0) >> 1), fe_canon(acc));
    }
}
__global__ __launch_bounds__(FP_BLOCK) void pn_r1cs_extend_wave_kernel(const u32* __restrict__ ids, u64 n, const u64* __restrict__ ptr, const u32* __restrict__ first,
                                                                      const u32* __restrict__ cols, const u32* __restrict__ coef, u32* w) {
    const int lane = threadIdx.x & (PR_WAVE - 1);
    const u64 i = (u64)blockIdx.x * PR_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;                                                      // the whole wave leaves
    const u32 s = ids[i];
    const u64 k0 = ptr[s], k1 = ptr[s + 1], x0 = first[s];
    fe carry = fe_zero();
    for (u64 base = k0; base < k1; base += PR_WAVE) {
        const u64 k = base + lane;
        fe v = fe_zero();
        if (k < k1) v = fe_canon(pr_term(coef, cols, w, k));
#pragma unroll
        for (int d = 1; d < PR_WAVE; d <<= 1) {
            fe o;
#pragma unroll
            for (int l = 0; l < NR; ++l) o.l[l] = __shfl_up(v.l[l], d);
            if (lane >= d) v = fe_add(v, o);
        }
        const fe c = fe_canon(fe_renorm(fe_add(v, carry)));
        if (k < k1 && k > k0 && pn_stores(k - k0, k1 - k0)) pr_store(w, x0 + ((k - k0) >> 1), c);
#pragma unroll
        for (int l = 0; l < NR; ++l) carry.l[l] = __shfl(c.l[l], PR_WAVE - 1);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
void FRN_FN(pn_quotient_dev)(const u64* const* d_cols, u32 log_n, const u64* alpha, const u64* beta, const u64* gamma, const u64* k1, const u64* k2, u64* d_out, hipStream_t st) {
    const std::string who = "plonk next";
    const FpWords a = pk_scalar(who, alpha, "alpha"), b = pk_scalar(who, beta, "beta"), g = pk_scalar(who, gamma, "gamma"), w1 = pk_scalar(who, k1, "k1"), w2 = pk_scalar(who, k2, "k2");
    if (log_n + 2 > (u32)FRN_S) throw std::runtime_error("plonk next: the coset of 2^" + std::to_string(log_n + 2) + " points for n = 2^" + std::to_string(log_n) + " exceeds the field's 2-adicity");
    ZK_REQUIRE(d_cols && d_out, "plonk next: null argument");
    const u64 m = 4ull << log_n;
    PnCols cs{};
    for (int c = 0; c < PN_NCOL; ++c) {
        cs.c[c] = (const u32*)d_cols[c];
        ZK_REQUIRE(cs.c[c], "plonk next: quotient: column " + std::to_string(c) + " is null");
        fp_aligned({cs.c[c]});
        ZK_REQUIRE(pk_apart(d_out, cs.c[c], m), "plonk next: quotient: the output overlaps column " + std::to_string(c));
    }
    fp_aligned({d_out});
    DevBuf pc;
    pc.reserve(sizeof(PkConsts));
    hipLaunchKernelGGL(pk_setup_kernel, dim3(1), dim3(64), 0, st, a, b, g, w1, w2, (PkConsts*)pc.p);
    hipLaunchKernelGGL(pn_quotient_kernel, dim3(fp_blocks(m)), dim3(FP_BLOCK), 0, st, cs, (const PkConsts*)pc.p, (u32*)d_out, m);
    ZK_HIP(hipGetLastError());
}
void FRN_FN(pn_gate_check_dev)(const u64* const* d_cols, u64 n, u64* n_bad, u64* first_bad, hipStream_t st) {
    ZK_REQUIRE(d_cols && n_bad && first_bad, "plonk next: null argument");
    fp_limit(n);
    u64 stat[2] = {0, ~0ull};
    if (n) {
        PnGateCols cs{};
        for (int c = 0; c < PN_GATE_NCOL; ++c) {
            cs.c[c] = (const u32*)d_cols[c];
            ZK_REQUIRE(cs.c[c], "plonk next: gate check: column " + std::to_string(c) + " is null");
            fp_aligned({cs.c[c]});
        }
        DevBuf ds;
        ds.reserve(16);
        h2d_sync(ds.p, stat, 16);
        hipLaunchKernelGGL(pn_gate_kernel, dim3(fp_blocks(n)), dim3(FP_BLOCK), 0, st, cs, n, (unsigned long long*)ds.p);
        ZK_HIP(hipGetLastError());
        d2h_sync(stat, ds.p, 16);
    }
    *n_bad = stat[0];
    *first_bad = stat[1];
}

// ---- the chain rule (include/zkgpu.h states it in full) -----------------------------------------------------------------------------------
// PrCompiler's normalisation, short folds, linear and product cases and refusals; a fold of m >= 3 signals is a chain: a running sum down
// column c, two terms a row, row j constraining the c of row j + 1 through q_N = -1.  `pending` is a chain's value that must stand in c of
// the row emitted next.
struct PnCompiler : PrCompiler {
    bool has_pending = false;
    u32 pending = 0;
    PnCompiler(const FrHost& f, PlonkR1cs& hh) : PrCompiler(f, hh) {}
    void emit_n(u32 origin, u32 a, u32 b, u32 c, const u64* ql, const u64* qr, const u64* qo, const u64* qm, const u64* qc, const u64* qn) {
        emit(origin, a, b, c, ql, qr, qo, qm, qc);
        h.sel_n.insert(h.sel_n.end(), qn, qn + 4);
        has_pending = false;
    }
    // a row of its own for a chain's value: every selector zero, c = the value
    void land(u32 origin) {
        if (has_pending) emit_n(origin, 0, 0, pending, zero, zero, zero, zero, zero, zero);
    }
    // rows 1 .. k of the chain over sig; closed: the last row carries q_C = k0 and no q_N, and defines no auxiliary.  -> the chain's value
    u32 chain(u32 origin, const PrSide& sig, bool closed, const u64* k0) {
        const u64 m = sig.size(), k = (m + 1) / 2, n_aux = closed ? k - 1 : k, n_terms = closed ? 2 * (k - 1) : m;
        ZK_REQUIRE(h.n_vars + n_aux <= 0xFFFFFFFFull, "plonk r1cs: constraint " + std::to_string(origin) + ": the gate table needs " + std::to_string(h.n_vars + n_aux) +
                                                         " variables, a variable id has 32 bits");
        const u32 first = (u32)h.n_vars;
        h.seg_first.push_back(first);
        for (u64 j = 0; j < n_terms; ++j) { h.seg_wire.push_back(sig[j].w); h.seg_coef.insert(h.seg_coef.end(), sig[j].c, sig[j].c + 4); }
        h.seg_ptr.push_back(h.seg_wire.size());
        h.max_terms = std::max<u64>(h.max_terms, n_terms);
        for (u64 j = 0; j < k; ++j) {
            const bool has_b = 2 * j + 1 < m, last = j + 1 == k;
            const u32 c = j ? first + (u32)j - 1 : (has_pending ? pending : 0);
            emit_n(origin, sig[2 * j].w, has_b ? sig[2 * j + 1].w : 0, c, sig[2 * j].c, has_b ? sig[2 * j + 1].c : zero, j ? one : zero, zero, closed && last ? k0 : zero,
                   closed && last ? zero : minus_one);
        }
        h.n_vars += n_aux;
        if (!closed) { has_pending = true; pending = first + (u32)k - 1; }
        return first + (u32)k - 1;
    }
    void constraint_n(u32 i, const g16::Row& row) {
        PrSide S[3];
        u64 k[3][4];
        for (int s = 0; s < 3; ++s) {
            const g16::Lc& lc = row.lc[s];
            PrSide raw(lc.col.size());
            for (size_t t = 0; t < lc.col.size(); ++t) {
                ZK_REQUIRE(lc.col[t] < h.n_wires, "plonk r1cs: constraint " + std::to_string(i) + ": wire " + std::to_string(lc.col[t]) + ", the file has " + std::to_string(h.n_wires) + " wires");
                raw[t].w = lc.col[t];
                std::memcpy(raw[t].c, &lc.coeff[8 * t], 32);
            }
            S[s] = normalise(std::move(raw), k[s]);
        }
        u64 k0[4], nkc[4];
        mul(k[0], k[1], k0);
        neg(k[2], nkc);
        F.add(k0, nkc, k0);                                                  // kA kB - kC
        if (S[0].empty() || S[1].empty()) {                                  // linear, as plonk_r1cs_impl.hip.h; four signals or more are one closed chain
            const int other = S[0].empty() ? 1 : 0;
            const u64* kk = k[1 - other];
            PrSide L;
            for (PrTerm t : S[other]) { mul(kk, t.c, t.c); L.push_back(t); }
            for (PrTerm t : S[2]) { neg(t.c, t.c); L.push_back(t); }
            u64 none[4];
            L = normalise(std::move(L), none);
            if (L.empty()) {
                ZK_REQUIRE(is_zero(k0), "plonk r1cs: constraint " + std::to_string(i) + " is 0 = k with k not zero: no witness satisfies it");
                return;
            }
            if (L.size() >= 4) { chain(i, L, true, k0); return; }
            PrTerm pad; pad.w = 0; std::memcpy(pad.c, zero, 32);
            while (L.size() < 3) L.push_back(pad);
            emit_n(i, L[0].w, L[1].w, L[2].w, L[0].c, L[1].c, L[2].c, zero, k0, zero);
            return;
        }
        // product: the short folds first (plonk_r1cs_impl.hip.h's gate), then the chains of A, B, C in that order -- each lands in row 1
        // of the next, C's in the closing gate
        PrTerm t[3];
        for (int s = 0; s < 3; ++s) {
            t[s].w = 0; std::memcpy(t[s].c, S[s].empty() ? zero : one, 32);
            if (S[s].size() == 1) t[s] = S[s][0];
            if (S[s].size() != 2) continue;
            const size_t before = h.origin.size();
            t[s] = reduce(i, S[s], 1)[0];
            h.sel_n.insert(h.sel_n.end(), 4 * (h.origin.size() - before), 0);
        }
        for (int s = 0; s < 3; ++s)
            if (S[s].size() >= 3) t[s].w = chain(i, S[s], false, zero);
        if (has_pending && pending != t[2].w) land(i);
        u64 qm[4], ql[4], qr[4], qo[4];
        mul(t[0].c, t[1].c, qm);
        mul(t[0].c, k[1], ql);
        mul(k[0], t[1].c, qr);
        neg(t[2].c, qo);
        emit_n(i, t[0].w, t[1].w, t[2].w, ql, qr, qo, qm, k0, zero);
    }
};

// the .r1cs -> the handle's tables under the chain rule.  Host only.
PlonkR1cs* FRN_FN(pn_r1cs_new)(const void* r1cs, size_t len) {
    ZK_REQUIRE(r1cs, "plonk r1cs: null input");
    const Curve& cv = fp_curve();
    const g16::R1cs rc = g16::parse_r1cs((const uint8_t*)r1cs, len, cv);   // refuses a file over another field
    std::unique_ptr<PlonkR1cs> h(new PlonkR1cs);
    h->curve = &cv;
    h->store_step = 2;
    h->n_wires = rc.n_wires;
    ZK_REQUIRE((u64)rc.n_pub_out + rc.n_pub_in < rc.n_wires, "plonk r1cs: header: fewer wires than public signals");
    h->n_public = rc.n_pub_out + rc.n_pub_in;
    h->n_constraints = rc.rows.size();
    h->n_vars = rc.n_wires;
    h->seg_ptr.push_back(0);
    const FrHost F(cv);
    PnCompiler pc(F, *h);
    for (size_t i = 0; i < rc.rows.size(); ++i) pc.constraint_n((u32)i, rc.rows[i]);
    return h.release();
}

// d_w: n_vars elements, the first n_wires in the stored form; fills the rest, every second prefix of a segment and its last
void FRN_FN(pn_r1cs_extend_dev)(PlonkR1cs& h, u64* d_w, hipStream_t st) {
    ZK_REQUIRE(h.store_step == 2, "plonk r1cs: the handle was not compiled under the chain rule");
    if (!pr_upload(h, d_w, st)) return;
    if (h.n_short)
        hipLaunchKernelGGL(pn_r1cs_extend_kernel, dim3(fp_blocks(h.n_short)), dim3(FP_BLOCK), 0, st, (const u32*)h.d_short.p, h.n_short, (const u64*)h.d_ptr.p, (const u32*)h.d_first.p,
                           (const u32*)h.d_wire.p, (const u32*)h.d_coef.p, (u32*)d_w);
    if (h.n_long)
        hipLaunchKernelGGL(pn_r1cs_extend_wave_kernel, dim3((unsigned)((h.n_long + PR_WAVES - 1) / PR_WAVES)), dim3(FP_BLOCK), 0, st, (const u32*)h.d_long.p, h.n_long, (const u64*)h.d_ptr.p,
                           (const u32*)h.d_first.p, (const u32*)h.d_wire.p, (const u32*)h.d_coef.p, (u32*)d_w);
    ZK_HIP(hipGetLastError());
}
