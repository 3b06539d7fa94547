// The R1CS import of the PLONK prover, generic over the scalar field: an .r1cs compiled on the host to a gate table of
// fan-in 2, and the values of the auxiliary variables that table adds, computed on the device from a witness at every proof.  Included by
// groth16.hip after plonk_impl.hip.h, in the same namespace: it uses that file's forms (pk_plain), frpoly_impl.hip.h's word helpers and
// fr_rows_impl.hip.h's frn_canon_to_fe_kernel.  No include guard on purpose.
//
// The rule (include/zkgpu.h states it in full).  Wire w is variable w, auxiliaries follow from n_wires in emission order.  A side of a
// constraint is normalised (equal wires added, zeros dropped, wire 0 taken out as the constant k, signals by ascending wire).  reduce(sig,
// keep) folds the first m = len - keep + 1 signals into m - 1 auxiliaries x_j = sum_{i <= j + 1} c_i w[s_i]: every auxiliary is a PREFIX of
// its side's sum over ORIGINAL wires, none reads another.  One fold is one segment: (first auxiliary, m terms).
//
// Forms (plonk_impl.hip.h).  A stored element is the plain integer P(w) = w R mod r (< 2^256 < 6r as far as these kernels care; what
// _mont_dev leaves is canonical).  A coefficient is uploaded once, in internal form I(c) = c R' (< 2r, frn_canon_to_fe_kernel).
// fe_mul(I(c), P(w)) = c w R is plain again, sums of plain values are plain, a stored prefix is the canonical representative of its sum.
//
// Bounds, against fe29_impl.hip.h's A B <= 68 ("<" is the value's bound in multiples of r):
//   pk_r1cs_extend_kernel, one lane per segment of fewer than PLONK_R1CS_WAVE_MIN_TERMS terms
//     p        = fe_mul(I(c), P(w))                         2 x 6 = 12                                             < 2r
//     acc      = the first p, then fe_renorm(acc + p)       acc + p < 4r, times R' mod r (< r): 4                  < 2r
//     store    = fe_canon(acc)                              (acc < 2r)                                             canonical
//   The renormalised sum IS the running sum: one product per term, one reduction per stored prefix, and no cadence to keep
//   (frn_row_sum lets four products pile up because it stores nothing in between; here every prefix is stored).
//   pk_r1cs_extend_wave_kernel, one wave per longer segment, 64 terms a step, lane l on term 64 i + l
//     p        = fe_canon(fe_mul(I(c), P(w))), 0 past the end    12 -> < 2r -> canonical                           < r
//     scan     = six __shfl_up steps of fe_add over the lanes: after step s a lane holds at most 2^s values < r    < 64r
//     v        = scan + carry, carry = the previous step's stored value of lane 63 (canonical; 0 at the start)     < 65r
//     store    = fe_canon(fe_renorm(v))                     65 x 1 = 65                                            canonical
//   Without the fe_canon of p the scan would reach 128r and need a reduction half way; fe_canon is a subtraction and a select.
//   The limbs: fe_add carries after every step, so a limb below the top one is < 2^29 and a sum of two < 2^30; the top limb of a value
//   < 65r < 2^262 is < 2^30.
// Neither kernel uses LDS, atomics or scratch.  Lanes past a segment's end take part in the shuffles and store nothing.
constexpr int PR_WAVE = 64, PR_WAVES = FP_BLOCK / PR_WAVE;                   // the waves of a workgroup, one long segment each
static_assert(PLONK_R1CS_WAVE_MIN_TERMS >= 2, "plonk r1cs: a segment has at least two terms");

__device__ __forceinline__ fe pr_term(const u32* __restrict__ coef, const u32* __restrict__ cols, const u32* w, u64 k) {
    return fe_mul(fp_fe_load(coef, k), pk_plain(w, cols[k]));
}
__device__ __forceinline__ void pr_store(u32* w, u64 i, const fe& canon) {
    u32 o[NL];
    fp_pack(canon, o);
    fp_store_words(w, i, o);
}
// ids: the n segments of this launch.  Segment s has the terms [ptr[s], ptr[s + 1]) and stores term t >= 1's prefix at first[s] + t - 1.
// w is read below n_wires and written from n_wires on (the host checked every wire and every auxiliary id).
__global__ __launch_bounds__(FP_BLOCK) void pk_r1cs_extend_kernel(const u32* __restrict__ ids, u64 n, const u64* __restrict__ ptr, const u32* __restrict__ first,
                                                                 const u32* __restrict__ cols, const u32* __restrict__ coef, u32* w) {
    const u64 i = (u64)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 s = ids[i];
    const u64 k0 = ptr[s], k1 = ptr[s + 1];
    u64 x = first[s];
    fe acc = pr_term(coef, cols, w, k0);
    for (u64 k = k0 + 1; k < k1; ++k, ++x) {
        acc = fe_renorm(fe_add(acc, pr_term(coef, cols, w, k)));
        pr_store(w, x, fe_canon(acc));
    }
}
__global__ __launch_bounds__(FP_BLOCK) void pk_r1cs_extend_wave_kernel(const u32* __restrict__ ids, u64 n, const u64* __restrict__ ptr, const u32* __restrict__ first,
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
        if (k < k1 && k > k0) pr_store(w, x0 + (k - k0) - 1, c);
#pragma unroll
        for (int l = 0; l < NR; ++l) carry.l[l] = __shfl(c.l[l], PR_WAVE - 1);
    }
}

// ---- host side: the compile rule ------------------------------------------------------------------------------------------------------
struct PrTerm { u32 w; u64 c[4]; };                                          // a wire and its canonical coefficient
typedef std::vector<PrTerm> PrSide;

struct PrCompiler {
    const FrHost& F;
    PlonkR1cs& h;
    u64 zero[4] = {0, 0, 0, 0}, one[4] = {1, 0, 0, 0}, minus_one[4];
    PrCompiler(const FrHost& f, PlonkR1cs& hh) : F(f), h(hh) { neg(one, minus_one); }
    static bool is_zero(const u64* a) { return !(a[0] | a[1] | a[2] | a[3]); }
    void neg(const u64* a, u64* out) const {
        if (is_zero(a)) { std::memcpy(out, a, 32); return; }
        u64 br = 0, t[4];
        for (int i = 0; i < 4; ++i) { const unsigned __int128 d = (unsigned __int128)F.p[i] - a[i] - br; t[i] = (u64)d; br = (u64)(d >> 64) & 1; }
        std::memcpy(out, t, 32);
    }
    void mul(const u64* a, const u64* b, u64* out) const { u64 t[4]; F.to_mont(a, t); F.mul(t, b, out); }   // canonical times canonical
    // equal wires added, zeros dropped, wire 0 out as k, the signals by ascending wire
    PrSide normalise(PrSide side, u64* k) const {
        std::stable_sort(side.begin(), side.end(), [](const PrTerm& x, const PrTerm& y) { return x.w < y.w; });
        PrSide out;
        std::memset(k, 0, 32);
        for (size_t i = 0; i < side.size();) {
            PrTerm t = side[i];
            for (++i; i < side.size() && side[i].w == t.w; ++i) F.add(t.c, side[i].c, t.c);
            if (is_zero(t.c)) continue;
            if (t.w == 0) std::memcpy(k, t.c, 32);
            else out.push_back(t);
        }
        return out;
    }
    void emit(u32 origin, u32 a, u32 b, u32 c, const u64* ql, const u64* qr, const u64* qo, const u64* qm, const u64* qc) {
        const u64* q[5] = {ql, qr, qo, qm, qc};
        for (int s = 0; s < 5; ++s) h.sel[s].insert(h.sel[s].end(), q[s], q[s] + 4);
        h.wire[0].push_back(a); h.wire[1].push_back(b); h.wire[2].push_back(c);
        h.origin.push_back(origin);
    }
    PrSide reduce(u32 origin, const PrSide& sig, size_t keep) {
        if (sig.size() <= keep) return sig;
        const u64 m = sig.size() - keep + 1;
        ZK_REQUIRE(h.n_vars + (m - 1) <= 0xFFFFFFFFull, "plonk r1cs: constraint " + std::to_string(origin) + ": the gate table needs " + std::to_string(h.n_vars + m - 1) +
                                                             " variables, a variable id has 32 bits");
        const u32 first = (u32)h.n_vars;
        h.seg_first.push_back(first);
        for (u64 j = 0; j < m; ++j) { h.seg_wire.push_back(sig[j].w); h.seg_coef.insert(h.seg_coef.end(), sig[j].c, sig[j].c + 4); }
        h.seg_ptr.push_back(h.seg_wire.size());
        h.max_terms = std::max<u64>(h.max_terms, m);
        emit(origin, sig[0].w, sig[1].w, first, sig[0].c, sig[1].c, minus_one, zero, zero);
        for (u64 j = 2; j < m; ++j) emit(origin, first + (u32)j - 2, sig[j].w, first + (u32)j - 1, one, sig[j].c, minus_one, zero, zero);
        h.n_vars += m - 1;
        PrSide out;
        PrTerm x; x.w = first + (u32)m - 2; std::memcpy(x.c, one, 32);
        out.push_back(x);
        out.insert(out.end(), sig.begin() + m, sig.end());
        return out;
    }
    void constraint(u32 i, const g16::Row& row) {
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
        if (S[0].empty() || S[1].empty()) {                                  // linear: kA B_sig - C_sig, or kB A_sig - C_sig
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
            L = reduce(i, L, 3);
            PrTerm pad; pad.w = 0; std::memcpy(pad.c, zero, 32);
            while (L.size() < 3) L.push_back(pad);
            emit(i, L[0].w, L[1].w, L[2].w, L[0].c, L[1].c, L[2].c, zero, k0);
            return;
        }
        const PrTerm a = reduce(i, S[0], 1)[0], b = reduce(i, S[1], 1)[0];
        PrTerm c; c.w = 0; std::memcpy(c.c, zero, 32);
        if (!S[2].empty()) c = reduce(i, S[2], 1)[0];
        u64 qm[4], ql[4], qr[4], qo[4];
        mul(a.c, b.c, qm);
        mul(a.c, k[1], ql);
        mul(k[0], b.c, qr);
        neg(c.c, qo);
        emit(i, a.w, b.w, c.w, ql, qr, qo, qm, k0);
    }
};

// the .r1cs -> the handle's tables.  Host only: a machine without a device compiles and reads them back.
PlonkR1cs* FRN_FN(pk_r1cs_new)(const void* r1cs, size_t len) {
    ZK_REQUIRE(r1cs, "plonk r1cs: null input");
    const Curve& cv = fp_curve();
    const g16::R1cs rc = g16::parse_r1cs((const uint8_t*)r1cs, len, cv);   // refuses a file over another field
    std::unique_ptr<PlonkR1cs> h(new PlonkR1cs);
    h->curve = &cv;
    h->n_wires = rc.n_wires;
    ZK_REQUIRE((u64)rc.n_pub_out + rc.n_pub_in < rc.n_wires, "plonk r1cs: header: fewer wires than public signals");
    h->n_public = rc.n_pub_out + rc.n_pub_in;
    h->n_constraints = rc.rows.size();
    h->n_vars = rc.n_wires;
    h->seg_ptr.push_back(0);
    const FrHost F(cv);
    PrCompiler pc(F, *h);
    for (size_t i = 0; i < rc.rows.size(); ++i) pc.constraint((u32)i, rc.rows[i]);
    return h.release();
}

// the segment table to the device, on the first extension of a handle -> false when there is no segment
static bool pr_upload(PlonkR1cs& h, u64* d_w, hipStream_t st) {
    ZK_REQUIRE(h.curve == &fp_curve(), "plonk r1cs: the handle is over another field");
    ZK_REQUIRE(d_w, "plonk r1cs: null argument");
    fp_aligned({d_w});
    const u64 n_seg = h.seg_first.size(), n_terms = h.seg_wire.size();
    if (!n_seg) return false;
    if (!h.on_device) {
        u64 wave_min = PLONK_R1CS_WAVE_MIN_TERMS;
        if (const char* e = getenv("ZK_PLONK_R1CS_WAVE_MIN")) wave_min = std::max<u64>(2, strtoull(e, nullptr, 10));   // the knob of tools/plonk_time.py: either kernel alone
        std::vector<u32> ids_short, ids_long;
        for (u64 s = 0; s < n_seg; ++s) (h.seg_ptr[s + 1] - h.seg_ptr[s] < wave_min ? ids_short : ids_long).push_back((u32)s);
        h.d_ptr.reserve((n_seg + 1) * 8); h2d_sync(h.d_ptr.p, h.seg_ptr.data(), (n_seg + 1) * 8);
        h.d_first.reserve(n_seg * 4); h2d_sync(h.d_first.p, h.seg_first.data(), n_seg * 4);
        h.d_wire.reserve(n_terms * 4); h2d_sync(h.d_wire.p, h.seg_wire.data(), n_terms * 4);
        if (!ids_short.empty()) { h.d_short.reserve(ids_short.size() * 4); h2d_sync(h.d_short.p, ids_short.data(), ids_short.size() * 4); }
        if (!ids_long.empty()) { h.d_long.reserve(ids_long.size() * 4); h2d_sync(h.d_long.p, ids_long.data(), ids_long.size() * 4); }
        DevBuf canon;
        canon.reserve(n_terms * 32); h2d_sync(canon.p, h.seg_coef.data(), n_terms * 32);
        h.d_coef.reserve(n_terms * NR * 4);
        hipLaunchKernelGGL(frn_canon_to_fe_kernel, dim3((unsigned)((n_terms + 255) / 256)), dim3(256), 0, st, (const u32*)canon.p, (u32*)h.d_coef.p, n_terms);
        ZK_HIP(hipGetLastError());
        h.n_short = ids_short.size(); h.n_long = ids_long.size();
        h.on_device = true;
    }
    return true;
}
// d_w: n_vars elements, the first n_wires in the stored form; fills the rest.  The segment table goes up on the first call.
void FRN_FN(pk_r1cs_extend_dev)(PlonkR1cs& h, u64* d_w, hipStream_t st) {
    ZK_REQUIRE(h.store_step == 1, "plonk r1cs: the handle was compiled under the chain rule");
    if (!pr_upload(h, d_w, st)) return;
    if (h.n_short)
        hipLaunchKernelGGL(pk_r1cs_extend_kernel, dim3(fp_blocks(h.n_short)), dim3(FP_BLOCK), 0, st, (const u32*)h.d_short.p, h.n_short, (const u64*)h.d_ptr.p, (const u32*)h.d_first.p,
                           (const u32*)h.d_wire.p, (const u32*)h.d_coef.p, (u32*)d_w);
    if (h.n_long)
        hipLaunchKernelGGL(pk_r1cs_extend_wave_kernel, dim3((unsigned)((h.n_long + PR_WAVES - 1) / PR_WAVES)), dim3(FP_BLOCK), 0, st, (const u32*)h.d_long.p, h.n_long, (const u64*)h.d_ptr.p,
                           (const u32*)h.d_first.p, (const u32*)h.d_wire.p, (const u32*)h.d_coef.p, (u32*)d_w);
    ZK_HIP(hipGetLastError());
}
