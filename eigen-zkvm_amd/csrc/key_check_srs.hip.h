// groth16_key_check_srs: is this key a key for this circuit over this powers-of-tau file?  Included once by groth16.hip inside namespace zk,
// behind groth16_srs.hip.h (whose PairEq, rho_dev, rlc, Findings and skipped_entry it uses).  DESIGN.md 3.16 has the algebra.
//
// No group transform: with weights rho_j per wire, s = M rho over the rows and u = iNTT(s), sum_j rho_j m_j(tau) = sum_t u_t tau^t, so the random
// combination of a whole query is ONE multi-scalar sum against the file's monomial sections as they stand.  The scalar side (row sums with
// the public / other split, transforms, canonical scalars) is key_check_srs_impl.hip.h per scalar field; sums, pairings and point classes are
// the existing ones.  The three sums of X_S = sum_t (u^B alphaTauG1 + u^A betaTauG1 + u^C tauG1)[t] are one sum over the concatenated bases
// [alphaTauG1 | betaTauG1 | tauG1] (msm_dev takes one base and one scalar array; there is no point addition outside a sum), and tauG1 at the
// end of that buffer serves a, b_g1 and h as well.

namespace g16 {
// out[k] = rho[idx[k]]: a section's weights in the order of its points (8 words each)
__global__ __launch_bounds__(256) void kc_gather_rho_kernel(const u32* __restrict__ rho, const u32* __restrict__ idx, u64 n, u32* __restrict__ out) {
    const u64 k = blockIdx.x * 256ull + threadIdx.x;
    if (k >= n) return;
    const uint4* src = (const uint4*)(rho + (u64)idx[k] * 8);
    uint4* dst = (uint4*)(out + k * 8);
    dst[0] = src[0]; dst[1] = src[1];
}
struct KcMod { u32 w[8]; };
// the scalars of sum_{i < len} rho'_i (tauG1[i + m] - tauG1[i]) over tauG1[0 .. 2m - 1): (-rho' mod r | 0 | rho'), zero from len on
__global__ __launch_bounds__(256) void kc_h_scalars_kernel(const u32* __restrict__ rho, u64 m, u64 len, KcMod r, u32* __restrict__ out) {
    const u64 t = blockIdx.x * 256ull + threadIdx.x;
    if (t >= 2 * m - 1) return;
    u32 v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const u64 i = t < m ? t : t - m;
    if (t != m - 1 && i < len) {
        u32 any = 0;
        for (int k = 0; k < 8; ++k) { v[k] = rho[i * 8 + k]; any |= v[k]; }
        if (t < m && any) {                                 // r - rho'
            u64 br = 0;
            for (int k = 0; k < 8; ++k) { const u64 d = (u64)r.w[k] - v[k] - br; v[k] = (u32)d; br = (d >> 32) & 1; }
        }
    }
    for (int k = 0; k < 8; ++k) out[t * 8 + k] = v[k];
}

// one query of the key as the check sees it: the finite points (Montgomery) side by side, where each sat in the section, its wire, its weight
struct KcsSection {
    const char* name; Group g; const PointVec* pv; u64 want;
    std::vector<u32> wire;                                  // by index in the section (h: the index itself)
    std::vector<u64> pos;                                   // by finite point: its index in the section
    DevBuf pts, rho;
    const char* skip = nullptr;                             // why it is not compared
    u64 finite_below(u64 len) const { return (u64)(std::lower_bound(pos.begin(), pos.end(), len) - pos.begin()); }
};
}  // namespace g16

std::string groth16_key_check_srs(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, const Srs* srs,
                                  const uint8_t* seed, uint32_t max_findings) {
    using namespace g16;
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(r1cs && params && srs, "groth16 key check: null input");
    ZK_REQUIRE(srs->curve == &cv, std::string("groth16 key check: the powers-of-tau file was opened for ") + srs->curve->name);
    const auto t0 = clk::now();
    const R1cs rc = parse_r1cs((const uint8_t*)r1cs, r1cs_len, cv);
    const Params pk = parse_params((const uint8_t*)params, params_len, 4 * (int)cv.fq_words);
    const Circuit C(rc);
    ZK_REQUIRE((int)srs->power >= C.logm, "groth16 key check: the file has power " + std::to_string(srs->power) + ", the circuit's " + std::to_string(C.n_rows) +
                                               " rows need power " + std::to_string(C.logm));
    const auto t1 = clk::now();
    hipStream_t st = cur_stream();
    const MsmOps& M = cv.msm();
    const Groth16Ops& FR = cv.groth16();
    const u64 m = C.m, nh = m - 1, nw = C.n_wires;
    const u32 ni = C.ni;
    const size_t P1 = cv.point_words(G1), P2 = cv.point_words(G2), B1 = 4 * P1, B2 = 4 * P2;
    Findings F({"query_mismatch", "vk_mismatch"}, max_findings);
    std::string skipped;
    double ms_rows_tr[2] = {0, 0}, ms_sum = 0, ms_pair = 0;
    u64 n_row_sums = 0, n_sums = 0;

    // 1. the sections, in the order of the report: which wire each entry stands for (write_params: every input, then the others with A-density;
    //    b: every wire with B-density), the finite points, their classes.  Infinity is what a wire no row mentions has in l: it takes no part in a
    //    sum, and where the circuit wants a finite point its term is missing from the key's side
    enum { S_A, S_B1, S_B2, S_IC, S_L, S_H, N_SEC };
    KcsSection sec[N_SEC];
    {
        std::vector<u32> wa, wb, wic(ni), wl(C.n_aux), wh(nh);
        for (u32 j = 0; j < nw; ++j) {
            if (j < ni || C.a_aux[j]) wa.push_back(j);
            if (C.b_any[j]) wb.push_back(j);
        }
        for (u32 j = 0; j < ni; ++j) wic[j] = j;
        for (u32 j = 0; j < C.n_aux; ++j) wl[j] = ni + j;
        for (u64 i = 0; i < nh; ++i) wh[i] = (u32)i;
        const struct { const char* name; Group g; const PointVec* pv; std::vector<u32>* w; } def[N_SEC] = {
            {"a", G1, &pk.a, &wa}, {"b_g1", G1, &pk.b_g1, &wb}, {"b_g2", G2, &pk.b_g2, &wb}, {"ic", G1, &pk.ic, &wic}, {"l", G1, &pk.l, &wl}, {"h", G1, &pk.h, &wh}};
        for (int s = 0; s < N_SEC; ++s) { sec[s].name = def[s].name; sec[s].g = def[s].g; sec[s].pv = def[s].pv; sec[s].wire = *def[s].w; sec[s].want = def[s].w->size(); }
    }
    ZK_REQUIRE(nw + nh < (1ull << 32), "groth16 key check: 2^32 weights or more");
    DevBuf d_res, d_gamma, d_delta;
    d_res.reserve((N_SEC + 2) * 64);
    d_gamma.reserve(B2 + 4); d_delta.reserve(B2 + 4);
    for (int s = 0; s < N_SEC; ++s) {
        KcsSection& S = sec[s];
        if (S.pv->n != S.want) { S.skip = "a wrong length"; continue; }
        const size_t pw = S.g == G1 ? P1 : P2;
        std::vector<u32> w;
        for (u64 i = 0; i < S.pv->n; ++i)
            if (!S.pv->inf[i]) { S.pos.push_back(i); w.insert(w.end(), S.pv->w.begin() + i * pw, S.pv->w.begin() + (i + 1) * pw); }
        const u64 n = S.pos.size();
        S.pts.reserve(n * pw * 4 + 4);
        if (n) h2d_sync(S.pts.p, w.data(), n * pw * 4);
        cv.pairing().points_check[S.g](S.pts.p, pw, n, 0, 1, d_res.u() + 8 * s, st);
    }
    h2d_sync(d_gamma.p, pk.vk[3].w.data(), B2); h2d_sync(d_delta.p, pk.vk[5].w.data(), B2);
    cv.pairing().points_check[G2](d_gamma.p, P2, 1, 0, 1, d_res.u() + 8 * N_SEC, st);
    cv.pairing().points_check[G2](d_delta.p, P2, 1, 0, 1, d_res.u() + 8 * (N_SEC + 1), st);
    u64 res[N_SEC + 2][8];
    d2h_sync(res, d_res.p, sizeof res);
    auto any_class = [&](int s) { return res[s][0] || res[s][2] || res[s][4] || res[s][6]; };
    const bool gamma_bad = any_class(N_SEC), delta_bad = any_class(N_SEC + 1);
    for (int s = 0; s < N_SEC; ++s) {
        KcsSection& S = sec[s];
        if (!S.skip && any_class(s)) S.skip = "an invalid point";
        if (!S.skip && ((s == S_IC && gamma_bad) || ((s == S_L || s == S_H) && delta_bad))) S.skip = "an invalid point";
        if (S.skip) { skipped += (skipped.empty() ? "" : ",") + skipped_entry("query_mismatch", S.name, S.skip); continue; }
        M.fq_canon_to_mont_dev(S.pts.p, S.pos.size() * (S.g == G1 ? 2 : 4), st);
    }
    M.fq_canon_to_mont_dev(d_gamma.p, 4, st); M.fq_canon_to_mont_dev(d_delta.p, 4, st);

    // 2. the file's sections: [alphaTauG1 | betaTauG1 | tauG1] (m, m, 2m - 1 points) and tauG2 (m); the vk fields word for word
    DevBuf base1, tau2, d_gen2, d_one;
    base1.reserve((4 * m - 1) * B1 + 4); tau2.reserve(m * B2 + 4); d_gen2.reserve(B2); d_one.reserve(8);
    const uint8_t* f = srs->file.data();
    uint8_t* b1 = (uint8_t*)base1.p;
    const void* tau1 = b1 + 2 * m * B1;
    h2d_sync(b1, f + srs->off[4], m * B1); h2d_sync(b1 + m * B1, f + srs->off[5], m * B1); h2d_sync(b1 + 2 * m * B1, f + srs->off[2], (2 * m - 1) * B1);
    h2d_sync(tau2.p, f + srs->off[3], m * B2);
    const u64 one = 1;
    h2d_sync(d_one.p, &one, 8);
    cv.group(G2).mul_generator_dev(d_one.u(), 1, d_gen2.p, st);
    {
        DevBuf d_vk;
        d_vk.reserve(2 * B1 + B2);
        uint8_t* v = (uint8_t*)d_vk.p;
        h2d_sync(v, f + srs->off[4], B1); h2d_sync(v + B1, f + srs->off[5], B1); h2d_sync(v + 2 * B1, f + srs->off[6], B2);
        M.fq_mont_to_canon_dev(d_vk.p, 2 * 2 + 4, st);
        std::vector<uint8_t> want(2 * B1 + B2);
        d2h_sync(want.data(), d_vk.p, want.size());
        const struct { const char* field; int idx; size_t at, len; } vf[3] = {{"alpha_g1", 0, 0, B1}, {"beta_g1", 1, B1, B1}, {"beta_g2", 2, 2 * B1, B2}};
        for (const auto& e : vf)
            if (pk.vk[e.idx].inf[0] || std::memcmp(pk.vk[e.idx].w.data(), want.data() + e.at, e.len) != 0) F.add("vk_mismatch", std::string("\"field\":\"") + e.field + "\"");
    }

    // 3. the weights (rho_j per wire, then rho'_i per h entry), each section's in the order of its points, and the circuit's matrices
    DevBuf d_rho;
    rho_dev(seed, nw + nh, d_rho, st, "groth16 key check");
    for (int s = 0; s < N_SEC; ++s) {
        KcsSection& S = sec[s];
        const u64 n = S.pos.size();
        if (S.skip || !n) continue;
        std::vector<u32> idx(n);
        for (u64 k = 0; k < n; ++k) idx[k] = (s == S_H ? (u32)nw : 0u) + S.wire[S.pos[k]];
        DevBuf d_idx;
        d_idx.reserve(n * 4); S.rho.reserve(n * 32 + 4);
        h2d_sync(d_idx.p, idx.data(), n * 4);
        hipLaunchKernelGGL(kc_gather_rho_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const u32*)d_rho.p, (const u32*)d_idx.p, n, (u32*)S.rho.p);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipStreamSynchronize(st));
    }
    DevBuf mat_ptr[3], mat_cols[3], mat_coef[3];
    KcMatrix mat[3];
    for (int w = 0; w < 3; ++w) {
        const Circuit::Csr& X = C.mat[w];
        const size_t nt = X.cols.size();
        DevBuf canon;
        mat_ptr[w].reserve(X.ptr.size() * 8); mat_cols[w].reserve(nt * 4 + 4); mat_coef[w].reserve(nt * 36 + 4); canon.reserve(nt * 32 + 4);
        h2d_sync(mat_ptr[w].p, X.ptr.data(), X.ptr.size() * 8);
        if (nt) { h2d_sync(mat_cols[w].p, X.cols.data(), nt * 4); h2d_sync(canon.p, X.coef.data(), nt * 32); }
        FR.kc_coef_dev((const u32*)canon.p, nt, (u32*)mat_coef[w].p, st);
        ZK_HIP(hipStreamSynchronize(st));
        mat[w] = KcMatrix{(const u64*)mat_ptr[w].p, (const u32*)mat_cols[w].p, (const u32*)mat_coef[w].p, C.n_rows};
    }
    // u^A, u^B (pub + aux) and per partition [u^B_S | u^A_S | u^C_S], the scalars of X_S over base1
    DevBuf u_sum[2], xs[2], hs;
    for (auto& b : u_sum) b.reserve(m * 32 + 4);
    for (auto& b : xs) b.reserve(3 * m * 32 + 4);
    hs.reserve((2 * m - 1) * 32 + 4);
    u32 bound_now[3] = {~0u, ~0u, ~0u};                     // the wire bound each matrix's vectors were last made for
    auto coeffs = [&](u32 bound, int mask) {
        static const u64 slot[3] = {1, 0, 2};               // A goes with betaTauG1, B with alphaTauG1, C with tauG1
        for (int w = 0; w < 3; ++w) {
            if (!((mask >> w) & 1) || bound_now[w] == bound) continue;
            u32 *xp = (u32*)xs[0].p + slot[w] * m * 8, *xa = (u32*)xs[1].p + slot[w] * m * 8;
            FR.kc_coeffs_dev(mat[w], (const u32*)d_rho.p, ni, bound, C.logm, xp, xa, w < 2 ? (u32*)u_sum[w].p : nullptr, ms_rows_tr, st);
            bound_now[w] = bound; ++n_row_sums;
        }
    };
    // sum scalars_i P_i -> the sum is infinity
    auto sum = [&](Group g, const void* pts, const DevBuf& sc, u64 n, DevBuf& out) {
        const auto ta = clk::now();
        bool inf = true;
        if (n) { inf = rlc(cv, g, pts, sc, n, out, st); ++n_sums; }
        ms_sum += since(ta, clk::now());
        return inf;
    };
    PairEq same(cv, st);
    auto paired = [&](const void* a1, const void* a2, const void* c1, const void* c2) {
        const auto ta = clk::now();
        const bool ok = same(a1, a2, c1, c2);
        ms_pair += since(ta, clk::now());
        return ok;
    };
    DevBuf lhs, rhs;
    lhs.reserve(B2 + 4); rhs.reserve(B2 + 4);               // either group's point and its flag word
    // the equation of section s for its first len entries, the circuit's side over the wires below bound
    auto holds = [&](int s, u64 len, u32 bound) {
        KcsSection& S = sec[s];
        const size_t B = S.g == G1 ? B1 : B2;
        const bool li = sum(S.g, S.pts.p, S.rho, S.finite_below(len), lhs);
        bool ri;
        if (s == S_H) {
            KcMod r;
            std::memcpy(r.w, cv.r, 32);
            hipLaunchKernelGGL(kc_h_scalars_kernel, dim3((unsigned)((2 * m - 1 + 255) / 256)), dim3(256), 0, st, (const u32*)d_rho.p + nw * 8, m, len, r, (u32*)hs.p);
            ZK_HIP(hipGetLastError());
            ri = sum(G1, tau1, hs, 2 * m - 1, rhs);
        } else if (s == S_IC || s == S_L) {
            coeffs(bound, 7);
            ri = sum(G1, base1.p, xs[s == S_IC ? 0 : 1], 3 * m, rhs);
        } else {
            coeffs(bound, s == S_A ? 1 : 2);
            ri = sum(S.g, s == S_B2 ? tau2.p : tau1, u_sum[s == S_A ? 0 : 1], m, rhs);
        }
        if (li || ri) return li && ri;
        if (s == S_IC) return paired(lhs.p, d_gamma.p, rhs.p, d_gen2.p);
        if (s == S_L || s == S_H) return paired(lhs.p, d_delta.p, rhs.p, d_gen2.p);
        std::vector<uint8_t> pts(2 * B);
        d2h_sync(pts.data(), lhs.p, B); d2h_sync(pts.data() + B, rhs.p, B);
        return std::memcmp(pts.data(), pts.data() + B, B) == 0;
    };
    for (int s = 0; s < N_SEC; ++s) {
        KcsSection& S = sec[s];
        const u64 n = S.pv->n;
        if (S.skip || !n) continue;                        // an empty section of the right length: the circuit's side is empty as well
        if (holds(s, n, (u32)nw)) continue;
        u64 lo = 0, hi = n;                                 // the prefix of lo entries holds, that of hi fails
        while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if (holds(s, mid, S.wire[mid])) lo = mid; else hi = mid; }
        F.add("query_mismatch", std::string("\"section\":\"") + S.name + "\",\"first_index\":" + std::to_string(hi - 1) +
                                    (s == S_H ? std::string() : ",\"wire\":" + std::to_string(S.wire[hi - 1])));
    }
    ZK_HIP(hipStreamSynchronize(st));
    std::string js = std::string("{\"curve\":\"") + cv.name + "\",\"power\":" + std::to_string(srs->power) + ",\"domain_log\":" + std::to_string(C.logm) +
                     ",\"n_wires\":" + std::to_string(nw) + ",\"n_public\":" + std::to_string(ni - 1) + ",\"checked\":{\"row_sums\":" + std::to_string(n_row_sums) +
                     ",\"transforms\":" + std::to_string(2 * n_row_sums) + ",\"sums\":" + std::to_string(n_sums) + ",\"pairs\":" + std::to_string(same.pairs) +
                     "},\"skipped\":[" + skipped + "]," + F.tail();
    if (const char* env = getenv("ZK_KEY_CHECK_TIMING"); env && *env && strcmp(env, "0")) {
        char buf[200];
        snprintf(buf, sizeof buf, ",\"timing_ms\":{\"parse\":%.3f,\"row_sums\":%.3f,\"transforms\":%.3f,\"sums\":%.3f,\"pairings\":%.3f}", since(t0, t1), ms_rows_tr[0],
                 ms_rows_tr[1], ms_sum, ms_pair);
        js += buf;
    }
    return js + "}";
}
