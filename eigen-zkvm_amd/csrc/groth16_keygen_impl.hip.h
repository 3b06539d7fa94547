// Groth16 key generation on the device, generic over the curve; included after groth16_impl.hip.h inside the scalar
// field's namespace; [k]G for full-width scalars (fixedbase_impl.hip.h) and the base-field conversions come from the curve table.
// Restates bellman_ce groth16/generator.rs generate_parameters with an explicit trapdoor (the reference draws it from
// its rng: groth16/src/groth16.rs:77-86 circuit_specific_setup -> generate_random_parameters) over the circuit
// g16::Circuit describes -- the same rows, input rows and domain the prover uses:
//   tau^i, i < m, and t(tau) = tau^m - 1                       one power-table launch
//   L_i(tau)                                                   one inverse transform of the powers, as bellman does
//   a_j, b_j, c_j(tau) = sum over the wire's column            column-major matrices built on the host, one wave per wire,
//                                                              summed in a fixed order: no atomics
//   h_i = tau^i t(tau) / delta, l_j | ic_j = (beta a_j + alpha b_j + c_j) / (delta | gamma)
//   the points of all of them                                  mul_generator_fr_dev: one launch per group and scalar array
// and writes Parameters::write's layout; points at infinity are dropped from a, b_g1, b_g2 (generator.rs), in wire order.
// No include guard on purpose.

struct KgConsts {
    fe tau2[32];                       // tau^(2^b)
    fe alpha, beta, dinv, ginv, zt_dinv;   // 1/delta, 1/gamma, t(tau)/delta
    u32 zt_zero;                       // tau^m = 1
};
__device__ __forceinline__ fe kg_from_canon(const u32* w) {
    fe x;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int bit = LB * k, wi = bit >> 5, s = bit & 31;
        u32 v = wi < NL ? w[wi] >> s : 0;
        if (s > 32 - LB && wi + 1 < NL) v |= w[wi + 1] << (32 - s);
        x.l[k] = v & LMASK;
    }
    fe c;
#pragma unroll
    for (int k = 0; k < NR; ++k) c.l[k] = RRP29(k);
    return fe_mul(x, c);
}
__global__ void kg_setup_kernel(const u32* __restrict__ td /* tau, alpha, beta, gamma, delta: 8 words each, canonical */, int logm, KgConsts* __restrict__ kc) {
    if (threadIdx.x || blockIdx.x) return;
    fe t = kg_from_canon(td), tm = t;
    for (int b = 0; b < 32; ++b) {
        if (b == logm) tm = t;
        kc->tau2[b] = t;
        t = fe_sqr(t);
    }
    if (logm >= 32) tm = t;
    const fe zt = fe_renorm(fe_sub<2>(tm, fe_one()));
    kc->zt_zero = fe_is_zero_m(zt) ? 1u : 0u;
    kc->alpha = kg_from_canon(td + 8); kc->beta = kg_from_canon(td + 16);
    kc->ginv = fe_inv(kg_from_canon(td + 24)); kc->dinv = fe_inv(kg_from_canon(td + 32));
    kc->zt_dinv = fe_mul(zt, kc->dinv);
}
// h_i = tau^i t(tau) / delta, canonical
__global__ __launch_bounds__(256) void kg_h_kernel(const u32* __restrict__ pow, u64 m, const KgConsts* __restrict__ kc, u32* __restrict__ out, u64 n_out) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n_out) return;
    fe_store_canon(fe_mul(soa_load(pow, m, i), kc->zt_dinv), out + i * NL);
}
// one matrix by columns: the terms of wire j are [ptr[j], ptr[j + 1]), each a row and a coefficient (internal form, element-major)
struct KgCsc { const u64* ptr; const u32* rows; const u32* coef; };
__device__ __forceinline__ fe kg_column_sum(const KgCsc& M, u32 j, u32 lane, const u32* __restrict__ L, u64 m) {
    fe acc = fe_zero();
    int pending = 0;
    for (u64 k = M.ptr[j] + lane; k < M.ptr[j + 1]; k += 64) {
        fe cf;
#pragma unroll
        for (int l = 0; l < NR; ++l) cf.l[l] = M.coef[k * NR + l];
        acc = fe_add(acc, fe_mul(cf, soa_load(L, m, M.rows[k])));
        if (++pending == 4) { acc = fe_renorm(acc); pending = 0; }     // < 2q + 4 * 2q between renormalisations
    }
    if (pending) acc = fe_renorm(acc);
    for (int d = 32; d >= 1; d >>= 1) {                                 // the wave's 64 partial sums, always in this order
        fe o;
#pragma unroll
        for (int l = 0; l < NR; ++l) o.l[l] = __shfl_down(acc.l[l], d, 64);
        acc = fe_renorm(fe_add(acc, o));
    }
    return acc;                                                         // lane 0 holds the column's sum
}
// One wave per wire (a wire such as ONE can sit in every row; most sit in two or three): a_j, b_j and
// x_j = (beta a_j + alpha b_j + c_j) / (gamma for inputs | delta), canonical
__global__ __launch_bounds__(256) void kg_wire_sums_kernel(const KgCsc A, const KgCsc B, const KgCsc Cm, const u32* __restrict__ L, u64 m, u32 n_wires, u32 ni,
                                                           const KgConsts* __restrict__ kc, u32* __restrict__ sc_a, u32* __restrict__ sc_b, u32* __restrict__ sc_x) {
    const u32 j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n_wires) return;
    const fe a = kg_column_sum(A, j, lane, L, m), b = kg_column_sum(B, j, lane, L, m), c = kg_column_sum(Cm, j, lane, L, m);
    if (lane) return;
    fe_store_canon(a, sc_a + (u64)j * NL); fe_store_canon(b, sc_b + (u64)j * NL);
    const fe e = fe_add(fe_add(fe_mul(kc->beta, a), fe_mul(kc->alpha, b)), c);   // < 6q
    fe_store_canon(fe_mul(e, j < ni ? kc->ginv : kc->dinv), sc_x + (u64)j * NL);
}

// td: the trapdoor, 5 x 8 canonical words, non-zero and below r.  out: the key's bytes.  ms: transform, column sums, G1 points,
// G2 points, serialisation.  Every device buffer that held the trapdoor or a scalar derived from it is overwritten before return.
void keygen_run(const Curve& cv, const g16::Circuit& C, const u32* td, std::vector<uint8_t>& out, double* ms) {
    hipStream_t st = cur_stream();
    const u64 m = C.m, nh = m - 1, nw = C.n_wires;
    const FrDomain& D = frn_domain(C.logm, st);
    const MsmOps& M = cv.msm();
    const size_t P1 = cv.point_words(G1), P2 = cv.point_words(G2);
    const u64 n1 = 3 + 3 * nw + nh, n2 = 3 + nw;
    // G1 scalars: [alpha beta delta | x (ic, then l) | h | a | b];  G2: [beta gamma delta], then the b of the G1 array
    const u64 o_x = 3, o_h = o_x + nw, o_a = o_h + nh, o_b = o_a + nw;
    DevBuf d_td, d_kc, pw, tmp, sc1, sc2, csc_ptr[3], csc_rows[3], csc_coef[3], pts1, pts2;
    d_td.reserve(40 * 4); d_kc.reserve(sizeof(KgConsts));
    pw.reserve(m * NR * 4); tmp.reserve(m * NR * 4); sc1.reserve(n1 * 32); sc2.reserve(3 * 32);
    struct Wipe {                                                       // also on the way out of an exception
        hipStream_t st; std::vector<DevBuf*> v;
        ~Wipe() { for (DevBuf* b : v) if (b->p) (void)hipMemsetAsync(b->p, 0, b->bytes, st); (void)hipStreamSynchronize(st); }
    } wipe{st, {&d_td, &d_kc, &pw, &tmp, &sc1, &sc2}};
    auto now = [&] { ZK_HIP(hipStreamSynchronize(st)); return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };

    auto t0 = now();
    h2d_sync(d_td.p, td, 40 * 4);
    KgConsts* kc = (KgConsts*)d_kc.p;
    hipLaunchKernelGGL(kg_setup_kernel, dim3(1), dim3(64), 0, st, (const u32*)d_td.p, C.logm, kc);
    ZK_HIP(hipGetLastError());
    u32 zt_zero = 0;
    d2h_sync(&zt_zero, &kc->zt_zero, 4);
    ZK_REQUIRE(!zt_zero, "groth16 keygen: tau^m = 1 for the domain of 2^" + std::to_string(C.logm) + " rows: t(tau) = 0, the key would be useless");
    u32* S1 = (u32*)sc1.p;
    u32 vk1[24] = {td[8], td[9], td[10], td[11], td[12], td[13], td[14], td[15], td[16], td[17], td[18], td[19], td[20], td[21], td[22], td[23],
                         td[32], td[33], td[34], td[35], td[36], td[37], td[38], td[39]};
    h2d_sync(S1, vk1, 96);                                              // alpha, beta, delta
    g16::wipe(vk1, sizeof vk1);
    h2d_sync(sc2.p, td + 16, 96);                                       // beta, gamma, delta
    hipLaunchKernelGGL(frn_pow_table_kernel, dim3(frn_blocks(m)), dim3(256), 0, st, (const fe*)kc->tau2, (const fe*)nullptr, (u32*)pw.p, m);
    if (nh) hipLaunchKernelGGL(kg_h_kernel, dim3(frn_blocks(nh)), dim3(256), 0, st, (const u32*)pw.p, m, (const KgConsts*)kc, S1 + o_h * 8, nh);
    ZK_HIP(hipGetLastError());
    const u32* L = frn_transform(D, (u32*)pw.p, (u32*)tmp.p, true, nullptr, (const u32*)D.minv(), 1, st);   // powers -> L_i(tau)
    auto t1 = now();
    ms[0] = since(t0, t1);

    KgCsc csc[3];
    DevBuf raw;                                                         // canonical coefficients on their way to the internal form: one block, reused
    raw.reserve(std::max({C.mat[0].cols.size(), C.mat[1].cols.size(), C.mat[2].cols.size()}) * 32 + 4);
    for (int w = 0; w < 3; ++w) {                                       // CSR -> CSC, rows of a column in increasing order; one host copy at a time
        std::vector<u64> ptr;
        std::vector<u32> rows, coef;
        g16::csc_of(C.mat[w], nw, ptr, rows, coef);
        const size_t nt = rows.size();
        csc_ptr[w].reserve(ptr.size() * 8); csc_rows[w].reserve(nt * 4 + 4); csc_coef[w].reserve(nt * NR * 4 + 4);
        h2d_sync(csc_ptr[w].p, ptr.data(), ptr.size() * 8);
        if (nt) {
            h2d_sync(csc_rows[w].p, rows.data(), nt * 4);
            h2d_sync(raw.p, coef.data(), nt * 32);                      // ordered on st behind the previous matrix's conversion
            hipLaunchKernelGGL(frn_canon_to_fe_kernel, dim3(frn_blocks(nt)), dim3(256), 0, st, (const u32*)raw.p, (u32*)csc_coef[w].p, (u64)nt);
            ZK_HIP(hipGetLastError());
        }
        csc[w] = KgCsc{(const u64*)csc_ptr[w].p, (const u32*)csc_rows[w].p, (const u32*)csc_coef[w].p};
    }
    hipLaunchKernelGGL(kg_wire_sums_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, st, csc[0], csc[1], csc[2], L, m, (u32)nw, C.ni, (const KgConsts*)kc,
                       S1 + o_a * 8, S1 + o_b * 8, S1 + o_x * 8);
    ZK_HIP(hipGetLastError());
    auto t2 = now();
    ms[1] = since(t1, t2);

    pts1.reserve(n1 * P1 * 4); pts2.reserve(n2 * P2 * 4);
    M.g[G1].mul_generator_fr_dev((const u64*)sc1.p, n1, pts1.p, st);
    auto t3 = now();
    ms[2] = since(t2, t3);
    M.g[G2].mul_generator_fr_dev((const u64*)sc2.p, 3, pts2.p, st);
    M.g[G2].mul_generator_fr_dev((const u64*)(S1 + o_b * 8), nw, (u32*)pts2.p + 3 * P2, st);
    auto t4 = now();
    ms[3] = since(t3, t4);

    g16::write_params(cv, C, pts1, pts2, out, st);
    ms[4] = since(t4, std::chrono::steady_clock::now());
}
