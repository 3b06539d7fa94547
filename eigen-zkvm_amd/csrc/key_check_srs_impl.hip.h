// The scalar side of groth16_key_check_srs (key_check_srs.hip.h): from the weights rho_j (one per wire, 128 bits) and one
// matrix M of the circuit the coefficient vectors u_pub = iNTT(M rho|pub), u_aux = iNTT(M rho|aux) and their sum, as canonical scalars for
// the multi-scalar sums.  Included by groth16.hip inside each scalar field's namespace, behind frntt_impl.hip.h.  No include guard on
// purpose.
//
// Arithmetic: a coefficient in internal form (c R') times the PLAIN integer rho is c rho R' / R' = c rho, a plain residue below 2q -- one
// product per term (verify_sums_impl.hip.h uses the same step); the two sums of a row are brought to internal form by one product with
// R'^2 each on the way out, which is also what brings them below 2q, the transform's input contract (frn_r1cs_eval_kernel's).

// rho_col: the first 4 of its 8 words, as the 29-bit limbs of the same integer (below 2^128 < q)
__device__ __forceinline__ fe kcs_rho_limbs(const u32* __restrict__ rho, u64 col) {
    const uint4 v = *(const uint4*)(rho + col * 8);          // 32 B per weight: the address is 16 B aligned
    const u32 w[NL] = {v.x, v.y, v.z, v.w, 0u, 0u, 0u, 0u};
    fe x;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int bit = LB * k, wi = bit >> 5, s = bit & 31;
        u32 u = wi < NL ? w[wi] >> s : 0;
        if (s > 32 - LB && wi + 1 < NL) u |= w[wi + 1] << (32 - s);
        x.l[k] = u & LMASK;
    }
    return x;
}
// One lane per row of a CSR matrix (coeffs in internal form, element-major, as frn_canon_to_fe_kernel leaves them): in one pass over the
// row's terms out_pub[i] = sum coef rho_col over col < min(ni, bound) and out_aux[i] = the same over ni <= col < bound.  bound = n_wires
// for the whole check; the bisection lowers it instead of rewriting rho, so the matrix -- 36 B a term, the traffic of this kernel -- is
// read once for both partitions and not at all beyond the bound.  Rows n_rows .. n are the domain's zero padding.  Limb-major, below 2q.
__global__ __launch_bounds__(256) void kc_rows_rho_kernel(const u64* __restrict__ row_ptr, const u32* __restrict__ cols, const u32* __restrict__ coeffs,
                                                          const u32* __restrict__ rho, u64 n_rows, u32 ni, u32 bound, u32* __restrict__ out_pub,
                                                          u32* __restrict__ out_aux, u64 n) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    fe acc[2] = {fe_zero(), fe_zero()};
    int pending[2] = {0, 0};
    if (i < n_rows) {
        for (u64 k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
            const u32 col = cols[k];
            if (col >= bound) continue;
            fe cf;
#pragma unroll
            for (int l = 0; l < NR; ++l) cf.l[l] = coeffs[k * NR + l];
            const fe t = fe_mul(cf, kcs_rho_limbs(rho, col));
            if (col < ni) {
                acc[0] = fe_add(acc[0], t);
                if (++pending[0] == 4) { acc[0] = fe_renorm(acc[0]); pending[0] = 0; }   // < 2q + 4 * 2q between renormalisations
            } else {
                acc[1] = fe_add(acc[1], t);
                if (++pending[1] == 4) { acc[1] = fe_renorm(acc[1]); pending[1] = 0; }
            }
        }
    }
    fe rr2;
#pragma unroll
    for (int k = 0; k < NR; ++k) rr2.l[k] = RRP29(k);
    soa_store(out_pub, n, i, fe_mul(acc[0], rr2));
    soa_store(out_aux, n, i, fe_mul(acc[1], rr2));
}
// the two coefficient vectors (limb-major, as the transform leaves them) -> canonical scalars: pub, aux and, where asked for, pub + aux
__global__ __launch_bounds__(256) void kc_coeffs_out_kernel(const u32* __restrict__ u_pub, const u32* __restrict__ u_aux, u64 n, u32* __restrict__ out_pub,
                                                            u32* __restrict__ out_aux, u32* __restrict__ out_sum) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const fe p = soa_load(u_pub, n, i), a = soa_load(u_aux, n, i);   // below 2q: the transform's last product
    fe_store_canon(p, out_pub + i * NL);
    fe_store_canon(a, out_aux + i * NL);
    if (out_sum) fe_store_canon(fe_add(p, a), out_sum + i * NL);
}

// canonical coefficients (8 words a term) -> the internal form kc_rows_rho_kernel reads (9 words a term)
void kc_coef_dev(const u32* d_canon, u64 n, u32* d_fe, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(frn_canon_to_fe_kernel, dim3(frn_blocks(n)), dim3(256), 0, st, d_canon, d_fe, n);
    ZK_HIP(hipGetLastError());
}
// d_pub, d_aux, d_sum (may be null): 2^logm canonical scalars each.  ms (may be null): += the milliseconds of the row sums and of the
// transforms with what follows them
void kc_coeffs_dev(const KcMatrix& M, const u32* d_rho, u32 ni, u32 bound, int logm, u32* d_pub, u32* d_aux, u32* d_sum, double* ms, hipStream_t st) {
    using clk = std::chrono::steady_clock;
    const FrDomain& D = frn_domain(logm, st);
    const u64 m = 1ull << logm;
    ZK_REQUIRE(M.n_rows <= m, "groth16 key check: more rows than the domain holds");
    DevBuf buf[4];
    for (auto& b : buf) b.reserve(m * NR * 4);
    u32* v[2] = {(u32*)buf[0].p, (u32*)buf[1].p};
    u32* s[2] = {(u32*)buf[2].p, (u32*)buf[3].p};
    ZK_HIP(hipStreamSynchronize(st));
    const auto t0 = clk::now();
    hipLaunchKernelGGL(kc_rows_rho_kernel, dim3(frn_blocks(m)), dim3(256), 0, st, M.ptr, M.cols, M.coef, d_rho, M.n_rows, ni, bound, v[0], v[1], m);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));
    const auto t1 = clk::now();
    if (frn_transform_batch(D, v, s, 2, true, nullptr, (const u32*)D.minv(), 1, st)) std::swap(v, s);
    hipLaunchKernelGGL(kc_coeffs_out_kernel, dim3(frn_blocks(m)), dim3(256), 0, st, (const u32*)v[0], (const u32*)v[1], m, d_pub, d_aux, d_sum);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));                       // the scratch goes back to the pool
    if (ms) {
        ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        ms[1] += std::chrono::duration<double, std::milli>(clk::now() - t1).count();
    }
}
