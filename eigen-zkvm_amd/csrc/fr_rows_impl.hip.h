// What the Groth16 prover (frntt_impl.hip.h) and the witness check (r1cs_check.hip) share of the scalar-field work on an R1CS: the
// witness conversion, the sum of one row of a CSR matrix, the way back to canonical words.  Included inside a namespace that has already
// pulled in fr29_consts.hip.h + fe29_impl.hip.h.  No include guard on purpose.

__device__ __forceinline__ fe fe_renorm(const fe& a) { return fe_mul(a, fe_one()); }   // any value < 68q -> < 2q

// canonical integers (8 x u32 each, < r) -> internal form, element-major (9 x u32 each): the witness
__global__ __launch_bounds__(256) void frn_canon_to_fe_kernel(const u32* __restrict__ in, u32* __restrict__ out, u64 n) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    u32 w[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) w[k] = in[i * NL + k];
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
    x = fe_mul(x, c);
#pragma unroll
    for (int k = 0; k < NR; ++k) out[i * NR + k] = x.l[k];
}

// ProvingAssignment::enforce's eval() for row i of a CSR matrix: sum coeff * w[col], < 2q.  coeffs and wit in internal form,
// element-major (9 x u32 each)
__device__ __forceinline__ fe frn_row_sum(const u64* __restrict__ row_ptr, const u32* __restrict__ cols, const u32* __restrict__ coeffs,
                                          const u32* __restrict__ wit, u64 i) {
    fe acc = fe_zero();
    int pending = 0;
    for (u64 k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
        fe cf, x;
        const u64 col = cols[k];
#pragma unroll
        for (int l = 0; l < NR; ++l) { cf.l[l] = coeffs[k * NR + l]; x.l[l] = wit[col * NR + l]; }
        acc = fe_add(acc, fe_mul(cf, x));
        if (++pending == 4) { acc = fe_renorm(acc); pending = 0; }   // < 2q + 4 * 2q between renormalisations
    }
    if (pending) acc = fe_renorm(acc);
    return acc;
}
__device__ __forceinline__ void fe_store_canon(const fe& a /* Montgomery, < 68q */, u32* __restrict__ out) {
    fe one = fe_zero(); one.l[0] = 1;
    const fe x = fe_canon(fe_mul(a, one));
#pragma unroll
    for (int jj = 0; jj < NL; ++jj) {
        const int bit = 32 * jj, k = bit / LB, s = bit % LB;
        u32 v = x.l[k] >> s;
        if (k + 1 < NR) v |= x.l[k + 1] << (LB - s);
        if (k + 2 < NR && 2 * LB - s < 32) v |= x.l[k + 2] << (2 * LB - s);
        out[jj] = v;
    }
}
