// The scalar-field side of the witness check (r1cs_check.hip), generic over the field; included inside the scalar field's namespace
// after fr29_consts.hip.h + fe29_impl.hip.h + fr_rows_impl.hip.h.  Values travel as the prover's do: canonical 8 x u32 at the boundary,
// 9 x 29-bit limbs (Montgomery, R' = 2^261) inside; the row sums are the prover's own (frn_row_sum).  No include guard on purpose.

struct FrField {
    typedef u32 word_t;
    static constexpr int CW = NL, IW = NR;               // words of a canonical / an internal element
    struct val { fe v; };

    static __device__ __forceinline__ void row_abc(const Csr3& m, const u32* __restrict__ wit, u64 i, val& a, val& b, val& c) {
        a.v = frn_row_sum(m.ptr[0], m.cols[0], (const u32*)m.coef[0], wit, i);
        b.v = frn_row_sum(m.ptr[1], m.cols[1], (const u32*)m.coef[1], wit, i);
        c.v = frn_row_sum(m.ptr[2], m.cols[2], (const u32*)m.coef[2], wit, i);
    }
    // a b != c.  Both sides keep the Montgomery factor, so their canonical representatives are compared as they are: a product of two
    // values < 2q is < 2q, and fe_canon of a normalised value < 2q is the one representative below q
    static __device__ __forceinline__ bool differs(const val& a, const val& b, const val& c) {
        const fe l = fe_canon(fe_mul(a.v, b.v)), r = fe_canon(c.v);
        u32 d = 0;
#pragma unroll
        for (int k = 0; k < NR; ++k) d |= l.l[k] ^ r.l[k];
        return d != 0;
    }
    static __device__ __forceinline__ void store(const val& x, u32* __restrict__ out) { fe_store_canon(x.v, out); }
    static __device__ __forceinline__ bool one_wire_bad(const u32* __restrict__ canon) {
        u32 d = canon[0] ^ 1u;
#pragma unroll
        for (int k = 1; k < NL; ++k) d |= canon[k];
        return d != 0;
    }
    // n canonical elements -> internal form (the witness once per run, the coefficients once per handle)
    static void to_internal(const u32* d_canon, u32* d_out, u64 n, hipStream_t st) {
        if (n == 0) return;
        hipLaunchKernelGGL(frn_canon_to_fe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_canon, d_out, n);
        ZK_HIP(hipGetLastError());
    }
    static std::string dec(const u32* v) { return g16::words_to_dec(v, NL); }
};
