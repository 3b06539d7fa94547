// The scalars of a powers-of-tau contribution, made where they are used: out_i = s t^(i0 + i) for the points i0, i0 + 1, ... of a section.
// Included inside a scalar field's namespace after frntt_impl.hip.h (groth16.hip); no include guard on purpose.
// Each lane builds its own power from the square chain t^(2^j), j < 29, that the host made (29 products in Fr there, at most 29 here per
// point, against the ~250 point operations the scalar then costs): no 2^29 host products and no host copy of the scalars.
// tab: 30 x NL words, Montgomery R = 2^256 (fr_host.h): s, then t^(2^j).  out: NL canonical words per scalar, what mul_scalars takes.
constexpr int CER_CHAIN = 29;                                       // exponents below 2^29: a file of power 28 has 2^29 - 1 tauG1 points
__global__ __launch_bounds__(256) void ecn_powers_kernel(const u32* __restrict__ tab, u64 i0, u64 n, u32* __restrict__ out) {
    __shared__ fe tb[CER_CHAIN + 1];
    if (threadIdx.x <= CER_CHAIN) {
        u32 w[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) w[k] = tab[threadIdx.x * NL + k];
        tb[threadIdx.x] = fe_from_std(w);
    }
    __syncthreads();
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const u64 e = i0 + i;
    fe acc = tb[0];
    for (int b = 0; b < CER_CHAIN; ++b)
        if ((e >> b) & 1) acc = fe_mul(acc, tb[1 + b]);
    fe_store_canon(acc, out + i * NL);
}
void powers_dev(const u32* d_tab, u64 i0, u64 n, u32* d_out, hipStream_t st) {
    if (n == 0) return;
    ZK_REQUIRE(i0 + n <= (1ull << CER_CHAIN), "powers: exponent out of range");
    hipLaunchKernelGGL(ecn_powers_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_tab, i0, n, d_out);
    ZK_HIP(hipGetLastError());
}
