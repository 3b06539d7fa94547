// In-register radix-2 DIF transforms shared by the NTT passes (ntt.hip) and the FRI fold (stark.hip).
#pragma once
#include "gl.hip.h"
#include <type_traits>

namespace zk {

__host__ __device__ constexpr int bitrev_c(int x, int bits) {
    int r = 0;
    for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}

// compile-time loop
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); static_for<B + 1, E>(f); }
}

// exponent e of the twiddle w_{2*half}^j = 2^e (forward) or 2^-e (inverse), 2*half <= 64:
// w_64 = MG.0[6] = 2^39, w_{64/m} = 2^(39 m); e is taken mod 192 (the order of 2)
__host__ __device__ constexpr int tw_pow2_exp(int half, int j, bool inv) {
    int e = (39 * (32 / half) * j) % 192;
    return inv ? (192 - e) % 192 : e;
}

// 2^LOG-point DIF NTT in registers, natural order in; X[k] ends up in x[bitrev(k)].  LOG <= 6: every
// twiddle is +-2^e, applied as a shift (2^96 = -1 folds into the order of the subtraction).
// PAIR: a layer walks its butterflies two at a time, their sums, differences and shifts as the four- and two-chain forms of gl.hip.h
// (gl::bfly2_m, gl::mul_pow2_2): two blocks of the same j, or j and j + 1 in the first layer, which has one block.  The same bits.
// The NTT passes take it; the FRI fold keeps the single form.
template <int LOG, bool INV, bool PAIR = false>
__device__ __forceinline__ void ntt_reg(u64 (&x)[1 << LOG]) {
    static_assert(LOG <= 6, "power-of-two twiddles exist up to order 64");
    constexpr int n = 1 << LOG;
    if constexpr (PAIR && LOG >= 2) {
        // one pair: (a0, b0) with exponent e0 and (a1, b1) with e1; 2^96 = -1 swaps the operands of that butterfly (the sum does not care)
        auto pair = [&](auto E0, auto E1, u64& a0, u64& b0, u64& a1, u64& b1) {
            constexpr int e0 = decltype(E0)::value, e1 = decltype(E1)::value;
            constexpr bool n0 = e0 >= 96, n1 = e1 >= 96;
            u64 s0, d0, s1, d1;
            gl::bfly2_m(n0 ? b0 : a0, n0 ? a0 : b0, n1 ? b1 : a1, n1 ? a1 : b1, s0, d0, s1, d1);
            a0 = s0; a1 = s1;
            gl::mul_pow2_2<n0 ? e0 - 96 : e0, n1 ? e1 - 96 : e1>(d0, d1, b0, b1);
        };
        static_for<0, LOG>([&](auto LI) {
            constexpr int half = 1 << (LOG - 1 - decltype(LI)::value);
            if constexpr (2 * half < n) {
                static_for<0, half>([&](auto JI) {
                    constexpr int j = decltype(JI)::value;
                    using E = std::integral_constant<int, tw_pow2_exp(half, j, INV)>;
#pragma unroll
                    for (int blk = 0; blk < n; blk += 4 * half)
                        pair(E{}, E{}, x[blk + j], x[blk + j + half], x[blk + 2 * half + j], x[blk + 2 * half + j + half]);
                });
            } else {
                static_for<0, half / 2>([&](auto JI) {
                    constexpr int j = 2 * decltype(JI)::value;
                    pair(std::integral_constant<int, tw_pow2_exp(half, j, INV)>{}, std::integral_constant<int, tw_pow2_exp(half, j + 1, INV)>{},
                         x[j], x[j + half], x[j + 1], x[j + 1 + half]);
                });
            }
        });
        return;
    }
    static_for<0, LOG>([&](auto LI) {
        constexpr int half = 1 << (LOG - 1 - decltype(LI)::value);
        static_for<0, half>([&](auto JI) {
            constexpr int j = decltype(JI)::value;
            constexpr int e = tw_pow2_exp(half, j, INV);
#pragma unroll
            for (int blk = 0; blk < n; blk += 2 * half) {
                const u64 a = x[blk + j], b = x[blk + j + half];
                x[blk + j] = gl::add_m(a, b);
                if constexpr (e >= 96) x[blk + j + half] = gl::mul_pow2<e - 96>(gl::sub_m(b, a));
                else                   x[blk + j + half] = gl::mul_pow2<e>(gl::sub_m(a, b));
            }
        });
    });
}

}  // namespace zk
