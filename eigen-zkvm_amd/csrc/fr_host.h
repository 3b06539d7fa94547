// The scalar field of a curve on the host: 4 x 64-bit Montgomery arithmetic for the handful of values that are cheaper to make here than
// to launch a kernel for -- the twiddles of a group transform (ecntt.hip), the inverse of a contribution's delta and the responses of
// a ceremony's proofs of knowledge (groth16.hip).
// Not constant time, so secrets pass through it only where the caller wipes them (FrHost::wipe).
#pragma once
#include "curve.h"
#include <cstring>

namespace zk {

struct FrHost {
    typedef unsigned __int128 u128;
    u64 p[4], ninv, r2[4], one[4];
    explicit FrHost(const Curve& cv) {
        for (int i = 0; i < 4; ++i) p[i] = (u64)cv.r[2 * i] | ((u64)cv.r[2 * i + 1] << 32);
        u64 x = 1;
        for (int i = 0; i < 6; ++i) x *= 2 - p[0] * x;              // 1 / p[0] mod 2^64 (Newton)
        ninv = 0 - x;
        u64 v[4] = {1, 0, 0, 0};
        for (int i = 0; i < 512; ++i) {                             // 2^512 mod r by doubling (r < 2^255: a double fits)
            if (i == 256) std::memcpy(one, v, 32);
            dbl(v);
        }
        std::memcpy(r2, v, 32);
    }
    bool geq_p(const u64* a) const {
        for (int i = 3; i >= 0; --i) { if (a[i] > p[i]) return true; if (a[i] < p[i]) return false; }
        return true;
    }
    void sub_p(u64* a) const {
        u64 br = 0;
        for (int i = 0; i < 4; ++i) { const u128 d = (u128)a[i] - p[i] - br; a[i] = (u64)d; br = (u64)(d >> 64) & 1; }
    }
    void dbl(u64* a) const {
        for (int i = 3; i > 0; --i) a[i] = (a[i] << 1) | (a[i - 1] >> 63);
        a[0] <<= 1;
        if (geq_p(a)) sub_p(a);
    }
    // out = a + b mod r for a, b < r (either form); out may alias an operand
    void add(const u64* a, const u64* b, u64* out) const {
        u64 t[4]; u128 c = 0;
        for (int i = 0; i < 4; ++i) { c += (u128)a[i] + b[i]; t[i] = (u64)c; c >>= 64; }
        if (geq_p(t)) sub_p(t);                                     // r < 2^255: the sum fits
        std::memcpy(out, t, 32);
    }
    // out = a b / 2^256 mod r (CIOS); out may alias an operand
    void mul(const u64* a, const u64* b, u64* out) const {
        u64 t[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) {
            u128 c = 0;
            for (int j = 0; j < 4; ++j) { c += (u128)a[j] * b[i] + t[j]; t[j] = (u64)c; c >>= 64; }
            c += t[4]; t[4] = (u64)c; t[5] = (u64)(c >> 64);
            const u64 m = t[0] * ninv;
            c = ((u128)m * p[0] + t[0]) >> 64;
            for (int j = 1; j < 4; ++j) { c += (u128)m * p[j] + t[j]; t[j - 1] = (u64)c; c >>= 64; }
            c += t[4]; t[3] = (u64)c; t[4] = t[5] + (u64)(c >> 64);
        }
        if (t[4] || geq_p(t)) sub_p(t);
        std::memcpy(out, t, 32);
    }
    void to_mont(const u64* canon, u64* out) const { mul(canon, r2, out); }
    void from_mont(const u64* m, u64* out) const { const u64 o[4] = {1, 0, 0, 0}; mul(m, o, out); }
    // out = a^e, a and out in Montgomery form, e a plain 256-bit integer
    void pow(const u64* a, const u64* e, u64* out) const {
        u64 acc[4], base[4];
        std::memcpy(acc, one, 32); std::memcpy(base, a, 32);
        for (int b = 255; b >= 0; --b) {
            mul(acc, acc, acc);
            if ((e[b >> 6] >> (b & 63)) & 1) mul(acc, base, acc);
        }
        std::memcpy(out, acc, 32);
        wipe(acc, 32); wipe(base, 32);
    }
    void inv(const u64* a, u64* out) const {                        // a^(r - 2)
        u64 e[4] = {p[0] - 2, p[1], p[2], p[3]};                    // r is odd and > 2: no borrow
        pow(a, e, out);
    }
    // the 2^log_n-th root of unity of zk_fr_<curve>_ntt: 7^((r - 1) / 2^log_n), Montgomery form
    void omega(int log_n, u64* out) const {
        u64 e[4] = {p[0] - 1, p[1], p[2], p[3]}, seven[4] = {7, 0, 0, 0}, g[4];
        for (int s = 0; s < log_n; ++s) { for (int i = 0; i < 3; ++i) e[i] = (e[i] >> 1) | (e[i + 1] << 63); e[3] >>= 1; }
        to_mont(seven, g);
        pow(g, e, out);
    }
    int two_adicity() const { return __builtin_ctzll(p[0] - 1); }   // 28 and 32: the low word of r - 1 is not zero
    static void wipe(void* q, size_t n) { volatile uint8_t* v = (volatile uint8_t*)q; for (size_t i = 0; i < n; ++i) v[i] = 0; }
};

}  // namespace zk
