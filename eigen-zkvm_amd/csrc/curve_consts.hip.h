// The base fields Fq of BN254 and BLS12-381 for fe29_impl.hip.h (29-bit limbs): what msm.hip and pairing.hip both build on.
#pragma once
#include "zk_internal.h"
namespace zk {
namespace bn254 {
constexpr int NL = 8;  // 32-bit limbs of Fq
// q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47 (alt_bn128 base field); external R = 2^256
constexpr int NR = 9;  // 29-bit limbs of the internal representation, R' = 2^261
constexpr u32 QINV29 = 0x04866389u;  // -q^-1 mod 2^29
__host__ __device__ constexpr u32 Q29(int i) {
    constexpr u32 v[9] = {0x187cfd47u, 0x010460b6u, 0x1c72a34fu, 0x02d522d0u, 0x1585d978u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu};
    return v[i];
}
__host__ __device__ constexpr u32 ONE29(int i) {
    constexpr u32 v[9] = {0x157ccc21u, 0x141c2758u, 0x185230d3u, 0x014c0419u, 0x0aa36fb9u, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u};
    return v[i];
}
__host__ __device__ constexpr u32 CIN29(int i) {
    constexpr u32 v[9] = {0x13349ca1u, 0x1a5d84a8u, 0x0a3e5cacu, 0x100249e0u, 0x12b951e8u, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u};
    return v[i];
}
__host__ __device__ constexpr u32 COUT29(int i) {
    constexpr u32 v[9] = {0x058f0d9du, 0x1aea1c6eu, 0x11c2cf74u, 0x11d651ebu, 0x1462c0a7u, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u};
    return v[i];
}
__host__ __device__ constexpr u32 Q2_29(int i) {
    constexpr u32 v[9] = {0x10f9fa8eu, 0x0208c16du, 0x18e5469eu, 0x05aa45a1u, 0x0b0bb2f0u, 0x05b68181u, 0x014dc282u, 0x1cb84c68u, 0x0060c89cu};
    return v[i];
}
__host__ __device__ constexpr u32 Q4_29(int i) {
    constexpr u32 v[9] = {0x01f3f51cu, 0x041182dbu, 0x11ca8d3cu, 0x0b548b43u, 0x161765e0u, 0x0b6d0302u, 0x029b8504u, 0x197098d0u, 0x00c19139u};
    return v[i];
}
__host__ __device__ constexpr u32 Q8_29(int i) {
    constexpr u32 v[9] = {0x03e7ea38u, 0x082305b6u, 0x03951a78u, 0x16a91687u, 0x0c2ecbc0u, 0x16da0605u, 0x05370a08u, 0x12e131a0u, 0x01832273u};
    return v[i];
}
__host__ __device__ constexpr u32 RRP29(int i) {  // R'^2 mod q: canonical integers -> internal form (key files store canonical coordinates)
    constexpr u32 v[9] = {0x059bac10u, 0x0d1503a3u, 0x018016b8u, 0x10ab0ca8u, 0x02632639u, 0x02c0169fu, 0x169bfd53u, 0x11869d4cu, 0x002a11a6u};
    return v[i];
}
}  // namespace bn254
namespace bls12_381 {
constexpr int NL = 12;
// q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab; external R = 2^384
constexpr int NR = 14;  // 29-bit limbs of the internal representation, R' = 2^406
constexpr u32 QINV29 = 0x1ffcfffdu;  // -q^-1 mod 2^29
__host__ __device__ constexpr u32 Q29(int i) {
    constexpr u32 v[14] = {0x1fffaaabu, 0x0ff7ffffu, 0x14ffffeeu, 0x17fffd62u, 0x0f6241eau, 0x09507b58u, 0x0afd9cc3u, 0x109e70a2u, 0x1764774bu, 0x121a5d66u, 0x12c6e9edu, 0x12ffcd34u, 0x00111ea3u, 0x0000000du};
    return v[i];
}
__host__ __device__ constexpr u32 ONE29(int i) {
    constexpr u32 v[14] = {0x03a9fb84u, 0x0ba00690u, 0x071288f1u, 0x0f59bcc5u, 0x126cb614u, 0x0585bf36u, 0x1b85ac3du, 0x1cf856fau, 0x1891ecbdu, 0x1a7eec05u, 0x155a88f0u, 0x0741ac6du, 0x1317c30fu, 0x00000009u};
    return v[i];
}
__host__ __device__ constexpr u32 CIN29(int i) {
    constexpr u32 v[14] = {0x1fddebbdu, 0x1a4f5474u, 0x0291f399u, 0x14d03b3cu, 0x0f6cad2cu, 0x1b4cabcau, 0x1592827cu, 0x021c6ac7u, 0x1ec52a84u, 0x16fd5ec4u, 0x0c960da6u, 0x0fd2af6bu, 0x13263591u, 0x0000000bu};
    return v[i];
}
__host__ __device__ constexpr u32 COUT29(int i) {
    constexpr u32 v[14] = {0x0002fffdu, 0x10480000u, 0x0300009du, 0x08001788u, 0x158baebfu, 0x0c2ba9e3u, 0x1d157d22u, 0x0a6e0a4au, 0x0d77ce58u, 0x1d12b763u, 0x1701c6a5u, 0x1501c926u, 0x1f65ec3fu, 0x0000000au};
    return v[i];
}
__host__ __device__ constexpr u32 Q2_29(int i) {
    constexpr u32 v[14] = {0x1fff5556u, 0x1fefffffu, 0x09ffffdcu, 0x0ffffac5u, 0x1ec483d5u, 0x12a0f6b0u, 0x15fb3986u, 0x013ce144u, 0x0ec8ee97u, 0x0434bacdu, 0x058dd3dbu, 0x05ff9a69u, 0x00223d47u, 0x0000001au};
    return v[i];
}
__host__ __device__ constexpr u32 Q4_29(int i) {
    constexpr u32 v[14] = {0x1ffeaaacu, 0x1fdfffffu, 0x13ffffb9u, 0x1ffff58au, 0x1d8907aau, 0x0541ed61u, 0x0bf6730du, 0x0279c289u, 0x1d91dd2eu, 0x0869759au, 0x0b1ba7b6u, 0x0bff34d2u, 0x00447a8eu, 0x00000034u};
    return v[i];
}
__host__ __device__ constexpr u32 Q8_29(int i) {
    constexpr u32 v[14] = {0x1ffd5558u, 0x1fbfffffu, 0x07ffff73u, 0x1fffeb15u, 0x1b120f55u, 0x0a83dac3u, 0x17ece61au, 0x04f38512u, 0x1b23ba5cu, 0x10d2eb35u, 0x16374f6cu, 0x17fe69a4u, 0x0088f51cu, 0x00000068u};
    return v[i];
}
__host__ __device__ constexpr u32 RRP29(int i) {  // R'^2 mod q
    constexpr u32 v[14] = {0x15bef7aeu, 0x1031cd0eu, 0x02dd93e8u, 0x09226323u, 0x0e6e2cd2u, 0x11684daau, 0x1170e5dbu, 0x088e25b1u, 0x1b366399u, 0x1c536f47u, 0x0d1f9cbcu, 0x0278b67fu, 0x1ea66a2bu, 0x0000000cu};
    return v[i];
}
}  // namespace bls12_381
}  // namespace zk
