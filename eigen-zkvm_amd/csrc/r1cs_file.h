// The two .r1cs readers of the library and what they return, for the units that read a circuit: the prover and key generation
// (groth16.hip: 32-byte fields), the compressor's setup (c12_setup.hip: Goldilocks, with the custom-gate sections) and the witness
// check (r1cs_check.hip: both).  Each reader is defined where it always was; this header only declares it.  Internal, like zk_internal.h.
#pragma once
#include "zk_internal.h"
#include <array>
#include <map>
#include <string>
#include <vector>

namespace zk {

struct Curve;

namespace g16 {
struct Lc { std::vector<u32> col, coeff; };            // coeff: 8 x u32 canonical per term
struct Row { Lc lc[3]; };
struct R1cs { uint32_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0; std::vector<Row> rows; };
// r1cs_file.rs:185-270 from_reader over a 32-byte field (groth16.hip); the terms of a row side come ordered by wire
R1cs parse_r1cs(const uint8_t* b, size_t len, const Curve& cv);
std::string words_to_dec(const u32* w, int n);         // n little-endian words -> decimal text
}  // namespace g16

namespace c12 {
using Lc = std::map<u64, u64>;                            // wire -> coefficient, ordered by wire as the reference's BTreeMap
struct CustomGate { std::string name; std::vector<u64> params; };
struct CustomUse { u64 id; std::vector<u64> signals; };
struct R1csGL {
    uint32_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0;
    std::vector<std::array<Lc, 3>> rows;
    std::vector<CustomGate> gates;
    std::vector<CustomUse> uses;
};
// the same over the 8-byte field, sections 4 and 5 included (c12_setup.hip)
R1csGL parse_r1cs_gl(const uint8_t* b, size_t len);
}  // namespace c12

}  // namespace zk
