// What a powers-of-tau ceremony needs on the host alone: the .ptau container (walking its sections, writing a fresh file), the transcript
// of contributions (section 64 -- a layout of this project, NOT snarkjs's section 7), its hash chain, the challenges of its proofs of
// knowledge and a beacon's scalars.  Plain C++ over bytes, no device and no curve arithmetic, so that it can be compiled into a
// stand-alone program and run under the host sanitizers.  DESIGN.md 3.17 has the protocol; tests/ceremony_ref.py restates it in Python.
//
// Transcript payload: u32 version = 1, u32 count, then count records of
//   u32 kind (0 secret, 1 beacon) | u32 iter_log | 32 B beacon seed (zeros for a secret)
//   | three images after the contribution: tauG1[1], alphaTauG1[0], betaTauG1[0], each a G1 point in the file's layout
//   | three proofs, each R (a G1 point) and z (32 B canonical little-endian)
//   | 32 B chain hash h_i
// h_0 = SHA-256("zkgpu ptau transcript v1" | u32 n8 | u32 power); h_i = SHA-256("zkgpu rec v1" | h_{i-1} | the record before its hash).
// Proof j of a record over base B_j (the previous record's image j, or G1) and image Q_j = [s_j] B_j: R_j = [n_j] B_j,
// c_j = the first 16 bytes, little-endian, of SHA-256("zkgpu pok v1" | h_{i-1} | u8 j | B_j | Q_j | R_j), z_j = n_j + c_j s_j mod r.
#pragma once
#include "sha256.h"
#include <cstdio>
#include <stdexcept>
#include <vector>

namespace zk {
namespace cer {

constexpr uint32_t TRANSCRIPT_SECTION = 64;
static const char* const WHICH[3] = {"tau", "alpha", "beta"};

struct Bytes : std::vector<uint8_t> {
    Bytes& put(const void* p, size_t n) { insert(end(), (const uint8_t*)p, (const uint8_t*)p + n); return *this; }
    Bytes& str(const char* s) { return put(s, std::strlen(s)); }
    Bytes& u8(uint8_t v) { push_back(v); return *this; }
    Bytes& u32(uint32_t v) { for (int i = 0; i < 4; ++i) push_back((uint8_t)(v >> (8 * i))); return *this; }
    Bytes& u64(uint64_t v) { for (int i = 0; i < 8; ++i) push_back((uint8_t)(v >> (8 * i))); return *this; }
    void hash(uint8_t* out) const { sha256_raw(data(), size(), out); }
};
inline uint32_t rd_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t rd_u64(const uint8_t* p) { return (uint64_t)rd_u32(p) | (uint64_t)rd_u32(p + 4) << 32; }

// where section `id` of a .ptau container lies (the first one of that id); false when there is none
inline bool find_section(const uint8_t* file, size_t len, uint32_t id, size_t& off, uint64_t& size) {
    if (len < 12 || std::memcmp(file, "ptau", 4) != 0) throw std::runtime_error("ptau: Invalid magic number");
    const uint32_t n_sec = rd_u32(file + 8);
    size_t o = 12;
    for (uint32_t i = 0; i < n_sec; ++i) {
        if (len - o < 12) throw std::runtime_error("ptau: truncated file");
        const uint32_t t = rd_u32(file + o); const uint64_t sz = rd_u64(file + o + 4);
        o += 12;
        if (sz > len - o) throw std::runtime_error("ptau: truncated file");
        if (t == id) { off = o; size = sz; return true; }
        o += (size_t)sz;
    }
    return false;
}

struct Rec {
    uint32_t kind, iter_log;
    const uint8_t *start, *seed, *img[3], *R[3], *z[3], *hash;
};
inline size_t rec_bytes(size_t B1) { return 8 + 32 + 3 * B1 + 3 * (B1 + 32) + 32; }
// the records of a transcript payload; B1: bytes of a G1 point
inline std::vector<Rec> parse_transcript(const uint8_t* p, size_t n, size_t B1) {
    if (n < 8) throw std::runtime_error("ptau transcript: truncated section");
    if (rd_u32(p) != 1) throw std::runtime_error("ptau transcript: Unsupported version");
    const uint32_t count = rd_u32(p + 4);
    const size_t rb = rec_bytes(B1);
    if ((n - 8) / rb < count) throw std::runtime_error("ptau transcript: truncated section");
    if (n - 8 != (size_t)count * rb) throw std::runtime_error("ptau transcript: " + std::to_string(n - 8 - (size_t)count * rb) + " bytes behind the last record");
    std::vector<Rec> out(count);
    for (uint32_t i = 0; i < count; ++i) {
        const uint8_t* q = p + 8 + (size_t)i * rb;
        Rec& r = out[i];
        r.start = q; r.kind = rd_u32(q); r.iter_log = rd_u32(q + 4); r.seed = q + 8;
        if (r.kind > 1) throw std::runtime_error("ptau transcript: record " + std::to_string(i + 1) + " has an unknown kind");
        q += 40;
        for (int j = 0; j < 3; ++j, q += B1) r.img[j] = q;
        for (int j = 0; j < 3; ++j, q += B1 + 32) { r.R[j] = q; r.z[j] = q + B1; }
        r.hash = q;
    }
    return out;
}
inline void chain_start(uint32_t n8, uint32_t power, uint8_t* out) { Bytes().str("zkgpu ptau transcript v1").u32(n8).u32(power).hash(out); }
inline void record_hash(const uint8_t* prev, const uint8_t* rec_start, size_t B1, uint8_t* out) {
    Bytes().str("zkgpu rec v1").put(prev, 32).put(rec_start, rec_bytes(B1) - 32).hash(out);
}
// c: 16 bytes, little-endian
inline void challenge(const uint8_t* prev, int j, const uint8_t* base, const uint8_t* image, const uint8_t* R, size_t B1, uint8_t* c) {
    uint8_t d[32];
    Bytes().str("zkgpu pok v1").put(prev, 32).u8((uint8_t)j).put(base, B1).put(image, B1).put(R, B1).hash(d);
    std::memcpy(c, d, 16);
}
// a beacon's three scalars, 32 B little-endian each: d = SHA-256 iterated 2^iter_log times over the seed, scalar j = SHA-256(d | u8 j) cut to
// 253 bits -- below r on both curves, no reduction
inline void beacon_scalars(const uint8_t* seed, uint32_t iter_log, uint8_t* out /* 3 x 32 */) {
    if (iter_log > 40) throw std::runtime_error("ptau beacon: iter_log above 40");
    uint8_t d[32];
    std::memcpy(d, seed, 32);
    for (uint64_t i = 0; i < (1ull << iter_log); ++i) sha256_raw(d, 32, d);
    for (int j = 0; j < 3; ++j) {
        Bytes().put(d, 32).u8((uint8_t)j).hash(out + 32 * j);
        out[32 * j + 31] &= 0x1f;
    }
}

struct File {                                                       // a FILE* that closes, and a writer that notices a full disk
    FILE* f; std::string path;
    File(const char* p, const char* mode) : f(fopen(p, mode)), path(p) { if (!f) throw std::runtime_error("ptau: cannot open " + path); }
    ~File() { if (f) fclose(f); }
    void write(const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) throw std::runtime_error("ptau: cannot write " + path); }
    void section(uint32_t id, uint64_t size) { const Bytes h = Bytes().u32(id).u64(size); write(h.data(), h.size()); }
    void close() { FILE* g = f; f = nullptr; if (fclose(g) != 0) throw std::runtime_error("ptau: cannot write " + path); }
};
inline uint64_t section_count(uint32_t power, int id) { const uint64_t n = 1ull << power; return id == 2 ? 2 * n - 1 : id == 6 ? 1 : n; }
// a file for tau = alpha = beta = 1: every point the generator of its group, an empty transcript.  q: the base field's modulus, n8 bytes
// little-endian; g1, g2: the generators in the file's layout (B1, B2 bytes)
inline void write_new_file(const char* path, uint32_t n8, const uint8_t* q, uint32_t power, const uint8_t* g1, size_t B1, const uint8_t* g2, size_t B2) {
    if (power > 28) throw std::runtime_error("ptau: power " + std::to_string(power) + " is out of range");
    File f(path, "wb");
    const Bytes head = Bytes().str("ptau").u32(1).u32(7);
    f.write(head.data(), head.size());
    const Bytes h1 = Bytes().u32(n8).put(q, n8).u32(power).u32(power);
    f.section(1, h1.size()); f.write(h1.data(), h1.size());
    for (int id = 2; id <= 6; ++id) {
        const bool two = id == 3 || id == 6;
        const uint8_t* g = two ? g2 : g1; const size_t B = two ? B2 : B1;
        const uint64_t n = section_count(power, id);
        f.section((uint32_t)id, n * B);
        std::vector<uint8_t> buf;
        const uint64_t per = 4096;
        for (uint64_t k = 0; k < per && k < n; ++k) buf.insert(buf.end(), g, g + B);
        for (uint64_t done = 0; done < n; done += per) f.write(buf.data(), (size_t)((n - done < per ? n - done : per) * B));
    }
    const Bytes t = Bytes().u32(1).u32(0);
    f.section(TRANSCRIPT_SECTION, t.size()); f.write(t.data(), t.size());
    f.close();
}

}  // namespace cer
}  // namespace zk
