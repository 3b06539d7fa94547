// The host-only half of the ceremony (csrc/ceremony_host.h: container walk and writer, transcript parser, hash chain, challenges, beacon
// scalars) as a stand-alone program, so that it can run under the host sanitizers without the library or a device:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I eigen-zkvm_amd/csrc tools/ceremony_host_check.cpp -o ceremony_host_check
//   ceremony_host_check FILE.ptau G1_POINT_BYTES     walks the file, parses its transcript, recomputes the chain; prints what it found
//   ceremony_host_check --new OUT.ptau               writes a small new file (dummy generators) and reads it back
// Exit 0 whether the file is accepted or refused with a message; anything else is the sanitizer's or a crash.
#include "ceremony_host.h"
#include <cstdlib>
#include <fstream>
#include <iterator>

using namespace zk;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static void walk(const char* path, size_t B1) {
    const std::vector<uint8_t> file = slurp(path);
    size_t off; uint64_t size;
    if (!cer::find_section(file.data(), file.size(), 1, off, size) || size < 12) throw std::runtime_error("ptau: section 1 (header) is missing");
    const uint32_t n8 = cer::rd_u32(file.data() + off);
    if (size != 12 + (uint64_t)n8) throw std::runtime_error("ptau: header size");
    const uint32_t power = cer::rd_u32(file.data() + off + 4 + n8);
    if (!cer::find_section(file.data(), file.size(), cer::TRANSCRIPT_SECTION, off, size)) { printf("%s: no transcript\n", path); return; }
    const std::vector<cer::Rec> rec = cer::parse_transcript(file.data() + off, (size_t)size, B1);
    uint8_t prev[32], h[32], c[16], sc[96];
    cer::chain_start(n8, power, prev);
    size_t broken = 0;
    for (const cer::Rec& r : rec) {
        cer::record_hash(prev, r.start, B1, h);
        broken += std::memcmp(h, r.hash, 32) != 0;
        for (int j = 0; j < 3; ++j) cer::challenge(prev, j, r.img[j], r.img[j], r.R[j], B1, c);
        if (r.kind == 1 && r.iter_log <= 10) cer::beacon_scalars(r.seed, r.iter_log, sc);
        std::memcpy(prev, h, 32);
    }
    printf("%s: power %u, %zu record(s), %zu broken link(s), last hash %s\n", path, power, rec.size(), broken, sha256_hex(prev, 32).c_str());
}

int main(int argc, char** argv) {
    try {
        if (argc == 3 && std::string(argv[1]) == "--new") {
            std::vector<uint8_t> q(32, 0x11), g1(64, 0x22), g2(128, 0x33);
            cer::write_new_file(argv[2], 32, q.data(), 5, g1.data(), g1.size(), g2.data(), g2.size());
            walk(argv[2], 64);
            return 0;
        }
        if (argc != 3) { fprintf(stderr, "usage: ceremony_host_check FILE.ptau G1_POINT_BYTES | --new OUT.ptau\n"); return 2; }
        walk(argv[1], (size_t)atoi(argv[2]));
    } catch (const std::exception& e) {
        printf("%s: refused: %s\n", argv[1], e.what());
    }
    return 0;
}
