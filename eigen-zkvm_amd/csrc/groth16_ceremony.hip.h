// A powers-of-tau ceremony on the device: a fresh file, contributions and beacons with proofs of knowledge, and the check of the
// transcript they leave (ceremony_host.h has the layout and the hashes; DESIGN.md 3.17 the argument).  Included once by groth16.hip
// inside namespace zk, after groth16_srs.hip.h, whose file check, point classes and report style it shares.
//   srs_new         tau = alpha = beta = 1, host only
//   srs_contribute  every point of sections 2..6 times its own scalar -- ecn_powers_kernel makes the scalars, the per-point scalar product
//                   of ecntt.hip multiplies (G1 through the endomorphism split, G2 by the bit walk: this tree has no G2 endomorphism) --
//                   chunk by chunk through one bounded work buffer, straight into the output file
//   srs_verify      srs_check, the hash chain, every proof of knowledge, every beacon, and the last images against the file

namespace g16 {
static std::vector<uint8_t> generator_bytes(const Curve& cv, Group g) {
    std::vector<u32> w(cv.point_words(g));
    cv.group(g).generator_words(w.data());
    return std::vector<uint8_t>((const uint8_t*)w.data(), (const uint8_t*)w.data() + 4 * w.size());
}
// the file's transcript: present, and its records (pointers into the file's bytes)
static bool srs_records(const Srs& srs, std::vector<cer::Rec>& rec) {
    size_t off; uint64_t size;
    if (!cer::find_section(srs.file.data(), srs.file.size(), cer::TRANSCRIPT_SECTION, off, size)) return false;
    rec = cer::parse_transcript(srs.file.data() + off, (size_t)size, srs.curve->point_bytes(G1));
    return true;
}
static u64 srs_chunk() {                                             // points per chunk of a contribution; ZK_SRS_CHUNK, read once, is for tests
    static const u64 c = [] { const char* e = getenv("ZK_SRS_CHUNK"); const long long v = e ? atoll(e) : 0; return v >= 1 && v <= (1ll << 24) ? (u64)v : 1ull << 20; }();
    return c;
}
}  // namespace g16

void srs_new(const char* curve, uint32_t power, const char* path) {
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(path, "ptau: null path");
    const auto q = g16::q_bytes(cv), g1 = g16::generator_bytes(cv, G1), g2 = g16::generator_bytes(cv, G2);
    cer::write_new_file(path, 4 * cv.fq_words, q.data(), power, g1.data(), g1.size(), g2.data(), g2.size());
}

int64_t srs_transcript_count(const Srs& srs) {
    std::vector<cer::Rec> rec;
    return g16::srs_records(srs, rec) ? (int64_t)rec.size() : -1;
}

void srs_contribute(const Srs& srs, const char* out_path, const uint64_t* secrets, const uint8_t* beacon_seed, uint32_t beacon_iter_log) {
    using namespace g16;
    const Curve& cv = *srs.curve;
    ZK_REQUIRE(out_path, "ptau contribute: null path");
    ZK_REQUIRE(!(secrets && beacon_seed), "ptau contribute: a beacon takes no secrets");
    const size_t P1 = cv.point_words(G1), B1 = 4 * P1, B2 = cv.point_bytes(G2);
    const u64 N = 1ull << srs.power;
    const uint8_t* f = srs.file.data();
    std::vector<cer::Rec> old;
    srs_records(srs, old);
    // the three factors and the three nonces: canonical, wiped when the call ends however it ends
    u64 s[3][4], nonce[3][4], tab[1 + 29][4], tm[4];
    struct Guard { void* p[4]; size_t n[4]; ~Guard() { for (int i = 0; i < 4; ++i) wipe(p[i], n[i]); } } guard{{s, nonce, tab, tm}, {sizeof s, sizeof nonce, sizeof tab, sizeof tm}};
    uint32_t kind = 0;
    uint8_t seed32[32] = {};
    if (beacon_seed) {
        kind = 1;
        std::memcpy(seed32, beacon_seed, 32);
        uint8_t sc[96];
        cer::beacon_scalars(beacon_seed, beacon_iter_log, sc);
        std::memcpy(s, sc, 96);
    } else if (secrets) {
        std::memcpy(s, secrets, 96);
    } else {
        for (int j = 0; j < 3; ++j) draw_fr(cv, (u32*)s[j], "ptau contribute");
    }
    for (int j = 0; j < 3; ++j) {
        u32 any = 0; for (int i = 0; i < 8; ++i) any |= ((const u32*)s[j])[i];
        ZK_REQUIRE(any && cv.fr_canonical((const u32*)s[j]), "ptau contribute: a factor must be a non-zero canonical field element");
        draw_fr(cv, (u32*)nonce[j], "ptau contribute");
    }
    const FrHost F(cv);
    F.to_mont(s[0], tm);
    for (int b = 0; b < 29; ++b) { std::memcpy(tab[1 + b], tm, 32); F.mul(tm, tm, tm); }

    hipStream_t st = cur_stream();
    const u64 chunk = srs_chunk();
    const EcOps& E = cv.ec();
    DevBuf d_tab, d_k, d_pts, d_six, d_k6;
    d_tab.reserve(sizeof tab); d_k.reserve(chunk * 32); d_pts.reserve(chunk * B2); d_six.reserve(6 * B1); d_k6.reserve(6 * 32);
    struct Wipe { hipStream_t st; DevBuf* b[3]; ~Wipe() { for (DevBuf* x : b) if (x->p) (void)hipMemsetAsync(x->p, 0, x->bytes, st); (void)hipStreamSynchronize(st); } } dev_wipe{st, {&d_tab, &d_k, &d_k6}};

    // the bases of this contribution's proofs: the last record's images, or the file's own where it has no record
    const std::vector<uint8_t> gen1 = generator_bytes(cv, G1);
    const uint8_t* base[3];
    if (!old.empty()) for (int j = 0; j < 3; ++j) base[j] = old.back().img[j];
    else { base[0] = N >= 2 ? f + srs.off[2] + B1 : gen1.data(); base[1] = f + srs.off[4]; base[2] = f + srs.off[5]; }
    // images [s_j] B_j and commitments [n_j] B_j: six products in one launch
    std::vector<uint8_t> six(6 * B1), k6(6 * 32);
    for (int j = 0; j < 3; ++j) {
        std::memcpy(&six[j * B1], base[j], B1); std::memcpy(&six[(3 + j) * B1], base[j], B1);
        std::memcpy(&k6[j * 32], s[j], 32); std::memcpy(&k6[(3 + j) * 32], nonce[j], 32);
    }
    h2d_sync(d_six.p, six.data(), six.size()); h2d_sync(d_k6.p, k6.data(), k6.size());
    wipe(k6.data(), k6.size());
    E.g[G1].mul_scalars(d_six.p, P1, 6, (const u32*)d_k6.p, d_six.p, st);
    d2h_sync(six.data(), d_six.p, six.size());

    cer::File out(out_path, "wb");
    const uint64_t rb = cer::rec_bytes(B1);
    {
        const cer::Bytes head = cer::Bytes().str("ptau").u32(1).u32(7);
        out.write(head.data(), head.size());
        size_t off; uint64_t size;
        ZK_REQUIRE(cer::find_section(f, srs.file.size(), 1, off, size), "ptau: section 1 (header) is missing");
        out.section(1, size); out.write(f + off, (size_t)size);
    }
    for (int id = 2; id <= 6; ++id) {
        const Group g = SRS_GROUP[id];
        const size_t B = cv.point_bytes(g);
        const u64 n = srs_count(srs.power, id);
        out.section((uint32_t)id, n * B);
        // the section's leading factor: 1 for the tau sections, alpha, beta; betaG2 is the one point [beta] of exponent 0
        if (id == 4) F.to_mont(s[1], tab[0]); else if (id >= 5) F.to_mont(s[2], tab[0]); else std::memcpy(tab[0], F.one, 32);
        h2d_sync(d_tab.p, tab, sizeof tab);
        std::vector<uint8_t> host(std::min(n, chunk) * B);
        for (u64 i0 = 0; i0 < n; i0 += chunk) {
            const u64 m = std::min(chunk, n - i0);
            h2d_sync(d_pts.p, f + srs.off[id] + i0 * B, m * B);
            cv.groth16().powers_dev((const u32*)d_tab.p, i0, m, (u32*)d_k.p, st);
            (g == G1 ? E.g[G1].mul_scalars_glv : E.g[G2].mul_scalars)(d_pts.p, cv.point_words(g), m, (const u32*)d_k.p, d_pts.p, st);
            d2h_sync(host.data(), d_pts.p, m * B);
            out.write(host.data(), m * B);
        }
    }
    // the transcript: what was there, and this contribution's record
    uint8_t prev[32];
    if (old.empty()) cer::chain_start(4 * cv.fq_words, srs.power, prev); else std::memcpy(prev, old.back().hash, 32);
    cer::Bytes rec;
    rec.u32(kind).u32(kind ? beacon_iter_log : 0).put(seed32, 32);
    for (int j = 0; j < 3; ++j) rec.put(&six[j * B1], B1);
    for (int j = 0; j < 3; ++j) {
        uint8_t c16[16];
        cer::challenge(prev, j, base[j], &six[j * B1], &six[(3 + j) * B1], B1, c16);
        u64 c[4] = {0, 0, 0, 0}, z[4], sm[4];
        std::memcpy(c, c16, 16);
        F.to_mont(c, c); F.to_mont(s[j], sm); F.mul(c, sm, z); F.from_mont(z, z); F.add(z, nonce[j], z);   // z = n + c s mod r
        wipe(sm, 32);
        rec.put(&six[(3 + j) * B1], B1).put(z, 32);
    }
    uint8_t h[32];
    cer::Bytes chained = cer::Bytes().str("zkgpu rec v1").put(prev, 32).put(rec.data(), rec.size());
    chained.hash(h);
    rec.put(h, 32);
    ZK_REQUIRE(rec.size() == rb, "ptau contribute: record size");
    out.section(cer::TRANSCRIPT_SECTION, 8 + (old.size() + 1) * rb);
    const cer::Bytes th = cer::Bytes().u32(1).u32((uint32_t)old.size() + 1);
    out.write(th.data(), th.size());
    if (!old.empty()) out.write(old.front().start, old.size() * rb);
    out.write(rec.data(), rec.size());
    out.close();
}

std::string srs_verify(const Srs& srs, const uint8_t* seed, uint32_t max_findings) {
    using namespace g16;
    const Curve& cv = *srs.curve;
    const size_t P1 = cv.point_words(G1), B1 = 4 * P1;
    const u64 N = 1ull << srs.power;
    const uint8_t* f = srs.file.data();
    const std::string file_report = srs_check(srs, seed, max_findings);
    Findings F({"no_transcript", "chain_hash", "pok_invalid", "beacon_mismatch", "image_mismatch"}, max_findings);
    std::vector<cer::Rec> rec;
    const bool present = srs_records(srs, rec);
    const size_t n = rec.size();
    auto at = [](size_t i, int j) { return "\"contribution\":" + std::to_string(i + 1) + ",\"which\":\"" + cer::WHICH[j] + "\""; };
    hipStream_t st = cur_stream();
    const std::vector<uint8_t> gen1 = generator_bytes(cv, G1);
    if (!present) F.add("no_transcript", "\"section\":" + std::to_string(cer::TRANSCRIPT_SECTION));
    if (n) {
        // 1. the chain, and with the recomputed hashes the challenges
        std::vector<uint8_t> prev(32 * (n + 1));
        cer::chain_start(4 * cv.fq_words, srs.power, prev.data());
        for (size_t i = 0; i < n; ++i) {
            cer::record_hash(&prev[32 * i], rec[i].start, B1, &prev[32 * (i + 1)]);
            if (std::memcmp(&prev[32 * (i + 1)], rec[i].hash, 32) != 0) F.add("chain_hash", "\"contribution\":" + std::to_string(i + 1));
        }
        // 2. one launch for [z_j] B_j and [c_j] Q_j of every proof and for [scalar_j] B_j of every beacon; an image that is no point of the
        //    group, or infinity, fails its own proof and the next record's (whose base it is)
        std::vector<size_t> beacons;
        for (size_t i = 0; i < n; ++i) if (rec[i].kind == 1) beacons.push_back(i);
        const size_t np = 6 * n + 3 * beacons.size();
        std::vector<uint8_t> pts(np * B1), ks(np * 32, 0), img(3 * n * B1);
        auto base_of = [&](size_t i, int j) { return i ? rec[i - 1].img[j] : gen1.data(); };
        for (size_t i = 0; i < n; ++i)
            for (int j = 0; j < 3; ++j) {
                const size_t a = 3 * i + j, b = 3 * n + a;
                std::memcpy(&pts[a * B1], base_of(i, j), B1); std::memcpy(&ks[a * 32], rec[i].z[j], 32);
                std::memcpy(&pts[b * B1], rec[i].img[j], B1);
                cer::challenge(&prev[32 * i], j, base_of(i, j), rec[i].img[j], rec[i].R[j], B1, &ks[b * 32]);
                std::memcpy(&img[a * B1], rec[i].img[j], B1);
            }
        for (size_t q = 0; q < beacons.size(); ++q) {
            const size_t i = beacons[q];
            cer::beacon_scalars(rec[i].seed, rec[i].iter_log, &ks[(6 * n + 3 * q) * 32]);
            for (int j = 0; j < 3; ++j) std::memcpy(&pts[(6 * n + 3 * q + j) * B1], base_of(i, j), B1);
        }
        std::vector<char> bad_k(3 * n, 0);                             // a response that is no canonical scalar
        for (size_t a = 0; a < 3 * n; ++a)
            if (!cv.fr_canonical((const u32*)&ks[a * 32])) { bad_k[a] = 1; std::memset(&ks[a * 32], 0, 32); }
        DevBuf d_pts, d_k, d_img, d_res, d_diff;
        d_pts.reserve(np * B1); d_k.reserve(np * 32); d_img.reserve(3 * n * B1 + 4); d_res.reserve(3 * n * 64); d_diff.reserve(3 * n * B1);
        h2d_sync(d_pts.p, pts.data(), pts.size()); h2d_sync(d_k.p, ks.data(), ks.size()); h2d_sync(d_img.p, img.data(), img.size());
        for (size_t a = 0; a < 3 * n; ++a) cv.pairing().points_check[G1]((const u32*)d_img.p + a * P1, P1, 1, 0, 0, d_res.u() + 8 * a, st);
        cv.ec().g[G1].mul_scalars(d_pts.p, P1, np, (const u32*)d_k.p, d_pts.p, st);
        cv.ec().g[G1].diff(d_pts.p, (const u32*)d_pts.p + 3 * n * P1, 3 * n, d_diff.p, st);       // [z] B - [c] Q, to be R
        std::vector<u64> res(3 * n * 8);
        std::vector<uint8_t> diff(3 * n * B1), bq(3 * beacons.size() * B1);
        d2h_sync(res.data(), d_res.p, res.size() * 8); d2h_sync(diff.data(), d_diff.p, diff.size());
        if (!bq.empty()) d2h_sync(bq.data(), (const u32*)d_pts.p + 6 * n * P1, bq.size());
        auto image_bad = [&](size_t a) { return res[8 * a] || res[8 * a + 2] || res[8 * a + 4] || res[8 * a + 6]; };
        for (size_t i = 0; i < n; ++i)
            for (int j = 0; j < 3; ++j) {
                const size_t a = 3 * i + j;
                const bool ok = !bad_k[a] && !image_bad(a) && !(i && image_bad(a - 3)) && std::memcmp(&diff[a * B1], rec[i].R[j], B1) == 0;
                if (!ok) F.add("pok_invalid", at(i, j));
            }
        for (size_t q = 0; q < beacons.size(); ++q)
            for (int j = 0; j < 3; ++j)
                if (std::memcmp(&bq[(3 * q + j) * B1], rec[beacons[q]].img[j], B1) != 0) F.add("beacon_mismatch", at(beacons[q], j));
    }
    // 3. the last images are the file's (the generator where nobody has contributed); a file of power 0 has no tauG1[1]
    if (present) {
        const uint8_t* have[3] = {N >= 2 ? f + srs.off[2] + B1 : nullptr, f + srs.off[4], f + srs.off[5]};
        for (int j = 0; j < 3; ++j)
            if (have[j] && std::memcmp(have[j], n ? rec[n - 1].img[j] : gen1.data(), B1) != 0)
                F.add("image_mismatch", "\"contribution\":" + std::to_string(n) + ",\"which\":\"" + cer::WHICH[j] + "\"");
    }
    ZK_HIP(hipStreamSynchronize(st));
    return std::string("{\"curve\":\"") + cv.name + "\",\"power\":" + std::to_string(srs.power) + ",\"contributions\":" + std::to_string(n) + ",\"file\":" + file_report +
           "," + F.tail() + "}";
}

// ---- phase 2: contributions to a key's delta with proofs of knowledge ----------------------------------------------------------------------
// zk_groth16_contribution_check holds for any ratio its presenter knows (DESIGN.md 3.17 has the attack), so a chain of contributions carries
// a transcript beside the key -- bellman's layout has no room for one: "zkgk", u32 version = 1, u32 n8, u32 count, SHA-256 of the initial
// key; then per contribution SHA-256 of the new key | delta_g1 after | R | z (32 B canonical little-endian) | chain hash h_i.  Points in the
// key's own encoding.  The proof is the ceremony's Schnorr proof over base delta_g1 before and image delta_g1 after, with domains of its own:
// h_0 = SHA-256("zkgpu key transcript v1" | u32 n8 | initial hash), c = 16 bytes of SHA-256("zkgpu key pok v1" | h_{i-1} | B | Q | R),
// h_i = SHA-256("zkgpu key rec v1" | h_{i-1} | the record before its hash).
namespace g16 {
struct KeyRec { const uint8_t *start, *key_hash, *delta, *R, *z, *hash; };
constexpr size_t KEY_T_HEAD = 16 + 32;
static size_t key_rec_bytes(size_t B1) { return 32 + 2 * B1 + 32 + 32; }
static std::vector<KeyRec> parse_key_transcript(const uint8_t* p, size_t n, const Curve& cv) {
    const size_t B1 = cv.point_bytes(G1), rb = key_rec_bytes(B1);
    if (n < KEY_T_HEAD) throw std::runtime_error("key transcript: truncated file");
    if (std::memcmp(p, "zkgk", 4) != 0) throw std::runtime_error("key transcript: Invalid magic number");
    if (cer::rd_u32(p + 4) != 1) throw std::runtime_error("key transcript: Unsupported version");
    if (cer::rd_u32(p + 8) != 4 * cv.fq_words) throw std::runtime_error(std::string("key transcript: the file's field width is not ") + cv.name + "'s");
    const uint32_t count = cer::rd_u32(p + 12);
    if ((n - KEY_T_HEAD) / rb < count) throw std::runtime_error("key transcript: truncated file");
    if (n - KEY_T_HEAD != (size_t)count * rb) throw std::runtime_error("key transcript: bytes behind the last record");
    std::vector<KeyRec> out(count);
    for (uint32_t i = 0; i < count; ++i) {
        const uint8_t* q = p + KEY_T_HEAD + (size_t)i * rb;
        out[i] = KeyRec{q, q, q + 32, q + 32 + B1, q + 32 + 2 * B1, q + 64 + 2 * B1};
    }
    return out;
}
static void key_chain_start(uint32_t n8, const uint8_t* initial_hash, uint8_t* out) { cer::Bytes().str("zkgpu key transcript v1").u32(n8).put(initial_hash, 32).hash(out); }
static void key_challenge(const uint8_t* prev, const uint8_t* B, const uint8_t* Q, const uint8_t* R, size_t B1, uint8_t* c16) {
    uint8_t d[32];
    cer::Bytes().str("zkgpu key pok v1").put(prev, 32).put(B, B1).put(Q, B1).put(R, B1).hash(d);
    std::memcpy(c16, d, 16);
}
static void key_record_hash(const uint8_t* prev, const uint8_t* rec_start, size_t B1, uint8_t* out) {
    cer::Bytes().str("zkgpu key rec v1").put(prev, 32).put(rec_start, key_rec_bytes(B1) - 32).hash(out);
}
// n G1 points in the key's encoding (big-endian canonical coordinates) -> canonical little-endian words on the device, the sums' layout before
// fq_canon_to_mont_dev; bit 6 of byte 0 (infinity) or bit 7 gives the all-zero point
static void key_points_h2d(const Curve& cv, const std::vector<const uint8_t*>& pts, DevBuf& d) {
    const size_t B1 = cv.point_bytes(G1), cb = B1 / 2;
    std::vector<uint8_t> le(pts.size() * B1 + 4, 0);
    for (size_t i = 0; i < pts.size(); ++i) {
        if (pts[i][0] & 0xc0) continue;
        for (int c = 0; c < 2; ++c)
            for (size_t k = 0; k < cb; ++k) le[i * B1 + c * cb + k] = pts[i][c * cb + cb - 1 - k];
    }
    d.reserve(le.size());
    h2d_sync(d.p, le.data(), le.size());
}
// Montgomery device points -> the key's encoding on the host
static void key_points_d2h(const Curve& cv, DevBuf& d, u64 n, std::vector<uint8_t>& out, hipStream_t st) {
    DevBuf be;
    be.reserve(n * cv.point_bytes(G1));
    cv.msm().fq_mont_to_canon_dev(d.p, n * 2, st);
    points_to_be_dev((const u32*)d.p, n, (int)cv.fq_words, false, (u32*)be.p, st);
    out.resize(n * cv.point_bytes(G1));
    d2h_sync(out.data(), be.p, out.size());
}
}  // namespace g16

size_t groth16_key_transcript_size(const char* curve, uint32_t count) {
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    return g16::KEY_T_HEAD + (size_t)count * g16::key_rec_bytes(cv.point_bytes(G1));
}

void groth16_params_contribute_pok(const char* curve, const void* params, size_t len, const uint64_t* delta, const void* transcript, size_t t_len,
                                   void* out_params, void* out_transcript) {
    using namespace g16;
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(params && out_params && out_transcript && (transcript || !t_len), "groth16 contribute: null argument");
    const size_t P1 = cv.point_words(G1), B1 = 4 * P1, rb = key_rec_bytes(B1);
    const KeyLayout L = key_layout(cv, parse_params((const uint8_t*)params, len, 4 * (int)cv.fq_words));
    // where the chain stands: at this key
    uint8_t key_hash[32], prev[32];
    sha256_raw(params, len, key_hash);
    std::vector<KeyRec> old;
    if (t_len) {
        old = parse_key_transcript((const uint8_t*)transcript, t_len, cv);
        ZK_REQUIRE(std::memcmp(old.empty() ? (const uint8_t*)transcript + 16 : old.back().key_hash, key_hash, 32) == 0, "groth16 contribute: the transcript does not end at this key");
    }
    if (old.empty()) key_chain_start(4 * cv.fq_words, key_hash, prev); else std::memcpy(prev, old.back().hash, 32);
    u64 k[4], nonce[4], sm[4];
    struct Guard { u64 *a, *b, *c; ~Guard() { wipe(a, 32); wipe(b, 32); wipe(c, 32); } } guard{k, nonce, sm};
    if (delta) std::memcpy(k, delta, 32); else draw_fr(cv, (u32*)k, "groth16 contribute");
    draw_fr(cv, (u32*)nonce, "groth16 contribute");
    const std::vector<uint8_t> base((const uint8_t*)params + L.delta_g1, (const uint8_t*)params + L.delta_g1 + B1);   // out_params may be params
    groth16_params_contribute(curve, params, len, (const uint64_t*)k, out_params);          // refuses a delta that is zero or not canonical
    const uint8_t* image = (const uint8_t*)out_params + L.delta_g1;
    // R = [n] delta_g1
    hipStream_t st = cur_stream();
    DevBuf d_b, d_n;
    d_n.reserve(32);
    struct Wipe { hipStream_t st; DevBuf* b; ~Wipe() { if (b->p) (void)hipMemsetAsync(b->p, 0, b->bytes, st); (void)hipStreamSynchronize(st); } } dev_wipe{st, &d_n};
    key_points_h2d(cv, {base.data()}, d_b);
    h2d_sync(d_n.p, nonce, 32);
    cv.msm().fq_canon_to_mont_dev(d_b.p, 2, st);
    cv.ec().g[G1].mul_scalars(d_b.p, P1, 1, (const u32*)d_n.p, d_b.p, st);
    std::vector<uint8_t> R;
    key_points_d2h(cv, d_b, 1, R, st);
    uint8_t c16[16], new_hash[32], h[32];
    key_challenge(prev, base.data(), image, R.data(), B1, c16);
    const FrHost F(cv);
    u64 c[4] = {0, 0, 0, 0}, z[4];
    std::memcpy(c, c16, 16);
    F.to_mont(c, c); F.to_mont(k, sm); F.mul(c, sm, z); F.from_mont(z, z); F.add(z, nonce, z);
    sha256_raw(out_params, len, new_hash);
    cer::Bytes rec;
    rec.put(new_hash, 32).put(image, B1).put(R.data(), B1).put(z, 32);
    cer::Bytes().str("zkgpu key rec v1").put(prev, 32).put(rec.data(), rec.size()).hash(h);
    rec.put(h, 32);
    cer::Bytes out;
    out.str("zkgk").u32(1).u32(4 * cv.fq_words).u32((uint32_t)old.size() + 1).put(t_len ? (const uint8_t*)transcript + 16 : key_hash, 32);
    if (!old.empty()) out.put(old.front().start, old.size() * rb);
    out.put(rec.data(), rec.size());
    std::memcpy(out_transcript, out.data(), out.size());
}

std::string groth16_key_transcript_check(const char* curve, const void* initial, size_t initial_len, const void* final_key, size_t final_len,
                                         const void* transcript, size_t t_len, const uint8_t* seed, uint32_t max_findings) {
    using namespace g16;
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(initial && final_key && transcript, "groth16 key transcript: null argument");
    const size_t P1 = cv.point_words(G1), B1 = 4 * P1;
    const KeyLayout L0 = key_layout(cv, parse_params((const uint8_t*)initial, initial_len, 4 * (int)cv.fq_words));
    const KeyLayout L1 = key_layout(cv, parse_params((const uint8_t*)final_key, final_len, 4 * (int)cv.fq_words));
    const std::vector<KeyRec> rec = parse_key_transcript((const uint8_t*)transcript, t_len, cv);
    const size_t n = rec.size();
    const std::string keys = groth16_contribution_check(curve, initial, initial_len, final_key, final_len, seed, max_findings);
    Findings F({"initial_key_mismatch", "chain_hash", "pok_invalid", "final_key_mismatch"}, max_findings);
    uint8_t hash0[32], hash1[32];
    sha256_raw(initial, initial_len, hash0); sha256_raw(final_key, final_len, hash1);
    const uint8_t* t_initial = (const uint8_t*)transcript + 16;
    if (std::memcmp(hash0, t_initial, 32) != 0) F.add("initial_key_mismatch", "\"what\":\"hash\"");
    std::vector<uint8_t> prev(32 * (n + 1));
    key_chain_start(4 * cv.fq_words, t_initial, prev.data());
    for (size_t i = 0; i < n; ++i) {
        key_record_hash(&prev[32 * i], rec[i].start, B1, &prev[32 * (i + 1)]);
        if (std::memcmp(&prev[32 * (i + 1)], rec[i].hash, 32) != 0) F.add("chain_hash", "\"contribution\":" + std::to_string(i + 1));
    }
    hipStream_t st = cur_stream();
    if (n) {
        // [z_i] B_i and [c_i] Q_i in one launch; B_1 is the initial key's delta_g1
        auto base_of = [&](size_t i) { return i ? rec[i - 1].delta : (const uint8_t*)initial + L0.delta_g1; };
        std::vector<const uint8_t*> pts(2 * n);
        std::vector<uint8_t> ks(2 * n * 32, 0);
        std::vector<char> bad_k(n, 0);
        for (size_t i = 0; i < n; ++i) {
            pts[i] = base_of(i); pts[n + i] = rec[i].delta;
            std::memcpy(&ks[i * 32], rec[i].z, 32);
            if (!cv.fr_canonical((const u32*)&ks[i * 32])) { bad_k[i] = 1; std::memset(&ks[i * 32], 0, 32); }
            key_challenge(&prev[32 * i], base_of(i), rec[i].delta, rec[i].R, B1, &ks[(n + i) * 32]);
        }
        DevBuf d_pts, d_k, d_res, d_diff;
        key_points_h2d(cv, pts, d_pts);
        d_k.reserve(ks.size()); d_res.reserve(n * 64); d_diff.reserve(n * B1);
        h2d_sync(d_k.p, ks.data(), ks.size());
        for (size_t i = 0; i < n; ++i) cv.pairing().points_check[G1]((const u32*)d_pts.p + (n + i) * P1, P1, 1, 0, 1, d_res.u() + 8 * i, st);
        cv.msm().fq_canon_to_mont_dev(d_pts.p, 2 * n * 2, st);
        cv.ec().g[G1].mul_scalars(d_pts.p, P1, 2 * n, (const u32*)d_k.p, d_pts.p, st);
        cv.ec().g[G1].diff(d_pts.p, (const u32*)d_pts.p + n * P1, n, d_diff.p, st);
        std::vector<u64> res(n * 8);
        d2h_sync(res.data(), d_res.p, res.size() * 8);
        std::vector<uint8_t> R;
        key_points_d2h(cv, d_diff, n, R, st);
        auto image_bad = [&](size_t i) { return res[8 * i] || res[8 * i + 2] || res[8 * i + 4] || res[8 * i + 6]; };
        for (size_t i = 0; i < n; ++i)
            if (bad_k[i] || image_bad(i) || (i && image_bad(i - 1)) || std::memcmp(&R[i * B1], rec[i].R, B1) != 0) F.add("pok_invalid", "\"contribution\":" + std::to_string(i + 1));
    }
    const uint8_t* last_delta = n ? rec[n - 1].delta : (const uint8_t*)initial + L0.delta_g1;
    if (std::memcmp(last_delta, (const uint8_t*)final_key + L1.delta_g1, B1) != 0) F.add("final_key_mismatch", "\"what\":\"delta_g1\"");
    else if (std::memcmp(n ? rec[n - 1].key_hash : t_initial, hash1, 32) != 0) F.add("final_key_mismatch", "\"what\":\"hash\"");
    ZK_HIP(hipStreamSynchronize(st));
    return std::string("{\"curve\":\"") + cv.name + "\",\"contributions\":" + std::to_string(n) + ",\"keys\":" + keys + "," + F.tail() + "}";
}
