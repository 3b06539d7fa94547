// A Groth16 key without a trapdoor: from a powers-of-tau file, then contributions to delta.  Included once by groth16.hip inside namespace
// zk, after the key check (whose rho kernel and point classes it shares).  DESIGN.md 3.14 has the algebra.
//   srs_open                  the snarkjs .ptau container, host only
//   srs_check                 every point, and that the sections are the powers they claim (random linear combinations + pairings)
//   groth16_keygen_from_srs   the key for the trapdoor (tau, alpha, beta, 1, 1) nobody knows: inverse group transforms give the Lagrange
//                             bases in the group, column sums over the circuit's matrices the queries, differences the h query
//   groth16_params_contribute delta <- delta delta', l and h <- l / delta', h / delta'
//   groth16_contribution_check  what a contribution may and may not have changed
// The group work is ecntt.hip's (curve.h EcOps); sums and pairings are the existing ones.

namespace g16 {
static const char* const SRS_SECTION[7] = {"", "header", "tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2"};
static const Group SRS_GROUP[7] = {G1, G1, G1, G2, G1, G1, G2};
static u64 srs_count(uint32_t power, int id) { return cer::section_count(power, id); }   // ceremony_host.h: the writer counts the same way

// e(a1, a2) == e(b1, b2) for device points in the layout of the sums (all zero = infinity)
struct PairEq {
    const Curve& cv; hipStream_t st; DevBuf d_p1, d_p2, d_gt; u64 pairs = 0;
    PairEq(const Curve& c, hipStream_t s) : cv(c), st(s) { d_p1.reserve(2 * cv.point_bytes(G1)); d_p2.reserve(2 * cv.point_bytes(G2)); d_gt.reserve(2 * cv.gt_bytes()); }
    bool operator()(const void* a1, const void* a2, const void* b1, const void* b2) {
        const size_t B1 = cv.point_bytes(G1), B2 = cv.point_bytes(G2);
        ZK_HIP(hipMemcpyAsync(d_p1.p, a1, B1, hipMemcpyDeviceToDevice, st));
        ZK_HIP(hipMemcpyAsync((uint8_t*)d_p1.p + B1, b1, B1, hipMemcpyDeviceToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_p2.p, a2, B2, hipMemcpyDeviceToDevice, st));
        ZK_HIP(hipMemcpyAsync((uint8_t*)d_p2.p + B2, b2, B2, hipMemcpyDeviceToDevice, st));
        pairing_dev(cv, d_p1.p, d_p2.p, 2, d_gt.p, 1, st);
        std::vector<uint8_t> gt(2 * cv.gt_bytes());
        d2h_sync(gt.data(), d_gt.p, gt.size());
        pairs += 2;
        return std::memcmp(gt.data(), gt.data() + cv.gt_bytes(), cv.gt_bytes()) == 0;
    }
};
// rho_i of kc_rho_kernel for i < n; seed: 32 bytes, or null for the operating system's
static void rho_dev(const uint8_t* seed, u64 n, DevBuf& d_rho, hipStream_t st, const char* who) {
    uint8_t sd[32];
    if (seed) std::memcpy(sd, seed, 32); else os_random(sd, 32, who);
    DevBuf d_seed; d_seed.reserve(32); d_rho.reserve(n * 32 + 4);
    h2d_sync(d_seed.p, sd, 32);
    wipe(sd, 32);
    if (n) hipLaunchKernelGGL(kc_rho_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const u32*)d_seed.p, n, (u32*)d_rho.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));
}
// out = sum rho_i P_i (the point, then the flag word of the sums); -> the sum is infinity
static bool rlc(const Curve& cv, Group g, const void* d_pts, const DevBuf& d_rho, u64 n, DevBuf& out, hipStream_t st) {
    const size_t B = cv.point_bytes(g);
    if (!out.p) out.reserve(B + 4);
    cv.group(g).msm_dev(d_pts, d_rho.p, n, out.p, st);
    u32 flag = 0;
    d2h_sync(&flag, (const uint8_t*)out.p + B, 4);
    if (flag) ZK_HIP(hipMemsetAsync(out.p, 0, B, st));
    return flag != 0;
}
// the findings of a report, kind by kind, and its tail
struct Findings {
    std::vector<const char*> kinds; std::vector<std::string> found; std::vector<u64> counts; uint32_t max;
    Findings(std::initializer_list<const char*> k, uint32_t mx) : kinds(k), found(k.size()), counts(k.size(), 0), max(mx) {}
    void add(const char* kind, const std::string& body) {
        size_t i = 0;
        while (std::strcmp(kinds[i], kind)) ++i;
        if (counts[i]++ < max) found[i] += (found[i].empty() ? "" : ",") + ("{\"kind\":\"" + std::string(kind) + "\"," + body + "}");
    }
    void point_classes(const char* section, const u64* res) {
        for (int c = 0; c < 4; ++c)
            if (res[2 * c]) add(KC_CLASS_NAMES[c], std::string("\"section\":\"") + section + "\",\"n_points\":" + std::to_string(res[2 * c]) + ",\"first_index\":" + std::to_string(res[2 * c + 1]));
    }
    std::string tail() const {
        std::string js = "\"counts\":{";
        for (size_t k = 0; k < kinds.size(); ++k) js += std::string(k ? "," : "") + "\"" + kinds[k] + "\":" + std::to_string(counts[k]);
        js += "},\"findings\":[";
        bool first = true;
        for (const auto& f : found)
            if (!f.empty()) { js += (first ? "" : ",") + f; first = false; }
        return js + "]";
    }
};
static std::vector<uint8_t> q_bytes(const Curve& cv) {               // the base field's modulus, little-endian, as the header carries it
    const size_t qb = 4 * (size_t)cv.fq_words;
    std::vector<uint8_t> q(qb, 0);
    const std::string qh = cv.pairing().q_hex;
    for (size_t i = 0; i < qh.size() && i < 2 * qb; ++i) {
        const char c = qh[qh.size() - 1 - i];
        const int d = c >= '0' && c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
        q[i / 2] |= (uint8_t)(d << (4 * (i & 1)));
    }
    return q;
}
static std::string skipped_entry(const char* check, const char* section, const char* reason) {
    return std::string("{\"check\":\"") + check + "\",\"section\":\"" + section + "\",\"reason\":\"" + reason + "\"}";
}
}  // namespace g16

Srs* srs_open(const char* curve, const char* path) {
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(path, "ptau: null path");
    auto s = std::make_unique<Srs>();
    s->curve = &cv;
    {
        FILE* f = fopen(path, "rb");
        ZK_REQUIRE(f, std::string("ptau: cannot open ") + path);
        std::unique_ptr<FILE, int (*)(FILE*)> guard_f(f, fclose);
        ZK_REQUIRE(fseek(f, 0, SEEK_END) == 0, std::string("ptau: cannot read ") + path);
        const long len = ftell(f);
        ZK_REQUIRE(len >= 0 && fseek(f, 0, SEEK_SET) == 0, std::string("ptau: cannot read ") + path);
        s->file.resize((size_t)len);
        ZK_REQUIRE(fread(s->file.data(), 1, s->file.size(), f) == s->file.size(), std::string("ptau: cannot read ") + path);
    }
    g16::Reader rd{s->file.data(), s->file.size(), 0, "ptau"};
    if (std::memcmp(rd.take(4), "ptau", 4) != 0) throw std::runtime_error("ptau: Invalid magic number");
    if (rd.u32le() != 1) throw std::runtime_error("ptau: Unsupported version");
    const uint32_t n_sec = rd.u32le();
    std::map<uint32_t, std::pair<size_t, uint64_t>> sec;
    for (uint32_t i = 0; i < n_sec; ++i) {
        const uint32_t t = rd.u32le(); const uint64_t sz = rd.u64le();
        if (!sec.count(t)) sec[t] = {rd.o, sz};                             // contributions and a prepared file's Lagrange sections are walked over
        rd.take(sz);
    }
    auto missing = [&](int id) { return std::string("ptau: section ") + std::to_string(id) + " (" + g16::SRS_SECTION[id] + ") is missing"; };
    if (!sec.count(1)) throw std::runtime_error(missing(1));
    g16::Reader h{s->file.data() + sec[1].first, (size_t)sec[1].second, 0, "ptau header"};
    const uint32_t n8 = h.u32le();
    const std::vector<uint8_t> q = g16::q_bytes(cv);
    const size_t qb = q.size();
    if (n8 != qb || sec[1].second != 12 + (uint64_t)n8 || std::memcmp(h.take(n8), q.data(), qb) != 0)
        throw std::runtime_error(std::string("ptau: the file's prime is not the base field of ") + cv.name);
    s->power = h.u32le(); s->ceremony_power = h.u32le();
    ZK_REQUIRE(s->power <= 28, "ptau: power " + std::to_string(s->power) + " is out of range");
    for (int id = 2; id <= 6; ++id) {
        if (!sec.count(id)) throw std::runtime_error(missing(id));
        const uint64_t want = g16::srs_count(s->power, id) * cv.point_bytes(g16::SRS_GROUP[id]);
        if (sec[id].second != want)
            throw std::runtime_error(std::string("ptau: section ") + std::to_string(id) + " (" + g16::SRS_SECTION[id] + ") has " + std::to_string(sec[id].second) +
                                     " bytes, power " + std::to_string(s->power) + " needs " + std::to_string(want));
        s->off[id] = sec[id].first;
    }
    return s.release();
}

std::string srs_check(const Srs& srs, const uint8_t* seed, uint32_t max_findings) {
    using namespace g16;
    const Curve& cv = *srs.curve;
    hipStream_t st = cur_stream();
    const PairingOps& po = cv.pairing();
    const u64 N = 1ull << srs.power;
    Findings F({"infinity", "coordinate_range", "not_on_curve", "not_in_subgroup", "not_generator", "not_powers", "beta_mismatch"}, max_findings);
    std::string skipped;
    auto skip = [&](const char* check, int id) { skipped += (skipped.empty() ? "" : ",") + skipped_entry(check, SRS_SECTION[id], "an invalid point"); };
    // 1. every point of the sections used: on its curve, in the subgroup, not infinity
    DevBuf d[7], d_res;
    d_res.reserve(7 * 64);
    u64 n_pts[2] = {0, 0};
    for (int id = 2; id <= 6; ++id) {
        const u64 n = srs_count(srs.power, id);
        const Group g = SRS_GROUP[id];
        d[id].reserve(n * cv.point_bytes(g) + 4);
        h2d_sync(d[id].p, srs.file.data() + srs.off[id], n * cv.point_bytes(g));
        po.points_check[g](d[id].p, cv.point_words(g), n, 0, 0, d_res.u() + 8 * id, st);
        n_pts[g] += n;
    }
    u64 res[7][8];
    d2h_sync(res, d_res.p, sizeof res);
    bool bad[7] = {};
    for (int id = 2; id <= 6; ++id) {
        for (int c = 0; c < 4; ++c) bad[id] = bad[id] || res[id][2 * c];
        F.point_classes(SRS_SECTION[id], res[id]);
    }
    // 2. tauG1[0] = G1, tauG2[0] = G2
    const size_t B1 = cv.point_bytes(G1), B2 = cv.point_bytes(G2);
    DevBuf d_one, d_gen1, d_gen2;
    d_one.reserve(8); d_gen1.reserve(B1); d_gen2.reserve(B2);
    const u64 one = 1;
    h2d_sync(d_one.p, &one, 8);
    cv.group(G1).mul_generator_dev(d_one.u(), 1, d_gen1.p, st);
    cv.group(G2).mul_generator_dev(d_one.u(), 1, d_gen2.p, st);
    std::vector<uint8_t> gen(B2);
    d2h_sync(gen.data(), d_gen1.p, B1);
    if (std::memcmp(gen.data(), srs.file.data() + srs.off[2], B1) != 0) F.add("not_generator", "\"section\":\"tauG1\"");
    d2h_sync(gen.data(), d_gen2.p, B2);
    if (std::memcmp(gen.data(), srs.file.data() + srs.off[3], B2) != 0) F.add("not_generator", "\"section\":\"tauG2\"");
    // 3. consecutive entries of a section differ by the factor tau: with A = sum rho_i S[i + 1] and B = sum rho_i S[i],
    //    e(A, G2) = e(B, tau G2) for a G1 section and e(G1, A) = e(tau G1, B) for tauG2; a section that is not such a sequence survives with
    //    probability 2^-128
    PairEq same(cv, st);
    if (N >= 2) {
        DevBuf d_rho, sa, sb;
        rho_dev(seed, 2 * N - 2, d_rho, st, "srs check");
        const void* tau_g1 = (const uint8_t*)d[2].p + B1;                   // tauG1[1], tauG2[1]
        const void* tau_g2 = (const uint8_t*)d[3].p + B2;
        for (int id = 2; id <= 5; ++id) {
            const Group g = SRS_GROUP[id];
            const int other = g == G1 ? 3 : 2;
            if (bad[id] || bad[other]) { skip("not_powers", id); continue; }
            const u64 n = srs_count(srs.power, id) - 1;
            const size_t B = cv.point_bytes(g);
            const bool ia = rlc(cv, g, (const uint8_t*)d[id].p + B, d_rho, n, sa, st), ib = rlc(cv, g, d[id].p, d_rho, n, sb, st);
            bool ok = ia == ib;
            if (ok && !ia) ok = g == G1 ? same(sa.p, d_gen2.p, sb.p, tau_g2) : same(d_gen1.p, sa.p, tau_g1, sb.p);
            if (!ok) F.add("not_powers", std::string("\"section\":\"") + SRS_SECTION[id] + "\"");
            sa.release(); sb.release();
        }
    }
    // 4. betaG2 carries the beta of betaTauG1
    if (bad[5] || bad[6]) skip("beta_mismatch", 6);
    else if (!same(d[5].p, d_gen2.p, d_gen1.p, d[6].p)) F.add("beta_mismatch", "\"section\":\"betaG2\"");
    ZK_HIP(hipStreamSynchronize(st));
    return std::string("{\"curve\":\"") + cv.name + "\",\"power\":" + std::to_string(srs.power) + ",\"checked\":{\"g1_points\":" + std::to_string(n_pts[G1]) +
           ",\"g2_points\":" + std::to_string(n_pts[G2]) + ",\"pairs\":" + std::to_string(same.pairs) + "},\"skipped\":[" + skipped + "]," + F.tail() + "}";
}

Groth16Key* groth16_keygen_from_srs(const char* curve, const void* r1cs, size_t r1cs_len, const Srs* srs) {
    using clk = std::chrono::steady_clock;
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(r1cs && srs, "groth16 setup: null input");
    ZK_REQUIRE(srs->curve == &cv, std::string("groth16 setup: the powers-of-tau file was opened for ") + srs->curve->name);
    const g16::R1cs rc = g16::parse_r1cs((const uint8_t*)r1cs, r1cs_len, cv);
    const g16::Circuit C(rc);
    ZK_REQUIRE((int)srs->power >= C.logm, "groth16 setup: the file has power " + std::to_string(srs->power) + ", the circuit's " + std::to_string(C.n_rows) +
                                               " rows need power " + std::to_string(C.logm));
    hipStream_t st = cur_stream();
    auto now = [&] { ZK_HIP(hipStreamSynchronize(st)); return clk::now(); };
    auto since = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const EcOps& E = cv.ec();
    const u64 m = C.m, nh = m - 1, nw = C.n_wires;
    const size_t P1 = cv.point_words(G1), P2 = cv.point_words(G2), B1 = 4 * P1, B2 = 4 * P2;
    const u64 n1 = 3 + 3 * nw + nh, n2 = 3 + nw;
    const u64 o_x = 3, o_h = o_x + nw, o_a = o_h + nh, o_b = o_a + nw;     // write_params' layout
    auto key = std::make_unique<Groth16Key>();
    key->curve = &cv;
    DevBuf pts1, pts2, tau1, tau2, al, be, d_one;
    pts1.reserve(n1 * B1); pts2.reserve(n2 * B2);
    u32 *p1 = (u32*)pts1.p, *p2 = (u32*)pts2.p;
    const uint8_t* f = srs->file.data();

    auto t0 = now();
    // vk: alpha_g1 beta_g1 [delta_g1 = G1] | beta_g2 [gamma_g2 = delta_g2 = G2]
    h2d_sync(p1, f + srs->off[4], B1); h2d_sync(p1 + P1, f + srs->off[5], B1); h2d_sync(p2, f + srs->off[6], B2);
    d_one.reserve(8);
    const u64 one = 1;
    h2d_sync(d_one.p, &one, 8);
    cv.group(G1).mul_generator_dev(d_one.u(), 1, p1 + 2 * P1, st);
    cv.group(G2).mul_generator_dev(d_one.u(), 1, p2 + P2, st);
    ZK_HIP(hipMemcpyAsync(p2 + 2 * P2, p2 + P2, B2, hipMemcpyDeviceToDevice, st));
    // h_i = [tau^i (tau^m - 1)] G1 = tauG1[i + m] - tauG1[i]
    tau1.reserve((2 * m - 1) * B1); tau2.reserve(m * B2); al.reserve(m * B1); be.reserve(m * B1);
    h2d_sync(tau1.p, f + srs->off[2], (2 * m - 1) * B1); h2d_sync(tau2.p, f + srs->off[3], m * B2);
    h2d_sync(al.p, f + srs->off[4], m * B1); h2d_sync(be.p, f + srs->off[5], m * B1);
    E.g[G1].diff((const u32*)tau1.p + m * P1, tau1.p, nh, p1 + o_h * P1, st);
    auto t1 = now();
    key->ms[2] = since(t0, t1);
    // [L_i]_1, [L_i]_2, [alpha L_i]_1, [beta L_i]_1: the first m powers are the coefficients' side of the evaluations at the domain
    group_ntt_dev(cv, G1, tau1.p, C.logm, true, st);
    group_ntt_dev(cv, G1, al.p, C.logm, true, st);
    group_ntt_dev(cv, G1, be.p, C.logm, true, st);
    auto t2 = now();
    group_ntt_dev(cv, G2, tau2.p, C.logm, true, st);
    auto t3 = now();
    key->ms[0] = since(t1, t2); key->ms[3] = since(t2, t3);
    // the circuit's matrices by columns
    DevBuf csc_ptr[3], csc_rows[3], csc_coef[3];
    EcCsc csc[3];
    for (int w = 0; w < 3; ++w) {
        std::vector<u64> ptr;
        std::vector<u32> rows, coef;
        g16::csc_of(C.mat[w], nw, ptr, rows, coef);
        const size_t nt = rows.size();
        csc_ptr[w].reserve(ptr.size() * 8); csc_rows[w].reserve(nt * 4 + 4); csc_coef[w].reserve(nt * 32 + 4);
        h2d_sync(csc_ptr[w].p, ptr.data(), ptr.size() * 8);
        if (nt) { h2d_sync(csc_rows[w].p, rows.data(), nt * 4); h2d_sync(csc_coef[w].p, coef.data(), nt * 32); }
        csc[w] = EcCsc{(const u64*)csc_ptr[w].p, (const u32*)csc_rows[w].p, (const u32*)csc_coef[w].p, nullptr};
    }
    auto with = [](EcCsc c, const void* base) { c.base = (const u32*)base; return c; };
    const EcCsc a_set[1] = {with(csc[0], tau1.p)}, b_set[1] = {with(csc[1], tau1.p)}, b2_set[1] = {with(csc[1], tau2.p)};
    const EcCsc x_set[3] = {with(csc[1], al.p), with(csc[0], be.p), with(csc[2], tau1.p)};   // alpha b_j + beta a_j + c_j
    E.g[G1].column_sums(a_set, 1, cv.r, (u32)nw, p1 + o_a * P1, st);
    E.g[G1].column_sums(b_set, 1, cv.r, (u32)nw, p1 + o_b * P1, st);
    E.g[G1].column_sums(x_set, 3, cv.r, (u32)nw, p1 + o_x * P1, st);
    auto t4 = now();
    E.g[G2].column_sums(b2_set, 1, cv.r, (u32)nw, p2 + 3 * P2, st);
    auto t5 = now();
    key->ms[1] = since(t3, t4); key->ms[3] += since(t4, t5);
    g16::write_params(cv, C, pts1, pts2, key->params, st);
    key->ms[4] = since(t5, clk::now());
    return key.release();
}

namespace g16 {
// where the sections of a key's bytes lie: offset and count of h and l, offsets of delta_g1 and delta_g2
struct KeyLayout { size_t delta_g1, delta_g2, h, l; u64 nh, nl; };
static KeyLayout key_layout(const Curve& cv, const Params& P) {
    const size_t B1 = cv.point_bytes(G1), B2 = cv.point_bytes(G2);
    KeyLayout L;
    L.delta_g1 = 2 * B1 + 2 * B2; L.delta_g2 = L.delta_g1 + B1;
    L.h = L.delta_g2 + B2 + 4 + P.ic.n * B1 + 4; L.nh = P.h.n;
    L.l = L.h + P.h.n * B1 + 4; L.nl = P.l.n;
    return L;
}
}  // namespace g16

void groth16_params_contribute(const char* curve, const void* params, size_t len, const uint64_t* delta, void* out) {
    using namespace g16;
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(params && out, "groth16 contribute: null argument");
    const Params P = parse_params((const uint8_t*)params, len, 4 * (int)cv.fq_words);
    const KeyLayout L = key_layout(cv, P);
    const FrHost F(cv);
    u64 k[8], t[4];                                                         // delta', 1 / delta': canonical
    struct KGuard { u64 *a, *b; ~KGuard() { wipe(a, 64); wipe(b, 32); } } k_guard{k, t};
    if (delta) {
        std::memcpy(k, delta, 32);
        u32 any = 0; for (int i = 0; i < 8; ++i) any |= ((const u32*)k)[i];
        ZK_REQUIRE(any && cv.fr_canonical((const u32*)k), "groth16 contribute: delta must be a non-zero canonical field element");
    } else draw_fr(cv, (u32*)k, "groth16 contribute");
    F.to_mont(k, t); F.inv(t, t); F.from_mont(t, k + 4);
    hipStream_t st = cur_stream();
    const size_t P1 = cv.point_words(G1), P2 = cv.point_words(G2), B1 = 4 * P1, B2 = 4 * P2;
    const int cw = (int)cv.fq_words;
    const u64 n1 = L.nh + L.nl + 1;                                         // [h | l | delta_g1]
    DevBuf d_k, g1, g2, be1, be2;
    d_k.reserve(64); g1.reserve(n1 * B1); g2.reserve(B2); be1.reserve(n1 * B1); be2.reserve(B2);
    struct Wipe { hipStream_t st; DevBuf* b; ~Wipe() { if (b->p) (void)hipMemsetAsync(b->p, 0, b->bytes, st); (void)hipStreamSynchronize(st); } } dev_wipe{st, &d_k};
    h2d_sync(d_k.p, k, 64);
    u32* q = (u32*)g1.p;
    if (L.nh) h2d_sync(q, P.h.w.data(), L.nh * B1);
    if (L.nl) h2d_sync(q + L.nh * P1, P.l.w.data(), L.nl * B1);
    h2d_sync(q + (L.nh + L.nl) * P1, P.vk[4].w.data(), B1);
    h2d_sync(g2.p, P.vk[5].w.data(), B2);
    const MsmOps& M = cv.msm();
    M.fq_canon_to_mont_dev(g1.p, n1 * 2, st); M.fq_canon_to_mont_dev(g2.p, 4, st);
    const u32* dk = (const u32*)d_k.p;
    cv.ec().g[G1].mul_scalar(q, L.nh + L.nl, dk + 8, q, st);
    cv.ec().g[G1].mul_scalar(q + (L.nh + L.nl) * P1, 1, dk, q + (L.nh + L.nl) * P1, st);
    cv.ec().g[G2].mul_scalar(g2.p, 1, dk, g2.p, st);
    M.fq_mont_to_canon_dev(g1.p, n1 * 2, st); M.fq_mont_to_canon_dev(g2.p, 4, st);
    points_to_be_dev((const u32*)g1.p, n1, cw, false, (u32*)be1.p, st);
    points_to_be_dev((const u32*)g2.p, 1, cw, true, (u32*)be2.p, st);
    std::vector<uint8_t> h1(n1 * B1), h2(B2);
    d2h_sync(h1.data(), be1.p, h1.size()); d2h_sync(h2.data(), be2.p, B2);
    uint8_t* o = (uint8_t*)out;
    std::memmove(o, params, len);
    if (L.nh) std::memcpy(o + L.h, h1.data(), L.nh * B1);
    if (L.nl) std::memcpy(o + L.l, h1.data() + L.nh * B1, L.nl * B1);
    std::memcpy(o + L.delta_g1, h1.data() + (L.nh + L.nl) * B1, B1);
    std::memcpy(o + L.delta_g2, h2.data(), B2);
}

std::string groth16_contribution_check(const char* curve, const void* old_params, size_t old_len, const void* new_params, size_t new_len,
                                       const uint8_t* seed, uint32_t max_findings) {
    using namespace g16;
    const Curve& cv = curve_of(curve, GROTH16_NAMES);
    ZK_REQUIRE(old_params && new_params, "groth16 contribution check: null argument");
    const Params A = parse_params((const uint8_t*)old_params, old_len, 4 * (int)cv.fq_words);
    const Params B = parse_params((const uint8_t*)new_params, new_len, 4 * (int)cv.fq_words);
    Findings F({"size", "changed", "coordinate_range", "not_on_curve", "not_in_subgroup", "infinity", "delta_mismatch", "not_scaled"}, max_findings);
    std::string skipped;
    hipStream_t st = cur_stream();
    const size_t P1 = cv.point_words(G1), P2 = cv.point_words(G2), B1 = 4 * P1, B2 = 4 * P2;
    const MsmOps& M = cv.msm();
    // 1. what a contribution leaves alone
    static const char* const vk_names[6] = {"alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "delta_g1", "delta_g2"};
    auto same_pv = [](const PointVec& x, const PointVec& y) { return x.n == y.n && x.w == y.w && x.inf == y.inf; };
    const struct { const char* name; const PointVec *a, *b; } fixed[8] = {{vk_names[0], &A.vk[0], &B.vk[0]}, {vk_names[1], &A.vk[1], &B.vk[1]}, {vk_names[2], &A.vk[2], &B.vk[2]},
                                                                         {vk_names[3], &A.vk[3], &B.vk[3]}, {"ic", &A.ic, &B.ic}, {"a", &A.a, &B.a},
                                                                         {"b_g1", &A.b_g1, &B.b_g1}, {"b_g2", &A.b_g2, &B.b_g2}};
    for (const auto& s : fixed) {
        if (s.a->n != s.b->n) F.add("size", std::string("\"section\":\"") + s.name + "\",\"have\":" + std::to_string(s.b->n) + ",\"want\":" + std::to_string(s.a->n));
        else if (!same_pv(*s.a, *s.b)) {
            const size_t pw = s.a->n ? s.a->w.size() / s.a->n : 1;
            u64 first = 0;
            while (first < s.a->n && s.a->inf[first] == s.b->inf[first] && std::equal(s.a->w.begin() + first * pw, s.a->w.begin() + (first + 1) * pw, s.b->w.begin() + first * pw)) ++first;
            F.add("changed", std::string("\"section\":\"") + s.name + "\",\"first_index\":" + std::to_string(first));
        }
    }
    // 2. the new delta: both points valid, and the same delta in both groups
    DevBuf d_res, d_gen1, d_gen2, d_one, od[2], nd[2];
    d_res.reserve(4 * 64); d_one.reserve(8); d_gen1.reserve(B1); d_gen2.reserve(B2);
    const u64 one = 1;
    h2d_sync(d_one.p, &one, 8);
    cv.group(G1).mul_generator_dev(d_one.u(), 1, d_gen1.p, st);
    cv.group(G2).mul_generator_dev(d_one.u(), 1, d_gen2.p, st);
    for (int g = 0; g < 2; ++g) {
        const size_t Bg = g ? B2 : B1;
        od[g].reserve(Bg + 4); nd[g].reserve(Bg + 4);
        h2d_sync(od[g].p, A.vk[4 + g].w.data(), Bg); h2d_sync(nd[g].p, B.vk[4 + g].w.data(), Bg);
        cv.pairing().points_check[g](nd[g].p, g ? P2 : P1, 1, 0, 1, d_res.u() + 8 * g, st);
        M.fq_canon_to_mont_dev(od[g].p, g ? 4 : 2, st); M.fq_canon_to_mont_dev(nd[g].p, g ? 4 : 2, st);
    }
    u64 res[4][8] = {};
    d2h_sync(res, d_res.p, 2 * 64);
    bool delta_bad = false;
    for (int g = 0; g < 2; ++g) {
        for (int c = 0; c < 4; ++c) delta_bad = delta_bad || res[g][2 * c];
        F.point_classes(vk_names[4 + g], res[g]);
    }
    PairEq same(cv, st);
    if (delta_bad) skipped += skipped_entry("delta_mismatch", "delta", "an invalid point");
    else if (!same(nd[0].p, d_gen2.p, d_gen1.p, nd[1].p)) F.add("delta_mismatch", "\"section\":\"delta\"");
    // 3. l and h: valid points, and l'_i delta' = l_i delta for all i at once -- e(sum rho_i l'_i, delta' G2) = e(sum rho_i l_i, delta G2).  Points at
    //    infinity (a wire no row mentions) stay where they were and take no part in the sums
    const struct { const char* name; const PointVec *a, *b; } scaled[2] = {{"l", &A.l, &B.l}, {"h", &A.h, &B.h}};
    for (int q = 0; q < 2; ++q) {
        const auto& s = scaled[q];
        if (s.a->n != s.b->n) { F.add("size", std::string("\"section\":\"") + s.name + "\",\"have\":" + std::to_string(s.b->n) + ",\"want\":" + std::to_string(s.a->n)); continue; }
        const u64 n = s.a->n;
        if (!n) continue;
        DevBuf dn, dold, d_rho, sa, sb;
        dn.reserve(n * B1 + 4); dold.reserve(n * B1 + 4);
        std::vector<u32> wa, wb;                                            // the finite points, side by side
        u64 kept = 0, first_inf_diff = n;
        for (u64 i = 0; i < n; ++i) {
            if (s.a->inf[i] != s.b->inf[i]) { if (first_inf_diff == n) first_inf_diff = i; continue; }
            if (s.a->inf[i]) continue;
            wa.insert(wa.end(), s.a->w.begin() + i * P1, s.a->w.begin() + (i + 1) * P1);
            wb.insert(wb.end(), s.b->w.begin() + i * P1, s.b->w.begin() + (i + 1) * P1);
            ++kept;
        }
        if (first_inf_diff != n) { F.add("not_scaled", std::string("\"section\":\"") + s.name + "\",\"first_index\":" + std::to_string(first_inf_diff)); continue; }
        if (!kept) continue;
        h2d_sync(dn.p, wb.data(), kept * B1); h2d_sync(dold.p, wa.data(), kept * B1);
        cv.pairing().points_check[G1](dn.p, P1, kept, 0, 1, d_res.u() + 8 * (2 + q), st);
        d2h_sync(res[2 + q], d_res.u() + 8 * (2 + q), 64);
        bool bad = false;
        for (int c = 0; c < 4; ++c) bad = bad || res[2 + q][2 * c];
        F.point_classes(s.name, res[2 + q]);
        if (bad || delta_bad) { skipped += (skipped.empty() ? "" : ",") + skipped_entry("not_scaled", s.name, "an invalid point"); continue; }
        M.fq_canon_to_mont_dev(dn.p, kept * 2, st); M.fq_canon_to_mont_dev(dold.p, kept * 2, st);
        rho_dev(seed, kept, d_rho, st, "groth16 contribution check");
        const bool ia = rlc(cv, G1, dn.p, d_rho, kept, sa, st), ib = rlc(cv, G1, dold.p, d_rho, kept, sb, st);
        bool ok = ia == ib;
        if (ok && !ia) ok = same(sa.p, nd[1].p, sb.p, od[1].p);
        if (!ok) F.add("not_scaled", std::string("\"section\":\"") + s.name + "\"");
    }
    ZK_HIP(hipStreamSynchronize(st));
    return std::string("{\"curve\":\"") + cv.name + "\",\"sections\":{\"h\":" + std::to_string(B.h.n) + ",\"l\":" + std::to_string(B.l.n) + "},\"checked\":{\"pairs\":" +
           std::to_string(same.pairs) + "},\"skipped\":[" + skipped + "]," + F.tail() + "}";
}
