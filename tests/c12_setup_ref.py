"""TEST INFRASTRUCTURE ONLY.  CPU restatement of the reference's compressor12 setup, line for line and serial:
  r1cs2plonk            recursion/src/r1cs2plonk.rs:50-227
  plonk_info / render   recursion/src/compressor12/plonk_setup.rs:54-79, :102-158, :172-207
  plonk_setup           plonk_setup.rs:210-768, the serial chain of swaps of :692-728 included
  write_exec            recursion/src/compressor12/compressor12_setup.rs:51-83
and a writer / reader of the R1CS container (algebraic/src/r1cs_file.rs:50-270) so that every test builds its circuit in
memory.  The reference holds no known-answer vector for this path (its one r1cs2plonk test is #[ignore]d and needs a file
it does not ship): PARITY UNPINNED beyond this restatement; tests/test_gpu_c12_setup.py adds the independent check (a proof
of the generated PIL over the generated constants must verify).  Nothing here touches the GPU or the product."""
import json
import struct

P = 0xFFFFFFFF00000001
R = (1 << 64) % P
K = 12275445934081160404                                  # helper.rs:16-23
TEMPLATES = ("CMulAdd", "Poseidon12", "EvPol4", "FFT4")


def root_of_unity(n_bits):                                # constant.rs:54-68 MG.0[n_bits]
    w = pow(7, 0xFFFFFFFF, P)
    for _ in range(32 - n_bits):
        w = w * w % P
    return w


# ---- the R1CS container ---------------------------------------------------------------------------------------------------
def write_r1cs(n_wires, n_pub_out, n_pub_in, n_prv_in, constraints, custom_gates=(), custom_uses=(), field_size=8, prime=P,
               section_order=None):
    """constraints: [(A, B, C)] with each side a list of (wire, coefficient); custom_gates: [(name, [parameters])];
    custom_uses: [(id, [signals])] -> the bytes of a .r1cs file"""
    fe = lambda v: int(v).to_bytes(field_size, "little")
    head = struct.pack("<I", field_size) + fe(prime) + struct.pack("<IIIIQI", n_wires, n_pub_out, n_pub_in, n_prv_in, n_wires, len(constraints))
    cons = b""
    for abc in constraints:
        for lc in abc:
            cons += struct.pack("<I", len(lc)) + b"".join(struct.pack("<I", w) + fe(c) for w, c in lc)
    secs = {1: head, 2: cons, 3: b"".join(struct.pack("<Q", i) for i in range(n_wires))}
    if custom_gates or custom_uses:
        secs[4] = struct.pack("<I", len(custom_gates)) + b"".join(
            name.encode() + b"\0" + struct.pack("<I", len(ps)) + b"".join(fe(p) for p in ps) for name, ps in custom_gates)
        secs[5] = struct.pack("<I", len(custom_uses)) + b"".join(
            struct.pack("<II", gid, len(sig)) + b"".join(struct.pack("<II", s & 0xFFFFFFFF, s >> 32) for s in sig) for gid, sig in custom_uses)
    order = section_order or sorted(secs)
    out = b"r1cs" + struct.pack("<II", 1, len(order))
    for t in order:
        out += struct.pack("<IQ", t, len(secs[t])) + secs[t]
    return out


def read_r1cs(b):
    """r1cs_file.rs:185-270 + reader.rs:198-214 -> dict"""
    assert b[:4] == b"r1cs", "Invalid magic number"
    version, n_sec = struct.unpack_from("<II", b, 4)
    assert version == 1
    o, secs = 12, {}
    for _ in range(n_sec):
        t, sz = struct.unpack_from("<IQ", b, o); o += 12
        secs[t] = b[o:o + sz]; o += sz
    h = secs[1]
    fs = struct.unpack_from("<I", h)[0]
    assert fs == 8 and int.from_bytes(h[4:12], "little") == P, "Different prime"
    n_wires, n_pub_out, n_pub_in, n_prv_in, _labels, n_cons = struct.unpack_from("<IIIIQI", h, 12)
    c, o, constraints = secs[2], 0, []
    for _ in range(n_cons):
        abc = []
        for _ in range(3):
            n = struct.unpack_from("<I", c, o)[0]; o += 4
            lc = []
            for _ in range(n):
                w, v = struct.unpack_from("<IQ", c, o); o += 12
                assert v < P
                lc.append((w, v))
            abc.append(sorted(lc, key=lambda t: t[0]))                  # r1cs_file.rs:83
        constraints.append(tuple(abc))
    gates, uses = [], []
    if 4 in secs:
        g, o = secs[4], 4
        for _ in range(struct.unpack_from("<I", g)[0]):
            e = g.index(b"\0", o); name = g[o:e].decode(); o = e + 1
            n = struct.unpack_from("<I", g, o)[0]; o += 4
            gates.append((name, [struct.unpack_from("<Q", g, o + 8 * i)[0] for i in range(n)])); o += 8 * n
    if 5 in secs:
        w = struct.unpack("<%dI" % (len(secs[5]) // 4), secs[5])
        pos = 1
        for _ in range(w[0]):
            gid, n = w[pos], w[pos + 1]; pos += 2
            uses.append((gid, [w[pos + 2 * j + 1] * 0x100000000 + w[pos + 2 * j] for j in range(n)])); pos += 2 * n
    return {"num_inputs": 1 + n_pub_in + n_pub_out, "num_outputs": n_pub_out, "num_variables": n_wires, "constraints": constraints,
            "custom_gates": gates, "custom_gates_uses": uses}


# ---- r1cs2plonk.rs:50-227 ----------------------------------------------------------------------------------------------------
def r1cs2plonk(r1cs):
    """-> (gates [(sl, sr, so, qm, ql, qr, qo, qc)], additions [(a, b, ca, cb)]); BTreeMap = a dict walked in key order"""
    n_var = [r1cs["num_variables"]]
    pc, pa = [], []
    items = lambda lc: sorted(lc.items())

    def normalize(lc):
        for k in [k for k, v in lc.items() if v == 0]: del lc[k]

    def join(lc1, k, lc2):
        res = {}
        for key, val in items(lc1): res[key] = (k * val + res.get(key, 0)) % P
        for key, val in items(lc2): res[key] = (val + res.get(key, 0)) % P
        normalize(res)
        return res

    def reduce_coefs(lc, max_c):
        k, cs = 0, []
        for key, val in items(lc):
            if key == 0: k = (k + val) % P
            elif val != 0: cs.append((key, val))
        while len(cs) > max_c:
            c1 = cs.pop(0); c2 = cs.pop(0)
            so = n_var[0]; n_var[0] += 1
            pc.append((c1[0], c2[0], so, 0, -c1[1] % P, -c2[1] % P, 1, 0))
            pa.append((c1[0], c2[0], c1[1], c2[1]))
            cs.append((so, 1))
        s, c = [x[0] for x in cs], [x[1] for x in cs]
        while len(c) < max_c: s.append(0); c.append(0)
        return k, s, c

    def add_constraint_mul(la, lb, lc):
        A = reduce_coefs(la, 1); B = reduce_coefs(lb, 1); C = reduce_coefs(lc, 1)
        pc.append((A[1][0], B[1][0], C[1][0], A[2][0] * B[2][0] % P, A[2][0] * B[0] % P, A[0] * B[2][0] % P, -C[2][0] % P, (A[0] * B[0] - C[0]) % P))

    def add_constraint_sum(lc):
        C = reduce_coefs(lc, 3)
        pc.append((C[1][0], C[1][1], C[1][2], 0, C[2][0], C[2][1], C[2][2], C[0]))

    def to_map(lc):
        res = {}
        for w, v in lc:
            assert w not in res
            res[w] = v
        return res

    def lc_type(lc):
        k, n = 0, 0
        for key in sorted(lc):
            if lc[key] == 0: del lc[key]
            elif key == 0: k = (k + lc[key]) % P
            else: n += 1
        return str(n) if n > 0 else ("k" if k != 0 else "0")

    for c in r1cs["constraints"]:
        la, lb, lc = to_map(c[0]), to_map(c[1]), to_map(c[2])
        ta, tb = lc_type(la), lc_type(lb)
        if ta == "0" or tb == "0":
            normalize(lc); add_constraint_sum(lc)
        elif ta == "k": add_constraint_sum(join(lb, la[0], lc))
        elif tb == "k": add_constraint_sum(join(la, lb[0], lc))
        else: add_constraint_mul(la, lb, lc)
    return pc, pa


def str_key(g):                                           # r1cs2plonk.rs:30-39
    return ",".join("%x" % v for v in g[3:8])


def log2_any(v):
    return v.bit_length() - 1 if v else 0


# ---- plonk_setup.rs ------------------------------------------------------------------------------------------------------------
COLS = ["PARTIAL", "POSEIDON12", "GATE", "CMULADD", "EVPOL4", "FFT4"]


def plonk_setup(r1cs, cposeidon, force_n_bits=0):
    """-> dict(n_bits, n_publics, n_used, n_const, gates, adds, s_map [12][n_used], const [N][n_const] as a list of rows).
    cposeidon: the 372 row constants (the caller brings the project's own table)."""
    pg, pa = r1cs2plonk(r1cs)
    uses = {}
    for g in pg: uses[str_key(g)] = uses.get(str_key(g), 0) + 1                                       # :54-78
    n_plonk = sum((u - 1) // 2 + 1 for u in uses.values())
    n_plonk = (n_plonk - 1) // 2 + 1
    cmuladd_id = poseidon_id = evpol_id = 0                                                           # :102-128
    fft_params = {}
    for i, (name, params) in enumerate(r1cs["custom_gates"]):
        if name == "CMulAdd": cmuladd_id = i; assert not params
        elif name == "Poseidon12": poseidon_id = i; assert not params
        elif name == "EvPol4": evpol_id = i; assert not params
        elif name == "FFT4": fft_params[i] = params
        else: raise ValueError("Invalid custom gate " + name)
    n_cmuladd = n_poseidon = n_fft = n_evpol = 0                                                      # :130-146
    for gid, _ in r1cs["custom_gates_uses"]:
        if gid == cmuladd_id: n_cmuladd += 1
        elif gid == poseidon_id: n_poseidon += 1
        elif gid in fft_params: n_fft += 1
        elif gid == evpol_id: n_evpol += 1
        else: raise ValueError("Custom gate not defined %d" % gid)
    n_publics = r1cs["num_inputs"] + r1cs["num_outputs"] - 1                                          # :183-197
    n_public_rows = (n_publics - 1) // 12 + 1
    n_used = n_public_rows + n_plonk + n_cmuladd + n_poseidon * 31 + n_fft * 2 + n_evpol * 2
    n_bits = log2_any(n_used - 1) + 1
    if force_n_bits > 0: n_bits = force_n_bits
    N = 1 << n_bits
    # the PIL's constant columns, in declaration order (compressor12_pil.rs:50-82)
    col = {("L%d" % (i + 1), 0): i for i in range(n_public_rows)}
    nc = n_public_rows
    for j in range(12): col[("S", j)] = nc + j
    for j in range(12): col[("C", j)] = nc + 12 + j
    for j, name in enumerate(COLS): col[(name, 0)] = nc + 24 + j
    n_const = nc + 30
    const = [[0] * n_const for _ in range(N)]

    def put(name, k, row, v): const[row][col[(name, k)]] = v % P

    s_map = [[0] * n_used for _ in range(12)]
    r = 0
    for i in range(n_public_rows):                                                                    # :230-252
        for name in COLS: put(name, 0, r + i, 0)
        for k in range(12): put("C", k, r + i, 0)
    for i in range(n_publics): s_map[i % 12][r + i // 12] = 1 + i
    for i in range(n_publics, n_public_rows * 12): s_map[i % 12][r + i // 12] = 0
    r += n_public_rows
    partial_rows, half_rows = {}, []                                                                  # :268-343
    for c in pg:
        k = str_key(c)
        pr = partial_rows.get(k)
        if pr is not None:
            for t in range(3): s_map[pr["n_used"] * 3 + t][pr["row"]] = c[t]
            pr["n_used"] += 1
            if pr["n_used"] == 2:
                half_rows.append(dict(pr)); del partial_rows[k]
            elif pr["n_used"] == 4:
                del partial_rows[k]
        elif half_rows:
            pr = half_rows.pop(0)
            for i, v in zip([9, 6, 7, 8, 10, 11], [c[3], c[4], c[5], c[6], c[7], 0]): put("C", i, pr["row"], v)
            for t in range(3): s_map[pr["n_used"] * 3 + t][pr["row"]] = c[t]
            pr["n_used"] += 1
            partial_rows[k] = pr
        else:
            for i, v in zip([3, 0, 1, 2, 4, 5], [c[3], c[4], c[5], c[6], c[7], 0]): put("C", i, r, v)
            for name, v in zip(["GATE", "POSEIDON12", "PARTIAL", "CMULADD", "EVPOL4", "FFT4"], [1, 0, 0, 0, 0, 0]): put(name, 0, r, v)
            for t in range(3): s_map[t][r] = c[t]
            partial_rows[k] = {"row": r, "n_used": 1}
            r += 1
    for k in sorted(partial_rows):                                                                    # :346-360 (BTreeMap<String, _> order)
        pr = partial_rows[k]
        if pr["n_used"] == 1:
            for t in range(3): s_map[3 + t][pr["row"]] = s_map[t][pr["row"]]
            pr["n_used"] += 1
            half_rows.append(dict(pr))
        elif pr["n_used"] == 3:
            for t in range(3): s_map[9 + t][pr["row"]] = s_map[6 + t][pr["row"]]
        else:
            raise AssertionError("meet error when terminate the empty rows")
    for hr in half_rows:                                                                              # :362-379
        for t in range(6, 12): s_map[t][hr["row"]] = 0
        for i in [9, 6, 7, 8, 10, 11]: put("C", i, hr["row"], 0)
    for gid, sig in r1cs["custom_gates_uses"]:                                                        # :383-663
        if gid == poseidon_id:
            assert len(sig) == 31 * 12
            for j in range(31):
                for k in range(12):
                    s_map[k][r + j] = sig[j * 12 + k]
                    put("C", k, r + j, cposeidon[j * 12 + k])
                for name in ["GATE", "CMULADD", "EVPOL4", "FFT4"]: put(name, 0, r + j, 0)
                put("POSEIDON12", 0, r + j, 1 if j < 30 else 0)
                tt = 0 if not (4 <= j < 26) else 1
                put("PARTIAL", 0, r + j, tt if j < 30 else 0)
            r += 31
        elif gid == cmuladd_id:
            if r < n_used:
                for j in range(12): s_map[j][r] = sig[j]
            for name in ["GATE", "POSEIDON12", "PARTIAL", "EVPOL4", "FFT4"]: put(name, 0, r, 0)
            put("CMULADD", 0, r, 1)
            for i in range(12): put("C", i, r, 1 if i in (9, 10) else 0)
            r += 1
        elif gid in fft_params:
            for j in range(12):
                s_map[j][r] = sig[j]; s_map[j][r + 1] = sig[12 + j]
            for name in ["GATE", "POSEIDON12", "CMULADD", "PARTIAL", "EVPOL4"]: put(name, 0, r, 0)
            put("FFT4", 0, r, 1)
            for name in COLS: put(name, 0, r + 1, 0)
            first_w, inc_w, scale, t = fft_params[gid]
            first_w2 = first_w * first_w % P
            if t == 4:
                for i in [6, 7, 8]: put("C", i, r, 0)
                for i, v in enumerate([scale, scale * first_w2, scale * first_w, scale * first_w * first_w2, scale * first_w * inc_w,
                                       scale * first_w * first_w2 * inc_w]): put("C", i, r, v)
            elif t == 2:
                for i in range(6): put("C", i, r, 0)
                for i, v in zip([6, 7, 8], [scale, scale * first_w, scale * first_w * inc_w]): put("C", i, r, v)
            else:
                raise ValueError("invalid FFT4 type: %d" % t)
            for i in [9, 10, 11]: put("C", i, r, 0)
            for k in range(12): put("C", k, r + 1, 0)
            r += 2
        elif gid == evpol_id:
            for j in range(12):
                s_map[j][r] = sig[j]; put("C", j, r, 0)
            for j in range(9):
                s_map[j][r + 1] = sig[12 + j]; put("C", j, r + 1, 0)
            for j in range(9, 12):
                s_map[j][r + 1] = 0; put("C", j, r + 1, 0)
            for name in ["GATE", "POSEIDON12", "CMULADD", "PARTIAL", "FFT4"]: put(name, 0, r, 0)
            put("EVPOL4", 0, r, 1)
            for name in COLS: put(name, 0, r + 1, 0)
            r += 2
        else:
            raise ValueError("Custom gate not defined: %d" % gid)
    connect_s(const, s_map, n_used, r, n_bits, n_const, col[("S", 0)])                                # :665-728
    while r < N:                                                                                      # :731-757
        for name in COLS: put(name, 0, r, 0)
        for k in range(12): put("C", k, r, 0)
        r += 1
    for i in range(n_public_rows):                                                                    # :759-765
        for j in range(N): put("L%d" % (i + 1), 0, j, 0)
        put("L%d" % (i + 1), 0, i, 1)
    return {"n_bits": n_bits, "n_publics": n_publics, "n_used": n_used, "n_const": n_const, "gates": pg, "adds": pa, "s_map": s_map, "const": const}


def connect_s(const, s_map, n_used, r, n_bits, n_const, col0):
    """plonk_setup.rs:665-728: the identity S[j][i] = w^i ks[j-1] by a running power, then the serial chain of swaps.
    s_map: [12][n_used]; writes columns [col0, col0 + 12) of const (a list of N rows)"""
    ks = [K]
    for _ in range(10): ks.append(ks[-1] * K % P)
    w, wn = 1, root_of_unity(n_bits)
    for i in range(1 << n_bits):
        const[i][col0] = w
        for j in range(1, 12): const[i][col0 + j] = w * ks[j - 1] % P
        w = w * wn % P
    last_signal = {}
    for i in range(r):
        for j in range(12):
            if i < n_used:
                key = s_map[j][i]
                if key == 0: continue
                ls = last_signal.get(key)
                if ls is not None:
                    left, right = const[ls[0]][col0 + ls[1]], const[i][col0 + j]
                    const[i][col0 + j] = left
                    const[ls[0]][col0 + ls[1]] = right
                else:
                    last_signal[key] = (i, j)


def sigma(s_map_rows, n_bits):
    """the wiring alone for a [n_used][12] map (the .exec order) -> [N][12] rows"""
    n_used = len(s_map_rows)
    const = [[0] * 12 for _ in range(1 << n_bits)]
    connect_s(const, [[row[j] for row in s_map_rows] for j in range(12)], n_used, n_used, n_bits, 12, 0)
    return const


def write_exec(adds, s_map):
    """compressor12_setup.rs:51-83 (coefficients as the raw words of an FGL: value * 2^64 mod p; serde_json's compact form)"""
    assert len(s_map) == 12, "s_map should have 12 rows"
    n = len(s_map[0])
    buff = [0] * (2 + len(adds) * 4 + 12 * n)
    buff[0], buff[1] = len(adds), n
    for i, (a, b, ca, cb) in enumerate(adds):
        buff[2 + i * 4: 6 + i * 4] = [a, b, ca * R % P, cb * R % P]
    for c in range(12):
        for i in range(n):
            buff[2 + len(adds) * 4 + 12 * i + c] = s_map[c][i]
    return json.dumps(buff, separators=(",", ":"))


def project_cposeidon():
    """the project's own table of the 372 Poseidon12 row constants (tools/poseidong_round_constants.h)"""
    import pathlib, re
    text = (pathlib.Path(__file__).resolve().parent.parent / "tools" / "poseidong_round_constants.h").read_text()
    v = [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", text)]
    assert len(v) == 372
    return v
