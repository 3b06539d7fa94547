"""TEST INFRASTRUCTURE ONLY.  The yardstick of zk_groth16_key_check_srs (include/zkgpu.h) where the test knows the trapdoor: build the key
the CPU oracle's generate_parameters restatement gives for (tau, alpha, beta, gamma, delta) and compare the key under test with it
section by section, point by point.  Same `findings` and `counts` as the device's report: per section the first index that differs and,
through the density order of the section (bellman's trackers: every input, then the other wires that meet an A row; every wire that
meets a B row), the wire it stands for.  It does not restate the randomised check: no weights, no sums, no pairings.  A section whose
length differs from the oracle's is not compared (the device lists it under "skipped").  Nothing here touches the GPU or the product."""
import struct

SECTIONS = ("a", "b_g1", "b_g2", "ic", "l", "h")                             # the order of the report
VK_FIELDS = ("alpha_g1", "beta_g1", "beta_g2")
_cache = {}


def layout(g, pb):
    """bellman's Parameters bytes -> {name: (count, offset of the first point, bytes per point)}; g: oracle/groth16.Groth16Oracle"""
    s1, s2 = 16 * g.nl, 32 * g.nl
    o, out = 0, {}
    for name, sz in (("alpha_g1", s1), ("beta_g1", s1), ("beta_g2", s2), ("gamma_g2", s2), ("delta_g1", s1), ("delta_g2", s2)):
        out[name] = (1, o, sz); o += sz
    for name, sz in (("ic", s1), ("h", s1), ("l", s1), ("a", s1), ("b_g1", s1), ("b_g2", s2)):
        n = struct.unpack(">I", pb[o:o + 4])[0]
        out[name] = (n, o + 4, sz); o += 4 + n * sz
    assert o == len(pb)
    return out


def get(g, pb, name, i):
    n, o, sz = layout(g, pb)[name]
    return pb[o + (i % n) * sz:o + (i % n + 1) * sz]


def put(g, pb, name, i, data):
    """the key with entry i of a section replaced by an encoded point"""
    n, o, sz = layout(g, pb)[name]
    assert len(data) == sz
    return pb[:o + (i % n) * sz] + data + pb[o + (i % n + 1) * sz:]


def swap(g, pb, name, i, j):
    return put(g, put(g, pb, name, i, get(g, pb, name, j)), name, j, get(g, pb, name, i))


def split_key(g, pb):
    """-> {name: [the encoded bytes of each point]}"""
    return {name: [pb[o + i * sz:o + (i + 1) * sz] for i in range(n)] for name, (n, o, sz) in layout(g, pb).items()}


def wires(g, r1cs):
    """{section: the wire of each entry} (h: None)"""
    cir = g.circuit(r1cs)
    ni = cir["num_inputs"]
    a_aux, b_in, b_aux = g.densities(cir)
    wa, wb = list(range(ni)) + a_aux, b_in + b_aux
    return {"a": wa, "b_g1": wb, "b_g2": wb, "ic": list(range(ni)), "l": list(range(ni, cir["n_wires"])), "h": None}


def oracle_key(g, r1cs, trapdoor):
    """the oracle's key bytes for this circuit and trapdoor (remembered: the cases of a test share it and leave it unchanged)"""
    key = (g.curve, id(r1cs), tuple(trapdoor))
    if key not in _cache:
        _cache[key] = (r1cs, g.params_bytes(g.setup(r1cs, *trapdoor)))       # r1cs is kept so that its id stays its own
    return _cache[key][1]


def report(g, r1cs, params_bytes, trapdoor, max_findings=16):
    """trapdoor: (tau, alpha, beta) of the powers-of-tau file, then the key's gamma and delta"""
    want, have = split_key(g, oracle_key(g, r1cs, trapdoor)), split_key(g, params_bytes)
    w = wires(g, r1cs)
    queries, vks = [], []
    for name in SECTIONS:
        if len(have[name]) != len(want[name]): continue
        k = next((i for i, (x, y) in enumerate(zip(have[name], want[name])) if x != y), None)
        if k is None: continue
        f = dict(kind="query_mismatch", section=name, first_index=k)
        if w[name] is not None: f["wire"] = w[name][k]
        queries.append(f)
    for name in VK_FIELDS:
        if have[name] != want[name]: vks.append(dict(kind="vk_mismatch", field=name))
    return dict(counts=dict(query_mismatch=len(queries), vk_mismatch=len(vks)), findings=queries[:max_findings] + vks[:max_findings])
