"""TEST INFRASTRUCTURE ONLY.  Circuits and damaged keys for the groth16_key_check tests: byte surgery on bellman's Parameters layout."""
import pathlib
import struct
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
import key_check_ref as K  # noqa: E402


def circuit(r, n_mul, seed=5):
    """oracle/groth16.synthetic_r1cs without its last wire, which no row mentions (its `l` entry is the point at infinity, and
    a key that holds one is not clean)"""
    r1cs, w = G.synthetic_r1cs(r, n_mul, seed=seed)
    r1cs = dict(r1cs, n_wires=r1cs["n_wires"] - 1)
    return r1cs, w[:-1]


def layout(tag, pb):
    """-> {section: (count, offset of the first point, bytes per point)}, {"count:" + section: offset of its count}"""
    cb = K.CURVES[tag].coord_bytes
    s1, s2 = 2 * cb, 4 * cb
    o, out = 0, {}
    for name, g in K.VK_POINTS:
        out[name] = (1, o, s2 if g else s1); o += s2 if g else s1
    for name in ("ic", "h", "l", "a", "b_g1", "b_g2"):
        n = struct.unpack(">I", pb[o:o + 4])[0]
        sz = s2 if name == "b_g2" else s1
        out["count:" + name] = o; out[name] = (n, o + 4, sz); o += 4 + n * sz
    assert o == len(pb)
    return out


def get_point(tag, pb, section, i):
    n, o, sz = layout(tag, pb)[section]
    if i < 0: i += n
    cb = K.CURVES[tag].coord_bytes
    v = [int.from_bytes(pb[o + i * sz + k * cb:o + i * sz + (k + 1) * cb], "big") for k in range(sz // cb)]
    return (v[1], v[0], v[3], v[2]) if sz == 4 * cb else tuple(v)


def set_point(tag, pb, section, i, coords):
    """coords: canonical integers (G2: x.c0, x.c1, y.c0, y.c1), or None for the infinity encoding"""
    n, o, sz = layout(tag, pb)[section]
    if i < 0: i += n
    cb = K.CURVES[tag].coord_bytes
    if coords is None: enc = bytes([0x40]) + bytes(sz - 1)
    else:
        v = (coords[1], coords[0], coords[3], coords[2]) if sz == 4 * cb else coords
        enc = b"".join(int(x).to_bytes(cb, "big") for x in v)
    return pb[:o + i * sz] + enc + pb[o + (i + 1) * sz:]


def truncate(tag, pb, section, drop):
    """the section without its last `drop` points, its count fixed up"""
    L = layout(tag, pb)
    n, o, sz = L[section]
    return pb[:L["count:" + section]] + struct.pack(">I", n - drop) + pb[o:o + (n - drop) * sz] + pb[o + n * sz:]


def off_curve(tag, pb, section, i):
    c = list(get_point(tag, pb, section, i)); c[-1] = (c[-1] + 1) % K.CURVES[tag].q
    return set_point(tag, pb, section, i, c)


def doubled(tag, pb, section, i):
    C = K.CURVES[tag]; g = 1 if section.endswith("g2") else 0
    c = get_point(tag, pb, section, i)
    p = ((c[0], c[1]), (c[2], c[3])) if g else ((c[0], 0), (c[1], 0))
    return set_point(tag, pb, section, i, C.coords(C.add(p, p), g))


def twist_point_outside_subgroup(tag):
    C = K.CURVES[tag]; x = 1
    while True:
        p = C.lift_x((x, 1), 1); x += 1
        if p and C.mul(p, C.r) is not None: return C.coords(p, 1)
