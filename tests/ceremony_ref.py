"""The powers-of-tau ceremony's transcript in plain Python (hashlib, integers, the oracle's CPU curve): what csrc/ceremony_host.h and
csrc/groth16_ceremony.hip.h do, restated from the layout in include/zkgpu.h and DESIGN.md 3.17 -- container walk, record parsing, chain
hashes, challenges, beacon scalars, the Schnorr equation, and a builder of records from known secrets and nonces.

A transcript is section 64 of the .ptau container: u32 version = 1, u32 count, then records of
  u32 kind | u32 iter_log | 32 B seed | 3 images (G1 points, file layout) | 3 x (R, z of 32 B little-endian) | 32 B chain hash."""
import hashlib, struct
import numpy as np

SECTION = 64
WHICH = ("tau", "alpha", "beta")
B1 = {"BN128": 64, "BLS12381": 96}
R = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}


class TranscriptError(ValueError):
    pass


def sha(*parts):
    return hashlib.sha256(b"".join(parts)).digest()


def sections(file_bytes):
    """[(id, offset of the payload, size)] of a .ptau container"""
    if file_bytes[:4] != b"ptau":
        raise TranscriptError("ptau: Invalid magic number")
    n_sec = struct.unpack_from("<I", file_bytes, 8)[0]
    out, o = [], 12
    for _ in range(n_sec):
        if len(file_bytes) - o < 12:
            raise TranscriptError("ptau: truncated file")
        sid, size = struct.unpack_from("<IQ", file_bytes, o)
        o += 12
        if size > len(file_bytes) - o:
            raise TranscriptError("ptau: truncated file")
        out.append((sid, o, size)); o += size
    return out


def section(file_bytes, sid):
    for s, o, size in sections(file_bytes):
        if s == sid:
            return file_bytes[o:o + size]
    return None


def rec_bytes(b1):
    return 8 + 32 + 3 * b1 + 3 * (b1 + 32) + 32


def parse(payload, b1):
    """the records of a transcript payload as dicts of bytes"""
    if len(payload) < 8:
        raise TranscriptError("ptau transcript: truncated section")
    version, count = struct.unpack_from("<II", payload, 0)
    if version != 1:
        raise TranscriptError("ptau transcript: Unsupported version")
    rb = rec_bytes(b1)
    if (len(payload) - 8) // rb < count:
        raise TranscriptError("ptau transcript: truncated section")
    if len(payload) - 8 != count * rb:
        raise TranscriptError("ptau transcript: bytes behind the last record")
    out = []
    for i in range(count):
        q = payload[8 + i * rb:8 + (i + 1) * rb]
        kind, it = struct.unpack_from("<II", q, 0)
        if kind > 1:
            raise TranscriptError("ptau transcript: unknown kind")
        o = 40
        img = [q[o + j * b1:o + (j + 1) * b1] for j in range(3)]; o += 3 * b1
        proofs = [(q[o + j * (b1 + 32):o + j * (b1 + 32) + b1], q[o + j * (b1 + 32) + b1:o + (j + 1) * (b1 + 32)]) for j in range(3)]
        out.append(dict(kind=kind, iter_log=it, seed=q[8:40], img=img, R=[p[0] for p in proofs], z=[p[1] for p in proofs], hash=q[-32:], body=q[:-32]))
    return out


def chain_start(n8, power):
    return sha(b"zkgpu ptau transcript v1", struct.pack("<II", n8, power))


def record_hash(prev, body):
    return sha(b"zkgpu rec v1", prev, body)


def challenge(prev, j, base, image, commit):
    return int.from_bytes(sha(b"zkgpu pok v1", prev, bytes([j]), base, image, commit)[:16], "little")


def beacon_scalars(seed, iter_log):
    d = seed
    for _ in range(1 << iter_log):
        d = hashlib.sha256(d).digest()
    return [int.from_bytes(sha(d, bytes([j])), "little") & ((1 << 253) - 1) for j in range(3)]


def serialize(records):
    """records as parse() gives them (body and hash) -> the section's payload"""
    return struct.pack("<II", 1, len(records)) + b"".join(r["body"] + r["hash"] for r in records)


def body_of(r):
    return struct.pack("<II", r["kind"], r["iter_log"]) + r["seed"] + b"".join(r["img"]) + b"".join(R_ + z for R_, z in zip(r["R"], r["z"]))


def rehash(records, n8, power):
    """bodies rebuilt from the fields and the chain recomputed: what a forger who edits a field would do"""
    prev = chain_start(n8, power)
    for r in records:
        r["body"] = body_of(r); r["hash"] = prev = record_hash(prev, r["body"])
    return records


def replace_section(file_bytes, sid, payload):
    """the container with section sid's payload replaced"""
    out = bytearray(file_bytes[:12])
    for s, o, size in sections(file_bytes):
        body = payload if s == sid else file_bytes[o:o + size]
        out += struct.pack("<IQ", s, len(body)) + body
    return bytes(out)


class Curve:
    """the oracle's CPU curve behind points in the file's layout (bytes of little-endian u64 Montgomery words; all zero = infinity)"""

    def __init__(self, g16, tag):
        self.g, self.tag, self.r, self.b1 = g16, tag, R[tag], B1[tag]

    def _pt(self, b):
        return None if not any(b) else np.frombuffer(b, dtype="<u8").astype(np.uint64)

    def _bytes(self, p):
        return bytes(self.b1) if p is None else np.asarray(p, dtype="<u8").tobytes()

    def mul(self, point_bytes, k):
        return self._bytes(self.g.mul(self.g.g1, self._pt(point_bytes), k))

    def lin2(self, p, a, q, b):
        """[a]p + [b]q"""
        return self._bytes(self.g.msm(self.g.g1, [self._pt(p), self._pt(q)], [a, b]))


def make_record(cv, prev_hash, bases, secrets, nonces, kind=0, iter_log=0, seed=bytes(32)):
    """a record from known factors and nonces, as srs_contribute builds it"""
    img = [cv.mul(b, s) for b, s in zip(bases, secrets)]
    Rs = [cv.mul(b, n) for b, n in zip(bases, nonces)]
    zs = [((n + challenge(prev_hash, j, bases[j], img[j], Rs[j]) * s) % cv.r).to_bytes(32, "little") for j, (s, n) in enumerate(zip(secrets, nonces))]
    r = dict(kind=kind, iter_log=iter_log, seed=seed, img=img, R=Rs, z=zs)
    r["body"] = body_of(r); r["hash"] = record_hash(prev_hash, r["body"])
    return r


def check(cv, records, n8, power, gen1, file_images=None):
    """the findings of zk_srs_verify's transcript part as a sorted list of (kind, contribution, which or None); file_images: the file's
    (tauG1[1] or None, alphaTauG1[0], betaTauG1[0])"""
    out = []
    prev = chain_start(n8, power)
    bases = [gen1] * 3
    for i, r in enumerate(records):
        h = record_hash(prev, r["body"])
        if h != r["hash"]:
            out.append(("chain_hash", i + 1, None))
        for j in range(3):
            z = int.from_bytes(r["z"][j], "little")
            c = challenge(prev, j, bases[j], r["img"][j], r["R"][j])
            ok = z < cv.r and any(r["img"][j])
            if ok:
                try:
                    ok = cv.lin2(bases[j], z, r["img"][j], cv.r - c) == r["R"][j]
                except Exception:
                    ok = False
            if not ok:
                out.append(("pok_invalid", i + 1, WHICH[j]))
            if r["kind"] == 1:
                try:
                    same = cv.mul(bases[j], beacon_scalars(r["seed"], r["iter_log"])[j]) == r["img"][j]
                except Exception:
                    same = False
                if not same:
                    out.append(("beacon_mismatch", i + 1, WHICH[j]))
        prev, bases = h, r["img"]
    if file_images is not None:
        for j in range(3):
            if file_images[j] is not None and file_images[j] != bases[j]:
                out.append(("image_mismatch", len(records), WHICH[j]))
    return sorted(out, key=lambda t: (t[0], t[1], t[2] or ""))
