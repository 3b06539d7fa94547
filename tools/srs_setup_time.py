"""Setup from a powers-of-tau file against setup from a trapdoor: python tools/srs_setup_time.py [log2_rows] [BN128|BLS12381 ...]

For each curve: tools/groth16_bench.make_circuit at 2^k rows (default 16), a file of power k from tools/make_test_ptau.py (known trapdoor:
timing only), then wall clock and the library's own split (zk_groth16_keygen_timing) of
  file      zk_groth16_keygen_from_srs: G1 transforms | G1 column sums | uploads and h differences | G2 transform and sums | serialisation
  trapdoor  zk_groth16_keygen_new:      transform | column sums | G1 points | G2 points | serialisation
and of the file's check (Srs.check) and one contribution.  The two keys must be the same bytes.  One warm-up call each, then one timed."""
import importlib, pathlib, random, sys, tempfile, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
import eigen_zkvm_amd
import groth16_bench as GB
import make_test_ptau as MP
zk = eigen_zkvm_amd; zk.init(0)
dev = importlib.import_module("eigen_zkvm_amd.groth16")

args = sys.argv[1:]
curves = [a for a in args if a in MP.CURVES] or list(MP.CURVES)
logs = [int(a) for a in args if a.isdigit()]
log_rows = logs[0] if logs else 16


def timed(fn):
    fn()
    t0 = time.perf_counter(); out = fn()
    return out, (time.perf_counter() - t0) * 1e3


for tag in curves:
    r = MP.CURVES[tag]["r"]; rng = random.Random(14)
    rb, _wit, ni, n_wires = GB.make_circuit(r, log_rows)
    td = [rng.randrange(1, r) for _ in range(3)]
    with tempfile.TemporaryDirectory() as d:
        p = pathlib.Path(d) / "t.ptau"
        p.write_bytes(MP.build_ptau(zk, tag, log_rows, *td))
        srs = dev.Srs(tag, p)
        rep, ms_check = timed(lambda: srs.check())
        assert not rep["findings"], rep
        ms_f = []
        (pb, _vk), wall_f = timed(lambda: dev.keygen(tag, rb, srs=srs, check_srs=False, timing=ms_f))
        srs.free()
    ms_t = []
    (pb_t, _), wall_t = timed(lambda: dev.keygen(tag, rb, td + [1, 1], timing=ms_t))
    assert pb == pb_t, "the two setups disagree"
    _, ms_c = timed(lambda: dev.contribute(tag, pb))
    f = lambda v: " | ".join("%.1f" % x for x in v)
    print("%s 2^%d rows, %d wires, key %d bytes" % (tag, log_rows, n_wires, len(pb)))
    print("  file      %9.1f ms   = %s" % (wall_f, f(ms_f)))
    print("  trapdoor  %9.1f ms   = %s" % (wall_t, f(ms_t)))
    print("  srs check %9.1f ms   contribute %9.1f ms" % (ms_check, ms_c))
