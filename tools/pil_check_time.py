"""pil_verify timing: python tools/pil_check_time.py [--proof] nbits [nbits ...]

PilCheck.run on the PoseidonG PIL (tools/poseidong.py) with the trace tools/libtracegen.so makes, as bench.py makes it; constants and
trace already on the device; HIP events on the null stream, median of 5 after one warm-up.  The program's share is timed on its own
(the report of a clean trace needs nothing else: PoseidonG has no set identity).  --proof adds, for the same trace, the proof time
(median of 3, trace resident) and the step timers of a proof whose constraint programs run in the bytecode evaluator."""
import json, os, pathlib, statistics, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import torch
import eigen_zkvm_amd
import poseidong as PG
zk = eigen_zkvm_amd; zk.init(0)
args = [a for a in sys.argv[1:] if a != "--proof"]
with_proof = "--proof" in sys.argv[1:]


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


for nbits in [int(a) for a in args]:
    pil = PG.pil(nbits)
    const, cm = PG.consts(nbits), PG.trace(nbits, None, PG.FIRST_ZERO, seed=nbits)
    d_const, d_cm = zk.DevArray.from_host(const), zk.DevArray.from_host(cm)
    chk = zk.PilCheck(pil)
    rep = chk.run(d_const, d_cm)                                              # warm-up: uploads the program, takes the buffers
    assert rep["findings"] == [], rep["findings"][:3]
    out = {"nbits": nbits, "polIdentities": rep["checked"]["polIdentities"], "pil_check_ms": round(timed(lambda: chk.run(d_const, d_cm), 5), 3)}
    chk.free()
    if with_proof:
        stark = __import__("importlib").import_module("eigen_zkvm_amd.stark")
        ss, pj = PG.stark_struct(nbits), json.dumps(PG.program(nbits))
        for mode in ("jit", "bytecode"):
            setup = stark.NativeStarkSetup(const, pj, json.dumps(ss), eval_mode=mode)
            setup.gen_bytes(d_cm)
            out["proof_ms_" + mode] = round(timed(lambda: setup.gen_bytes(d_cm), 3), 3)
            if mode == "bytecode":
                os.environ["ZK_STARK_TIMING"] = "quiet"
                setup.gen_bytes(d_cm)
                out["bytecode_proof_stages_ms"] = setup.last_timing(); os.environ.pop("ZK_STARK_TIMING", None)
            setup.free()
    d_const.free(); d_cm.free()
    print(json.dumps(out), flush=True)
