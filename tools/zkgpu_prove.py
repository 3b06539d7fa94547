#!/usr/bin/env python3
"""zkgpu_prove -- the prover sub-commands of the reference's `eigen-zkit` on libzkgpu (last row):

  zkgpu_prove.py stark_prove -s starkStruct.json -p circuit.pil.json --o circuit.const --m circuit.cm \\
                             -c verifier.circom --i zkin.json [--norm_stage] [--skip_main] [--agg_stage] [--prover_addr A] \\
                             [--program starkinfo_program.json]
  zkgpu_prove.py groth16_setup -c BN128 --r1cs circuit.r1cs -p g16.key -v verification_key.json [-t]
  zkgpu_prove.py groth16_prove -c BN128 --r1cs circuit.r1cs -w witness.wtns -p g16.key --public-input public_input.json --proof proof.json [--verify verification_key.json]
  zkgpu_prove.py groth16_verify -c BN128 -v verification_key.json --public-input public_input.json --proof proof.json
  zkgpu_prove.py groth16_verify -c BN128 -v verification_key.json --batch proofs.json
  zkgpu_prove.py pil_verify -p circuit.pil.json --o circuit.const --m circuit.cm [--report out.json]
  zkgpu_prove.py wtns_check -c BN128|BLS12381|GL --r1cs circuit.r1cs --wtns witness.wtns [--sym circuit.sym] [--report out.json] [--max-findings N]
  zkgpu_prove.py groth16_setup ... --ptau ceremony.ptau [--no-check-srs]
  zkgpu_prove.py groth16_contribute -c BN128 -p in.key -o out.key [-v verification_key.json] [--check]
  zkgpu_prove.py groth16_contribution_check -c BN128 --old a.key --new b.key
  zkgpu_prove.py groth16_key_check -c BN128|BLS12381 --r1cs circuit.r1cs -p g16.key [-v verification_key.json] [--ptau pot.ptau [--no-check-srs]] [--report out.json] [--max-findings N]
  zkgpu_prove.py stark_verify -s starkStruct.json -p circuit.pil.json --o circuit.const --i zkin.json [--program FILE]
  zkgpu_prove.py compressor12_setup --r circuit.r1cs --c c12.const --p c12.pil --e c12.exec [--force_n_bits K] [--pil-json c12.pil.json]
  zkgpu_prove.py compressor12_exec --wtns witness.wtns --p c12.pil --e c12.exec --m c12.cm
  zkgpu_prove.py join_zkin --zkin1 a.zkin.json --zkin2 b.zkin.json --zkinout out.zkin.json
  zkgpu_prove.py stark_aggregate --gpus N --num_proof 8 --workspace DIR [--workers 4] [--keep_proofs]     (starts its own N ranks;
  [torchrun --nproc-per-node N] zkgpu_prove.py stark_aggregate ...                                         or runs under torchrun)

Flags, defaults and file formats are zkit's (zkit/src/main.rs:98-123 StarkProveOpt, :185-196 Groth16SetupOpt, :199-217 Groth16ProveOpt;
starky/src/prove.rs:30-160, groth16/src/api.rs:144-205).  What differs, and why:
  * stark_prove needs the code generator's output, `{"starkinfo": StarkInfo, "program": Program}` (serde names, starkinfo.rs:27-95):
    `--program FILE`, or -- when the file is absent -- the library's own generator (zk_starkinfo_generate) if this build has one.
    The reference runs `StarkInfo::new` in process; with the Rust shim (bindings/rust/starky-hip) that is still what happens.
  * `-c/--circom`: the circom verifier text comes from `pil2circom` (template rendering, out of scope): the flag is
    accepted, the file is NOT written and a warning on stderr says so.
  * groth16_prove: `-w` takes the `.wtns` the witness calculator wrote (zkit passes the .wasm and an input.json and runs the
    calculator in process, api.rs:150-160: WASM execution is out of scope); `-i` is accepted and ignored.
  * stark_prove verifies its own proof before it writes anything, as the reference does (prove.rs:124-132; `--no_verify` skips it).
  * pil_verify: the trace check the reference runs between building a trace and proving it (starkjs/src/pil_verifier.js:46, pilcom's
    verifyPil), on the device: one line `fileName:line: <kind> ...` per violated constraint, exit 0 when there is none and 1 otherwise;
    `--report` also writes the whole report as JSON.  `stark_prove --check-trace` runs it first and stops with the findings (exit 1)
    before any setup.
  * groth16_key_check: the proving key against its circuit on the device (the reference reads keys unchecked): section lengths, every
    point on its curve, in the subgroup and finite, b_g1 / b_g2 and the beta / delta pairs tied by pairings, `-v` against the embedded
    verification key.  One line per finding, exit 1 with findings.  Without `--ptau` it cannot check h, l, ic and a against the circuit's
    polynomials: `groth16_prove --verify` is the functional test.  With `--ptau FILE` (snarkjs's `zkey verify`) it then checks the file
    (`--no-check-srs` skips that) and every query of the key, alpha and beta against the circuit over that file; `--report` then holds
    the three reports.  `groth16_prove --check-key` runs it first and stops before the witness is touched;
    `groth16_setup --check-key` runs it on the key it has just made.
  * wtns_check: `snarkjs wtns check` on the device (the reference has no counterpart): every constraint of the .r1cs as written, wire 0,
    and over GL every use of the compressor's custom gates; one line per finding, exit 0 when there is none and 1 otherwise; `--sym` takes
    circom's .sym file and prints every wire with its signal name; `--report` also writes the whole report as JSON.
    `groth16_prove --check-witness` runs it first and stops with the findings (exit 1) before the proving key is read;
    `compressor12_exec --check-witness R1CS` does the same in front of the exec.
  * stark_verify: the check alone, on a zkin file (the reference exposes it only inside stark_prove).
  * compressor12_setup: `--pil-json OUT` also writes the compiled PIL (tools/pilc.py; the reference leaves that step to pilcom), so
    that the next command can be stark_prove.  compressor12_exec: the witness comes as a `.wtns` with 8-byte field elements
    (`--wtns`; zkit runs the circuit's .wasm on `--i`, and WASM execution is out of scope); the number of rows is read from the
    `let N: int = 2**k` line of the .pil.
  * stark_aggregate: test/stark_aggregation.sh:70-73 + :83-156 through eigen-zkvm_amd/aggregation.py -- NUM_PROOF recursion tasks
    sharded over the ranks (one process per GPU), their recursive1 nodes (root1 + digest of the whole proof) all-gathered, joined as
    a tree; the circuits are the synthetic ones of tools/aggregation_workload.py (the real ones are circom-compiled verifiers), so
    the join tree is a workload-shaped stand-in: its root commits to the leaves' proofs, it does not attest them -- each proof's
    validity is the per-proof self check (`each_proof_self_checked`).  Writes aggregation.json
    (every task's roots, the join tree's root, timings) into --workspace on rank 0.
Exit status 0 on success, 1 with the library's message on stderr otherwise (zkit: anyhow error -> exit 1)."""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))


def _zk():
    import eigen_zkvm_amd
    zk = eigen_zkvm_amd
    if zk.lib().zk_device_count() < 1:
        raise SystemExit("zkgpu_prove: no GPU visible (the library has no CPU fallback)")
    zk.init(0)
    return zk


def finding_line(f):
    """one finding of a pil_verify report as `fileName:line: <kind> ...`"""
    head = "%s:%s: %s" % (f["fileName"], f["line"], f["kind"])
    k = f["kind"]
    if k == "identity":
        return "%s %d: %s row(s) are not 0, first row %s (value %s)" % (head, f["index"], f["n_rows"], f["first_row"], f["value"])
    if k == "selector":
        return "%s of %s %d, side %s: %s row(s) outside {0, 1}, first row %s (value %s)" % (head, f["identity"], f["index"], f["side"], f["n_rows"], f["first_row"], f["value"])
    if k == "plookup":
        return "%s %d: %s selected row(s) look up a tuple the table lacks, first row %s (%s)" % (head, f["index"], f["n_rows"], f["first_row"], ", ".join(f["values"]))
    if k == "permutation":
        side = lambda r, v: "none" if r is None else "row %s (%s)" % (r, ", ".join(v))
        return "%s %d: %s f row(s) and %s t row(s) unmatched; first f %s, first t %s" % (
            head, f["index"], f["n_f_unmatched"], f["n_t_unmatched"], side(f["first_f_row"], f["f_values"]), side(f["first_t_row"], f["t_values"]))
    if k == "connection_value":
        return "%s %d: %s S value(s) name no cell, first at column %d row %s (%s)" % (head, f["index"], f["n_cells"], f["col"], f["row"], f["value"])
    return "%s %d: %s wired cell(s) differ, first column %d row %s (%s) against column %d row %s (%s)" % (
        head, f["index"], f["n_cells"], f["col"], f["row"], f["value"], f["partner_col"], f["partner_row"], f["partner_value"])


def _check_trace(a, stark):
    """-> the pil_verify report of the files the arguments name"""
    import numpy as np
    pil = json.load(open(a.piljson))
    const = np.memmap(a.const_pols, dtype="<u8", mode="r")
    cm = np.memmap(a.cm_pols, dtype="<u8", mode="r")
    chk = stark.PilCheck(pil)
    if const.size != chk.n * pil["nConstants"] or cm.size != chk.n * pil["nCommitments"]:
        raise SystemExit("zkgpu_prove: %s / %s do not hold %d rows of %d / %d columns" % (a.const_pols, a.cm_pols, chk.n, pil["nConstants"], pil["nCommitments"]))
    try:
        return chk.run(const, cm)
    finally:
        chk.free()


def pil_verify(a):
    import importlib
    _zk()
    report = _check_trace(a, importlib.import_module("eigen_zkvm_amd.stark"))
    if a.report:
        with open(a.report, "w") as f:
            json.dump(report, f, indent=1)
    for f in report["findings"]:
        print(finding_line(f))
    if report["findings"]:
        raise SystemExit(1)
    print("zkgpu_prove: %s satisfies %s (%d rows; %s)" % (a.cm_pols, a.piljson, report["n"], ", ".join("%d %s" % (v, k) for k, v in report["checked"].items())))


def read_sym(text):
    """circom's .sym file, one line per signal `label,wire,component,name` -> {wire: name}; a wire several names map to keeps
    the first, lines of wire -1 (signals the compiler removed) are skipped"""
    names = {}
    for line in text.splitlines():
        parts = line.strip().split(",", 3)
        if len(parts) < 4:
            continue
        try:
            wire = int(parts[1])
        except ValueError:
            continue
        if wire >= 0:
            names.setdefault(wire, parts[3])
    return names


def wtns_finding_line(f, names=None):
    """one finding of a wtns_check report as a line; names: {wire: signal name} of a .sym file"""
    wire = lambda w: "w%d (%s)" % (w, names[w]) if names and w in names else "w%d" % w
    k = f["kind"]
    if k == "one_wire":
        return "one_wire: wire 0 holds %s, not 1" % f["value"]
    if k == "constraint":
        side = lambda lc: " + ".join("%s*%s" % (c, wire(w)) for w, c in lc) or "0"
        return "constraint %d: a*b != c with a = %s, b = %s, c = %s; a: %s; b: %s; c: %s" % (
            f["index"], f["a"], f["b"], f["c"], side(f["wires"]["a"]), side(f["wires"]["b"]), side(f["wires"]["c"]))
    at = "row %d column %d" % (f["row"], f["column"]) if k == "poseidon12" else "output %d" % f["position"]
    return "%s use %d: %s, %s holds %s, the inputs force %s" % (k, f["use"], at, wire(f["wire"]), f["value"], f["expected"])


def _check_witness(field, r1cs_file, wtns_file, max_findings=16):
    """-> the wtns_check report of the files"""
    import importlib
    dev = importlib.import_module("eigen_zkvm_amd.r1cs")
    values, n = dev.wtns_payload(pathlib.Path(wtns_file).read_bytes(), field)
    chk = dev.R1csCheck(field, pathlib.Path(r1cs_file).read_bytes())
    try:
        return chk.run(values, max_findings=max_findings, n_values=n), chk.info
    finally:
        chk.free()


def _stop_on_findings(report, sym=None, out=sys.stderr):
    names = read_sym(pathlib.Path(sym).read_text()) if sym else None
    for f in report["findings"]:
        print(wtns_finding_line(f, names), file=out)
    if report["findings"] or any(report["n_failing"].values()):
        raise SystemExit(1)


def wtns_check(a):
    _zk()
    report, info = _check_witness(a.curve_type, a.circuit_file, a.wtns, a.max_findings)
    if a.report:
        with open(a.report, "w") as f:
            json.dump(report, f, indent=1)
    _stop_on_findings(report, a.sym, out=sys.stdout)
    print("zkgpu_prove: %s satisfies %s (%d constraints, %d custom-gate uses)" % (a.wtns, a.circuit_file, info["n_constraints"], info["n_custom_uses"]))


def stark_prove(a):
    import importlib
    import time
    t_start = time.perf_counter()
    import numpy as np
    zk = _zk()
    stark = importlib.import_module("eigen_zkvm_amd.stark")
    if a.check_trace:                                                      # pil_verifier.js:46 in front of the proof: nothing is set up for a bad trace
        findings = _check_trace(a, stark)["findings"]
        for f in findings:
            print(finding_line(f), file=sys.stderr)
        if findings:
            raise SystemExit(1)
    t_init = time.perf_counter()
    ss = json.load(open(a.stark_struct))
    pil = json.load(open(a.piljson))
    # polsarray.rs:137-217: headerless LE u64, row-major.  Mapped, not read: the library's upload is the one pass over the bytes
    # (np.fromfile would copy 5 GB at 2^24 rows before the first of them moves to the GPU)
    const = np.memmap(a.const_pols, dtype="<u8", mode="r")
    cm = np.memmap(a.cm_pols, dtype="<u8", mode="r")
    n = 1 << ss["nBits"]
    if const.size != n * pil["nConstants"] or cm.size != n * pil["nCommitments"]:
        raise SystemExit("zkgpu_prove: %s / %s do not hold 2^%d rows of %d / %d columns"
                         % (a.const_pols, a.cm_pols, ss["nBits"], pil["nConstants"], pil["nCommitments"]))
    if a.program:
        program_json = open(a.program).read()
    elif hasattr(stark, "generate_program"):
        program_json = stark.generate_program(json.dumps(pil), json.dumps(ss))
    else:
        raise SystemExit("zkgpu_prove: --program FILE is required (this build has no code generator)")
    t_gen = time.perf_counter()
    setup = stark.NativeStarkSetup(const, program_json, json.dumps(ss), prover_addr=a.prover_addr if ss.get("verificationHashType") != "GL" else None,
                                   self_check=not a.no_verify, eval_mode=a.eval)  # prove.rs:124-132: assert!(stark_verify(..)) before anything is written
    t_setup = time.perf_counter()
    zkin = setup.gen_json(cm)
    t_prove = time.perf_counter()
    with open(a.zkin, "w") as f:
        f.write(zkin)
    split = {"init_s": round(t_init - t_start, 3), "inputs_and_starkinfo_s": round(t_gen - t_init, 3), "setup_s": round(t_setup - t_gen, 3),
             "prove_s": round(t_prove - t_setup, 3), "write_s": round(time.perf_counter() - t_prove, 3), "total_s": round(time.perf_counter() - t_start, 3),
             "setup_split": setup.setup_timing(), "self_check": not a.no_verify}
    setup.free()
    # prove.rs:134-150 always renders the circom verifier into -c; pil2circom is out of scope here: say so when the flag was given
    if a.circom_file:
        print("zkgpu_prove: warning: no circom verifier is written to %s (pil2circom is out of scope of this backend; "
              "the reference's stark_prove writes it)" % a.circom_file, file=sys.stderr)
    print("zkgpu_prove: timing %s" % json.dumps(split), file=sys.stderr)        # prove.rs:95 #[time_profiler("stark_prove")] has the one number
    print("zkgpu_prove: proof of 2^%d rows %swritten to %s (rootC %s)" % (ss["nBits"], "" if a.no_verify else "verified and ", a.zkin, json.loads(zkin)["rootC"]))


def _setup_from_files(a, stark, self_check=False):
    import numpy as np
    ss = json.load(open(a.stark_struct))
    pil = json.load(open(a.piljson))
    const = np.fromfile(a.const_pols, dtype="<u8")
    program_json = open(a.program).read() if a.program else stark.generate_program(json.dumps(pil), json.dumps(ss))
    return stark.NativeStarkSetup(const, program_json, json.dumps(ss), self_check=self_check), ss


def stark_verify(a):
    import importlib
    _zk()
    stark = importlib.import_module("eigen_zkvm_amd.stark")
    setup, ss = _setup_from_files(a, stark)
    ok = setup.verify(open(a.zkin).read())
    why = "" if ok else setup.last_reject()
    setup.free()
    if not ok:
        raise SystemExit("zkgpu_prove: %s does not verify: %s" % (a.zkin, why))
    print("zkgpu_prove: %s verifies (2^%d rows, %s hash)" % (a.zkin, ss["nBits"], ss["verificationHashType"]))


def join_zkin(a):
    """zkit join_zkin --zkin1 A --zkin2 B --zkinout OUT (zkit/src/main.rs JoinZkinExecOpt -> starky/src/zkin_join.rs:9-57); host-only"""
    import importlib
    A = importlib.import_module("eigen_zkvm_amd.aggregation")
    with open(a.zkinout, "w") as f:
        f.write(A.join_zkin_text(open(a.zkin1).read(), open(a.zkin2).read()))
    print("zkgpu_prove: %s + %s -> %s" % (a.zkin1, a.zkin2, a.zkinout))


def stark_aggregate(a):
    import importlib
    import os
    import time
    sys.path.insert(0, str(ROOT / "tools"))
    from eigen_zkvm_amd import launcher
    if a.gpus > 1 and not launcher.under_launcher():                       # --gpus N with no torchrun in front: become the launcher (before any GPU call)
        raise SystemExit(launcher.spawn_ranks([str(pathlib.Path(__file__).resolve())] + a._argv, a.gpus, json_stdout=False))
    import eigen_zkvm_amd as zk
    local_rank = int(os.environ.get("ZK_AGG_DEVICE", os.environ.get("LOCAL_RANK", "0")))   # ZK_AGG_DEVICE: ranks sharing one GPU (tests)
    if zk.lib().zk_device_count() <= local_rank:
        raise SystemExit("zkgpu_prove: no GPU for local rank %d (the library has no CPU fallback)" % local_rank)
    zk.init(local_rank)
    A = importlib.import_module("eigen_zkvm_amd.aggregation")
    import aggregation_workload as AW
    ex = A.RootExchange.from_env(local_rank)
    n = a.num_proof
    per_rank = (n + ex.world - 1) // ex.world
    pool = AW.pool(zk, workers=max(1, min(a.workers, per_rank)), keep_proofs=a.keep_proofs, self_check=not a.no_verify)
    inputs = [pool.task_inputs(u) for u in A.shard_units(n, ex.rank, ex.world)]
    ex.barrier()
    t0 = time.perf_counter()
    res = A.aggregate(pool, inputs, n, ex)
    (dt,) = ex.max([time.perf_counter() - t0])
    seen = ex.gather([ex.rank])
    if ex.rank == 0:
        ws = pathlib.Path(a.workspace); ws.mkdir(parents=True, exist_ok=True)
        out = {"num_proof": n, "ranks": ex.world, "ranks_seen": len({r[0] for r in seen}), "seconds": round(dt, 4),
               # per proof: the library's stark_verify ran on it before it was handed out (prove.rs:124-132).  NOT a statement about the
               # join tree: recursive2 is a stand-in that takes the children's (root, proof digest) as inputs and does not re-verify them
               "each_proof_self_checked": not a.no_verify, "node": "root1 (4 words) + sha256 digest of the whole zkin (4 words)",
               "tasks": {str(u): {k: [str(w) for w in r] for k, r in zip(("fibonacci", "c12", "recursive1"), res["by_task"][u])} for u in sorted(res["by_task"])},
               "join_tree": dict(res["join_tree"], root=[str(w) for w in res["join_tree"]["root"]])}
        (ws / "aggregation.json").write_text(json.dumps(out, indent=1) + "\n")
        print("zkgpu_prove: %d tasks on %d rank(s), %d joins in %d levels, %.3f s; root %s -> %s"
              % (n, ex.world, res["join_tree"]["joins"], res["join_tree"]["levels"], dt, out["join_tree"]["root"], ws / "aggregation.json"))
    if a.keep_proofs:
        ws = pathlib.Path(a.workspace); ws.mkdir(parents=True, exist_ok=True)
        for i, (kind, z) in enumerate(pool.proofs):
            (ws / ("rank%d_%03d_%s.zkin.json" % (ex.rank, i, kind))).write_bytes(z)
        for i, (_node, text) in enumerate(pool.join_inputs):                 # what `zkit join_zkin` writes in front of every recursive2 step (children proved on this rank)
            (ws / ("rank%d_join%03d_input.zkin.json" % (ex.rank, i))).write_text(text)
    pool.free()
    ex.barrier()


def compressor12_setup(a):
    """recursion/src/compressor12/compressor12_setup.rs:18-48: .r1cs -> .pil, .const (row-major u64, polsarray.rs:184-), .exec"""
    import importlib
    _zk()
    dev = importlib.import_module("eigen_zkvm_amd.compressor12")
    S = dev.Compressor12Setup.from_r1cs(pathlib.Path(a.r1cs_file).read_bytes(), a.force_n_bits)
    pil = S.pil
    pathlib.Path(a.pil_file).write_text(pil)
    S.consts_host().astype("<u8").tofile(a.const_file)
    pathlib.Path(a.exec_file).write_text(S.exec_text)
    if a.pil_json:
        sys.path.insert(0, str(ROOT / "tools"))
        import pilc
        pathlib.Path(a.pil_json).write_text(pilc.dumps(pilc.compile_pil(a.pil_file, pil)))
    print("zkgpu_prove: compressor of 2^%d rows (%d used), %d constant columns, %d gates, %d additions -> %s %s %s"
          % (S.n_bits, S.n_used, S.n_const, S.n_gates, S.n_adds, a.pil_file, a.const_file, a.exec_file))
    S.free()


def compressor12_exec(a):
    """recursion/src/compressor12/compressor12_exec.rs:17-103 after the witness calculator: .wtns + .exec -> .cm"""
    import importlib
    import re
    import struct
    import numpy as np
    _zk()
    dev = importlib.import_module("eigen_zkvm_amd.compressor12")
    if not a.wtns:
        raise SystemExit("zkgpu_prove: compressor12_exec needs --wtns FILE (running the .wasm on --i is out of scope)")
    if a.check_witness:                                                    # nothing is executed for a bad witness
        _stop_on_findings(_check_witness("GL", a.check_witness, a.wtns)[0])
    b = pathlib.Path(a.wtns).read_bytes()
    if b[:4] != b"wtns" or len(b) < 12:
        raise SystemExit("zkgpu_prove: %s is not a .wtns file" % a.wtns)
    secs, o = {}, 12
    for _ in range(struct.unpack_from("<I", b, 8)[0]):
        t, sz = struct.unpack_from("<IQ", b, o); o += 12
        secs[t] = b[o:o + sz]; o += sz
    fs = struct.unpack_from("<I", secs[1])[0]
    if fs != 8 or int.from_bytes(secs[1][4:12], "little") != 0xFFFFFFFF00000001:
        raise SystemExit("zkgpu_prove: %s is not a witness over Goldilocks (8-byte field elements)" % a.wtns)
    n = struct.unpack_from("<I", secs[1], 12)[0]
    w = np.frombuffer(secs[2], dtype="<u8", count=n)
    m = re.search(r"let\s+N\s*:\s*int\s*=\s*2\*\*(\d+)", pathlib.Path(a.pil_file).read_text())
    if not m:
        raise SystemExit("zkgpu_prove: no `let N: int = 2**k` in %s" % a.pil_file)
    E = dev.Compressor12Exec(pathlib.Path(a.exec_file).read_text(), n)
    E.run(w, 1 << int(m.group(1))).to_host().astype("<u8").tofile(a.commit_file)
    E.free()
    print("zkgpu_prove: %d wires -> 2^%s rows of 12 columns in %s" % (n, m.group(1), a.commit_file))


def _check_key(curve, r1cs_bytes, pk_bytes, vk_text=None, max_findings=16, report_file=None, out=sys.stderr):
    """groth16_key_check of the files' bytes: the finding lines and what was skipped, then exit 1 when there is a finding"""
    import importlib
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    report = dev.key_check(curve, r1cs_bytes, pk_bytes, vk_json=vk_text, max_findings=max_findings)
    if report_file:
        with open(report_file, "w") as f:
            json.dump(report, f, indent=1)
    for f in report["findings"]:
        print(dev.key_check_line(f), file=out)
    for s in report["skipped"]:                                            # every reason to skip comes with a finding: say it before the exit
        print(dev.key_check_skipped_line(s), file=out)
    if any(report["counts"].values()):
        raise SystemExit(1)
    return report


def _key_check_ptau(a):
    """groth16_key_check --ptau: the key's own check, the file's (unless --no-check-srs), then the key against circuit and file; every
    finding a line, the three reports side by side under --report, exit 1 when any of them has a finding"""
    import importlib
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    r1cs, pk = pathlib.Path(a.circuit_file).read_bytes(), pathlib.Path(a.pk_file).read_bytes()
    reports = {"key_check": dev.key_check(a.curve_type, r1cs, pk, vk_json=pathlib.Path(a.vk_file).read_text() if a.vk_file else None,
                                          max_findings=a.max_findings), "srs_check": None}
    srs = dev.Srs(a.curve_type, a.ptau)
    try:
        if not a.no_check_srs:
            reports["srs_check"] = srs.check(max_findings=a.max_findings)
        reports["key_check_srs"] = dev.key_check_srs(a.curve_type, r1cs, pk, srs, max_findings=a.max_findings)
    finally:
        srs.free()
    if a.report:
        with open(a.report, "w") as f:
            json.dump(reports, f, indent=1)
    lines = {"key_check": dev.key_check_line, "srs_check": dev.srs_check_line, "key_check_srs": dev.key_check_srs_line}
    bad = False
    for name, line in lines.items():
        rep = reports[name]
        if rep is None:
            continue
        for f in rep["findings"]:
            print(line(f))
        for k in rep["skipped"]:
            print(dev.key_check_skipped_line(k))
        bad = bad or any(rep["counts"].values())
    if bad:
        raise SystemExit(1)
    c = reports["key_check_srs"]["checked"]
    print("zkgpu_prove: %s is a key of %s over %s%s (%d row sums, %d transforms, %d sums, %d pairs)"
          % (a.pk_file, a.circuit_file, a.ptau, " (the file itself was not checked)" if a.no_check_srs else "", c["row_sums"], c["transforms"], c["sums"], c["pairs"]))


def groth16_key_check(a):
    if a.no_check_srs and not a.ptau:
        raise SystemExit("zkgpu_prove: --no-check-srs says how to treat --ptau FILE and means nothing without it")
    _zk()
    if a.ptau:
        return _key_check_ptau(a)
    rep = _check_key(a.curve_type, pathlib.Path(a.circuit_file).read_bytes(), pathlib.Path(a.pk_file).read_bytes(),
                     pathlib.Path(a.vk_file).read_text() if a.vk_file else None, a.max_findings, a.report, out=sys.stdout)
    print("zkgpu_prove: %s is a well-formed key of %s (%d G1 and %d G2 points, %d pairs; h, l, ic, a are not checked against the circuit's polynomials)"
          % (a.pk_file, a.circuit_file, rep["checked"]["g1_points"], rep["checked"]["g2_points"], rep["checked"]["pairs"]))


def groth16_setup(a):
    """groth16/src/api.rs:42-66: circuit_specific_setup, then the key and verification_key.json written to their files"""
    import importlib
    if a.no_check_srs and not a.ptau:
        raise SystemExit("zkgpu_prove: --no-check-srs says how to treat --ptau FILE and means nothing without it")
    _zk()
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    r1cs = pathlib.Path(a.circuit_file).read_bytes()
    srs = None
    if a.ptau:                                                            # extension: tau, alpha, beta from a ceremony's file, gamma = delta = 1
        srs = dev.Srs(a.curve_type, a.ptau)
        if not a.no_check_srs:                                            # a bad file makes no key
            report = srs.check()
            for f in report["findings"]:
                print(dev.srs_check_line(f), file=sys.stderr)
            for k in report["skipped"]:
                print(dev.key_check_skipped_line(k), file=sys.stderr)
            if any(report["counts"].values()):
                raise SystemExit(1)
            print("zkgpu_prove: %s is a well-formed powers-of-tau file of power %d (%d G1 and %d G2 points)"
                  % (a.ptau, srs.power, report["checked"]["g1_points"], report["checked"]["g2_points"]))
    pk, vk = dev.keygen(a.curve_type, r1cs, to_hex=a.to_hex, srs=srs, check_srs=False)   # checked above, line by line
    if srs is not None:
        srs.free()
        print("zkgpu_prove: delta = 1 in this key: it needs at least one groth16_contribute before it is used")
    pathlib.Path(a.pk_file).write_bytes(pk)
    pathlib.Path(a.vk_file).write_text(vk)
    print("zkgpu_prove: %s key written to %s (%d bytes), verification key to %s" % (a.curve_type, a.pk_file, len(pk), a.vk_file))
    if a.check_key:
        _check_key(a.curve_type, r1cs, pk, vk)
        print("zkgpu_prove: the key passes groth16_key_check")


def _vk_json_of_key(curve, pk, to_hex=False):
    """verification_key.json of a key's bytes (json_utils.rs:285-303 over VerifyingKey::write's layout)"""
    nb = 32 if curve == "BN128" else 48
    o = 0
    num = lambda b: ("0x" + b.hex()) if to_hex else str(int.from_bytes(b, "big"))

    def g1():
        nonlocal o
        b = pk[o:o + 2 * nb]; o += 2 * nb
        if b[0] & 0x40:
            b = bytes(2 * nb - 1) + b"\x01"                               # CurveAffine::zero() is (0, 1)
        return {"x": num(b[:nb]), "y": num(b[nb:])}

    def g2():
        nonlocal o
        b = pk[o:o + 4 * nb]; o += 4 * nb
        return {"x": [num(b[nb:2 * nb]), num(b[:nb])], "y": [num(b[3 * nb:]), num(b[2 * nb:3 * nb])]}
    js = {"protocol": "groth16", "curve": curve}
    for name, f in (("vk_alpha_1", g1), ("vk_beta_1", g1), ("vk_beta_2", g2), ("vk_gamma_2", g2), ("vk_delta_1", g1), ("vk_delta_2", g2)):
        js[name] = f()
    n = int.from_bytes(pk[o:o + 4], "big"); o += 4
    js["IC"] = [g1() for _ in range(n)]
    return json.dumps(js, separators=(",", ":"))


def _check_contribution(curve, old, new, out=sys.stderr):
    import importlib
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    report = dev.contribution_check(curve, old, new)
    for f in report["findings"]:
        print(dev.contribution_check_line(f), file=out)
    for k in report["skipped"]:
        print(dev.key_check_skipped_line(k), file=out)
    if any(report["counts"].values()):
        raise SystemExit(1)
    return report


def groth16_contribute(a):
    """extension: one contribution to a key's delta, drawn from the operating system and forgotten"""
    import importlib
    _zk()
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    old = pathlib.Path(a.pk_file).read_bytes()
    new = dev.contribute(a.curve_type, old)
    if a.check:                                                           # nothing is written for a contribution that does not check
        _check_contribution(a.curve_type, old, new)
    pathlib.Path(a.out_file).write_bytes(new)
    if a.vk_file:
        pathlib.Path(a.vk_file).write_text(_vk_json_of_key(a.curve_type, new))
    print("zkgpu_prove: %s key with one more contribution to delta written to %s (%d bytes)%s"
          % (a.curve_type, a.out_file, len(new), ", verification key to %s" % a.vk_file if a.vk_file else ""))


def groth16_contribution_check(a):
    _zk()
    rep = _check_contribution(a.curve_type, pathlib.Path(a.old_file).read_bytes(), pathlib.Path(a.new_file).read_bytes(), out=sys.stdout)
    print("zkgpu_prove: %s is %s with a contribution to delta and nothing else changed (%d h and %d l points)"
          % (a.new_file, a.old_file, rep["sections"]["h"], rep["sections"]["l"]))


def groth16_prove(a):
    import importlib
    zk = _zk()
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    if a.check_key:                                                        # the witness is not touched for a bad key
        _check_key(a.curve_type, pathlib.Path(a.circuit_file).read_bytes(), pathlib.Path(a.pk_file).read_bytes())
    if a.check_witness:                                                    # the proving key is not read for a bad witness
        _stop_on_findings(_check_witness(a.curve_type, a.circuit_file, a.wasm_file)[0])
    r1cs, pk, wtns = (pathlib.Path(p).read_bytes() for p in (a.circuit_file, a.pk_file, a.wasm_file))
    if not wtns.startswith(b"wtns"):
        raise SystemExit("zkgpu_prove: -w must be the .wtns file of the witness calculator (running the .wasm is out of scope)")
    setup = dev.Groth16Setup(a.curve_type, r1cs, pk)
    w = dev.wtns_values(wtns, a.curve_type)
    proof, _ = setup.prove(w)
    if a.to_hex:
        raise SystemExit("zkgpu_prove: -t (hex output) is not implemented")
    to_int = lambda row: sum(int(v) << (64 * i) for i, v in enumerate(row))
    if a.verify_vk:                                                        # extension: the proof is checked before anything is written
        vk = dev.Groth16VerifyingKey(a.curve_type, pathlib.Path(a.verify_vk).read_text())
        verdict = vk.verify(proof, [to_int(w[i]) for i in range(1, setup.n_inputs)])
        vk.free()
        if verdict != dev.ACCEPTED:
            raise SystemExit("zkgpu_prove: verify failed: %s; nothing written" % dev.verdict_name(verdict))
    json.dump(proof, open(a.proof_file, "w"))
    json.dump([str(to_int(w[i])) for i in range(1, setup.n_inputs)], open(a.public_input_file, "w"))   # api.rs:175-177
    setup.free()
    print("zkgpu_prove: %s proof written to %s" % (a.curve_type, a.proof_file))


def groth16_verify(a):
    """groth16/src/api.rs:302-341: verification_key.json, public_input.json, proof.json -> accepted or not (on the device)"""
    import importlib
    _zk()
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    vk = dev.Groth16VerifyingKey(a.curve_type, pathlib.Path(a.vk_file).read_text())
    if a.batch:
        return groth16_verify_list(a, dev, vk)
    verdict = vk.verify(pathlib.Path(a.proof_file).read_text(), pathlib.Path(a.public_input_file).read_text())
    vk.free()
    if verdict != dev.ACCEPTED:
        raise SystemExit("zkgpu_prove: verify failed: %s" % dev.verdict_name(verdict))
    print("zkgpu_prove: %s proof %s accepted" % (a.curve_type, a.proof_file))


def groth16_verify_list(a, dev, vk):
    """--batch LIST.json (extension): an array of [proof.json, public_input.json] path pairs, relative to the list's directory.  All of
    them in one randomised pairing check; on refusal the per-proof path names every proof that is not accepted."""
    import numpy as np
    base = pathlib.Path(a.batch).resolve().parent
    pairs = json.loads(pathlib.Path(a.batch).read_text())
    if not isinstance(pairs, list) or not all(isinstance(e, list) and len(e) == 2 for e in pairs):
        raise SystemExit("zkgpu_prove: %s must be an array of [proof.json, public_input.json] pairs" % a.batch)
    early, pts, pubs = {}, [], []                               # verdicts the readers settle, and what goes to the device
    for i, (pf, uf) in enumerate(pairs):
        w = vk.proof_words((base / pf).read_text(), (base / uf).read_text())
        if isinstance(w, tuple):
            pts.append(w[0]); pubs.append(w[1])
        else:
            early[i] = w
    rest = [i for i in range(len(pairs)) if i not in early]
    verdict = dev.ACCEPTED
    if rest:
        allp = np.concatenate(pts)
        verdict, _ = vk.verify_aggregate(allp, pubs, locate=False)
    if verdict == dev.ACCEPTED and not early:
        vk.free()
        print("zkgpu_prove: %s all %d proofs of %s accepted" % (a.curve_type, len(pairs), a.batch))
        return
    each = dict(early)
    if rest:
        each.update(zip(rest, (int(v) for v in vk.verify_batch(allp, pubs))))
    vk.free()
    bad = [i for i in range(len(pairs)) if each[i] != dev.ACCEPTED]
    if not bad:
        raise RuntimeError("groth16_verify --batch: the aggregate check refused a batch whose proofs all pass one by one")
    for i in bad:
        print("zkgpu_prove: proof %d (%s): %s" % (i, pairs[i][0], dev.verdict_name(each[i])))
    raise SystemExit("zkgpu_prove: verify failed: %d of %d proofs not accepted" % (len(bad), len(pairs)))


def build_parser():
    ap = argparse.ArgumentParser(prog="zkgpu_prove", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("stark_prove", help="Stark proving (zkit/src/main.rs:98-123)")
    s.add_argument("-s", "--stark_stuct", dest="stark_struct", default="stark_struct.json")
    s.add_argument("-p", "--piljson", default="pil.json")
    s.add_argument("-n", "--norm_stage", action="store_true")
    s.add_argument("--skip_main", action="store_true")
    s.add_argument("-a", "--agg_stage", action="store_true")
    s.add_argument("--o", dest="const_pols", default="pols.const")
    s.add_argument("--m", dest="cm_pols", default="pols.cm")
    s.add_argument("-c", "--circom", dest="circom_file", default=None, help="accepted for zkit compatibility; nothing is written (warned)")
    s.add_argument("--i", dest="zkin", default="zkin.json")
    s.add_argument("--prover_addr", default="273030697313060285579891744179749754319274977764")
    s.add_argument("--program", help='{"starkinfo", "program"} JSON of the code generator (extension, see the module text)')
    s.add_argument("--no_verify", action="store_true", help="skip the self check of prove.rs:124-132 (extension)")
    s.add_argument("--eval", default="jit", choices=["jit", "bytecode"],
                   help="evaluator of the step programs (extension): jit = run-time compiled kernels; bytecode = the interpreter kernel, nothing is compiled")
    s.add_argument("--check-trace", dest="check_trace", action="store_true",
                   help="run pil_verify on the trace first and stop with its findings (exit 1) before any setup (extension)")
    s.set_defaults(fn=stark_prove)
    pv = sub.add_parser("pil_verify", help="check a trace against its PIL, row by row (starkjs/src/pil_verifier.js:46)")
    pv.add_argument("-p", "--piljson", default="pil.json")
    pv.add_argument("--o", dest="const_pols", default="pols.const")
    pv.add_argument("--m", dest="cm_pols", default="pols.cm")
    pv.add_argument("--report", default=None, metavar="OUT.json", help="also write the whole report")
    pv.set_defaults(fn=pil_verify)
    wc = sub.add_parser("wtns_check", help="check a witness against its R1CS, constraint by constraint (extension; `snarkjs wtns check`)")
    wc.add_argument("-c", dest="curve_type", default="BN128", choices=["BN128", "BLS12381", "GL"])
    wc.add_argument("--r1cs", dest="circuit_file", required=True)
    wc.add_argument("--wtns", required=True)
    wc.add_argument("--sym", default=None, help="circom's .sym file: wires are printed with their signal names")
    wc.add_argument("--report", default=None, metavar="OUT.json", help="also write the whole report")
    wc.add_argument("--max-findings", dest="max_findings", type=int, default=16, help="findings listed per kind (the counts are always exact)")
    wc.set_defaults(fn=wtns_check)
    v = sub.add_parser("stark_verify", help="stark_verify.rs:20-136 on a zkin file (extension: the reference runs it inside stark_prove only)")
    v.add_argument("-s", "--stark_stuct", dest="stark_struct", default="stark_struct.json")
    v.add_argument("-p", "--piljson", default="pil.json")
    v.add_argument("--o", dest="const_pols", default="pols.const")
    v.add_argument("--i", dest="zkin", default="zkin.json")
    v.add_argument("--program")
    v.set_defaults(fn=stark_verify)
    ag = sub.add_parser("stark_aggregate", help="test/stark_aggregation.sh:70-73,83-156: NUM_PROOF tasks sharded over the GPUs + the joins")
    ag.add_argument("--num_proof", type=int, default=8)
    ag.add_argument("--gpus", type=int, default=1, help="ranks to start (one process per GPU) when no launcher (torchrun) is in front")
    ag.add_argument("--workspace", default="/tmp/aggregation")
    ag.add_argument("--workers", type=int, default=4, help="provers in flight per GPU")
    ag.add_argument("--keep_proofs", action="store_true", help="write every proof's zkin into the workspace")
    ag.add_argument("--no_verify", action="store_true")
    ag.set_defaults(fn=stark_aggregate)
    j = sub.add_parser("join_zkin", help="zkin_join.rs:9-57: the input of one recursive2 step from two proofs")
    j.add_argument("--zkin1", required=True); j.add_argument("--zkin2", required=True); j.add_argument("--zkinout", required=True)
    j.set_defaults(fn=join_zkin)
    cs = sub.add_parser("compressor12_setup", help="Setup compressor12 for converting R1CS to PIL (zkit/src/main.rs:140-151)")
    cs.add_argument("--r", dest="r1cs_file", default="mycircuit.verifier.r1cs")
    cs.add_argument("--c", dest="const_file", default="mycircuit.c12.const")
    cs.add_argument("--p", dest="pil_file", default="mycircuit.c12.pil")
    cs.add_argument("--e", dest="exec_file", default="mycircuit.c12.exec")
    cs.add_argument("--force_n_bits", type=int, default=0)
    cs.add_argument("--pil-json", dest="pil_json", default=None, metavar="OUT", help="also write the compiled PIL (extension)")
    cs.set_defaults(fn=compressor12_setup)
    ce = sub.add_parser("compressor12_exec", help="Exec compressor12 (zkit/src/main.rs:155-168) from a .wtns")
    ce.add_argument("--i", dest="input_file", default="mycircuit.proof.zkin.json", help="accepted for zkit compatibility, not read")
    ce.add_argument("--w", dest="wasm_file", default="mycircuit.verifier.wasm", help="accepted for zkit compatibility, not run")
    ce.add_argument("--wtns", default=None, help="the witness the calculator wrote, 8-byte field elements (extension)")
    ce.add_argument("--p", dest="pil_file", default="mycircuit.c12.pil")
    ce.add_argument("--e", dest="exec_file", default="mycircuit.c12.exec")
    ce.add_argument("--m", dest="commit_file", default="mycircuit.c12.cm")
    ce.add_argument("--check-witness", dest="check_witness", default=None, metavar="R1CS",
                    help="run wtns_check of the witness against this .r1cs first and stop with its findings (exit 1) before the exec (extension)")
    ce.set_defaults(fn=compressor12_exec)
    k = sub.add_parser("groth16_setup", help="Setup groth16 (zkit/src/main.rs:185-196)")
    k.add_argument("-c", dest="curve_type", default="BN128")
    k.add_argument("--r1cs", dest="circuit_file", required=True)
    k.add_argument("-p", dest="pk_file", default="g16.zkey")
    k.add_argument("-v", dest="vk_file", default="verification_key.json")
    k.add_argument("-t", dest="to_hex", action="store_true", help="coordinates of the verification key as 0x strings")
    k.add_argument("--check-key", dest="check_key", action="store_true", help="run groth16_key_check on the key just made (extension)")
    k.add_argument("--ptau", default=None, metavar="FILE", help="take tau, alpha, beta from a powers-of-tau file instead of drawing a trapdoor (extension)")
    k.add_argument("--no-check-srs", dest="no_check_srs", action="store_true", help="with --ptau: skip the check of the file's points and structure")
    k.set_defaults(fn=groth16_setup)
    gc = sub.add_parser("groth16_contribute", help="multiply a key's delta by a fresh secret (extension)")
    gc.add_argument("-c", dest="curve_type", default="BN128")
    gc.add_argument("-p", dest="pk_file", required=True)
    gc.add_argument("-o", dest="out_file", required=True)
    gc.add_argument("-v", dest="vk_file", default=None, help="write the new key's verification_key.json here")
    gc.add_argument("--check", action="store_true", help="run groth16_contribution_check on the result before writing it")
    gc.set_defaults(fn=groth16_contribute)
    cc = sub.add_parser("groth16_contribution_check", help="check that a key is another one with a contribution to delta and no other change (extension)")
    cc.add_argument("-c", dest="curve_type", default="BN128")
    cc.add_argument("--old", dest="old_file", required=True)
    cc.add_argument("--new", dest="new_file", required=True)
    cc.set_defaults(fn=groth16_contribution_check)
    kc = sub.add_parser("groth16_key_check", help="check a proving key against its circuit: sizes, every point, the G1 / G2 copies (extension)")
    kc.add_argument("-c", dest="curve_type", default="BN128")
    kc.add_argument("--r1cs", dest="circuit_file", required=True)
    kc.add_argument("-p", dest="pk_file", default="g16.zkey")
    kc.add_argument("-v", dest="vk_file", default=None, help="a verification_key.json to compare with the key's embedded copy")
    kc.add_argument("--report", default=None, metavar="OUT.json", help="also write the whole report")
    kc.add_argument("--max-findings", dest="max_findings", type=int, default=16)
    kc.add_argument("--ptau", default=None, metavar="FILE", help="also check the key against the circuit's polynomials over this powers-of-tau file: h, l, ic, a, b and alpha, beta")
    kc.add_argument("--no-check-srs", dest="no_check_srs", action="store_true", help="with --ptau: do not check the file itself first")
    kc.set_defaults(fn=groth16_key_check)
    g = sub.add_parser("groth16_prove", help="Prove with groth16 (zkit/src/main.rs:199-217)")
    g.add_argument("-c", dest="curve_type", default="BN128")
    g.add_argument("--r1cs", dest="circuit_file", required=True)
    g.add_argument("-w", dest="wasm_file", required=True)
    g.add_argument("-p", dest="pk_file", default="g16.zkey")
    g.add_argument("-i", dest="input_file", default=None)
    g.add_argument("--public-input", dest="public_input_file", default="public_input.json")
    g.add_argument("--proof", dest="proof_file", default="proof.json")
    g.add_argument("-t", dest="to_hex", action="store_true")
    g.add_argument("--verify", dest="verify_vk", default=None, metavar="VK.json",
                   help="check the proof against this verification key before writing it (extension)")
    g.add_argument("--check-witness", dest="check_witness", action="store_true",
                   help="run wtns_check first and stop with its findings (exit 1) before the proving key is read (extension)")
    g.add_argument("--check-key", dest="check_key", action="store_true",
                   help="run groth16_key_check first and stop with its findings (exit 1) before the witness is touched (extension)")
    g.set_defaults(fn=groth16_prove)
    gv = sub.add_parser("groth16_verify", help="Verify with groth16 (zkit/src/main.rs:221-230)")
    gv.add_argument("-c", dest="curve_type", default="BN128")
    gv.add_argument("-v", dest="vk_file", default="verification_key.json")
    gv.add_argument("--public-input", dest="public_input_file", default="public_input.json")
    gv.add_argument("--proof", dest="proof_file", default="proof.json")
    gv.add_argument("--batch", dest="batch", default=None, metavar="LIST.json",
                    help="an array of [proof.json, public_input.json] path pairs, relative to the list: all of them in one randomised check (extension)")
    gv.set_defaults(fn=groth16_verify)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    a._argv = list(sys.argv[1:] if argv is None else argv)
    try:
        a.fn(a)
    except SystemExit:
        raise
    except Exception as e:                                                # anyhow error -> message + exit 1
        print("zkgpu_prove: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
