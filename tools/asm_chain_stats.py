#!/usr/bin/env python3
"""tools/asm_chain_stats.py LISTING.s KERNEL [KERNEL ...]: how tightly the vector instructions of a kernel are chained.

LISTING.s is what `hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S` writes; KERNEL is a substring of the (mangled) symbol, e.g.
`ntt_pass_kernelILi4ELi4ELb0ELb0E`.  Per matching kernel, from its label up to the first s_endpgm, one line with
  valu       vector instructions (mnemonics v_*)
  s_nop      written wait states, in all and by operand (`s_nop 1` = two states)
  asm_blocks inline-asm statements (;;#ASMSTART)
  adj_dep    the fraction of vector instructions that read a VGPR, vcc or an SGPR (pair) which the vector instruction immediately
             before them wrote -- such an instruction cannot issue at the back-to-back rate of independent ones
`--json` prints the same as one JSON object per kernel."""
import json
import re
import sys

CARRY_OUT = ("v_add_co_", "v_sub_co_", "v_subrev_co_", "v_addc_co_", "v_subb_co_", "v_subbrev_co_", "v_mad_u64_u32", "v_mad_i64_i32",
             "v_div_scale_")
NO_DEST = ("v_nop", "v_cmpx_")
REG = re.compile(r"\b([vsa])(\d+)\b|\b([vsa])\[(\d+):(\d+)\]|\b(vcc(?:_lo|_hi)?|exec(?:_lo|_hi)?)\b")


def regs(operand):
    """the registers an operand names: v3 -> {v3}, s[4:5] -> {s4, s5}, vcc -> {vcc}"""
    out = set()
    for m in REG.finditer(operand):
        if m.group(1):
            out.add(m.group(1) + m.group(2))
        elif m.group(3):
            out.update(m.group(3) + str(i) for i in range(int(m.group(4)), int(m.group(5)) + 1))
        else:
            out.add(m.group(6)[:3] if m.group(6).startswith("vcc") else m.group(6)[:4])
    return out


def split_operands(text):
    """operands of one instruction, modifiers (`row_newbcast:3`, `op_sel:[0,1]`) left with the operand they follow"""
    ops, depth, cur = [], 0, ""
    for ch in text:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append(cur.strip()); cur = ""
        else:
            cur += ch
    if cur.strip():
        ops.append(cur.strip())
    return ops


def writes_reads(mnemonic, operands):
    ops = split_operands(operands)
    if mnemonic.startswith(NO_DEST):
        n_dst = 0
    elif mnemonic.startswith(CARRY_OUT):
        n_dst = 2
    else:
        n_dst = 1
    w, r = set(), set()
    for i, op in enumerate(ops):
        op = op.split(" ")[0] if not op.startswith(("v[", "s[", "a[")) else op
        (w if i < n_dst else r).update(regs(op))
    if mnemonic.startswith("v_cmp_") and mnemonic.endswith("_e32"):
        w.add("vcc")
    if mnemonic.endswith("_e32") and mnemonic.startswith(("v_cndmask", "v_addc_co", "v_subb_co", "v_subbrev_co")):
        r.add("vcc")
    return w, r


def kernel_lines(lines, name):
    """{symbol: its lines up to the first s_endpgm} for every global label that contains `name`"""
    out, cur = {}, None
    for ln in lines:
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", ln)
        if m and not m.group(1).startswith((".L", "BB")):
            cur = m.group(1) if name in m.group(1) and m.group(1) not in out else None
            if cur:
                out[cur] = []
            continue
        if cur:
            code = ln.split(";")[0].strip() if ";;#" not in ln else ln.strip()
            out[cur].append(code)
            if code.startswith("s_endpgm"):
                cur = None
    return out


def stats(code_lines):
    valu = blocks = dep = 0
    nops = {}
    prev_w = None
    for code in code_lines:
        if code.startswith(";;#ASMSTART"):
            blocks += 1
            continue
        if not code or code.startswith((";", ".", "//")) or code.endswith(":"):
            continue
        parts = code.split(None, 1)
        mn, rest = parts[0], parts[1] if len(parts) > 1 else ""
        if mn == "s_nop":
            k = int(rest.strip(), 0)
            nops[k] = nops.get(k, 0) + 1
        elif mn.startswith("v_"):
            valu += 1
            w, r = writes_reads(mn, rest)
            if prev_w is not None and prev_w & r:
                dep += 1
            prev_w = w
    return {"valu": valu, "s_nop": sum(nops.values()), "s_nop_by_width": {str(k): nops[k] for k in sorted(nops)}, "asm_blocks": blocks,
            "adj_dep": round(dep / valu, 4) if valu else 0.0}


def main(argv):
    as_json = "--json" in argv
    args = [a for a in argv if a != "--json"]
    if len(args) < 2:
        print(__doc__); return 2
    lines = open(args[0]).read().splitlines()
    rc = 1
    for name in args[1:]:
        for sym, code in kernel_lines(lines, name).items():
            rc = 0
            st = stats(code)
            if as_json:
                print(json.dumps({"kernel": sym, **st}))
            else:
                by = " ".join(f"s_nop {k}: {v}" for k, v in st["s_nop_by_width"].items())
                print(f"{sym}  valu {st['valu']}  s_nop {st['s_nop']} ({by})  asm_blocks {st['asm_blocks']}  adj_dep {st['adj_dep']:.3f}")
    if rc:
        print("no kernel matches", args[1:], file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
