"""tools/asm_chain_stats.py on a small hand-written listing: the counts up to the first s_endpgm, the s_nop widths, the asm blocks and the
fraction of vector instructions that read what the vector instruction right before them wrote (a VGPR, vcc or an SGPR pair)."""
import importlib.util
import pathlib
import subprocess
import sys

TOOL = pathlib.Path(__file__).resolve().parent.parent / "tools" / "asm_chain_stats.py"

LISTING = """\
	.text
	.globl	_Z5otherv
_Z5otherv:
	v_mov_b32_e32 v0, 0
	s_endpgm
	.globl	_Z4demoILi4EEvPy
_Z4demoILi4EEvPy:                       ; @demo
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_lshlrev_b32_e32 v1, 3, v0             ; 1: first, no predecessor
	s_waitcnt lgkmcnt(0)
	global_load_dwordx2 v[2:3], v1, s[0:1]
	s_waitcnt vmcnt(0)
	;;#ASMSTART
	v_add_co_u32 v4, vcc, v2, v3            ; 2: reads neither v1
	s_nop 1
	v_addc_co_u32 v5, s[2:3], v3, v2, vcc   ; 3: reads vcc of 2 -> dependent
	;;#ASMEND
	s_nop 0
	;;#ASMSTART
	v_mad_u64_u32 v[6:7], s[6:7], 1, -1, v[4:5]   ; 4: reads v5 of 3 -> dependent
	v_mov_b32_e32 v9, v1                    ; 5: independent
	v_cndmask_b32_e64 v8, v4, v6, s[6:7]    ; 6: s[6:7] is of 4, not of 5 -> independent
	v_cndmask_b32_e64 v10, v8, v9, s[2:3]   ; 7: reads v8 of 6 -> dependent
	;;#ASMEND
.LBB1_2:
	s_nop 0
	v_mov_b32_dpp v11, v10 row_newbcast:3 row_mask:0xf bank_mask:0xf   ; 8: reads v10 of 7 -> dependent
	global_store_dwordx2 v1, v[10:11], s[0:1]
	s_endpgm
	v_mov_b32_e32 v0, v11                   ; behind the first exit: not counted
	s_nop 7
	s_endpgm
"""


def _tool():
    spec = importlib.util.spec_from_file_location("asm_chain_stats", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_counts_of_a_small_listing():
    t = _tool()
    kernels = t.kernel_lines(LISTING.splitlines(), "demoILi4E")
    assert list(kernels) == ["_Z4demoILi4EEvPy"]
    st = t.stats(kernels["_Z4demoILi4EEvPy"])
    assert st["valu"] == 8
    assert st["s_nop"] == 3 and st["s_nop_by_width"] == {"0": 2, "1": 1}
    assert st["asm_blocks"] == 2
    assert st["adj_dep"] == 0.5            # instructions 3, 4, 7 and 8 of 8


def test_operands_and_register_ranges():
    t = _tool()
    assert t.regs("v[6:7]") == {"v6", "v7"} and t.regs("s[2:3]") == {"s2", "s3"} and t.regs("vcc") == {"vcc"} and t.regs("-1") == set()
    w, r = t.writes_reads("v_mad_u64_u32", "v[6:7], s[6:7], v1, -1, v[4:5]")
    assert w == {"v6", "v7", "s6", "s7"} and r == {"v1", "v4", "v5"}
    w, r = t.writes_reads("v_addc_co_u32_e32", "v5, vcc, v3, v2, vcc")
    assert w == {"v5", "vcc"} and r == {"v3", "v2", "vcc"}
    w, r = t.writes_reads("v_cndmask_b32_e32", "v5, v3, v2")
    assert w == {"v5"} and r == {"v3", "v2", "vcc"}


def test_command_line(tmp_path):
    f = tmp_path / "demo.s"
    f.write_text(LISTING)
    out = subprocess.run([sys.executable, str(TOOL), str(f), "demo"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "valu 8" in out.stdout and "s_nop 3 (s_nop 0: 2 s_nop 1: 1)" in out.stdout and "asm_blocks 2" in out.stdout and "adj_dep 0.500" in out.stdout
    assert subprocess.run([sys.executable, str(TOOL), str(f), "absent"], capture_output=True).returncode == 1
