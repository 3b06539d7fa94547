// pil_verify: what the check-program generator (starkinfo_gen.hip), the interpreter (expr_bytecode.hip) and the checker
// (pil_check.hip) share.  Internal, like zk_internal.h.
#pragma once
#include "zk_internal.h"
#include "../../include/zkgpu.h"
#include <string>
#include <vector>

namespace zk {

// `check1 id, src`: an instruction of the checker's programs only.  As a zk_instr: op = ZK_OP_CHECK1, src[0] = the dim-1 value,
// dest.id = the identity's index, dest.stride = the number of identities of the program.  zk_program_assemble and
// zk_program_compile do not know it; bytecode_assemble takes it when `checker` is set.
constexpr uint32_t ZK_OP_CHECK1 = 64;
// buffer slots of a check program (zk_eval_ctx.bufs)
enum : uint32_t { PC_BUF_CM = 0, PC_BUF_CONST = 1, PC_BUF_SCRATCH = 2, PC_BUF_PUBLICS = 3, PC_BUF_RESULT = 15 };
// PC_BUF_RESULT: [3][n_ids] words -- count[id] (starts 0), first[id] (starts ~0), value[id]

Bytecode* bytecode_assemble(const zk_instr* code, uint32_t n_instr, bool checker);
// the second, tiny launch of a check program: one wave per identity, at row first[id], leaves value[id] (identities with count 0 are skipped)
void bytecode_run_first(Bytecode* b, const void* ctx, uint32_t nbits_domain, uint64_t next, uint32_t n_ids, hipStream_t st);

enum { PC_PLOOKUP = 0, PC_PERMUTATION = 1, PC_CONNECTION = 2 };
struct PilCheckSrc { std::string file; long long line = 0; };
// One set identity: its program fills the row-major scratch section [N][width].
//   plookup / permutation: columns f[0..k) | selF | t[0..k) | selT   (width 2k + 2; an absent selector is the number 1)
//   connection:            columns pols[0..k) | connections[0..k)    (width 2k)
struct PilCheckSet {
    int kind = 0; uint32_t index = 0, k = 0, width = 0;
    bool has_self = false, has_selt = false;
    PilCheckSrc src;
    std::vector<zk_instr> code;
};
struct PilCheckPublic { bool im = false; uint32_t pol_id = 0; uint64_t idx = 0; std::vector<zk_instr> code; };   // im: the program leaves the value in PC_BUF_PUBLICS
struct PilCheckProgram {
    uint64_t n = 0; uint32_t nbits = 0, n_cm = 0, n_const = 0;
    std::vector<PilCheckPublic> publics;
    std::vector<zk_instr> identities;            // every polynomial identity: its expression, then its check1
    std::vector<PilCheckSrc> identity_src;
    std::vector<PilCheckSet> sets;               // plookups, permutations, connections, each in PIL order
};
PilCheckProgram pil_check_generate(const std::string& pil_json);

// the checker (pil_check.hip): programs assembled at construction (no GPU), buffers from the pool from the first run on
struct PilCheck;
PilCheck* pil_check_new(const char* pil_json);
void pil_check_free(PilCheck* p);
const char* pil_check_listing(const PilCheck* p);
uint64_t pil_check_rows(const PilCheck* p);
void pil_check_widths(const PilCheck* p, uint32_t* n_const, uint32_t* n_cm);
// the report (JSON text); the constants and the trace are borrowed; `st` is the thread's current stream
std::string pil_check_run_dev(PilCheck* p, const u64* d_const, const u64* d_cm, uint64_t n_rows, hipStream_t st);

}  // namespace zk
