// wtns_check: a witness against its R1CS on the device (r1cs_check.hip), for the C ABI.  Internal, like zk_internal.h.
#pragma once
#include "zk_internal.h"
#include <string>

namespace zk {

struct R1csCheck;
// field: "BN128" | "BLS12381" | "GL"; the three matrices go to the device here, in CSR form
R1csCheck* r1cs_check_new(const char* field, const void* r1cs, size_t len);
void r1cs_check_free(R1csCheck* c);
void r1cs_check_info(const R1csCheck* c, uint32_t* n_wires, uint64_t* n_constraints, uint64_t* n_custom_uses, uint32_t* n_public);
size_t r1cs_check_value_bytes(const R1csCheck* c);                       // 32 or 8
bool r1cs_check_value_canonical(const R1csCheck* c, const void* value);  // a host value below the modulus
// the report (JSON text); d_witness: n_wires canonical values on the device, borrowed; `st` is the thread's current stream
std::string r1cs_check_run_dev(R1csCheck* c, const void* d_witness, uint32_t max_findings, hipStream_t st);

}  // namespace zk
