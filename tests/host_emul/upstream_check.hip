// TEST INFRASTRUCTURE: the per-cell functions of the upstream sums (noahmp_amd/csrc/nmp_dev_accum.hpp) compiled for the host, applied to
// whole windows; the atomic of a pass is a plain add here.  tests/test_upstream.py builds this file on demand and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_accum.hpp"

extern "C" {

void upstream_init_cells(int ni, int nj, const uint8_t* dir, const uint32_t* weight, const uint64_t* inflow, uint64_t* sum, uint64_t* pend_in,
                         uint64_t* pend_out, int32_t* jump, int flags) {
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) nmp::upstream_init_cell(ni, nj, dir, weight, inflow, sum, pend_in, pend_out, jump, flags, i, j);
}

// one pass, cells in ascending (reverse = 0) or descending order: the result must not depend on it.  Returns 1 when a cell pushed.
int upstream_pass_cells(int ni, int nj, uint64_t* sum, uint64_t* pend_in, uint64_t* pend_out, const int32_t* jump_old, int32_t* jump_new,
                        int reverse) {
  const uint32_t n = (uint32_t)ni * (uint32_t)nj;
  int changed = 0;
  for (uint32_t q = 0; q < n; q++)
    if (nmp::upstream_pass_cell(n, sum, pend_in, pend_out, jump_old, jump_new, reverse ? n - 1 - q : q)) changed = 1;
  return changed;
}

}  // extern "C"
