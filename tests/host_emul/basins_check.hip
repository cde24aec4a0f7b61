// TEST INFRASTRUCTURE: the per-cell functions of the watershed delineation (noahmp_amd/csrc/nmp_dev_basins.hpp) compiled for the host, applied
// to whole windows.  tests/test_basins.py builds this file on demand and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_basins.hpp"

extern "C" {

void basin_init_cells(int ni, int nj, const uint8_t* dir, const int32_t* seed, void* state, int32_t* label, int32_t* dist, int flags) {
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) nmp::basin_init_cell(ni, nj, dir, seed, (nmp::BasinState*)state, label, dist, flags, i, j);
}

// one pass state_old -> state_new; returns 1 when a pointer moved
int basin_jump_cells(int ni, int nj, const void* state_old, void* state_new) {
  const uint32_t n = (uint32_t)ni * (uint32_t)nj;
  int changed = 0;
  for (uint32_t c = 0; c < n; c++)
    if (nmp::basin_jump_cell(n, (const nmp::BasinState*)state_old, (nmp::BasinState*)state_new, c)) changed = 1;
  return changed;
}

// resolve in place, cells in ascending (reverse = 0) or descending order: the result must not depend on it.  Returns 1 when a label changed.
int basin_resolve_cells(int ni, int nj, const void* state, int32_t* label, int32_t* dist, int reverse) {
  const uint32_t n = (uint32_t)ni * (uint32_t)nj;
  int changed = 0;
  for (uint32_t q = 0; q < n; q++)
    if (nmp::basin_resolve_cell(n, (const nmp::BasinState*)state, label, dist, reverse ? n - 1 - q : q)) changed = 1;
  return changed;
}

}  // extern "C"
