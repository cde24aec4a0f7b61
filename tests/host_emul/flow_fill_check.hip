// TEST INFRASTRUCTURE: the per-cell functions of the depression filling (noahmp_amd/csrc/nmp_dev_flow_fill.hpp) compiled for the host, applied
// to whole windows.  tests/test_flow_fill.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_flow_fill.hpp"

extern "C" {

void fill_up_values(int n, const float* m, float* out) {
  for (int k = 0; k < n; k++) out[k] = nmp::fill_up(m[k]);
}

void fill_lift_values(int n, const float* m, float eps, float* out) {
  for (int k = 0; k < n; k++) out[k] = nmp::fill_lift(m[k], eps);
}

void fill_init_cells(int ni, int nj, const float* height, const uint8_t* outlet, uint8_t* fixed, float* w_old, int flags) {
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) nmp::fill_init_cell(ni, nj, height, outlet, fixed, w_old, flags, i, j);
}

// one pinned pass w_old -> w_new; returns 1 when a word changed
int fill_pass_cells(int ni, int nj, const float* height, const uint8_t* fixed, const float* w_old, float* w_new, float eps) {
  int changed = 0;
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) {
      const long c = (long)j * ni + i;
      w_new[c] = nmp::fill_pass_cell(ni, nj, height, fixed, w_old, eps, i, j);
      if (nmp::fill_bits(w_new[c]) != nmp::fill_bits(w_old[c])) changed = 1;
    }
  return changed;
}

}  // extern "C"
