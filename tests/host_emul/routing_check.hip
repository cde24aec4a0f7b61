// TEST INFRASTRUCTURE: the per-cell functions of the runoff routing (noahmp_amd/csrc/nmp_dev_routing.hpp) compiled for the host, applied to
// whole windows.  tests/test_routing.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_routing.hpp"

extern "C" {

// the three reciprocal distances as the entry point makes them
void flow_inverse_distances(float dx, float dy, float* inv3) {
  const nmp::FlowParams p = nmp::flow_params(1, 1, dx, dy);
  inv3[0] = p.inv_x; inv3[1] = p.inv_y; inv3[2] = p.inv_d;
}

void flow_terrain_cells(int ni, int nj, const float* height, float dx, float dy, uint8_t* dir) {
  const nmp::FlowParams p = nmp::flow_params(ni, nj, dx, dy);
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) dir[(long)j * ni + i] = nmp::flow_dir_cell(p, height, i, j);
}

void flow_inmask_cells(int ni, int nj, const uint8_t* dir, uint8_t* inmask) {
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) inmask[(long)j * ni + i] = nmp::flow_inmask_cell(ni, nj, dir, i, j);
}

// npass Jacobi passes between the two planes; returns the plane (0: a, 1: b) that holds the last pass; changed[p] = 1 where pass p changed a cell
int flow_accumulate_passes(int ni, int nj, const uint8_t* inmask, uint32_t* a, uint32_t* b, int npass, uint32_t* changed) {
  uint32_t* old_ = a; uint32_t* new_ = b;
  for (int p = 0; p < npass; p++) {
    changed[p] = 0;
    for (int j = 0; j < nj; j++)
      for (int i = 0; i < ni; i++) {
        const long c = (long)j * ni + i;
        new_[c] = nmp::flow_accumulate_cell(ni, nj, inmask, old_, i, j);
        if (new_[c] != old_[c]) changed[p] = 1;
      }
    uint32_t* t = old_; old_ = new_; new_ = t;
  }
  return old_ == a ? 0 : 1;
}

// one call of noahmp_hip_route_runoff over a window, in the form load_all chooses
void route_cells(int ni, int nj, const uint8_t* inmask, const int32_t* col_index, const float* area, const float* release, float* storage,
                 const float* out_old, float* out_new, const float* runoff_a, const float* runoff_b, float scale, long ncol, int load_all) {
  nmp::RouteCellArgs r;
  r.inmask = inmask; r.col_index = col_index; r.area = area; r.release = release; r.storage = storage; r.out_old = out_old; r.out_new = out_new;
  r.runoff_a = runoff_a; r.runoff_b = runoff_b; r.scale = scale; r.ni = ni; r.nj = nj; r.ncol = ncol;
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) {
      if (load_all) nmp::route_cell<true>(r, i, j);
      else nmp::route_cell<false>(r, i, j);
    }
}

}  // extern "C"
