// TEST INFRASTRUCTURE: the per-cell functions of the kinematic-wave routing (noahmp_amd/csrc/nmp_dev_channel.hpp) compiled for the host,
// applied to whole windows.  tests/test_channel.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_channel.hpp"

extern "C" {

// one call of noahmp_hip_flow_channel over a window; exactly one of height and slope
void channel_geom_cells(int ni, int nj, const float* height, const float* slope, const uint8_t* dir, const float* manning, float* length,
                        float* conv, float dx, float dy, float smin) {
  nmp::ChannelGeomArgs g;
  g.height = height; g.slope = slope; g.dir = dir; g.manning = manning; g.length = length; g.conv = conv;
  g.p = nmp::flow_params(ni, nj, dx, dy);
  g.dx = dx; g.dy = dy; g.d = nmp::channel_diagonal(dx, dy); g.smin = smin;
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) nmp::channel_geom_cell(g, i, j);
}

// one call of noahmp_hip_route_kinematic over a window; diag (two words, or NULL) receives the maximum and the count as the atomics give them
void kinematic_cells(int ni, int nj, const uint8_t* inmask, const int32_t* col_index, const float* area, const float* width, const float* length,
                     const float* conv, float* storage, const float* out_old, float* out_new, const float* runoff_a, const float* runoff_b,
                     float* depth, uint32_t* diag, float scale, float dt, long ncol) {
  nmp::KinematicCellArgs r;
  r.inmask = inmask; r.col_index = col_index; r.area = area; r.width = width; r.length = length; r.conv = conv; r.storage = storage;
  r.out_old = out_old; r.out_new = out_new; r.runoff_a = runoff_a; r.runoff_b = runoff_b; r.depth = depth; r.scale = scale; r.dt = dt;
  r.ni = ni; r.nj = nj; r.ncol = ncol;
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) {
      const nmp::KinematicReport rep = nmp::kinematic_cell<true>(r, i, j);
      if (!diag) continue;
      if (rep.cr_bits > diag[0]) diag[0] = rep.cr_bits;
      diag[1] += rep.capped;
    }
}

}  // extern "C"
