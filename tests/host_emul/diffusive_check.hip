// TEST INFRASTRUCTURE: the per-cell functions of the diffusive-wave routing (noahmp_amd/csrc/nmp_dev_diffusive.hpp) and the per-entry
// function of noahmp_hip_lake_depth (nmp_dev_lakes.hpp) compiled for the host, applied to whole windows and lists.
// tests/test_diffusive.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_diffusive.hpp"
#include "nmp_dev_lakes.hpp"

namespace {

template <bool LOAD_ALL_HD>
void cells(const nmp::DiffusiveCellArgs& r, uint32_t* diag) {
  for (int j = 0; j < r.nj; j++)
    for (int i = 0; i < r.ni; i++) {
      const nmp::DiffusiveReport rep = nmp::diffusive_cell<true, LOAD_ALL_HD>(r, i, j);
      if (!diag) continue;
      if (rep.cr_bits > diag[0]) diag[0] = rep.cr_bits;
      diag[1] += rep.capped;
      diag[2] += rep.limited;
      diag[3] += rep.blocked;
    }
}

}  // namespace

extern "C" {

// one call of noahmp_hip_flow_drop over a window; exactly one of height and slope
void flow_drop_cells(int ni, int nj, const float* height, const float* slope, const uint8_t* dir, float* drop, float dx, float dy) {
  nmp::FlowDropArgs g;
  g.height = height; g.slope = slope; g.dir = dir; g.drop = drop;
  g.ni = ni; g.nj = nj; g.dx = dx; g.dy = dy; g.d = nmp::channel_diagonal(dx, dy);
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) nmp::flow_drop_cell(g, i, j);
}

// one call of noahmp_hip_route_diffusive over a window; diag (four words, or NULL) receives the maximum and the counts as the atomics
// give them; load_all: the form of the downstream-depth access
void diffusive_cells(int ni, int nj, const uint8_t* inmask, const int32_t* col_index, const uint8_t* dir, const float* area, const float* width,
                     const float* length, const float* conv, const float* manning, const float* drop, float* storage, const float* out_old,
                     float* out_new, const float* runoff_a, const float* runoff_b, const float* depth_old, float* depth_new, uint32_t* diag,
                     float scale, float dt, float limit, long ncol, int load_all) {
  nmp::DiffusiveCellArgs r;
  r.inmask = inmask; r.col_index = col_index; r.dir = dir; r.area = area; r.width = width; r.length = length; r.conv = conv;
  r.manning = manning; r.drop = drop; r.storage = storage; r.out_old = out_old; r.out_new = out_new; r.runoff_a = runoff_a;
  r.runoff_b = runoff_b; r.depth_old = depth_old; r.depth_new = depth_new; r.scale = scale; r.dt = dt; r.limit = limit;
  r.ni = ni; r.nj = nj; r.ncol = ncol;
  if (load_all) cells<true>(r, diag);
  else cells<false>(r, diag);
}

// one call of noahmp_hip_lake_depth over a member list
void lake_depth_entries(const int32_t* member_cell, const int32_t* member_lake, long long nmember, const long long* volume, const double* area,
                        const double* datum, const float* bed, float* depth, int nlake, long long ncell, double q) {
  nmp::LakeDepthArgs t;
  t.member_cell = member_cell; t.member_lake = member_lake; t.volume = volume; t.area = area; t.datum = datum; t.bed = bed; t.depth = depth;
  t.nmember = nmember; t.ncell = ncell; t.nlake = nlake; t.q = q;
  for (long long e = 0; e < nmember; e++) nmp::lake_depth_entry(t, e);
}

}  // extern "C"
