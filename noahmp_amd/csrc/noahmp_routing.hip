// Runoff routing on a D8 network (no reference counterpart; the contract is the text in include/noahmp_hip.h, the arithmetic is
// nmp_dev_routing.hpp): directions of steepest strict descent, the byte of upstream neighbours, the upstream cell count, and the per-step
// linear reservoirs.
//
// All four: ONE launch per call, one thread per window cell in row-major order.  The lanes of a wave are neighbours along i, so each of
// the 8 possible neighbour reads is a row segment shifted by +-1 -- coalesced, and shared with the neighbouring rows' workgroups through
// the L2: from memory a plane is read about once.  A cell GATHERS (it sums what its upstream neighbours released, in ascending k); nothing
// is pushed, so there are no float atomics and the bits do not depend on the order of arrival.
// noahmp_hip_route_runoff has two forms of the neighbour loads (nmp_dev_routing.hpp::route_cell): the library launches the one that
// loads all eight neighbours and selects (23 VGPRs, no scratch, 8 waves per SIMD); -DNMP_ROUTE_LOAD_ALL=0 builds the other, which loads
// only the neighbours whose bit is set (14 VGPRs; mean in-degree about 1, but eight branches in a row, each waiting for its own load).
// Same bits.  The first is the faster by a factor of 1.8 at 7 077 888 cells (the figures: profiles/routing_bench.md), so it is the library's.
// No kernel uses LDS, a barrier, atomics or scratch.  Arguments go by value, nothing is allocated, nothing waits on the host.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_routing.hpp"
#include "nmp_engine_host.hpp"

#ifndef NMP_ROUTE_LOAD_ALL
#define NMP_ROUTE_LOAD_ALL 1
#endif

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::bad_spacing, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;

// c < ni*nj <= 2^31 - 1: the cell index and its division fit 32 bits
#define NMP_ROUTE_CELL_INDEX(ncell, ni)                                 \
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;       \
  if (c >= (ncell)) return;                                             \
  const int j = (int)(c / (unsigned)(ni)), i = (int)(c - (unsigned)j * (unsigned)(ni))

struct FlowTerrainKArgs {
  const float* height; uint8_t* dir;
  unsigned ncell;
  FlowParams p;
};

__global__ void __launch_bounds__(kBlock) noahmp_flow_terrain_kernel(const FlowTerrainKArgs k) {
  NMP_ROUTE_CELL_INDEX(k.ncell, k.p.ni);
  k.dir[c] = flow_dir_cell(k.p, k.height, i, j);
}

struct FlowInmaskKArgs {
  const uint8_t* dir; uint8_t* inmask;
  unsigned ncell;
  int ni, nj;
};

__global__ void __launch_bounds__(kBlock) noahmp_flow_inmask_kernel(const FlowInmaskKArgs k) {
  NMP_ROUTE_CELL_INDEX(k.ncell, k.ni);
  k.inmask[c] = flow_inmask_cell(k.ni, k.nj, k.dir, i, j);
}

struct FlowAccKArgs {
  const uint8_t* inmask; const uint32_t* acc_old; uint32_t* acc_new; uint32_t* changed;
  unsigned ncell;
  int ni, nj;
};

__global__ void __launch_bounds__(kBlock) noahmp_flow_accumulate_kernel(const FlowAccKArgs k) {
  NMP_ROUTE_CELL_INDEX(k.ncell, k.ni);
  const uint32_t a = flow_accumulate_cell(k.ni, k.nj, k.inmask, k.acc_old, i, j);
  k.acc_new[c] = a;
  if (a != k.acc_old[c]) *k.changed = 1u;                          // every writer stores the same word: no atomic
}

struct RouteKArgs {
  RouteCellArgs r;
  unsigned ncell;
};

__global__ void __launch_bounds__(kBlock) noahmp_route_runoff_kernel(const RouteKArgs k) {
  NMP_ROUTE_CELL_INDEX(k.ncell, k.r.ni);
  route_cell<NMP_ROUTE_LOAD_ALL != 0>(k.r, i, j);
}

const char* kWindowText = "window: ni, nj >= 0 and ni*nj <= 2^31 - 1";

}  // namespace

extern "C" {

int noahmp_hip_flow_terrain(const noahmp_flow_terrain* ft, void* stream) {
  const char* me = "noahmp_hip_flow_terrain";
  if (!ft) return refuse(-105, "%s: the argument block is NULL", me);
  if (!ft->height || !ft->dir) return refuse(-105, "%s: height and dir are required", me);
  if (bad_window(ft->ni, ft->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (bad_spacing(ft->dx, ft->dy)) return refuse(-105, "%s: dx and dy must be finite and > 0", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)ft->ni * (unsigned)ft->nj;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  FlowTerrainKArgs k;
  memset(&k, 0, sizeof(k));
  k.height = ft->height; k.dir = ft->dir; k.ncell = ncell;
  k.p = flow_params(ft->ni, ft->nj, ft->dx, ft->dy);
  hipLaunchKernelGGL(noahmp_flow_terrain_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_flow_inmask(const uint8_t* dir, uint8_t* inmask, int32_t ni, int32_t nj, void* stream) {
  const char* me = "noahmp_hip_flow_inmask";
  if (!dir || !inmask) return refuse(-105, "%s: dir and inmask are required", me);
  if (dir == inmask) return refuse(-105, "%s: dir and inmask must be different planes (a cell reads its neighbours' dir)", me);
  if (bad_window(ni, nj)) return refuse(-105, "%s: %s", me, kWindowText);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)ni * (unsigned)nj;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  FlowInmaskKArgs k;
  memset(&k, 0, sizeof(k));
  k.dir = dir; k.inmask = inmask; k.ncell = ncell; k.ni = ni; k.nj = nj;
  hipLaunchKernelGGL(noahmp_flow_inmask_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_flow_accumulate(const uint8_t* inmask, const uint32_t* acc_old, uint32_t* acc_new, uint32_t* changed, int32_t ni, int32_t nj,
                               void* stream) {
  const char* me = "noahmp_hip_flow_accumulate";
  if (!inmask || !acc_old || !acc_new || !changed) return refuse(-105, "%s: inmask, acc_old, acc_new and changed are required", me);
  if (acc_old == acc_new) return refuse(-105, "%s: acc_old and acc_new must be different planes (a Jacobi pass)", me);
  if (bad_window(ni, nj)) return refuse(-105, "%s: %s", me, kWindowText);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)ni * (unsigned)nj;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  FlowAccKArgs k;
  memset(&k, 0, sizeof(k));
  k.inmask = inmask; k.acc_old = acc_old; k.acc_new = acc_new; k.changed = changed; k.ncell = ncell; k.ni = ni; k.nj = nj;
  hipLaunchKernelGGL(noahmp_flow_accumulate_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_route_runoff(const noahmp_route* r, int64_t ncol, void* stream) {
  const char* me = "noahmp_hip_route_runoff";
  if (!r) return refuse(-105, "%s: the argument block is NULL", me);
  if (!r->inmask || !r->col_index || !r->area || !r->release || !r->storage || !r->out_old || !r->out_new || !r->runoff_a)
    return refuse(-105, "%s: inmask, col_index, area, release, storage, out_old, out_new and runoff_a are required", me);
  if (r->out_old == r->out_new) return refuse(-105, "%s: out_old and out_new must be different planes (a cell reads its neighbours' out_old)", me);
  if (bad_window(r->ni, r->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (bad_count(ncol)) return refuse(-105, "%s: ncol: 0 .. 2^31 - 1 columns", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)r->ni * (unsigned)r->nj;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  RouteKArgs k;
  memset(&k, 0, sizeof(k));
  k.r.inmask = r->inmask; k.r.col_index = r->col_index; k.r.area = r->area; k.r.release = r->release; k.r.storage = r->storage;
  k.r.out_old = r->out_old; k.r.out_new = r->out_new; k.r.runoff_a = r->runoff_a; k.r.runoff_b = r->runoff_b; k.r.scale = r->scale;
  k.r.ni = r->ni; k.r.nj = r->nj; k.r.ncol = (long)ncol;
  k.ncell = ncell;
  hipLaunchKernelGGL(noahmp_route_runoff_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
