// Diffusive-wave routing on the D8 network: backwater (no reference counterpart; the contract is the text in include/noahmp_hip.h, the
// arithmetic is nmp_dev_diffusive.hpp).  noahmp_hip_route_kinematic releases Manning's discharge at the BED slope; here the friction slope
// is the slope of the water surface to the downstream cell, drop + (h - hd), with hd the downstream cell's depth at the end of the call
// before.  A cell whose surface does not stand above its downstream cell's releases nothing, so water pools behind an adverse bed, on a
// flat and in front of a lake that stands above the bed of an inflowing channel (noahmp_hip_lake_depth, noahmp_lakes.hip).
//
// noahmp_hip_flow_drop        once per terrain: ONE launch, one thread per window cell: the bed drop to the downstream cell.  No LDS, no
//                             atomics.
// noahmp_hip_route_diffusive  the per-step call: ONE launch, one thread per window cell in row-major order.  The gather, the plane loads,
//                             the LDS libm tables and the scheduling barrier are those of noahmp_route_kinematic_kernel; one sqrtf and
//                             one more division per cell with a downstream cell.  The ONE new access is hd, whose address depends on
//                             dir[c].  NMP_DIFFUSIVE_LOAD_ALL = 0: one dependent load (dir[c] must have arrived before it is issued);
//                             1: eight loads from addresses made legal, issued with the gather, then a select by k.  The default is
//                             the faster one on an MI355X (profiles/diffusive_bench.md); tests build the other as a variant library.
//                             The four diag words are integer results: the maximum by a butterfly and the three counts by ballots
//                             within a wave, the four waves of a workgroup through LDS, and thread 0 sends at most one atomicMax and
//                             three atomicAdd, none where there is nothing to report and no atomicMax that cannot raise the word.
// Arguments go by value, nothing is allocated, nothing waits on the host.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_diffusive.hpp"
#include "nmp_engine_host.hpp"

// 1: a scheduling barrier between the loads of a cell and its arithmetic (the loads are in flight before the powf_); 0: the compiler's order
#ifndef NMP_DIFFUSIVE_PIN
#define NMP_DIFFUSIVE_PIN 1
#endif
// the downstream depth: 0: one load at an address that depends on dir[c]; 1: eight loads from addresses made legal, then a select
#ifndef NMP_DIFFUSIVE_LOAD_ALL
#define NMP_DIFFUSIVE_LOAD_ALL 0
#endif

using namespace nmp;
using nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::bad_spacing, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
static_assert(kBlock % kWave == 0, "whole waves");

struct DropKArgs {
  FlowDropArgs g;
  unsigned ncell;
};

__global__ void __launch_bounds__(kBlock) noahmp_flow_drop_kernel(const DropKArgs k) {
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;  // c < ni*nj <= 2^31 - 1: the index and its division fit 32 bits
  if (c >= k.ncell) return;
  const int j = (int)(c / (unsigned)k.g.ni), i = (int)(c - (unsigned)j * (unsigned)k.g.ni);
  flow_drop_cell(k.g, i, j);
}

struct DiffusiveKArgs {
  DiffusiveCellArgs r;
  uint32_t* diag;
  unsigned ncell;
};

__global__ void __launch_bounds__(kBlock) noahmp_route_diffusive_kernel(const DiffusiveKArgs k) {
  libm::libm_stage_tables();                                       // holds a __syncthreads(): every thread of the workgroup, before any return
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  DiffusiveReport rep;
  rep.cr_bits = 0u; rep.capped = 0u; rep.limited = 0u; rep.blocked = 0u;
  if (c < k.ncell) {                                               // a predicate, not a return: every lane reaches the reduction
    const int j = (int)(c / (unsigned)k.r.ni), i = (int)(c - (unsigned)j * (unsigned)k.r.ni);
    rep = diffusive_cell<NMP_DIFFUSIVE_PIN != 0, NMP_DIFFUSIVE_LOAD_ALL != 0>(k.r, i, j);
  }
  if (!k.diag) return;                                             // the same for every thread of the launch
  const unsigned long long capped = __ballot(rep.capped != 0u);
  const unsigned long long limited = __ballot(rep.limited != 0u);
  const unsigned long long blocked = __ballot(rep.blocked != 0u);
  uint32_t mx = rep.cr_bits;
#pragma unroll
  for (int w = kWave / 2; w >= 1; w >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)mx, w, kWave);
    mx = other > mx ? other : mx;
  }
  // the waves of the workgroup through LDS, then thread 0: every atomic of a launch goes to the same four words, which the memory side
  // serialises, so there are as few as the words allow
  __shared__ uint32_t s_max[kWaves], s_cnt[3][kWaves];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_max[threadIdx.x / kWave] = mx;
    s_cnt[0][threadIdx.x / kWave] = (uint32_t)__popcll(capped);
    s_cnt[1][threadIdx.x / kWave] = (uint32_t)__popcll(limited);
    s_cnt[2][threadIdx.x / kWave] = (uint32_t)__popcll(blocked);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t bmax = 0u, bcnt[3] = {0u, 0u, 0u};
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    bmax = s_max[w] > bmax ? s_max[w] : bmax;
#pragma unroll
    for (int n = 0; n < 3; n++) bcnt[n] += s_cnt[n][w];
  }
  // diag[0] only grows during a launch, so a value read earlier is a lower bound of the word: a maximum that does not exceed it cannot
  // change the word and sends nothing
  if (bmax && bmax > __hip_atomic_load(k.diag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(k.diag, bmax);
#pragma unroll
  for (int n = 0; n < 3; n++)
    if (bcnt[n]) atomicAdd(k.diag + 1 + n, bcnt[n]);
}

const char* kWindowText = "window: ni, nj >= 0 and ni*nj <= 2^31 - 1";

// two planes of na and nb bytes that share a byte (or start at the same address, whatever the sizes)
bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  if (!a || !b) return false;
  return x == y || (x < y ? y - x < na : x - y < nb);
}

}  // namespace

extern "C" {

int noahmp_hip_flow_drop(const noahmp_flow_drop* fd, void* stream) {
  const char* me = "noahmp_hip_flow_drop";
  if (!fd) return refuse(-105, "%s: the argument block is NULL", me);
  if (!fd->dir || !fd->drop) return refuse(-105, "%s: dir and drop are required", me);
  if ((fd->height != nullptr) == (fd->slope != nullptr)) return refuse(-105, "%s: exactly one of height and slope is given", me);
  if (bad_window(fd->ni, fd->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (bad_spacing(fd->dx, fd->dy)) return refuse(-105, "%s: dx and dy must be finite and > 0", me);
  const uint64_t n = (uint64_t)fd->ni * (uint64_t)fd->nj;
  if (overlap(fd->drop, 4u * n, fd->height, 4u * n) || overlap(fd->drop, 4u * n, fd->slope, 4u * n) || overlap(fd->drop, 4u * n, fd->dir, n))
    return refuse(-105, "%s: drop must not share words with height, slope or dir (a cell reads its neighbour's height)", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)n;
  if (ncell == 0) return 0;
  DropKArgs k;
  memset(&k, 0, sizeof(k));
  k.g.height = fd->height; k.g.slope = fd->slope; k.g.dir = fd->dir; k.g.drop = fd->drop;
  k.g.ni = fd->ni; k.g.nj = fd->nj; k.g.dx = fd->dx; k.g.dy = fd->dy; k.g.d = channel_diagonal(fd->dx, fd->dy);
  k.ncell = ncell;
  hipLaunchKernelGGL(noahmp_flow_drop_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_route_diffusive(const noahmp_route_diffusive* r, int64_t ncol, void* stream) {
  const char* me = "noahmp_hip_route_diffusive";
  if (!r) return refuse(-105, "%s: the argument block is NULL", me);
  if (!r->inmask || !r->col_index || !r->dir || !r->area || !r->width || !r->length || !r->conv || !r->manning || !r->drop || !r->storage ||
      !r->out_old || !r->out_new || !r->runoff_a || !r->depth_old || !r->depth_new)
    return refuse(-105, "%s: inmask, col_index, dir, area, width, length, conv, manning, drop, storage, out_old, out_new, runoff_a, depth_old and depth_new are required", me);
  if (r->out_old == r->out_new) return refuse(-105, "%s: out_old and out_new must be different planes (a cell reads its neighbours' out_old)", me);
  if (r->depth_old == r->depth_new)
    return refuse(-105, "%s: depth_old and depth_new must be different planes (a cell reads its downstream cell's depth_old)", me);
  if (bad_window(r->ni, r->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (bad_count(ncol)) return refuse(-105, "%s: ncol: 0 .. 2^31 - 1 columns", me);
  if (!(isfinite(r->dt) && r->dt > 0.f)) return refuse(-105, "%s: dt must be finite and > 0", me);
  if (!(isfinite(r->limit) && r->limit > 0.f)) return refuse(-105, "%s: limit must be finite and > 0", me);
  const uint64_t n = (uint64_t)r->ni * (uint64_t)r->nj;
  if (overlap(r->depth_new, 4u * n, r->storage, 4u * n) || overlap(r->depth_new, 4u * n, r->out_old, 4u * n) ||
      overlap(r->depth_new, 4u * n, r->out_new, 4u * n) || overlap(r->depth_new, 4u * n, r->depth_old, 4u * n))
    return refuse(-105, "%s: depth_new must not share words with storage, out_old, out_new or depth_old", me);
  if (((uintptr_t)r->diag & 3u) != 0) return refuse(-105, "%s: diag is four 4-byte words and must be aligned to 4 bytes", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)n;
  if (ncell == 0) return 0;
  DiffusiveKArgs k;
  memset(&k, 0, sizeof(k));
  k.r.inmask = r->inmask; k.r.col_index = r->col_index; k.r.dir = r->dir; k.r.area = r->area; k.r.width = r->width; k.r.length = r->length;
  k.r.conv = r->conv; k.r.manning = r->manning; k.r.drop = r->drop;
  k.r.storage = r->storage; k.r.out_old = r->out_old; k.r.out_new = r->out_new; k.r.runoff_a = r->runoff_a; k.r.runoff_b = r->runoff_b;
  k.r.depth_old = r->depth_old; k.r.depth_new = r->depth_new; k.r.scale = r->scale; k.r.dt = r->dt; k.r.limit = r->limit;
  k.r.ni = r->ni; k.r.nj = r->nj; k.r.ncol = (long)ncol;
  k.diag = r->diag;
  k.ncell = ncell;
  hipLaunchKernelGGL(noahmp_route_diffusive_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
