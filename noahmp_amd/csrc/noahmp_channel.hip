// Kinematic-wave routing with Manning friction on the D8 network (no reference counterpart; the contract is the text in
// include/noahmp_hip.h, the arithmetic is nmp_dev_channel.hpp).  Where noahmp_hip_route_runoff releases a constant fraction, here a cell
// releases Q*dt with Q = conv * R^(2/3) * A of a rectangular section whose depth follows from what the cell holds: a flood wave travels
// faster than a trickle.
//
// noahmp_hip_flow_channel     once per terrain: ONE launch, one thread per window cell: the flow length along the cell's direction and
//                             conv = sqrt(max(s, smin)) / n.  No LDS, no atomics.
// noahmp_hip_route_kinematic  the per-step call: ONE launch, one thread per window cell in row-major order.  The gather of
//                             noahmp_hip_route_runoff (eight loads from addresses made legal, then selects), the plane loads, one
//                             libm::powf_ and three IEEE divisions per cell that holds water.  The libm tables are staged in LDS by
//                             every workgroup (a barrier: every thread passes it before any can leave).  The two diag words are integer
//                             results: the lanes of a wave are reduced first (a ballot for the count, a butterfly for the maximum), the
//                             four waves of a workgroup through LDS, and thread 0 sends at most one atomicMax and one atomicAdd, none
//                             where the workgroup has nothing to report and no atomicMax that cannot raise the word.  Lanes past the
//                             last cell and ring cells take part with 0.  (One atomic pair per WAVE where every wave reports cost
//                             2.50 / 0.317 ms at 7 077 888 / 884 736 cells against 0.072 / 0.012 ms without diag: same-address
//                             atomics serialise at the memory side.)
// Arguments go by value, nothing is allocated, nothing waits on the host.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_channel.hpp"
#include "nmp_engine_host.hpp"

// 1: a scheduling barrier between the loads of a cell and its arithmetic (the loads are in flight before the powf_); 0: the compiler's order
#ifndef NMP_CHANNEL_PIN
#define NMP_CHANNEL_PIN 1
#endif

using namespace nmp;
using nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::bad_spacing, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
static_assert(kBlock % kWave == 0, "whole waves");

struct ChannelKArgs {
  ChannelGeomArgs g;
  unsigned ncell;
};

__global__ void __launch_bounds__(kBlock) noahmp_flow_channel_kernel(const ChannelKArgs k) {
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;  // c < ni*nj <= 2^31 - 1: the index and its division fit 32 bits
  if (c >= k.ncell) return;
  const int j = (int)(c / (unsigned)k.g.p.ni), i = (int)(c - (unsigned)j * (unsigned)k.g.p.ni);
  channel_geom_cell(k.g, i, j);
}

struct KinematicKArgs {
  KinematicCellArgs r;
  uint32_t* diag;
  unsigned ncell;
};

__global__ void __launch_bounds__(kBlock) noahmp_route_kinematic_kernel(const KinematicKArgs k) {
  libm::libm_stage_tables();                                       // holds a __syncthreads(): every thread of the workgroup, before any return
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  KinematicReport rep;
  rep.cr_bits = 0u; rep.capped = 0u;
  if (c < k.ncell) {                                               // a predicate, not a return: every lane reaches the reduction
    const int j = (int)(c / (unsigned)k.r.ni), i = (int)(c - (unsigned)j * (unsigned)k.r.ni);
    rep = kinematic_cell<NMP_CHANNEL_PIN != 0>(k.r, i, j);
  }
  if (!k.diag) return;                                             // the same for every thread of the launch
  const unsigned long long capped = __ballot(rep.capped != 0u);
  uint32_t mx = rep.cr_bits;
#pragma unroll
  for (int w = kWave / 2; w >= 1; w >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)mx, w, kWave);
    mx = other > mx ? other : mx;
  }
  // the waves of the workgroup through LDS, then thread 0: every atomic of a launch goes to the same two words, which the memory side
  // serialises, so there are as few as the words allow
  __shared__ uint32_t s_max[kBlock / kWave], s_cnt[kBlock / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_max[threadIdx.x / kWave] = mx;
    s_cnt[threadIdx.x / kWave] = (uint32_t)__popcll(capped);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t bmax = 0u, bcnt = 0u;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; w++) {
    bmax = s_max[w] > bmax ? s_max[w] : bmax;
    bcnt += s_cnt[w];
  }
  // diag[0] only grows during a launch, so a value read earlier is a lower bound of the word: a maximum that does not exceed it cannot
  // change the word and sends nothing
  if (bmax && bmax > __hip_atomic_load(k.diag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(k.diag, bmax);
  if (bcnt) atomicAdd(k.diag + 1, bcnt);
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

int noahmp_hip_flow_channel(const noahmp_flow_channel* fc, void* stream) {
  const char* me = "noahmp_hip_flow_channel";
  if (!fc) return refuse(-105, "%s: the argument block is NULL", me);
  if (!fc->dir || !fc->manning || !fc->length || !fc->conv) return refuse(-105, "%s: dir, manning, length and conv are required", me);
  if ((fc->height != nullptr) == (fc->slope != nullptr)) return refuse(-105, "%s: exactly one of height and slope is given", me);
  if (bad_window(fc->ni, fc->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (bad_spacing(fc->dx, fc->dy)) return refuse(-105, "%s: dx and dy must be finite and > 0", me);
  if (!(isfinite(fc->smin) && fc->smin > 0.f)) return refuse(-105, "%s: smin must be finite and > 0", me);
  const uint64_t n = (uint64_t)fc->ni * (uint64_t)fc->nj;
  if (overlap(fc->length, 4u * n, fc->conv, 4u * n)) return refuse(-105, "%s: length and conv must be different planes", me);
  const void* outs[2] = {fc->length, fc->conv};
  for (const void* o : outs) {
    if (overlap(o, 4u * n, fc->height, 4u * n) || overlap(o, 4u * n, fc->slope, 4u * n) || overlap(o, 4u * n, fc->manning, 4u * n) ||
        overlap(o, 4u * n, fc->dir, n))
      return refuse(-105, "%s: length and conv must not share words with height, slope, dir or manning (a cell reads its neighbour's height)", me);
  }
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)n;
  if (ncell == 0) return 0;
  ChannelKArgs k;
  memset(&k, 0, sizeof(k));
  k.g.height = fc->height; k.g.slope = fc->slope; k.g.dir = fc->dir; k.g.manning = fc->manning; k.g.length = fc->length; k.g.conv = fc->conv;
  k.g.p = flow_params(fc->ni, fc->nj, fc->dx, fc->dy);
  k.g.dx = fc->dx; k.g.dy = fc->dy; k.g.d = channel_diagonal(fc->dx, fc->dy); k.g.smin = fc->smin;
  k.ncell = ncell;
  hipLaunchKernelGGL(noahmp_flow_channel_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_route_kinematic(const noahmp_route_kinematic* r, int64_t ncol, void* stream) {
  const char* me = "noahmp_hip_route_kinematic";
  if (!r) return refuse(-105, "%s: the argument block is NULL", me);
  if (!r->inmask || !r->col_index || !r->area || !r->width || !r->length || !r->conv || !r->storage || !r->out_old || !r->out_new || !r->runoff_a)
    return refuse(-105, "%s: inmask, col_index, area, width, length, conv, storage, out_old, out_new and runoff_a are required", me);
  if (r->out_old == r->out_new) return refuse(-105, "%s: out_old and out_new must be different planes (a cell reads its neighbours' out_old)", me);
  if (bad_window(r->ni, r->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (bad_count(ncol)) return refuse(-105, "%s: ncol: 0 .. 2^31 - 1 columns", me);
  if (!(isfinite(r->dt) && r->dt > 0.f)) return refuse(-105, "%s: dt must be finite and > 0", me);
  const uint64_t n = (uint64_t)r->ni * (uint64_t)r->nj;
  if (overlap(r->depth, 4u * n, r->storage, 4u * n) || overlap(r->depth, 4u * n, r->out_old, 4u * n) || overlap(r->depth, 4u * n, r->out_new, 4u * n))
    return refuse(-105, "%s: depth must not share words with storage, out_old or out_new", me);
  if (((uintptr_t)r->diag & 3u) != 0) return refuse(-105, "%s: diag is two 4-byte words and must be aligned to 4 bytes", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const unsigned ncell = (unsigned)n;
  if (ncell == 0) return 0;
  KinematicKArgs k;
  memset(&k, 0, sizeof(k));
  k.r.inmask = r->inmask; k.r.col_index = r->col_index; k.r.area = r->area; k.r.width = r->width; k.r.length = r->length; k.r.conv = r->conv;
  k.r.storage = r->storage; k.r.out_old = r->out_old; k.r.out_new = r->out_new; k.r.runoff_a = r->runoff_a; k.r.runoff_b = r->runoff_b;
  k.r.depth = r->depth; k.r.scale = r->scale; k.r.dt = r->dt;
  k.r.ni = r->ni; k.r.nj = r->nj; k.r.ncol = (long)ncol;
  k.diag = r->diag;
  k.ncell = ncell;
  hipLaunchKernelGGL(noahmp_route_kinematic_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
