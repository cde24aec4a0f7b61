// Lakes on the D8 network: level-pool storage and outflow (no reference counterpart; the contract is the text in include/noahmp_hip.h, the
// arithmetic is nmp_dev_lakes.hpp).  Members of a lake have release == 0 or conv == 0: the routing kernels, which stay as they are, let
// them hold everything that reaches them and release exactly +0.  After each routing launch:
//
// noahmp_hip_lake_take     ONE launch, one thread per entry of the member list: the whole quanta of a member's storage leave the cell
//                          and are added to the lake's inflow word, a 64-bit INTEGER sum.  Every atomic of a lake goes to one word, and
//                          same-address atomics serialise at the memory side (noahmp_channel.hip: about 23 ns each), so there are as few
//                          as the list allows: a wave whose valid entries all name one lake is reduced with a butterfly, the waves of a
//                          workgroup go through LDS, and thread 0 sends one atomic per run of equal lakes.  A wave with mixed lakes sends
//                          one atomic per lane that took something.  -DNMP_LAKES_PER_LANE=1: every lane sends its own (the measured
//                          alternative, tools/lakes_bench.py).
// noahmp_hip_lake_release  ONE launch, one thread per lake: volume += inflow, the level-pool outflow of a weir and an orifice in float64,
//                          at most what the lake holds, cut to 24 significant bits so that it is a float32 value, written to
//                          out_new[outlet].  diag counts the lakes that released all they held: a ballot per wave, one atomic per wave
//                          that has something to report.
// noahmp_hip_lake_depth    ONE launch, one thread per entry of the take's member list, after the release: the lake's surface (datum +
//                          volume * quantum / area, float64) above the member's bed is written to the depth plane the diffusive routing
//                          call (noahmp_diffusive.hip) reads in its next launch: a channel that drains into the lake sees its stage.
//                          No LDS, no atomics.
// Arguments go by value, nothing is allocated, nothing waits on the host.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_lakes.hpp"
#include "nmp_engine_host.hpp"

#ifndef NMP_LAKES_PER_LANE
#define NMP_LAKES_PER_LANE 0
#endif

using namespace nmp;
using nmp_host::refuse, nmp_host::bad_count, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
static_assert(kBlock % kWave == 0, "whole waves");

__device__ __forceinline__ void add_words(long long* word, long long n) {
  atomicAdd((unsigned long long*)word, (unsigned long long)n);     // two's complement: the same word as a signed add
}

__global__ void __launch_bounds__(kBlock) noahmp_lake_take_kernel(const LakeTakeArgs t) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  const LakeTaken r = lake_take_entry(t, e);                       // past the list: lake -1, n 0; every lane reaches the reduction
#if NMP_LAKES_PER_LANE
  if (r.lake >= 0 && r.n) add_words(t.inflow + r.lake, r.n);
#else
  const unsigned long long valid = __ballot(r.lake >= 0);
  int wlake = -1;
  long long wsum = 0;
  if (valid) {                                                     // the same for every lane of the wave
    const int first = __shfl(r.lake, (int)__ffsll(valid) - 1, kWave);
    const unsigned long long other = __ballot(r.lake >= 0 && r.lake != first);
    if (other == 0) {                                              // one lake: a butterfly over the 64 lanes
      long long s = r.n;
#pragma unroll
      for (int w = kWave / 2; w >= 1; w >>= 1) s += __shfl_xor(s, w, kWave);
      wlake = first; wsum = s;
    } else if (r.lake >= 0 && r.n) {
      add_words(t.inflow + r.lake, r.n);
    }
  }
  __shared__ int s_lake[kWaves];
  __shared__ long long s_sum[kWaves];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_lake[threadIdx.x / kWave] = wlake;
    s_sum[threadIdx.x / kWave] = wsum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int lake = -1;
  long long sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {                               // one atomic per run of equal lakes
    if (s_lake[w] != lake) {
      if (lake >= 0 && sum) add_words(t.inflow + lake, sum);
      lake = s_lake[w]; sum = 0;
    }
    sum += s_sum[w];
  }
  if (lake >= 0 && sum) add_words(t.inflow + lake, sum);
#endif
}

struct LakeReleaseKArgs {
  LakeReleaseArgs r;
  uint32_t* diag;
};

__global__ void __launch_bounds__(kBlock) noahmp_lake_release_kernel(const LakeReleaseKArgs k) {
  const int l = (int)(blockIdx.x * (unsigned)kBlock + threadIdx.x);
  uint32_t emptied = 0u;
  if (l < k.r.nlake) emptied = lake_release_one(k.r, l);
  if (!k.diag) return;                                             // the same for every thread of the launch
  const unsigned long long any = __ballot(emptied != 0u);
  if ((threadIdx.x & (kWave - 1)) == 0 && any) atomicAdd(k.diag, (uint32_t)__popcll(any));
}

__global__ void __launch_bounds__(kBlock) noahmp_lake_depth_kernel(const LakeDepthArgs t) {
  lake_depth_entry(t, (long long)blockIdx.x * kBlock + threadIdx.x);           // past the list: nothing
}

// two planes of na and nb bytes that share a byte (or start at the same address, whatever the sizes)
bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  if (!a || !b) return false;
  return x == y || (x < y ? y - x < na : x - y < nb);
}

// an exact power of two in [2^-40, 2^20]
bool bad_quantum(double q) {
  if (!(isfinite(q) && q > 0.0)) return true;
  int e = 0;
  const double m = frexp(q, &e);                                   // q = m * 2^e, m in [0.5, 1)
  return m != 0.5 || e - 1 < -40 || e - 1 > 20;
}

bool misaligned(const void* p, unsigned n) { return ((uintptr_t)p & (uintptr_t)(n - 1u)) != 0; }

const char* kQuantumText = "quantum must be an exact power of two in [2^-40, 2^20]";
const char* kNcellText = "ncell: 0 .. 2^31 - 1 cells";

}  // namespace

extern "C" {

int noahmp_hip_lake_take(const noahmp_lake_take* t, void* stream) {
  const char* me = "noahmp_hip_lake_take";
  if (!t) return refuse(-105, "%s: the argument block is NULL", me);
  if (bad_count(t->nmember)) return refuse(-105, "%s: nmember: 0 .. 2^31 - 1 entries", me);
  if (t->nlake < 0) return refuse(-105, "%s: nlake must be >= 0", me);
  if (bad_count(t->ncell)) return refuse(-105, "%s: %s", me, kNcellText);
  if (t->nmember > 0 && (!t->member_cell || !t->member_lake)) return refuse(-105, "%s: member_cell and member_lake are required where nmember > 0", me);
  if (t->ncell > 0 && !t->storage) return refuse(-105, "%s: storage is required where ncell > 0", me);
  if (t->nlake > 0 && !t->inflow) return refuse(-105, "%s: inflow is required where nlake > 0", me);
  if (bad_quantum(t->quantum)) return refuse(-105, "%s: %s", me, kQuantumText);
  if (misaligned(t->inflow, 8)) return refuse(-105, "%s: inflow holds 8-byte words and must be aligned to 8 bytes", me);
  const uint64_t nm = 4u * (uint64_t)t->nmember, ns = 4u * (uint64_t)t->ncell, ni = 8u * (uint64_t)t->nlake;
  const void* lists[2] = {t->member_cell, t->member_lake};
  for (const void* p : lists)
    if (overlap(t->storage, ns, p, nm) || overlap(t->inflow, ni, p, nm))
      return refuse(-105, "%s: storage and inflow must not share bytes with member_cell or member_lake", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  if (t->nmember == 0 || t->nlake == 0 || t->ncell == 0) return 0;
  LakeTakeArgs k;
  memset(&k, 0, sizeof(k));
  k.member_cell = t->member_cell; k.member_lake = t->member_lake; k.storage = t->storage; k.inflow = (long long*)t->inflow;
  k.nmember = (long long)t->nmember; k.ncell = (long long)t->ncell; k.nlake = t->nlake;
  k.q = t->quantum; k.invq = 1.0 / t->quantum; k.qf = (float)t->quantum;
  hipLaunchKernelGGL(noahmp_lake_take_kernel, grid_1d((long)t->nmember, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_lake_release(const noahmp_lake_release* r, void* stream) {
  const char* me = "noahmp_hip_lake_release";
  if (!r) return refuse(-105, "%s: the argument block is NULL", me);
  if (r->nlake < 0) return refuse(-105, "%s: nlake must be >= 0", me);
  if (r->nlake > 0 && (!r->volume || !r->inflow || !r->area || !r->weir_h || !r->weir_c || !r->weir_l || !r->orifice_h || !r->orifice_c ||
                       !r->orifice_a || !r->outlet_cell || !r->out_new))
    return refuse(-105, "%s: volume, inflow, area, weir_h, weir_c, weir_l, orifice_h, orifice_c, orifice_a, outlet_cell and out_new are required where nlake > 0", me);
  if (bad_count(r->ncell)) return refuse(-105, "%s: %s", me, kNcellText);
  if (bad_quantum(r->quantum)) return refuse(-105, "%s: %s", me, kQuantumText);
  if (!(isfinite(r->dt) && r->dt > 0.0)) return refuse(-105, "%s: dt must be finite and > 0", me);
  const void* words8[10] = {r->volume, r->inflow, r->area, r->weir_h, r->weir_c, r->weir_l, r->orifice_h, r->orifice_c, r->orifice_a, r->level};
  for (const void* p : words8)
    if (misaligned(p, 8)) return refuse(-105, "%s: volume, inflow, level and the parameter planes hold 8-byte words and must be aligned to 8 bytes", me);
  if (misaligned(r->outlet_cell, 4) || misaligned(r->out_new, 4) || misaligned(r->outflow, 4) || misaligned(r->diag, 4))
    return refuse(-105, "%s: outlet_cell, out_new, outflow and diag hold 4-byte words and must be aligned to 4 bytes", me);
  if (r->volume && r->volume == r->inflow) return refuse(-105, "%s: volume and inflow must be different planes", me);
  const uint64_t no = 4u * (uint64_t)r->ncell, n8 = 8u * (uint64_t)r->nlake, n4 = 4u * (uint64_t)r->nlake;
  for (const void* p : words8)
    if (overlap(r->out_new, no, p, n8)) return refuse(-105, "%s: out_new must not share bytes with a per-lake plane", me);
  if (overlap(r->out_new, no, r->outlet_cell, n4) || overlap(r->out_new, no, r->outflow, n4) || overlap(r->out_new, no, r->diag, 4u))
    return refuse(-105, "%s: out_new must not share bytes with a per-lake plane", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  if (r->nlake == 0) return 0;
  LakeReleaseKArgs k;
  memset(&k, 0, sizeof(k));
  k.r.volume = (long long*)r->volume; k.r.inflow = (long long*)r->inflow;
  k.r.area = r->area; k.r.weir_h = r->weir_h; k.r.weir_c = r->weir_c; k.r.weir_l = r->weir_l;
  k.r.orifice_h = r->orifice_h; k.r.orifice_c = r->orifice_c; k.r.orifice_a = r->orifice_a;
  k.r.outlet_cell = r->outlet_cell; k.r.out_new = r->out_new; k.r.level = r->level; k.r.outflow = r->outflow;
  k.r.ncell = (long long)r->ncell; k.r.q = r->quantum; k.r.invq = 1.0 / r->quantum; k.r.dt = r->dt; k.r.nlake = r->nlake;
  k.diag = r->diag;
  hipLaunchKernelGGL(noahmp_lake_release_kernel, grid_1d(r->nlake, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_lake_depth(const noahmp_lake_depth* t, void* stream) {
  const char* me = "noahmp_hip_lake_depth";
  if (!t) return refuse(-105, "%s: the argument block is NULL", me);
  if (bad_count(t->nmember)) return refuse(-105, "%s: nmember: 0 .. 2^31 - 1 entries", me);
  if (t->nlake < 0) return refuse(-105, "%s: nlake must be >= 0", me);
  if (bad_count(t->ncell)) return refuse(-105, "%s: %s", me, kNcellText);
  if (t->nmember > 0 && (!t->member_cell || !t->member_lake)) return refuse(-105, "%s: member_cell and member_lake are required where nmember > 0", me);
  if (t->ncell > 0 && (!t->bed || !t->depth)) return refuse(-105, "%s: bed and depth are required where ncell > 0", me);
  if (t->nlake > 0 && (!t->volume || !t->area || !t->datum)) return refuse(-105, "%s: volume, area and datum are required where nlake > 0", me);
  if (bad_quantum(t->quantum)) return refuse(-105, "%s: %s", me, kQuantumText);
  if (misaligned(t->volume, 8) || misaligned(t->area, 8) || misaligned(t->datum, 8))
    return refuse(-105, "%s: volume, area and datum hold 8-byte words and must be aligned to 8 bytes", me);
  if (misaligned(t->bed, 4) || misaligned(t->depth, 4)) return refuse(-105, "%s: bed and depth hold 4-byte words and must be aligned to 4 bytes", me);
  const uint64_t nm = 4u * (uint64_t)t->nmember, nc = 4u * (uint64_t)t->ncell, n8 = 8u * (uint64_t)t->nlake;
  if (overlap(t->depth, nc, t->member_cell, nm) || overlap(t->depth, nc, t->member_lake, nm) || overlap(t->depth, nc, t->bed, nc) ||
      overlap(t->depth, nc, t->volume, n8) || overlap(t->depth, nc, t->area, n8) || overlap(t->depth, nc, t->datum, n8))
    return refuse(-105, "%s: depth must not share bytes with member_cell, member_lake, bed, volume, area or datum", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  if (t->nmember == 0 || t->nlake == 0 || t->ncell == 0) return 0;
  LakeDepthArgs k;
  memset(&k, 0, sizeof(k));
  k.member_cell = t->member_cell; k.member_lake = t->member_lake; k.volume = (const long long*)t->volume; k.area = t->area; k.datum = t->datum;
  k.bed = t->bed; k.depth = t->depth;
  k.nmember = (long long)t->nmember; k.ncell = (long long)t->ncell; k.nlake = t->nlake; k.q = t->quantum;
  hipLaunchKernelGGL(noahmp_lake_depth_kernel, grid_1d((long)t->nmember, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
