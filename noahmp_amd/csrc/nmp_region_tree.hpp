// The summation tree S of include/noahmp_hip.h (NOAHMP_REG_SUM) and the offsets that cut sorted members into its chunks: shared by the
// region series (noahmp_regions.hip) and the budget-preserving regrid (noahmp_regrid_conserve.hip), so that both sum with the same bits.
// Members sorted by a key 0 .. ngroup-1 (non-members carry the key ngroup and sort behind the last group) are cut into chunks of 256
// consecutive members that never cross a group boundary; the partials of a group are cut the same way on the next level.
//
// Device code and kernels only, for .hip translation units; every including unit gets its own copy of the kernels (internal linkage).
#pragma once
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_regions.hpp"

namespace nmp {
namespace tree {
namespace {

constexpr int kChunk = NOAHMP_REG_CHUNK;
constexpr int kBlock = 256, kWaves = kBlock / 64;
static_assert(kChunk == 256, "a wave of 64 lanes holds four elements of a chunk per lane");

// roff[r] = first sorted cell whose key is >= r, r = 0 .. nregion (roff[nregion] = number of members)
__global__ void __launch_bounds__(kBlock) region_offsets_kernel(const unsigned* keys, long n, int nregion, int* roff) {
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  if (r > nregion) return;
  long lo = 0, hi = n;
  while (lo < hi) { const long mid = (lo + hi) >> 1; if (keys[mid] < (unsigned)r) lo = mid + 1; else hi = mid; }
  roff[r] = (int)lo;
}

// chunks region i contributes to the next level: ceil(span / 256); the scan's input
struct ChunkCount {
  const int* off; int nregion;
  __host__ __device__ int operator()(int i) const { return i < nregion ? (off[i + 1] - off[i] + kChunk - 1) / kChunk : 0; }
};

// cstart[c] = first element of chunk c, c = 0 .. total; chunk c ends at min(cstart[c] + 256, cstart[c+1]) (regions are adjacent)
__global__ void __launch_bounds__(kBlock) region_chunks_kernel(const int* off, const int* choff, int nregion, long bound, int* cstart, int* hdr_max) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  const int total = choff[nregion];
  if (c > total || c > bound) return;
  if (c == total) { cstart[c] = off[nregion]; return; }
  int lo = 0, hi = nregion;              // the last region whose first chunk is <= c: it is not empty
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (choff[mid] <= (int)c) lo = mid; else hi = mid - 1; }
  cstart[c] = off[lo] + kChunk * ((int)c - choff[lo]);
  if (hdr_max && (int)c == choff[lo]) atomicMax(hdr_max, choff[lo + 1] - choff[lo]);      // integer: the widest region of this level
}

// one chunk in a wave: lane l holds elements l, l+64, l+128, l+192.  v[i] = v[i] + v[i+h] for i < h, h = 128 .. 1; lane 0 has the result.
__device__ __forceinline__ double wave_fold(int op, double v0, double v1, double v2, double v3) {
  v0 = reg_combine(op, v0, v2); v1 = reg_combine(op, v1, v3);       // h = 128
  v0 = reg_combine(op, v0, v1);                                     // h = 64
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) v0 = reg_combine(op, v0, __shfl_down(v0, h, 64));
  return v0;
}

}  // namespace
}  // namespace tree
}  // namespace nmp
