// Runoff routing on a D8 network (noahmp_hip_flow_terrain / _flow_inmask / _flow_accumulate / noahmp_hip_route_runoff): the per-cell functions.
// __host__ __device__ like nmp_dev_wind.hpp: tests/host_emul/routing_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h, every rounding included.  Every line is one
// rounded float32 operation of that text, nothing may contract into an FMA, and there are no guards beyond those of the text.  A cell
// GATHERS from its neighbours in ascending k: no atomics, and the bits do not depend on who runs first.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#endif

namespace nmp {

#ifndef NMP_DEV
#define NMP_DEV __host__ __device__ __forceinline__
#endif

// neighbour k = 1..8 is E, NE, N, NW, W, SW, S, SE; two bits per k, value + 1 (k = 1 in the lowest pair).  The loops over k are unrolled,
// so every shift folds into a constant.
NMP_DEV int flow_di(int k) { return (int)((0x901Au >> (2 * (k - 1))) & 3u) - 1; }      // +1 +1  0 -1 -1 -1  0 +1
NMP_DEV int flow_dj(int k) { return (int)((0x01A9u >> (2 * (k - 1))) & 3u) - 1; }      //  0 +1 +1 +1  0 -1 -1 -1
NMP_DEV int flow_opposite(int k) { return ((k + 3) & 7) + 1; }

// what a window fixes for every cell: the three reciprocal distances of the text, made once (IEEE float32 operations: the same bits on
// either side)
struct FlowParams {
  int ni, nj;
  float inv_x, inv_y, inv_d;
};

NMP_DEV FlowParams flow_params(int ni, int nj, float dx, float dy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  FlowParams p;
  p.ni = ni; p.nj = nj;
  p.inv_x = 1.0f / dx;
  p.inv_y = 1.0f / dy;
  const float dx2 = dx * dx;
  const float dy2 = dy * dy;
  const float d2 = dx2 + dy2;
  const float d = sqrtf(d2);
  p.inv_d = 1.0f / d;
  return p;
}

NMP_DEV bool flow_inside(int ni, int nj, int i, int j) { return i >= 0 && i < ni && j >= 0 && j < nj; }

// one window cell of noahmp_hip_flow_terrain: the direction of steepest strict descent, 0 where there is none
NMP_DEV uint8_t flow_dir_cell(const FlowParams& p, const float* __restrict__ height, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long c = (long)j * p.ni + i;
  const float z0 = height[c];
  int best = 0;
  float sbest = 0.f;
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const int di = flow_di(k), dj = flow_dj(k);
    if (!flow_inside(p.ni, p.nj, i + di, j + dj)) continue;
    const float drop = z0 - height[c + (long)dj * p.ni + di];
    const float inv = (k & 1) ? ((k & 2) ? p.inv_y : p.inv_x) : p.inv_d;
    const float s = drop * inv;
    if (s > sbest) { best = k; sbest = s; }
  }
  return (uint8_t)best;
}

// one window cell of noahmp_hip_flow_inmask: bit k-1 = neighbour k drains into this cell
NMP_DEV uint8_t flow_inmask_cell(int ni, int nj, const uint8_t* __restrict__ dir, int i, int j) {
  const long c = (long)j * ni + i;
  unsigned m = 0;
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const int di = flow_di(k), dj = flow_dj(k);
    if (!flow_inside(ni, nj, i + di, j + dj)) continue;
    if ((int)dir[c + (long)dj * ni + di] == flow_opposite(k)) m |= 1u << (k - 1);       // opp(k) is 1..8: a byte outside 0..8 never matches
  }
  return (uint8_t)m;
}

// one window cell of noahmp_hip_flow_accumulate.  All eight words are loaded from an address made legal (the cell's own where the
// neighbour is outside) and the sum selects, as in route_cell<true>: eight loads in flight instead of eight branches in a row.
NMP_DEV uint32_t flow_accumulate_cell(int ni, int nj, const uint8_t* __restrict__ inmask, const uint32_t* __restrict__ acc_old, int i, int j) {
  const long c = (long)j * ni + i;
  const unsigned m = inmask[c];
  uint32_t v[8];
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const int di = flow_di(k), dj = flow_dj(k);
    v[k - 1] = acc_old[flow_inside(ni, nj, i + di, j + dj) ? c + (long)dj * ni + di : c];
  }
  uint32_t a = 1u;
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const bool take = ((m >> (k - 1)) & 1u) && flow_inside(ni, nj, i + flow_di(k), j + flow_dj(k));
    a += take ? v[k - 1] : 0u;
  }
  return a;
}

struct RouteCellArgs {
  const uint8_t* inmask; const int32_t* col_index;
  const float* area; const float* release;
  float* storage; const float* out_old; float* out_new;
  const float* runoff_a; const float* runoff_b;
  float scale;
  int ni, nj;
  long ncol;
};

// one window cell of noahmp_hip_route_runoff.  LOAD_ALL = true (the library): all eight neighbours are loaded from an address made legal
// (the cell's own where the neighbour is outside) and the sum selects: eight loads in flight.  false: only the neighbours of the set bits
// are loaded, each in a branch of its own (the lanes of a wave diverge, and a branch waits for its load before the next is tried): 1.8
// times slower at 7 M cells (profiles/routing_bench.md).  Both add the same operands in the same order: the same bits.
template <bool LOAD_ALL>
NMP_DEV void route_cell(const RouteCellArgs& r, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long c = (long)j * r.ni + i;
  const long d = (long)r.col_index[c];
  if (d < -1 || d >= r.ncol) return;                               // a ring cell: read by others and never written
  const unsigned m = r.inmask[c];
  float q = 0.f;
  if (LOAD_ALL) {
    float o[8];
#pragma unroll
    for (int k = 1; k <= 8; k++) {
      const int di = flow_di(k), dj = flow_dj(k);
      const bool in = flow_inside(r.ni, r.nj, i + di, j + dj);
      o[k - 1] = r.out_old[in ? c + (long)dj * r.ni + di : c];
    }
#pragma unroll
    for (int k = 1; k <= 8; k++) {
      const bool take = ((m >> (k - 1)) & 1u) && flow_inside(r.ni, r.nj, i + flow_di(k), j + flow_dj(k));
      const float qk = q + o[k - 1];
      q = take ? qk : q;
    }
  } else {
#pragma unroll
    for (int k = 1; k <= 8; k++) {
      const int di = flow_di(k), dj = flow_dj(k);
      if (!((m >> (k - 1)) & 1u) || !flow_inside(r.ni, r.nj, i + di, j + dj)) continue;
      q = q + r.out_old[c + (long)dj * r.ni + di];
    }
  }
  float v = 0.f;
  if (d >= 0) {
    float x = r.runoff_a[d];
    if (r.runoff_b) x = x + r.runoff_b[d];
    const float xs = x * r.scale;
    v = xs * r.area[c];
  }
  const float sv = r.storage[c] + v;
  const float s1 = sv + q;
  const float o = s1 * r.release[c];
  r.storage[c] = s1 - o;
  r.out_new[c] = o;
}

}  // namespace nmp
