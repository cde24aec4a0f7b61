// Watershed delineation on the D8 network (noahmp_hip_flow_basin_init / _jump / _resolve): the per-cell functions.
// __host__ __device__ like nmp_dev_routing.hpp: tests/host_emul/basins_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h.  Every word is an integer; a cell reads
// other cells' words of the OLD plane (jump) or words nobody writes in the same launch (resolve: roots are read, the others written), so
// the result does not depend on who runs first.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "nmp_dev_flow_fill.hpp"

namespace nmp {

constexpr int32_t kBasinNone = -1, kBasinPending = -2, kBasinCycle = -3;

// one cell's word: the cell its pointer has reached and the hops in between.  8 bytes, loaded and stored as one.
struct alignas(8) BasinState {
  int32_t ptr, hops;
};
static_assert(sizeof(BasinState) == 8, "one packed word per cell");

NMP_DEV int32_t basin_sat(int32_t a, int32_t b) {
  const int64_t s = (int64_t)a + (int64_t)b;
  return s > 0x7FFFFFFFLL ? 0x7FFFFFFF : (int32_t)s;
}

// down(c): the cell that c drains into, or -1.  k is used only when it is 1..8.
NMP_DEV int32_t basin_down(int ni, int nj, const uint8_t* __restrict__ dir, int i, int j) {
  const int32_t c = j * ni + i;                                     // ni*nj <= 2^31 - 1
  const int k = dir[c];
  if (k < 1 || k > 8) return -1;
  const int di = flow_di(k), dj = flow_dj(k);
  if (!flow_inside(ni, nj, i + di, j + dj)) return -1;
  return c + dj * ni + di;
}

// one window cell of noahmp_hip_flow_basin_init.  The ring bits of flags are the fill's: bits 4..7 = RING_W, _E, _S, _N
NMP_DEV void basin_init_cell(int ni, int nj, const uint8_t* __restrict__ dir, const int32_t* __restrict__ seed, BasinState* __restrict__ state,
                             int32_t* __restrict__ label, int32_t* __restrict__ dist, int flags, int i, int j) {
  const int32_t c = j * ni + i;
  BasinState s;
  s.ptr = c; s.hops = 0;
  int32_t l = kBasinPending, d = -1;
  if (!(fill_side_bits(ni, nj, i, j) & ((unsigned)flags >> 4))) {  // not RING
    const int32_t sd = seed ? seed[c] : -1;
    const int32_t dn = basin_down(ni, nj, dir, i, j);
    if (sd >= 0) {
      l = sd; d = 0;                                                 // SEED
    } else if (dn < 0) {
      l = kBasinNone; d = 0;                                         // TERMINAL
    } else {
      s.ptr = dn; s.hops = 1;                                        // FREE
    }
  }
  state[c] = s;
  label[c] = l;
  dist[c] = d;
}

// one window cell of noahmp_hip_flow_basin_jump: true when the pointer moved
NMP_DEV bool basin_jump_cell(uint32_t ncell, const BasinState* __restrict__ old, BasinState* __restrict__ neu, uint32_t c) {
  const BasinState a = old[c];
  if ((uint32_t)a.ptr >= ncell) {                                   // a state no init wrote: never followed
    neu[c] = a;
    return false;
  }
  const BasinState b = old[a.ptr];                                  // the gather: one 8-byte load
  BasinState n;
  n.ptr = b.ptr; n.hops = basin_sat(a.hops, b.hops);
  neu[c] = n;
  return b.ptr != a.ptr;
}

// one window cell of noahmp_hip_flow_basin_resolve: true when the word of label[c] changed.  label and dist are read at roots and written
// at the other cells (a cell with state (c, h != 0) writes itself and is read by nobody: its readers stop at rh != 0).
NMP_DEV bool basin_resolve_cell(uint32_t ncell, const BasinState* __restrict__ state, int32_t* label, int32_t* dist, uint32_t c) {
  const BasinState a = state[c];
  if ((uint32_t)a.ptr >= ncell) return false;
  int32_t l, d;
  if ((uint32_t)a.ptr == c) {
    if (a.hops == 0) return false;
    l = kBasinCycle; d = -1;
  } else {
    const BasinState r = state[a.ptr];
    if (r.ptr != a.ptr || r.hops != 0) {
      l = kBasinCycle; d = -1;
    } else {
      const int32_t lr = label[a.ptr];
      if (lr == kBasinPending) return false;
      if (lr == kBasinCycle) {
        l = kBasinCycle; d = -1;
      } else {
        l = lr; d = basin_sat(a.hops, dist[a.ptr]);
      }
    }
  }
  const bool moved = label[c] != l;
  label[c] = l;
  dist[c] = d;
  return moved;
}

}  // namespace nmp
