// Upstream sums on the D8 network (noahmp_hip_flow_upstream_init / _pass): the per-cell functions.
// __host__ __device__ like nmp_dev_basins.hpp: tests/host_emul/upstream_check.hip compiles the same functions for the CPU, where the one
// atomic of a pass is a plain add (the cells are visited one after the other there).
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h.  Every word is an integer and all
// arithmetic is mod 2^64; the only word two cells of a launch touch is pend_out[j], by an integer add, so the result does not depend on
// who runs first.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "nmp_dev_basins.hpp"

namespace nmp {

// pend[j] += v.  Device: the no-return 64-bit integer atomic (the result is unused), relaxed, agent scope.
NMP_DEV void upstream_add(uint64_t* pend, int32_t j, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)__hip_atomic_fetch_add((unsigned long long*)pend + j, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  pend[j] += v;
#endif
}

// one window cell of noahmp_hip_flow_upstream_init.  The ring bits of flags are the basins': bits 4..7 = RING_W, _E, _S, _N
NMP_DEV void upstream_init_cell(int ni, int nj, const uint8_t* __restrict__ dir, const uint32_t* __restrict__ weight,
                                const uint64_t* __restrict__ inflow, uint64_t* __restrict__ sum, uint64_t* __restrict__ pend_in,
                                uint64_t* __restrict__ pend_out, int32_t* __restrict__ jump, int flags, int i, int j) {
  const int32_t c = j * ni + i;                                     // ni*nj <= 2^31 - 1
  const unsigned ring = (unsigned)flags >> 4;
  const int32_t t = basin_down(ni, nj, dir, i, j);
  int32_t jp = -1;
  if (t >= 0) {
    const int tj = t / ni, ti = t - tj * ni;
    if (!(fill_side_bits(ni, nj, ti, tj) & ring)) jp = t;           // an edge into a ring cell is cut
  }
  uint64_t s;
  if (fill_side_bits(ni, nj, i, j) & ring) s = inflow ? inflow[c] : 0u;      // RING: what its owner says drains through it
  else s = weight ? (uint64_t)weight[c] : 1u;
  jump[c] = jp;
  sum[c] = s;
  pend_in[c] = 0u;
  pend_out[c] = 0u;
}

// one window cell of noahmp_hip_flow_upstream_pass: true when the cell pushed
NMP_DEV bool upstream_pass_cell(uint32_t ncell, uint64_t* __restrict__ sum, uint64_t* __restrict__ pend_in, uint64_t* pend_out,
                                const int32_t* __restrict__ jump_old, int32_t* __restrict__ jump_new, uint32_t c) {
  const uint64_t s = sum[c] + pend_in[c];                           // the deferred fold: what the pass before pushed to this cell
  const int32_t j = jump_old[c];
  sum[c] = s;
  pend_in[c] = 0u;
  if ((uint32_t)j >= ncell) {                                       // none, or a jump no init wrote: never followed
    jump_new[c] = -1;
    return false;
  }
  upstream_add(pend_out, j, s);
  jump_new[c] = jump_old[j];                                        // the gather: one 4-byte load
  return true;
}

}  // namespace nmp
