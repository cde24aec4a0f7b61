// Depression filling and flat resolution for the D8 network (no reference counterpart; the contract is the text in include/noahmp_hip.h,
// the arithmetic is nmp_dev_flow_fill.hpp): the surface W* on which every cell that can reach an outlet drains, as the fixed point of
//   w(c) <- min(w(c), max(z(c), lift(min over the neighbours n of w(n))))
// started from z at the outlets and +inf elsewhere.  The operator is monotone and the iterates only decrease, so EVERY order of updates,
// with stale or fresh neighbour values, ends at the same bits: the schedule below is free, the result is not.
//
// noahmp_hip_flow_fill_init   one launch, one thread per cell: fixed and w_old.
// noahmp_hip_flow_fill        one launch.  sweeps == 1: the pinned form, one thread per cell, one Jacobi application, no LDS.
//                             sweeps > 1: the tiled form.  A workgroup of 256 threads holds the w of a TILE_I x TILE_J tile plus a 1-cell halo
//   in LDS (34 rows of 66 words, 8 976 B).  Lane l of wave v owns column l of the tile, rows 8v .. 8v+7, with height, w and the fixed
//   bits of its eight cells in registers.  The lanes of a wave read row segments shifted by -1, 0, +1: 32 consecutive words per half
//   wave, so no two lanes of a half meet on a bank whatever the pitch.  A sweep walks the strip serially, upwards in even sweeps and
//   downwards in odd ones, so a value crosses a strip in one sweep; a lowered w is stored to LDS at once and neighbours -- the same wave's
//   lanes, and the other waves racing through their own strips -- read whatever is there: w_old's value or one this call has assigned
//   since.  The accesses are relaxed workgroup-scope atomics, which are plain ds_read_b32 / ds_write_b32.  The halo is loaded from w_old
//   and frozen.  The loop ends when a whole sweep lowered nothing (__syncthreads_or: then every read of that sweep saw final values, and
//   the tile is at its fixed point for this halo) or at `sweeps`.
// No kernel waits for another workgroup, none uses float atomics, global atomics or scratch; `changed` is a plain store of 1.  The
// ping-pong of w_old / w_new between launches is the only synchronisation between tiles.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_flow_fill.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_window, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;
constexpr int kTI = NOAHMP_FLOW_FILL_TILE_I, kTJ = NOAHMP_FLOW_FILL_TILE_J;
constexpr int kStrip = kTI * kTJ / kBlock;                         // rows a thread owns
constexpr int kPitch = kTI + 2, kRows = kTJ + 2;
static_assert(kTI == 64 && kStrip * kBlock == kTI * kTJ && kStrip >= 1 && kStrip <= 8, "one lane per tile column, at most 8 fixed bits");

struct FillKArgs {
  const float* height; const uint8_t* outlet; uint8_t* fixed; const float* w_old; float* w_new; float* w_init; uint32_t* changed;
  unsigned ncell, tiles_i;
  int ni, nj, flags, sweeps;
  float eps;
};

// c < ni*nj <= 2^31 - 1: the cell index and its division fit 32 bits
#define NMP_FILL_CELL_INDEX(ncell, ni)                                  \
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;       \
  if (c >= (ncell)) return;                                             \
  const int j = (int)(c / (unsigned)(ni)), i = (int)(c - (unsigned)j * (unsigned)(ni))

__global__ void __launch_bounds__(kBlock) noahmp_flow_fill_init_kernel(const FillKArgs k) {
  NMP_FILL_CELL_INDEX(k.ncell, k.ni);
  fill_init_cell(k.ni, k.nj, k.height, k.outlet, k.fixed, k.w_init, k.flags, i, j);
}

__global__ void __launch_bounds__(kBlock) noahmp_flow_fill_pinned_kernel(const FillKArgs k) {
  NMP_FILL_CELL_INDEX(k.ncell, k.ni);
  const float w = fill_pass_cell(k.ni, k.nj, k.height, k.fixed, k.w_old, k.eps, i, j);
  k.w_new[c] = w;
  if (fill_bits(w) != fill_bits(k.w_old[c])) *k.changed = 1u;      // every writer stores the same word: no atomic
}

__device__ __forceinline__ float lds_get(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_put(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// one sweep of a thread's strip, upwards (UP) or downwards: returns 1 when a cell was lowered.  r is a compile-time constant in every
// unrolled step, so z[] and w[] stay in registers.
template <bool UP>
__device__ __forceinline__ int fill_sweep(float* centre, const float (&z)[kStrip], float (&w)[kStrip], unsigned free_bits, float eps) {
  int lowered = 0;
#pragma unroll
  for (int rr = 0; rr < kStrip; rr++) {
    const int r = UP ? rr : kStrip - 1 - rr;
    float* p = centre + r * kPitch;                                 // this cell's word; its neighbours are +-1 and +-kPitch around it
    float m = fill_inf();
#pragma unroll
    for (int n = 1; n <= 8; n++) m = fill_min(m, lds_get(p + flow_dj(n) * kPitch + flow_di(n)));
    const float wn = fill_relax(w[r], z[r], m, eps);
    if (((free_bits >> r) & 1u) && wn < w[r]) {
      w[r] = wn;
      lds_put(p, wn);
      lowered = 1;
    }
  }
  return lowered;
}

__global__ void __launch_bounds__(kBlock) noahmp_flow_fill_tiled_kernel(const FillKArgs k) {
  __shared__ float lw[kRows * kPitch];
  const unsigned tj = blockIdx.x / k.tiles_i, ti = blockIdx.x - tj * k.tiles_i;
  const int i0 = (int)ti * kTI, j0 = (int)tj * kTJ;                 // the tile's first cell; i0 < ni and j0 < nj
  const int t = (int)threadIdx.x;
  // the tile plus its halo from w_old; +inf outside the window lowers nothing
  for (int e = t; e < kRows * kPitch; e += kBlock) {
    const int lj = e / kPitch, li = e - lj * kPitch;
    const long gi = (long)i0 + li - 1, gj = (long)j0 + lj - 1;      // 64 bits: i0 + 64 may pass 2^31 - 1 in a window of one row
    lw[e] = (gi >= 0 && gi < k.ni && gj >= 0 && gj < k.nj) ? k.w_old[gj * k.ni + gi] : fill_inf();
  }
  const int li = t & (kTI - 1), r0 = (t / kTI) * kStrip;           // column of the tile, first row of the strip
  const int gi = i0 + li;
  float z[kStrip], w[kStrip];
  unsigned free_bits = 0, in_bits = 0;
#pragma unroll
  for (int r = 0; r < kStrip; r++) {
    const int gj = j0 + r0 + r;
    const bool in = gi < k.ni && gj < k.nj;
    const long c = in ? (long)gj * k.ni + gi : 0;
    z[r] = k.height[c];
    w[r] = in ? k.w_old[c] : fill_inf();
    in_bits |= in ? 1u << r : 0u;
    free_bits |= (in && k.fixed[c] == 0) ? 1u << r : 0u;
  }
  __syncthreads();
  float* centre = &lw[(r0 + 1) * kPitch + li + 1];
  int ever = 0;
  for (int s = 0; s < k.sweeps; s++) {
    const int lowered = (s & 1) ? fill_sweep<false>(centre, z, w, free_bits, k.eps) : fill_sweep<true>(centre, z, w, free_bits, k.eps);
    ever |= lowered;
    if (!__syncthreads_or(lowered)) break;                           // the barrier also publishes this sweep's stores to the next
  }
#pragma unroll
  for (int r = 0; r < kStrip; r++)
    if ((in_bits >> r) & 1u) k.w_new[(long)(j0 + r0 + r) * k.ni + gi] = w[r];
  if (ever) *k.changed = 1u;                                       // a lowered w never comes back: its bits differ from w_old's
}

const char* kWindowText = "window: ni, nj >= 0 and ni*nj <= 2^31 - 1";
constexpr int kOutletMask = NOAHMP_FILL_OUTLET_W | NOAHMP_FILL_OUTLET_E | NOAHMP_FILL_OUTLET_S | NOAHMP_FILL_OUTLET_N;
constexpr int kRingMask = NOAHMP_FILL_RING_W | NOAHMP_FILL_RING_E | NOAHMP_FILL_RING_S | NOAHMP_FILL_RING_N;
static_assert(kOutletMask == 0xF && kRingMask == 0xF0, "fill_init_cell reads the side flags as two nibbles in the order W, E, S, N");

// what both entry points refuse; 0 when the block is acceptable
int fill_refuse(const noahmp_flow_fill* f, const char* me, bool pass) {
  if (!f) return refuse(-105, "%s: the argument block is NULL", me);
  if (pass) {
    if (!f->height || !f->fixed || !f->w_old || !f->w_new || !f->changed)
      return refuse(-105, "%s: height, fixed, w_old, w_new and changed are required", me);
    if (f->w_old == f->w_new) return refuse(-105, "%s: w_old and w_new must be different planes (a cell reads its neighbours' w_old)", me);
  } else if (!f->height || !f->fixed || !f->w_old) {
    return refuse(-105, "%s: height, fixed and w_old are required", me);
  }
  if (bad_window(f->ni, f->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (!(isfinite(f->eps) && f->eps >= 1e-30f))
    return refuse(-105, "%s: eps must be finite and >= 1e-30: eps divided by any length below 1e8 m must stay a normal float32, or "
                        "noahmp_hip_flow_terrain could round a drop of one lift to slope 0", me);
  if (f->sweeps < 1 || f->sweeps > NOAHMP_FLOW_FILL_MAX_SWEEPS)
    return refuse(-105, "%s: sweeps: 1 .. %d", me, NOAHMP_FLOW_FILL_MAX_SWEEPS);
  if (f->flags & ~(kOutletMask | kRingMask)) return refuse(-105, "%s: flags: unknown bits (NOAHMP_FILL_OUTLET_* and NOAHMP_FILL_RING_* only)", me);
  if ((f->flags & kOutletMask) & ((f->flags & kRingMask) >> 4))
    return refuse(-105, "%s: flags: a side is OUTLET or RING, not both", me);
  return 0;
}

FillKArgs fill_kargs(const noahmp_flow_fill* f) {
  FillKArgs k;
  memset(&k, 0, sizeof(k));
  k.height = f->height; k.outlet = f->outlet; k.fixed = f->fixed; k.w_old = f->w_old; k.w_new = f->w_new; k.w_init = f->w_old;
  k.changed = f->changed;
  k.ni = f->ni; k.nj = f->nj; k.flags = f->flags; k.sweeps = f->sweeps; k.eps = f->eps;
  k.ncell = (unsigned)f->ni * (unsigned)f->nj;
  k.tiles_i = ((unsigned)f->ni + (unsigned)kTI - 1u) / (unsigned)kTI;      // unsigned: ni + 63 may pass 2^31 - 1
  return k;
}

}  // namespace

extern "C" {

int noahmp_hip_flow_fill_init(const noahmp_flow_fill* f, void* stream) {
  int rc = fill_refuse(f, "noahmp_hip_flow_fill_init", false);
  if (rc) return rc;
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  const FillKArgs k = fill_kargs(f);
  if (k.ncell == 0) return 0;
  hipLaunchKernelGGL(noahmp_flow_fill_init_kernel, grid_1d(k.ncell, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_flow_fill(const noahmp_flow_fill* f, void* stream) {
  int rc = fill_refuse(f, "noahmp_hip_flow_fill", true);
  if (rc) return rc;
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  const FillKArgs k = fill_kargs(f);
  if (k.ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  if (k.sweeps == 1) {
    hipLaunchKernelGGL(noahmp_flow_fill_pinned_kernel, grid_1d(k.ncell, kBlock), dim3(kBlock), 0, s, k);
  } else {
    const unsigned tiles_j = ((unsigned)f->nj + (unsigned)kTJ - 1u) / (unsigned)kTJ;     // tiles_i * tiles_j < 2^27: a 1-D grid holds it
    hipLaunchKernelGGL(noahmp_flow_fill_tiled_kernel, dim3(k.tiles_i * tiles_j), dim3(kBlock), 0, s, k);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
