// Watershed delineation on the D8 network (no reference counterpart; the contract is the text in include/noahmp_hip.h, the per-cell
// functions are nmp_dev_basins.hpp): every cell's root -- the gauge, outlet or ring cell its flow path ends at -- and its hop count, by
// pointer doubling.  A pass replaces every pointer by its pointer's pointer and adds the hop counts, so after k passes a pointer spans 2^k
// cells: ceil(log2 L) + 1 launches for a longest path of L cells.  The fixed point is unique and every word is an integer.
//
// noahmp_hip_flow_basin_init      one launch, one thread per cell: state_old, label, dist.
// noahmp_hip_flow_basin_jump      one launch, one thread per cell: the cell's own 8-byte word (coalesced), its pointer's 8-byte word (the
//                                 gather, the only uncoalesced access), one 8-byte store (coalesced).  16 B read, 8 B written per cell.
//                                 sweeps > 1, the tiled form: a workgroup of 256 threads holds the words of a TILE_I x TILE_J tile in LDS
//   (two planes of 2048 words of 8 bytes, and for every word the place of its pointer inside the tile or -1: 40 KB).  Lane l of wave v owns
//   column l of the tile, rows 8v .. 8v+7, in registers.  An iteration is the pass restricted to pointers that stay inside the tile: Jacobi
//   between the two LDS planes, one barrier per iteration, until an iteration moves nothing (__syncthreads_or) or `sweeps`.  The result
//   is a function of state_old alone.  Then a cell whose pointer has left the tile gathers once from state_old, as the pinned form does.
// noahmp_hip_flow_basin_resolve   one launch, one thread per cell: the labels of the roots to every cell, in place.
// No atomics, no scratch, no wait for another workgroup; `changed` is a plain store of 1 (every writer stores the same word).  The
// ping-pong of state_old / state_new between launches is the only synchronisation between workgroups.
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_basins.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::refuse, nmp_host::bad_window, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;
static_assert(kBasinNone == NOAHMP_BASIN_NONE && kBasinPending == NOAHMP_BASIN_PENDING && kBasinCycle == NOAHMP_BASIN_CYCLE, "the header's labels");

constexpr int kTI = NOAHMP_FLOW_FILL_TILE_I, kTJ = NOAHMP_FLOW_FILL_TILE_J, kTile = kTI * kTJ;
constexpr int kStrip = kTile / kBlock;                              // rows a thread owns
static_assert(kTI == 64 && kStrip * kBlock == kTile && kTile <= 32767, "one lane per tile column; a place inside the tile fits 16 bits");

struct BasinKArgs {
  const uint8_t* dir; const int32_t* seed; BasinState* state_old; BasinState* state_new; int32_t* label; int32_t* dist; uint32_t* changed;
  unsigned ncell, tiles_i;
  int ni, nj, flags, sweeps;
};

__global__ void __launch_bounds__(kBlock) noahmp_flow_basin_init_kernel(const BasinKArgs k) {
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;  // c < ni*nj <= 2^31 - 1: the index and its division fit 32 bits
  if (c >= k.ncell) return;
  const int j = (int)(c / (unsigned)k.ni), i = (int)(c - (unsigned)j * (unsigned)k.ni);
  basin_init_cell(k.ni, k.nj, k.dir, k.seed, k.state_old, k.label, k.dist, k.flags, i, j);
}

__global__ void __launch_bounds__(kBlock) noahmp_flow_basin_jump_kernel(const BasinKArgs k) {
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  if (basin_jump_cell(k.ncell, k.state_old, k.state_new, c)) *k.changed = 1u;
}

__global__ void __launch_bounds__(kBlock) noahmp_flow_basin_jump_tiled_kernel(const BasinKArgs k) {
  __shared__ BasinState ent[2][kTile];                              // the words of the tile, two planes
  __shared__ int16_t loc[2][kTile];                                 // where a word's pointer lies inside the tile, -1 when it has left it
  const unsigned tj = blockIdx.x / k.tiles_i, ti = blockIdx.x - tj * k.tiles_i;
  const int i0 = (int)ti * kTI, j0 = (int)tj * kTJ;                 // the tile's first cell; i0 < ni and j0 < nj
  const int t = (int)threadIdx.x;
  const int li = t & (kTI - 1), r0 = (t / kTI) * kStrip;           // column of the tile, first row of the strip
  const long gi = (long)i0 + li;                                    // 64 bits: i0 + 63 may pass 2^31 - 1 in a window of one row
  BasinState e[kStrip];
  int l[kStrip];
  int32_t first[kStrip];
  unsigned in_bits = 0;
#pragma unroll
  for (int r = 0; r < kStrip; r++) {
    const int lc = (r0 + r) * kTI + li;
    const long gj = (long)j0 + r0 + r;
    const bool in = gi < k.ni && gj < k.nj;
    e[r].ptr = 0; e[r].hops = 0;
    l[r] = lc;                                                      // a cell beyond the window: a root nobody points at, never stored
    if (in) {
      e[r] = k.state_old[gj * k.ni + gi];
      l[r] = -1;
      const unsigned p = (unsigned)e[r].ptr;
      if (p < k.ncell) {                                            // a pointer outside the window is never followed
        const unsigned pj = p / (unsigned)k.ni, pi = p - pj * (unsigned)k.ni;
        if (pi - (unsigned)i0 < (unsigned)kTI && pj - (unsigned)j0 < (unsigned)kTJ) l[r] = (int)((pj - (unsigned)j0) * kTI + (pi - (unsigned)i0));
      }
      in_bits |= 1u << r;
    }
    first[r] = e[r].ptr;
    ent[0][lc] = e[r];
    loc[0][lc] = (int16_t)l[r];
  }
  __syncthreads();
  int cur = 0;
  for (int s = 0; s < k.sweeps; s++) {
    int moved = 0;
#pragma unroll
    for (int r = 0; r < kStrip; r++) {
      const int lc = (r0 + r) * kTI + li;
      if (l[r] >= 0) {                                              // the pass, inside the tile
        const BasinState b = ent[cur][l[r]];
        const int lb = loc[cur][l[r]];
        moved |= b.ptr != e[r].ptr;
        e[r].hops = basin_sat(e[r].hops, b.hops);
        e[r].ptr = b.ptr;
        l[r] = lb;
      }
      ent[cur ^ 1][lc] = e[r];
      loc[cur ^ 1][lc] = (int16_t)l[r];
    }
    cur ^= 1;
    if (!__syncthreads_or(moved)) break;                            // the barrier also publishes this iteration's plane to the next
  }
  int ever = 0;
#pragma unroll
  for (int r = 0; r < kStrip; r++) {
    if (!((in_bits >> r) & 1u)) continue;
    BasinState n = e[r];
    if (l[r] < 0 && (unsigned)n.ptr < k.ncell) {                    // the pointer has left the tile: one gather from state_old
      const BasinState b = k.state_old[n.ptr];
      n.hops = basin_sat(n.hops, b.hops);
      n.ptr = b.ptr;
    }
    k.state_new[((long)j0 + r0 + r) * k.ni + gi] = n;
    ever |= n.ptr != first[r];
  }
  if (ever) *k.changed = 1u;
}

__global__ void __launch_bounds__(kBlock) noahmp_flow_basin_resolve_kernel(const BasinKArgs k) {
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  if (basin_resolve_cell(k.ncell, k.state_old, k.label, k.dist, c)) *k.changed = 1u;
}

const char* kWindowText = "window: ni, nj >= 0 and ni*nj <= 2^31 - 1";
constexpr int kRingMask = NOAHMP_BASIN_RING_W | NOAHMP_BASIN_RING_E | NOAHMP_BASIN_RING_S | NOAHMP_BASIN_RING_N;
static_assert(kRingMask == 0xF0, "basin_init_cell reads the ring flags as the upper nibble in the order W, E, S, N, like the fill");

enum Call { kInit, kJump, kResolve };

bool misaligned(const void* p) { return ((uintptr_t)p & 7u) != 0; }

// what the three entry points refuse; 0 when the block is acceptable
int basin_refuse(const noahmp_flow_basin* b, const char* me, Call call) {
  if (!b) return refuse(-105, "%s: the argument block is NULL", me);
  if (call == kInit) {
    if (!b->dir || !b->state_old || !b->label || !b->dist) return refuse(-105, "%s: dir, state_old, label and dist are required", me);
  } else if (call == kJump) {
    if (!b->state_old || !b->state_new || !b->changed) return refuse(-105, "%s: state_old, state_new and changed are required", me);
    if (b->state_old == b->state_new)
      return refuse(-105, "%s: state_old and state_new must be different planes (a cell reads its pointer's state_old)", me);
  } else if (!b->state_old || !b->label || !b->dist || !b->changed) {
    return refuse(-105, "%s: state_old, label, dist and changed are required", me);
  }
  if (misaligned(b->state_old) || (call == kJump && misaligned(b->state_new)))
    return refuse(-105, "%s: a state plane is one 8-byte word per cell and must be aligned to 8 bytes", me);
  if (bad_window(b->ni, b->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (b->flags & ~kRingMask) return refuse(-105, "%s: flags: unknown bits (NOAHMP_BASIN_RING_* only)", me);
  if (b->sweeps < 1 || b->sweeps > NOAHMP_FLOW_BASIN_MAX_SWEEPS) return refuse(-105, "%s: sweeps: 1 .. %d", me, NOAHMP_FLOW_BASIN_MAX_SWEEPS);
  return 0;
}

BasinKArgs basin_kargs(const noahmp_flow_basin* b) {
  BasinKArgs k;
  memset(&k, 0, sizeof(k));
  k.dir = b->dir; k.seed = b->seed; k.state_old = (BasinState*)b->state_old; k.state_new = (BasinState*)b->state_new;
  k.label = b->label; k.dist = b->dist; k.changed = b->changed;
  k.ni = b->ni; k.nj = b->nj; k.flags = b->flags; k.sweeps = b->sweeps;
  k.ncell = (unsigned)b->ni * (unsigned)b->nj;
  k.tiles_i = ((unsigned)b->ni + (unsigned)kTI - 1u) / (unsigned)kTI;      // unsigned: ni + 63 may pass 2^31 - 1
  return k;
}

template <typename Kernel>
int basin_launch(const noahmp_flow_basin* b, void* stream, const char* me, Call call, Kernel kernel) {
  int rc = basin_refuse(b, me, call);
  if (rc) return rc;
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  const BasinKArgs k = basin_kargs(b);
  if (k.ncell == 0) return 0;
  hipLaunchKernelGGL(kernel, grid_1d(k.ncell, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int noahmp_hip_flow_basin_init(const noahmp_flow_basin* b, void* stream) {
  return basin_launch(b, stream, "noahmp_hip_flow_basin_init", kInit, noahmp_flow_basin_init_kernel);
}

int noahmp_hip_flow_basin_jump(const noahmp_flow_basin* b, void* stream) {
  const char* me = "noahmp_hip_flow_basin_jump";
  if (!b || b->sweeps <= 1) return basin_launch(b, stream, me, kJump, noahmp_flow_basin_jump_kernel);
  int rc = basin_refuse(b, me, kJump);
  if (rc) return rc;
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  const BasinKArgs k = basin_kargs(b);
  if (k.ncell == 0) return 0;
  const unsigned tiles_j = ((unsigned)b->nj + (unsigned)kTJ - 1u) / (unsigned)kTJ;       // tiles_i * tiles_j < 2^27: a 1-D grid holds it
  hipLaunchKernelGGL(noahmp_flow_basin_jump_tiled_kernel, dim3(k.tiles_i * tiles_j), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_flow_basin_resolve(const noahmp_flow_basin* b, void* stream) {
  return basin_launch(b, stream, "noahmp_hip_flow_basin_resolve", kResolve, noahmp_flow_basin_resolve_kernel);
}

}  // extern "C"
