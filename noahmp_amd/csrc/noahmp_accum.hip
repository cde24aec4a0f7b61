// Upstream sums on the D8 network (no reference counterpart; the contract is the text in include/noahmp_hip.h, the per-cell functions are
// nmp_dev_accum.hpp): for every cell the sum of a uint32 weight over the cells that drain through it, itself included, in uint64 words,
// by doubling.  jump[x] is the cell 2^k hops below x; in pass k + 1 every cell pushes what it holds to that cell and squares its jump, so a
// cell d hops above v with 2^k <= d < 2^(k+1) is counted once, through its ancestor 2^k hops above v: bit_length(L) + 1 launches for a
// longest path of L hops, where the Jacobi count of noahmp_hip_flow_accumulate needs L + 1.
//
// noahmp_hip_flow_upstream_init   one launch, one thread per cell: sum, pend_in, pend_out, jump_old.
// noahmp_hip_flow_upstream_pass   one launch, one thread per cell: its own words of sum, pend_in and jump_old (coalesced; 20 B read, 20 B
//                                 written), one 4-byte gather jump_old[j] and one 64-bit integer atomic add without return to pend_out[j],
//                                 one 4-byte store jump_new: 52 B per pushing cell.  What was pushed to a cell is folded into its sum when
//                                 the cell next runs (pend_out of this pass is pend_in of the next), so no plane is copied or zeroed in
//                                 between.
// The atomic is an integer add: exact, and independent of the order of arrival.  No LDS, no scratch, no wait for another workgroup;
// `changed` is a plain store of 1 (every writer stores the same word).
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_accum.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::refuse, nmp_host::bad_window, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;
constexpr int kRingMask = NOAHMP_UPSTREAM_RING_W | NOAHMP_UPSTREAM_RING_E | NOAHMP_UPSTREAM_RING_S | NOAHMP_UPSTREAM_RING_N;
static_assert(kRingMask == 0xF0 && NOAHMP_UPSTREAM_RING_W == NOAHMP_BASIN_RING_W && NOAHMP_UPSTREAM_RING_N == NOAHMP_BASIN_RING_N,
              "upstream_init_cell reads the ring flags as the upper nibble in the order W, E, S, N, like the basins");

struct UpstreamKArgs {
  const uint8_t* dir; const uint32_t* weight; const uint64_t* inflow;
  uint64_t* sum; uint64_t* pend_in; uint64_t* pend_out; int32_t* jump_old; int32_t* jump_new; uint32_t* changed;
  unsigned ncell;
  int ni, nj, flags;
};

__global__ void __launch_bounds__(kBlock) noahmp_flow_upstream_init_kernel(const UpstreamKArgs k) {
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;  // c < ni*nj <= 2^31 - 1: the index and its division fit 32 bits
  if (c >= k.ncell) return;
  const int j = (int)(c / (unsigned)k.ni), i = (int)(c - (unsigned)j * (unsigned)k.ni);
  upstream_init_cell(k.ni, k.nj, k.dir, k.weight, k.inflow, k.sum, k.pend_in, k.pend_out, k.jump_old, k.flags, i, j);
}

__global__ void __launch_bounds__(kBlock) noahmp_flow_upstream_pass_kernel(const UpstreamKArgs k) {
  const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  if (upstream_pass_cell(k.ncell, k.sum, k.pend_in, k.pend_out, k.jump_old, k.jump_new, c)) *k.changed = 1u;
}

const char* kWindowText = "window: ni, nj >= 0 and ni*nj <= 2^31 - 1";

enum Call { kInit, kPass };

bool misaligned(const void* p) { return ((uintptr_t)p & 7u) != 0; }

// two planes of nbytes each that share a byte (or start at the same address, whatever the size)
bool overlap(const void* a, const void* b, uint64_t nbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x == y || (x < y ? y - x < nbytes : x - y < nbytes);
}

// what the two entry points refuse; 0 when the block is acceptable
int upstream_refuse(const noahmp_flow_upstream* u, const char* me, Call call) {
  if (!u) return refuse(-105, "%s: the argument block is NULL", me);
  if (call == kInit) {
    if (!u->dir || !u->sum || !u->pend_in || !u->pend_out || !u->jump_old)
      return refuse(-105, "%s: dir, sum, pend_in, pend_out and jump_old are required", me);
  } else if (!u->sum || !u->pend_in || !u->pend_out || !u->jump_old || !u->jump_new || !u->changed) {
    return refuse(-105, "%s: sum, pend_in, pend_out, jump_old, jump_new and changed are required", me);
  }
  if (misaligned(u->sum) || misaligned(u->pend_in) || misaligned(u->pend_out) || (call == kInit && misaligned(u->inflow)))
    return refuse(-105, "%s: sum, pend_in, pend_out and inflow are one 8-byte word per cell and must be aligned to 8 bytes", me);
  if (bad_window(u->ni, u->nj)) return refuse(-105, "%s: %s", me, kWindowText);
  if (u->flags & ~kRingMask) return refuse(-105, "%s: flags: unknown bits (NOAHMP_UPSTREAM_RING_* only)", me);
  const uint64_t n = (uint64_t)u->ni * (uint64_t)u->nj;
  if (call == kPass && overlap(u->jump_old, u->jump_new, 4u * n))
    return refuse(-105, "%s: jump_old and jump_new must be different planes (a cell reads its jump's jump_old)", me);
  if (overlap(u->pend_in, u->pend_out, 8u * n))
    return refuse(-105, "%s: pend_in and pend_out must be different planes (a cell zeroes its pend_in while others add to pend_out)", me);
  if (overlap(u->sum, u->pend_in, 8u * n) || overlap(u->sum, u->pend_out, 8u * n))
    return refuse(-105, "%s: sum must not share words with pend_in or pend_out", me);
  return 0;
}

template <typename Kernel>
int upstream_launch(const noahmp_flow_upstream* u, void* stream, const char* me, Call call, Kernel kernel) {
  int rc = upstream_refuse(u, me, call);
  if (rc) return rc;
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  UpstreamKArgs k;
  memset(&k, 0, sizeof(k));
  k.dir = u->dir; k.weight = u->weight; k.inflow = u->inflow;
  k.sum = u->sum; k.pend_in = u->pend_in; k.pend_out = u->pend_out; k.jump_old = u->jump_old; k.jump_new = u->jump_new; k.changed = u->changed;
  k.ni = u->ni; k.nj = u->nj; k.flags = u->flags;
  k.ncell = (unsigned)u->ni * (unsigned)u->nj;
  if (k.ncell == 0) return 0;
  hipLaunchKernelGGL(kernel, grid_1d(k.ncell, kBlock), dim3(kBlock), 0, stream_of(stream), k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int noahmp_hip_flow_upstream_init(const noahmp_flow_upstream* u, void* stream) {
  return upstream_launch(u, stream, "noahmp_hip_flow_upstream_init", kInit, noahmp_flow_upstream_init_kernel);
}

int noahmp_hip_flow_upstream_pass(const noahmp_flow_upstream* u, void* stream) {
  return upstream_launch(u, stream, "noahmp_hip_flow_upstream_pass", kPass, noahmp_flow_upstream_pass_kernel);
}

}  // extern "C"
