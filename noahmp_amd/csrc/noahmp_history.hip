// Device-side history of a device-resident run: interval accumulators and point probes (no reference counterpart as a routine; the
// arithmetic is the reference's, nmp_dev_history.hpp).  A run that advances 7 M columns in ~3 ms cannot afford to bring whole arrays to the
// host every step (68 ms for the INOUT + OUT set); what land-surface output is made of -- fluxes integrated over the output interval, daily
// minima / maxima, a per-step series at a few cells -- is kept on the device instead and fetched at the output cadence.
//
// noahmp_hip_history_step: ONE launch per call.  A pure stream: per entry and column 4 B of src and 4 B of acc are read and 4 B written, plus
// the two class planes and the count plane once per column.  A thread owns four consecutive columns (16-byte loads / stores) and walks
// the entries itself, so the class test and the count are paid once per column; the probes are extra workgroups of the same grid.
// No atomics, nothing in LDS.  Arrays are caller-owned: nothing is allocated and nothing waits.
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_history.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kMaxEntries = NOAHMP_HIST_MAX_ENTRIES, kMaxPoints = NOAHMP_HIST_MAX_POINTS, kMaxProbeFields = NOAHMP_HIST_MAX_PROBE_FIELDS;
constexpr int kMaxLevels = 64;
constexpr int kBlock = 256, kBatch = 4;

struct StepKArgs {                       // by value (1.4 KB): no engine-owned buffer, no copy per call
  const float* src[kMaxEntries];
  float* acc[kMaxEntries];
  int nlev[kMaxEntries];
  int op[kMaxEntries];
  float scale[kMaxEntries];
  const float* xland; const float* xice; int* count;
  float xice_thres;
  int n, ni, any_layered;
  long ncol;
  unsigned col_blocks;                   // workgroups of the accumulators; the probes follow
  // probes
  const float* field[kMaxProbeFields];
  const int* column; float* ring;        // ring already points at the slot this call writes
  int npoint, nfield;
};

// four columns of one entry level
__device__ __forceinline__ float4 apply4(int op, float4 a, float4 x, float s, const bool* t) {
  a.x = t[0] ? hist_apply(op, a.x, x.x, s) : a.x;
  a.y = t[1] ? hist_apply(op, a.y, x.y, s) : a.y;
  a.z = t[2] ? hist_apply(op, a.z, x.z, s) : a.z;
  a.w = t[3] ? hist_apply(op, a.w, x.w, s) : a.w;
  return a;
}

__device__ __forceinline__ void probe_block(const StepKArgs& k) {
  const int t = (int)(blockIdx.x - k.col_blocks) * kBlock + (int)threadIdx.x;
  if (t >= k.npoint * k.nfield) return;
  const int f = t / k.npoint, pt = t - f * k.npoint;
  const int c = k.column[pt];
  // a probe column outside the block reads nothing (NaN in the ring says so)
  k.ring[t] = (c >= 0 && (long)c < k.ncol) ? k.field[f][c] : __uint_as_float(0x7FC00000u);
}

// VEC: every plane is 16-byte aligned and, if an entry is layered, rows are a multiple of four columns long
template <bool VEC>
__global__ void __launch_bounds__(kBlock) noahmp_history_step_kernel(const StepKArgs k) {
  if (blockIdx.x >= k.col_blocks) { probe_block(k); return; }
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (VEC) {
    const long c0 = t * 4;
    if (c0 >= k.ncol) return;
    if (c0 + 4 <= k.ncol) {
      const float4 xl = *(const float4*)(k.xland + c0), xi = *(const float4*)(k.xice + c0);
      const bool tk[4] = {hist_takes_part(xl.x, xi.x, k.xice_thres), hist_takes_part(xl.y, xi.y, k.xice_thres),
                          hist_takes_part(xl.z, xi.z, k.xice_thres), hist_takes_part(xl.w, xi.w, k.xice_thres)};
      if (!(tk[0] | tk[1] | tk[2] | tk[3])) return;                 // e.g. the skipped range of a sorted layout: no traffic
      if (k.count) {
        int4 n4 = *(const int4*)(k.count + c0);
        n4.x += tk[0]; n4.y += tk[1]; n4.z += tk[2]; n4.w += tk[3];
        *(int4*)(k.count + c0) = n4;
      }
      long row = 0; int i0 = 0;
      if (k.any_layered) { row = c0 / k.ni; i0 = (int)(c0 - row * k.ni); }
      for (int f0 = 0; f0 < k.n; f0 += kBatch) {
        // the loads of a batch of 2-D entries are issued before the first store (planes may alias as far as the compiler knows)
        float4 x[kBatch], a[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; u++)
          if (f0 + u < k.n && k.nlev[f0 + u] == 1) { x[u] = *(const float4*)(k.src[f0 + u] + c0); a[u] = *(const float4*)(k.acc[f0 + u] + c0); }
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const int f = f0 + u;
          if (f >= k.n) break;
          const int nk = k.nlev[f], op = k.op[f];
          const float s = k.scale[f];
          if (nk == 1) { *(float4*)(k.acc[f] + c0) = apply4(op, a[u], x[u], s, tk); continue; }
          for (int l = 0; l < nk; l++) {                            // (i,k,j) layout: level l of row `row`
            const size_t o = ((size_t)row * nk + l) * k.ni + i0;
            const float4 xv = *(const float4*)(k.src[f] + o), av = *(const float4*)(k.acc[f] + o);
            *(float4*)(k.acc[f] + o) = apply4(op, av, xv, s, tk);
          }
        }
      }
      return;
    }
    // the last, partial group of a block whose column count is no multiple of four (2-D entries only): one column at a time
    for (long c = c0; c < k.ncol; c++) {
      if (!hist_takes_part(k.xland[c], k.xice[c], k.xice_thres)) continue;
      if (k.count) k.count[c] += 1;
      for (int f = 0; f < k.n; f++) k.acc[f][c] = hist_apply(k.op[f], k.acc[f][c], k.src[f][c], k.scale[f]);
    }
    return;
  }
  // scalar path: one column per thread
  const long c = t;
  if (c >= k.ncol) return;
  if (!hist_takes_part(k.xland[c], k.xice[c], k.xice_thres)) return;
  if (k.count) k.count[c] += 1;
  long row = 0; int i0 = 0;
  if (k.any_layered) { row = c / k.ni; i0 = (int)(c - row * k.ni); }
  for (int f = 0; f < k.n; f++) {
    const int nk = k.nlev[f], op = k.op[f];
    const float s = k.scale[f];
    if (nk == 1) { k.acc[f][c] = hist_apply(op, k.acc[f][c], k.src[f][c], s); continue; }
    for (int l = 0; l < nk; l++) {
      const size_t o = ((size_t)row * nk + l) * k.ni + i0;
      k.acc[f][o] = hist_apply(op, k.acc[f][o], k.src[f][o], s);
    }
  }
}

struct FinKArgs {
  float* acc[kMaxEntries];
  float* dst[kMaxEntries];               // tile order, or NULL (reset only)
  int nlev[kMaxEntries];
  int op[kMaxEntries];
  unsigned flags[kMaxEntries];
  const int* count; const int* perm; const int* vegtyp;
  int iswater, n, ni, nj;
  float fill;
};

// dst column p <- acc column perm[p] (the gather of noahmp_hip_output_fields), mean and water mask applied, then the reset of the
// accumulator column just read (perm is a bijection: nobody else reads it).  One thread per destination column: output cadence, not hot.
__global__ void __launch_bounds__(kBlock) noahmp_history_finish_kernel(const FinKArgs k) {
  const long p = (long)blockIdx.x * kBlock + threadIdx.x;
  const long ncol = (long)k.ni * k.nj;
  if (p >= ncol) return;
  const long gsrc = k.perm ? k.perm[p] : p;
  if (gsrc < 0 || gsrc >= ncol) return;
  const int pj = (int)(p / k.ni), pi = (int)(p - (long)pj * k.ni);
  const int gj = (int)(gsrc / k.ni), gi = (int)(gsrc - (long)gj * k.ni);
  const bool water = k.vegtyp && k.vegtyp[gsrc] == k.iswater;
  const int cnt = k.count ? k.count[gsrc] : 0;
  for (int f = 0; f < k.n; f++) {
    const int nk = k.nlev[f], op = k.op[f];
    const bool mean = (k.flags[f] & NOAHMP_HIST_FIN_MEAN) != 0, reset = (k.flags[f] & NOAHMP_HIST_FIN_RESET) != 0;
    for (int l = 0; l < nk; l++) {
      const size_t so = ((size_t)gj * nk + l) * k.ni + gi;
      const float a = k.acc[f][so];
      if (k.dst[f]) k.dst[f][((size_t)pj * nk + l) * k.ni + pi] = water ? -1.E33f : hist_finish(a, cnt, mean, k.fill);   // netcdf_io:1971, 2041
      if (reset) k.acc[f][so] = hist_identity(op, a);
    }
  }
}

int check_entries(const char* who, int n, const noahmp_history_entry* e) {
  if (n < 0 || n > kMaxEntries) return refuse(-107, "%s: 0..%d entries per call (n = %d)", who, kMaxEntries, n);
  if (n > 0 && !e) return refuse(-105, "%s: entries are NULL", who);
  for (int f = 0; f < n; f++) {
    if (e[f].op < NOAHMP_HIST_SUM || e[f].op > NOAHMP_HIST_LAST) return refuse(-105, "%s: entry %d has op %d (NOAHMP_HIST_SUM .. NOAHMP_HIST_LAST)", who, f, e[f].op);
    if (!e[f].acc) return refuse(-105, "%s: entry %d has a NULL plane", who, f);
    if (e[f].nlev < 1 || e[f].nlev > kMaxLevels) return refuse(-105, "%s: entry %d has %d levels (1..%d)", who, f, e[f].nlev, kMaxLevels);
  }
  return 0;
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

}  // namespace

extern "C" {

int noahmp_hip_history_step(int n, const noahmp_history_entry* e, const noahmp_history_probes* p, const noahmp_step_args* a,
                            int32_t* count, void* stream) {
  static const char* who = "noahmp_hip_history_step";
  int rc = check_entries(who, n, e);
  if (rc) return rc;
  for (int f = 0; f < n; f++)
    if (!e[f].src) return refuse(-105, "%s: entry %d has a NULL plane", who, f);
  if (!a || !a->xland || !a->xice) return refuse(-105, "noahmp_hip_history_step: the step block and its XLAND / XICE planes are required");
  if (a->ims != a->its || a->ime != a->ite || a->jms != a->jts || a->jme != a->jte)
    return refuse(-105, "noahmp_hip_history_step: the memory block must be the tile");
  const int ni = a->ime - a->ims + 1, nj = a->jme - a->jms + 1;
  const long ncol = (long)ni * nj;
  if (bad_window(ni, nj)) return refuse(-105, "noahmp_hip_history_step: 0 .. 2^31 - 1 columns");
  if (p) {
    if (p->npoint < 0 || p->npoint > kMaxPoints) return refuse(-107, "%s: 0..%d probe points (npoint = %d)", who, kMaxPoints, p->npoint);
    if (p->nfield < 0 || p->nfield > kMaxProbeFields) return refuse(-107, "%s: 0..%d probe fields (nfield = %d)", who, kMaxProbeFields, p->nfield);
    if (p->npoint > 0 && p->nfield > 0) {
      if (!p->column || !p->field || !p->ring) return refuse(-105, "noahmp_hip_history_step: probes need column, field and ring");
      if (p->nslot < 1 || p->slot < 0) return refuse(-105, "noahmp_hip_history_step: probes need nslot >= 1 and slot >= 0");
      for (int f = 0; f < p->nfield; f++)
        if (!p->field[f]) return refuse(-105, "%s: probe field %d is a NULL plane", who, f);
    }
  }
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  hipStream_t s = stream_of(stream);
  StepKArgs k;
  memset(&k, 0, sizeof(k));
  bool vec = aligned16(a->xland) && aligned16(a->xice) && aligned16(count);
  for (int f = 0; f < n; f++) {
    k.src[f] = e[f].src; k.acc[f] = e[f].acc; k.nlev[f] = e[f].nlev; k.op[f] = e[f].op; k.scale[f] = e[f].scale;
    if (e[f].nlev > 1) k.any_layered = 1;
    vec = vec && aligned16(e[f].src) && aligned16(e[f].acc);
  }
  if (k.any_layered && (ni & 3)) vec = false;
  k.xland = a->xland; k.xice = a->xice; k.count = count; k.xice_thres = a->xice_thres;
  k.n = n; k.ni = ni; k.ncol = ncol;
  const long nthread = (n > 0 || count) ? (vec ? (ncol + 3) / 4 : ncol) : 0;
  k.col_blocks = grid_1d(nthread, kBlock).x;
  unsigned probe_blocks = 0;
  if (p && p->npoint > 0 && p->nfield > 0) {
    for (int f = 0; f < p->nfield; f++) k.field[f] = p->field[f];
    k.column = p->column; k.npoint = p->npoint; k.nfield = p->nfield;
    k.ring = p->ring + (size_t)(p->slot % p->nslot) * p->nfield * p->npoint;
    probe_blocks = grid_1d(p->npoint * p->nfield, kBlock).x;
  }
  const unsigned blocks = k.col_blocks + probe_blocks;
  if (blocks == 0) return 0;
  if (vec) hipLaunchKernelGGL(noahmp_history_step_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, k);
  else hipLaunchKernelGGL(noahmp_history_step_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_history_finish(int n, const noahmp_history_entry* e, void* const* dst, const uint32_t* fin_flags, const int32_t* count,
                              const int32_t* perm, const int32_t* ivgtyp_src, int iswater, float fill, int ni, int nj, void* stream) {
  static const char* who = "noahmp_hip_history_finish";
  int rc = check_entries(who, n, e);
  if (rc) return rc;
  if (n > 0 && !fin_flags) return refuse(-105, "noahmp_hip_history_finish: fin_flags is required");
  const long ncol = (long)ni * nj;
  if (bad_window(ni, nj)) return refuse(-105, "noahmp_hip_history_finish: 0 .. 2^31 - 1 columns");
  for (int f = 0; f < n; f++)
    if ((fin_flags[f] & NOAHMP_HIST_FIN_MEAN) && !count) return refuse(-105, "noahmp_hip_history_finish: NOAHMP_HIST_FIN_MEAN needs the count plane");
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  hipStream_t s = stream_of(stream);
  FinKArgs k;
  memset(&k, 0, sizeof(k));
  for (int f = 0; f < n; f++) {
    k.acc[f] = e[f].acc; k.dst[f] = dst ? (float*)dst[f] : nullptr; k.nlev[f] = e[f].nlev; k.op[f] = e[f].op; k.flags[f] = fin_flags[f];
  }
  k.count = count; k.perm = perm; k.vegtyp = ivgtyp_src; k.iswater = iswater; k.n = n; k.ni = ni; k.nj = nj; k.fill = fill;
  if (ncol > 0 && n > 0)
    hipLaunchKernelGGL(noahmp_history_finish_kernel, grid_1d(ncol, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
