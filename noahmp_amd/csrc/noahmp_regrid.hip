// Forcing regrid of a device-resident run (no reference counterpart: the reference reads forcing already on the model grid, netcdf_io:1140;
// the contract is the text in include/noahmp_hip.h, the arithmetic is nmp_dev_regrid.hpp).  With every resident option on, a 7 M-column
// step spends more time in the 311 MB forcing upload than in the column kernel; real forcing arrives on a grid 50-150 times coarser than
// the model's, so the coarse record is uploaded and the fine planes are made here.
//
// noahmp_hip_forcing_regrid: ONE launch per call.  A pure stream: per column 24 B of plan are read once and 4 B per entry written; the
// corner reads go to source planes of a few hundred KB that stay in L2.  A thread owns four consecutive columns (16-byte loads of the plan
// planes, 16-byte stores) and walks the entries itself, so the plan is paid once per column whatever n is; the corner loads of a batch of
// entries are issued before the first store of the batch.  No LDS, no atomics.  Arrays are caller-owned: nothing is allocated, nothing waits.
//
// noahmp_hip_forcing_regrid_met: the same kernel with a prologue in front of the entry loop (template parameter MET) that serves the met group
// -- t, p, q, lw regridded bilinearly and moved to the model's terrain height (nmp_dev_regrid.hpp::regrid_met: five expf_ and two powf_ per
// column, float64 inside) -- so a record still costs one launch.  All corner loads of the group and the dz load are issued before the first
// libm call; the only LDS is the 768 B of libm tables.  The MET = false instantiations are the kernels of noahmp_hip_forcing_regrid, unchanged.
//
// noahmp_hip_regrid_plan_latlon: one thread per target cell, once per run and tile.  The nearest-valid search runs only in the cells
// whose four corners are masked out; the unfilled count is an integer atomic add of the cells that have none (rare).
#include <string.h>
#include <type_traits>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_regrid.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kMaxEntries = NOAHMP_REGRID_MAX_ENTRIES;
constexpr int kMaxRadius = 16;
constexpr int kBlock = 256, kBatch = 2;

struct RegridKArgs {                     // by value (< 1 KB): no engine-owned buffer, no copy per call
  const float* src[kMaxEntries];
  float* dst[kMaxEntries];
  const float* adjust[kMaxEntries];
  float scale[kMaxEntries];
  float fill[kMaxEntries];
  int mode[kMaxEntries];
  const int* base; const int* near;
  const float* w[4];
  int n, nx, nxny, periodic;
  int any_bilinear, any_nearest;
  long ncell;
};

// the met group rides behind the entries' block: the MET = false kernels take RegridKArgs alone
struct RegridMetKArgs : RegridKArgs {
  const float* msrc[4];                  // t, p, q, lw (lw: NULL without longwave)
  float* mdst[4];
  const float* dz;
  float lapse, mfill;
  int has_lw;
};
template <bool MET> using KArgsOf = std::conditional_t<MET, RegridMetKArgs, RegridKArgs>;

// what one column needs from the plan to serve every entry
struct Col {
  int idx[4];                            // corner indices (BILINEAR)
  float w[4];
  int near;
  bool bil_ok, near_ok;
};

__device__ __forceinline__ Col make_col(const RegridKArgs& k, int base, int near, float w0, float w1, float w2, float w3) {
  Col c;
  c.w[0] = w0; c.w[1] = w1; c.w[2] = w2; c.w[3] = w3;
  c.idx[0] = c.idx[1] = c.idx[2] = c.idx[3] = 0;
  c.bil_ok = k.any_bilinear && regrid_corners(base, c.w, k.nx, k.nxny, k.periodic, c.idx);
  c.near = near;
  c.near_ok = k.any_nearest && regrid_near_ok(near, k.nxny);
  return c;
}

// the loads of one entry and column: a corner of weight zero, and every corner of a column that receives fill, is not read
__device__ __forceinline__ void load_corners(const RegridKArgs& k, int f, const Col& c, float* s) {
  const float* __restrict__ src = k.src[f];
  if (k.mode[f] == NOAHMP_REGRID_BILINEAR) {
#pragma unroll
    for (int q = 0; q < 4; q++) s[q] = (c.bil_ok && c.w[q] != 0.f) ? src[c.idx[q]] : 0.f;
  } else {
    s[0] = c.near_ok ? src[c.near] : 0.f;
  }
}

__device__ __forceinline__ float value(const RegridKArgs& k, int f, const Col& c, const float* s, float adj) {
  float v;
  if (k.mode[f] == NOAHMP_REGRID_BILINEAR) {
    if (!c.bil_ok) return k.fill[f];
    v = regrid_bilinear(c.w, s);
  } else {
    if (!c.near_ok) return k.fill[f];
    v = s[0];
  }
  return k.adjust[f] ? regrid_adjust(v, k.scale[f], adj) : v;
}

// The met group of one column: every corner load of its three or four sources and the dz load first, then the chain, then the stores.
__device__ __forceinline__ void met_group(const RegridMetKArgs& k, const Col& col, long c) {
  float s[4][4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    const float* __restrict__ src = k.msrc[f];
    const bool have = f < 3 || k.has_lw;
#pragma unroll
    for (int j = 0; j < 4; j++) s[f][j] = (have && col.bil_ok && col.w[j] != 0.f) ? src[col.idx[j]] : 0.f;
  }
  const float d = k.dz[c];
  __builtin_amdgcn_sched_barrier(0);     // the loads above are in flight before the first libm call
  RegridMet r;
  r.t = r.p = r.q = r.lw = k.mfill;
  if (col.bil_ok)
    r = regrid_met(regrid_bilinear(col.w, s[0]), regrid_bilinear(col.w, s[1]), regrid_bilinear(col.w, s[2]), regrid_bilinear(col.w, s[3]), d,
                   k.lapse, k.has_lw != 0);
  k.mdst[0][c] = r.t; k.mdst[1][c] = r.p; k.mdst[2][c] = r.q;
  if (k.has_lw) k.mdst[3][c] = r.lw;
}

// VEC: the plan planes, every dst and every adjust are 16-byte aligned and ncell is a multiple of four
// MET: noahmp_hip_forcing_regrid_met -- the met group in front of the unchanged entry loop.  Always one column per thread: with four the
// 64 corner values of a thread are live together (137 VGPRs, 3 waves per SIMD against 46 and 8) and the launch measured 18-38 % slower
// (DESIGN.md section 6), so <true, true> is never instantiated.
template <bool VEC, bool MET>
__global__ void __launch_bounds__(kBlock) noahmp_regrid_kernel(const KArgsOf<MET> k) {
  static_assert(!(VEC && MET), "the met group runs one column per thread");
  if constexpr (MET) libm::libm_stage_tables();      // holds a __syncthreads(): every thread of the workgroup, before any return
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  constexpr int NC = VEC ? 4 : 1;
  const long c0 = t * NC;
  if (c0 >= k.ncell) return;
  Col col[NC];
  if constexpr (VEC) {
    int4 b4 = make_int4(-1, -1, -1, -1), n4 = make_int4(-1, -1, -1, -1);
    float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0, w2 = w0, w3 = w0;
    if (k.any_bilinear) {
      b4 = *(const int4*)(k.base + c0);
      w0 = *(const float4*)(k.w[0] + c0); w1 = *(const float4*)(k.w[1] + c0);
      w2 = *(const float4*)(k.w[2] + c0); w3 = *(const float4*)(k.w[3] + c0);
    }
    if (k.any_nearest) n4 = *(const int4*)(k.near + c0);
    col[0] = make_col(k, b4.x, n4.x, w0.x, w1.x, w2.x, w3.x);
    col[1] = make_col(k, b4.y, n4.y, w0.y, w1.y, w2.y, w3.y);
    col[2] = make_col(k, b4.z, n4.z, w0.z, w1.z, w2.z, w3.z);
    col[3] = make_col(k, b4.w, n4.w, w0.w, w1.w, w2.w, w3.w);
  } else {
    int b = -1, nr = -1;
    float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
    if (k.any_bilinear) { b = k.base[c0]; w0 = k.w[0][c0]; w1 = k.w[1][c0]; w2 = k.w[2][c0]; w3 = k.w[3][c0]; }
    if (k.any_nearest) nr = k.near[c0];
    col[0] = make_col(k, b, nr, w0, w1, w2, w3);
  }
  if constexpr (MET) met_group(k, col[0], c0);
  for (int f0 = 0; f0 < k.n; f0 += kBatch) {
    // the corner loads of a batch of entries are in flight before its first store (planes may alias as far as the compiler knows)
    float s[kBatch][NC][4];
    float adj[kBatch][NC];
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int f = f0 + u;
      if (f >= k.n) break;
#pragma unroll
      for (int q = 0; q < NC; q++) load_corners(k, f, col[q], s[u][q]);
      if constexpr (VEC) {
        float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k.adjust[f]) a4 = *(const float4*)(k.adjust[f] + c0);
        adj[u][0] = a4.x; adj[u][1] = a4.y; adj[u][2] = a4.z; adj[u][3] = a4.w;
      } else {
        adj[u][0] = k.adjust[f] ? k.adjust[f][c0] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int f = f0 + u;
      if (f >= k.n) break;
      if constexpr (VEC) {
        float4 o;
        o.x = value(k, f, col[0], s[u][0], adj[u][0]);
        o.y = value(k, f, col[1], s[u][1], adj[u][1]);
        o.z = value(k, f, col[2], s[u][2], adj[u][2]);
        o.w = value(k, f, col[3], s[u][3], adj[u][3]);
        *(float4*)(k.dst[f] + c0) = o;
      } else {
        k.dst[f][c0] = value(k, f, col[0], s[u][0], adj[u][0]);
      }
    }
  }
}

struct PlanKArgs {
  const float* xlat; const float* xlon;
  const unsigned char* valid;
  int* plan;
  int* unfilled;
  long ncell;
  int nx, ny, periodic, radius;
  double lon0, lat0, dlon, dlat;
};

__global__ void __launch_bounds__(kBlock) noahmp_regrid_plan_kernel(const PlanKArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const RegridCell r = regrid_plan_cell(k.xlat[c], k.xlon[c], k.nx, k.ny, k.lon0, k.lat0, k.dlon, k.dlat, k.periodic, k.valid, k.radius);
  k.plan[c] = r.base;
  k.plan[k.ncell + c] = r.near;
#pragma unroll
  for (int q = 0; q < 4; q++) k.plan[(2 + q) * k.ncell + c] = __float_as_int(r.w[q]);
  if (r.base < 0) atomicAdd(k.unfilled, 1);
}

int check_source(const char* who, const noahmp_regrid_source* src) {
  if (!src) return refuse(-105, "%s: the source grid is NULL", who);
  if (src->nx < 2 || src->ny < 2 || (long)src->nx * src->ny > (1L << 30))
    return refuse(-105, "%s: the source grid needs nx, ny >= 2 and nx*ny <= 2^30 (nx = %d, ny = %d)", who, src->nx, src->ny);
  return 0;
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

int* h_unfilled = nullptr;               // page-locked landing place of the unfilled count

}  // namespace

namespace {

// both regrid calls: the checks, then ONE launch (with_met: noahmp_hip_forcing_regrid_met)
int regrid_call(const char* who, const int32_t* plan, int64_t ncell, const noahmp_regrid_source* src, bool with_met, const noahmp_regrid_met* met,
                int n, const noahmp_regrid_entry* e, void* stream) {
  if (n < 0 || n > kMaxEntries) return refuse(-107, "%s: 0..%d entries per call (n = %d)", who, kMaxEntries, n);
  int rc = check_source(who, src);
  if (rc) return rc;
  if (bad_count(ncell)) return refuse(-105, "%s: 0 .. 2^31 - 1 columns", who);
  if (!plan) return refuse(-105, "%s: the plan is NULL", who);
  if (n > 0 && !e) return refuse(-105, "%s: entries are NULL", who);
  for (int f = 0; f < n; f++) {
    if (e[f].mode < NOAHMP_REGRID_BILINEAR || e[f].mode > NOAHMP_REGRID_NEAREST) {
      return refuse(-105, "%s: entry %d has mode %d (NOAHMP_REGRID_BILINEAR, NOAHMP_REGRID_NEAREST)", who, f, e[f].mode);
    }
    if (!e[f].src || !e[f].dst) return refuse(-105, "%s: entry %d has a NULL plane", who, f);
  }
  if (with_met) {
    if (!met) return refuse(-105, "%s: met is NULL", who);
    if (!met->src_t || !met->src_p || !met->src_q || !met->dst_t || !met->dst_p || !met->dst_q || !met->dz) {
      return refuse(-105, "%s: met needs src_t, src_p, src_q, dst_t, dst_p, dst_q and dz", who);
    }
    if (met->src_lw && !met->dst_lw) return refuse(-105, "%s: met has src_lw but no dst_lw", who);
  }
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  if ((n == 0 && !with_met) || ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  RegridMetKArgs k;                      // the MET = false kernels receive its RegridKArgs part
  memset(&k, 0, sizeof(k));
  bool vec = aligned16(plan) && (ncell & 3) == 0;
  if (with_met) {
    k.msrc[0] = met->src_t; k.msrc[1] = met->src_p; k.msrc[2] = met->src_q; k.msrc[3] = met->src_lw;
    k.mdst[0] = met->dst_t; k.mdst[1] = met->dst_p; k.mdst[2] = met->dst_q; k.mdst[3] = met->src_lw ? met->dst_lw : nullptr;
    k.dz = met->dz; k.lapse = met->lapse; k.mfill = met->fill; k.has_lw = met->src_lw ? 1 : 0;
    k.any_bilinear = 1;
    vec = false;
  }
  for (int f = 0; f < n; f++) {
    k.src[f] = e[f].src; k.dst[f] = e[f].dst; k.adjust[f] = e[f].adjust; k.scale[f] = e[f].scale; k.fill[f] = e[f].fill; k.mode[f] = e[f].mode;
    if (e[f].mode == NOAHMP_REGRID_BILINEAR) k.any_bilinear = 1; else k.any_nearest = 1;
    vec = vec && aligned16(e[f].dst) && aligned16(e[f].adjust);
  }
  k.base = plan; k.near = plan + ncell;
  for (int q = 0; q < 4; q++) k.w[q] = (const float*)(plan + (2 + q) * ncell);
  k.n = n; k.nx = src->nx; k.nxny = src->nx * src->ny; k.periodic = src->periodic_x ? 1 : 0; k.ncell = ncell;
  const long nthread = vec ? ncell / 4 : ncell;
  const dim3 blocks = grid_1d(nthread, kBlock);
  const RegridKArgs& kk = k;
  if (with_met) {
    hipLaunchKernelGGL((noahmp_regrid_kernel<false, true>), blocks, dim3(kBlock), 0, s, k);
  } else {
    if (vec) hipLaunchKernelGGL((noahmp_regrid_kernel<true, false>), blocks, dim3(kBlock), 0, s, kk);
    else hipLaunchKernelGGL((noahmp_regrid_kernel<false, false>), blocks, dim3(kBlock), 0, s, kk);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

namespace nmp_host {
void regrid_finalize() {
  if (h_unfilled) hipHostFree(h_unfilled);
  h_unfilled = nullptr;
}
}  // namespace nmp_host

extern "C" {

int noahmp_hip_regrid_plan_size(int ni, int nj, int64_t* words) {
  if (bad_window(ni, nj) || !words) return refuse(-105, "noahmp_hip_regrid_plan_size: 0 .. 2^31 - 1 cells and a place for the size");
  *words = 6 * (int64_t)ni * nj + 1;
  return 0;
}

int noahmp_hip_regrid_plan_latlon(const float* xlat, const float* xlon, int ni, int nj, const noahmp_regrid_source* src,
                                  const uint8_t* valid_src, int search_radius, int32_t* plan, int64_t plan_words, int32_t* unfilled,
                                  void* stream) {
  static const char* who = "noahmp_hip_regrid_plan_latlon";
  int rc = check_source(who, src);
  if (rc) return rc;
  if (!(src->dlon > 0.0) || !(src->dlat != 0.0)) return refuse(-105, "%s: dlon > 0 and dlat != 0 are required", who);
  if (search_radius < 0 || search_radius > kMaxRadius) return refuse(-105, "%s: search_radius 0..%d (%d)", who, kMaxRadius, search_radius);
  const long ncell = (long)ni * nj;
  if (bad_window(ni, nj)) return refuse(-105, "%s: 0 .. 2^31 - 1 cells", who);
  if (!plan || (ncell > 0 && (!xlat || !xlon))) return refuse(-105, "%s: xlat, xlon and plan are required", who);
  if (plan_words < 6 * (int64_t)ncell + 1)
    return refuse(-105, "%s: the workspace has %lld words, noahmp_hip_regrid_plan_size asks for %lld", who, (long long)plan_words, (long long)(6 * (int64_t)ncell + 1));
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  hipStream_t s = stream_of(stream);
  if (!h_unfilled) HIPCHK(hipHostMalloc((void**)&h_unfilled, sizeof(int), hipHostMallocDefault));
  PlanKArgs k;
  memset(&k, 0, sizeof(k));
  k.xlat = xlat; k.xlon = xlon; k.valid = valid_src; k.plan = plan; k.unfilled = plan + 6 * ncell; k.ncell = ncell;
  k.nx = src->nx; k.ny = src->ny; k.periodic = src->periodic_x ? 1 : 0; k.radius = search_radius;
  k.lon0 = src->lon0; k.lat0 = src->lat0; k.dlon = src->dlon; k.dlat = src->dlat;
  HIPCHK(hipMemsetAsync(k.unfilled, 0, sizeof(int), s));
  if (ncell > 0) hipLaunchKernelGGL(noahmp_regrid_plan_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_unfilled, k.unfilled, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (unfilled) *unfilled = *h_unfilled;
  return 0;
}

int noahmp_hip_forcing_regrid(const int32_t* plan, int64_t ncell, const noahmp_regrid_source* src, int n, const noahmp_regrid_entry* e,
                              void* stream) {
  return regrid_call("noahmp_hip_forcing_regrid", plan, ncell, src, false, nullptr, n, e, stream);
}

int noahmp_hip_forcing_regrid_met(const int32_t* plan, int64_t ncell, const noahmp_regrid_source* src, const noahmp_regrid_met* met, int n,
                                  const noahmp_regrid_entry* e, void* stream) {
  return regrid_call("noahmp_hip_forcing_regrid_met", plan, ncell, src, true, met, n, e, stream);
}

}  // extern "C"
