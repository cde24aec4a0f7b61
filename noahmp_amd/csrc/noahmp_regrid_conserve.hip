// Budget-preserving regrid of a flux (precipitation) of a device-resident run: the bilinear field, optionally shaped by a fine pattern,
// rescaled per source cell so that the area-weighted mean over the model cells the source cell owns equals the source cell's value.  No
// reference counterpart (the reference reads forcing already on the model grid, netcdf_io:1140): the contract is the text in
// include/noahmp_hip.h, the arithmetic is nmp_dev_regrid_conserve.hpp.
//
// After the region series this is the second place where values of DIFFERENT columns are combined, and it sums the same way: the members
// of a group (the window cells a source cell owns, in ascending window index) are cut into chunks of 256 terms, a chunk is folded as a
// binary tree and the partials of a group are summed the same way, level by level (nmp_region_tree.hpp: the fold and the chunk offsets
// are the region series' own).  The column order of the destination only decides WHERE a cell's value is written (dst_index), never when
// its term is added.  No floating-point atomics anywhere.
//
// Plan (noahmp_hip_regrid_conserve_plan, on the device, into one caller-owned int32 workspace): the owner of every window cell from the
// regrid plan; a stable radix sort of the cells by owner with the window index as value; group offsets by binary search; chunk offsets of
// each level by exclusive scans; the members' areas in member order; D_s by the same tree; the clipped count from two flag bits per group
// (integer atomics).  The plan is immutable afterwards.
//
// Record (noahmp_hip_forcing_regrid_conserve, at most four launches, enqueued only): level 1 is the one pass over the members -- a wave
// owns a chunk, lane l holds elements l, l+64, l+128, l+192, the term is made on the fly from the member's five plan words, its gathered
// corners, its area and its pattern value; the plan words are shared by the entries of a call and the loads of a batch of entries are
// issued before the first fold.  The upper levels fold the partials; the last one turns N_s into what the group hands to its members
// (8 bytes per group and entry, a table that stays in L2).  The apply pass runs over the window in window order, recomputes v and
// multiplies: 24 B of plan and group per cell, 4 B of dst_index, 4 B per pattern read and 4 B per entry written.
#include <string.h>
#include <mutex>
#include <unordered_map>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "noahmp_hip.h"
#include "nmp_dev_regrid_conserve.hpp"
#include "nmp_region_tree.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::stream_of, nmp_host::grid_1d;
using tree::kChunk; using tree::kBlock; using tree::kWaves;
using tree::region_offsets_kernel; using tree::region_chunks_kernel; using tree::ChunkCount; using tree::wave_fold;

namespace {

constexpr int kMaxEntries = NOAHMP_REGRID_CONSERVE_MAX_ENTRIES;
#ifndef NMP_RC_CHUNKS_PER_WAVE
#define NMP_RC_CHUNKS_PER_WAVE 1
#endif
#ifndef NMP_RC_BATCH
#define NMP_RC_BATCH 1
#endif
constexpr int kChunksPerWave = NMP_RC_CHUNKS_PER_WAVE;      // consecutive chunks of one wave (level 1)
constexpr int kBatch = NMP_RC_BATCH;                        // entries whose loads are issued before the first fold / store
constexpr long kMaxCells = NOAHMP_REG_MAX_CELLS;

// the plan's header words
enum { H_SPARE, H_NI, H_NJ, H_NGROUP, H_NMEMBER, H_NCHUNK1, H_NCHUNK2, H_MAXC1, H_BAD, H_AREA, H_CLIPPED, H_WORDS = 16 };

struct Layout {                          // word offsets of the plan's sections, a function of (ni, nj, ngroup) alone
  long n, ngroup, b1, b2;
  long goff, choff1, choff2, cstart1, cstart2, member, group, aw, gflag, dsum, words;
};
inline long even(long x) { return (x + 1) & ~1L; }
Layout layout_of(int ni, int nj, long ngroup) {
  Layout l;
  l.n = (long)ni * nj; l.ngroup = ngroup;
  l.b1 = l.n / kChunk + ngroup + 1;      // chunks of level 1: every group ends with at most one partial chunk
  l.b2 = l.b1 / kChunk + ngroup + 1;
  long o = H_WORDS;
  l.goff = o; o += even(ngroup + 1);
  l.choff1 = o; o += even(ngroup + 1);
  l.choff2 = o; o += even(ngroup + 1);
  l.cstart1 = o; o += even(l.b1 + 1);
  l.cstart2 = o; o += even(l.b2 + 1);
  l.member = o; o += even(l.n);
  l.group = o; o += even(l.n);
  l.aw = o; o += even(l.n);
  l.gflag = o; o += even(ngroup);
  l.dsum = o; o += 2 * ngroup;           // float64, at an even word
  l.words = o;
  return l;
}

// what the host knows about a plan it built (the record call must not read the device to size its launches)
struct PlanInfo { int ni, nj, nx, ny, periodic, nmember, nchunk1, nchunk2, levels, has_area; Layout l; };
std::mutex g_mu;                         // g_plans
std::mutex g_plan_mu;                    // sc: one noahmp_hip_regrid_conserve_plan at a time
std::unordered_map<const void*, PlanInfo> g_plans;

struct Scratch {
  unsigned* keys_in = nullptr; unsigned* keys_out = nullptr; int* idx_in = nullptr; void* tmp = nullptr; double* part = nullptr;
  size_t keys_in_b = 0, keys_out_b = 0, idx_in_b = 0, tmp_b = 0, part_b = 0;
  int* h_hdr = nullptr;                  // pinned
} sc;

struct GroupResult { float val; int kind; };      // out = kind == RC_SCALE ? v * val : val

// ---------------------------------------------------------------------------------------------------------------- plan kernels
struct KeyArgs {
  const int* base; const int* near; const float* w[4];
  const float* area; const int* dst_index;
  unsigned* keys; int* idx; int* group; int* gflag; int* hdr;
  long n; int ni, nj, nx, nxny, periodic, edges;
};

__global__ void __launch_bounds__(kBlock) conserve_key_kernel(const KeyArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.n) return;
  const float w[4] = {k.w[0][c], k.w[1][c], k.w[2][c], k.w[3][c]};
  int idx[4];
  const int s = rc_group(k.base[c], k.near[c], w, k.nx, k.nxny, k.periodic, idx);
  k.group[c] = s;
  k.keys[c] = s < 0 ? (unsigned)k.nxny : (unsigned)s;               // non-members sort behind the last group
  k.idx[c] = (int)c;
  if (s < 0) return;
  if (k.area && !rc_area_ok(k.area[c])) k.hdr[H_BAD] = 1;           // every writer stores the same word
  const int j = (int)(c / k.ni), i = (int)(c - (long)j * k.ni);
  int bits = (!k.dst_index || k.dst_index[c] >= 0) ? 1 : 0;         // a written member
  if ((i == 0 && !(k.edges & NOAHMP_REGRID_EDGE_I_FIRST)) || (i == k.ni - 1 && !(k.edges & NOAHMP_REGRID_EDGE_I_LAST)) ||
      (j == 0 && !(k.edges & NOAHMP_REGRID_EDGE_J_FIRST)) || (j == k.nj - 1 && !(k.edges & NOAHMP_REGRID_EDGE_J_LAST)))
    bits |= 2;                                                      // a member on a side of the window that is no edge of the domain
  if ((k.gflag[s] & bits) != bits) atomicOr(k.gflag + s, bits);     // integer
}

// the members' areas in member order
__global__ void __launch_bounds__(kBlock) conserve_members_kernel(const int* member, const int* goff, int ngroup, const float* area, float* aw) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= goff[ngroup]) return;
  aw[m] = area[member[m]];
}

__global__ void __launch_bounds__(kBlock) conserve_clipped_kernel(const int* gflag, int ngroup, int* hdr) {
  const long s = (long)blockIdx.x * kBlock + threadIdx.x;
  if (s < ngroup && gflag[s] == 3) atomicAdd(hdr + H_CLIPPED, 1);
}

__global__ void conserve_header_kernel(int* hdr, const int* goff, const int* choff1, const int* choff2, int ni, int nj, int ngroup, int has_area) {
  hdr[H_NI] = ni; hdr[H_NJ] = nj; hdr[H_NGROUP] = ngroup; hdr[H_AREA] = has_area;
  hdr[H_NMEMBER] = goff[ngroup]; hdr[H_NCHUNK1] = choff1[ngroup]; hdr[H_NCHUNK2] = choff2[ngroup];
}

// ---------------------------------------------------------------------------------------------------------------- record kernels
struct L1Args {                          // by value
  const float* src[kMaxEntries];
  const float* pattern[kMaxEntries];
  const int* cstart; const int* member; const float* aw;
  const int* base; const float* w[4];
  double* out;                           // [n][nchunk]
  int n, nx, nxny, periodic, nchunk, area_only;
  long ncell;
};

// Level 1: a wave owns a chunk of 256 members.  area_only (the plan's D_s): the term is (double)area, nothing else is read.
__global__ void __launch_bounds__(kBlock) noahmp_regrid_conserve_level1_kernel(const L1Args k) {
  const int lane = threadIdx.x & 63;
  const long c0 = ((long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kChunksPerWave;
  for (int u = 0; u < kChunksPerWave; u++) {
    const long ch = c0 + u;
    if (ch >= k.nchunk) return;                                     // the same for every lane of the wave
    const int s = k.cstart[ch], e = min(s + kChunk, k.cstart[ch + 1]);
    int cell[4], idx[4][4];
    float a[4], w[4][4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int m = s + lane + 64 * q;
      cell[q] = m < e ? k.member[m] : -1;
      if (cell[q] < 0 || (long)cell[q] >= k.ncell) cell[q] = -1;    // padding: reads nothing, contributes +0.0
      a[q] = (cell[q] >= 0 && k.aw) ? k.aw[m] : 1.f;
    }
    if (k.area_only) {
      const double r = wave_fold(NOAHMP_REG_SUM, cell[0] >= 0 ? rc_term(a[0], 1.f) : 0.0, cell[1] >= 0 ? rc_term(a[1], 1.f) : 0.0,
                                 cell[2] >= 0 ? rc_term(a[2], 1.f) : 0.0, cell[3] >= 0 ? rc_term(a[3], 1.f) : 0.0);
      if (lane == 0) k.out[ch] = r;
      continue;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {                                   // the plan words of a member: once for all entries
      const int c = cell[q];
#pragma unroll
      for (int j = 0; j < 4; j++) { w[q][j] = c >= 0 ? k.w[j][c] : 0.f; idx[q][j] = 0; }
      ok[q] = c >= 0 && regrid_corners(k.base[c], w[q], k.nx, k.nxny, k.periodic, idx[q]);
    }
    for (int f0 = 0; f0 < k.n; f0 += kBatch) {
      float x[kBatch][4][4], pat[kBatch][4];
#pragma unroll
      for (int b = 0; b < kBatch; b++) {                            // the loads of a batch of entries before its first fold
        const int f = f0 + b;
        if (f >= k.n) break;
        const float* __restrict__ src = k.src[f];
        const float* __restrict__ pt = k.pattern[f];
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
          for (int j = 0; j < 4; j++) x[b][q][j] = (ok[q] && w[q][j] != 0.f) ? src[idx[q][j]] : 0.f;      // a corner of weight zero is never read
          pat[b][q] = (ok[q] && pt) ? pt[cell[q]] : 1.f;
        }
      }
#pragma unroll
      for (int b = 0; b < kBatch; b++) {
        const int f = f0 + b;
        if (f >= k.n) break;
        const bool hp = k.pattern[f] != nullptr;
        double t[4];
#pragma unroll
        for (int q = 0; q < 4; q++) t[q] = ok[q] ? rc_term(a[q], rc_value(regrid_bilinear(w[q], x[b][q]), hp, pat[b][q])) : 0.0;
        const double r = wave_fold(NOAHMP_REG_SUM, t[0], t[1], t[2], t[3]);
        if (lane == 0) k.out[(size_t)f * k.nchunk + ch] = r;
      }
    }
  }
}

struct UpArgs {
  const double* in; long nin;            // [n][nin]: the partials of the level below
  const int* cstart; int nchunk;
  double* out;                           // [n][nchunk]; the last level (chunk = group) of the plan: D_s
  int last_record;                       // the last level of a record: the group's result instead of its sum
  const float* src[kMaxEntries];
  const double* dsum; const int* goff;
  GroupResult* res;                      // [n][ngroup]
  double* group_sum;                     // N_s of entry 0 for the groups that have members, or NULL
};

// what the last level does with the sum r of group (or chunk) c of entry f
__device__ __forceinline__ void upper_store(const UpArgs& k, int f, long c, double r) {
  const size_t o = (size_t)f * k.nchunk + c;
  if (!k.last_record) { k.out[o] = r; return; }
  GroupResult gr;
  gr.kind = rc_group_result(k.src[f][c], k.dsum[c], r, &gr.val);
  k.res[o] = gr;
  if (f == 0 && k.group_sum && k.goff[c + 1] > k.goff[c]) k.group_sum[c] = r;
}

// the middle level: a wave folds one chunk of partials of entry blockIdx.y
__global__ void __launch_bounds__(kBlock) noahmp_regrid_conserve_upper_kernel(const UpArgs k) {
  const int lane = threadIdx.x & 63, f = blockIdx.y;
  const long c = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (c >= k.nchunk) return;
  const int s = k.cstart[c], e = min(s + kChunk, k.cstart[c + 1]);
  const double* in = k.in + (size_t)f * k.nin;
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { const int m = s + lane + 64 * q; v[q] = m < e ? in[m] : 0.0; }
  const double r = wave_fold(NOAHMP_REG_SUM, v[0], v[1], v[2], v[3]);
  if (lane == 0) upper_store(k, f, c, r);
}

// The last level (chunk = group): there are as many groups as source cells and nearly all of them have one partial, so a wave per group
// would be a hundred thousand waves of one element.  A wave takes 64 consecutive groups: a lane folds its own group when it has at most
// four partials -- the same tree written out: every fold of h >= 4 adds the padding's +0.0, then (v0 + v2) + (v1 + v3) -- and the
// groups with more are folded by the whole wave, one after the other.
__global__ void __launch_bounds__(kBlock) noahmp_regrid_conserve_last_kernel(const UpArgs k) {
  const int lane = threadIdx.x & 63, f = blockIdx.y;
  const long c0 = ((long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 64;
  if (c0 >= k.nchunk) return;                                       // the same for every lane of the wave
  const long c = c0 + lane;
  const double* in = k.in + (size_t)f * k.nin;
  int s = 0, cnt = 0;
  if (c < k.nchunk) { s = k.cstart[c]; cnt = min(kChunk, k.cstart[c + 1] - s); }
  if (c < k.nchunk && cnt <= 4) {
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) v[q] = (q < cnt ? in[s + q] : 0.0) + 0.0;
    upper_store(k, f, c, (v[0] + v[2]) + (v[1] + v[3]));
  }
  unsigned long long big = __ballot(c < k.nchunk && cnt > 4);
  while (big) {
    const int b = __ffsll((long long)big) - 1;
    big &= big - 1;
    const int sb = __shfl(s, b, 64), eb = sb + __shfl(cnt, b, 64);
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { const int m = sb + lane + 64 * q; v[q] = m < eb ? in[m] : 0.0; }
    const double r = wave_fold(NOAHMP_REG_SUM, v[0], v[1], v[2], v[3]);
    if (lane == 0) upper_store(k, f, c0 + b, r);
  }
}

struct ApplyArgs {
  const float* src[kMaxEntries];
  float* dst[kMaxEntries];
  const float* pattern[kMaxEntries];
  float fill[kMaxEntries];
  const int* group; const int* dst_index;
  const int* base; const float* w[4];
  const GroupResult* res;
  int n, nx, nxny, periodic, ngroup;
  long ncell, ndst;
};

// The apply pass: one window cell per thread, in window order.  v is made again from the corners (which are in L2) instead of being
// stored by level 1 and read back: a round trip of v would cost 8 B per cell and entry of HBM traffic, the recomputation none.
__global__ void __launch_bounds__(kBlock) noahmp_regrid_conserve_apply_kernel(const ApplyArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const long di = k.dst_index ? (long)k.dst_index[c] : c;
  if (di < 0 || di >= k.ndst) return;                               // a margin cell: summed, not written
  const int s = k.group[c];
  float w[4] = {0.f, 0.f, 0.f, 0.f};
  int idx[4] = {0, 0, 0, 0};
  bool ok = s >= 0 && s < k.ngroup;
  if (ok) {
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = k.w[j][c];
    ok = regrid_corners(k.base[c], w, k.nx, k.nxny, k.periodic, idx);
  }
  for (int f0 = 0; f0 < k.n; f0 += kBatch) {
    float x[kBatch][4], pat[kBatch];
    GroupResult gr[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; b++) {                              // the loads of a batch of entries before its first store
      const int f = f0 + b;
      if (f >= k.n) break;
      const float* __restrict__ src = k.src[f];
#pragma unroll
      for (int j = 0; j < 4; j++) x[b][j] = (ok && w[j] != 0.f) ? src[idx[j]] : 0.f;
      pat[b] = (ok && k.pattern[f]) ? k.pattern[f][c] : 1.f;
      gr[b].val = 0.f; gr[b].kind = RC_ZERO;
      if (ok) gr[b] = k.res[(size_t)f * k.ngroup + s];
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
      const int f = f0 + b;
      if (f >= k.n) break;
      float out = k.fill[f];
      if (ok) out = rc_out(gr[b].kind, gr[b].val, rc_value(regrid_bilinear(w, x[b]), k.pattern[f] != nullptr, pat[b]));
      k.dst[f][di] = out;
    }
  }
}

int check_source(const char* who, const noahmp_regrid_source* src) {
  if (!src) return refuse(-105, "%s: the source grid is NULL", who);
  if (src->nx < 2 || src->ny < 2 || (long)src->nx * src->ny > kMaxCells)
    return refuse(-105, "%s: the source grid needs nx, ny >= 2 and nx*ny <= 2^24 (nx = %d, ny = %d)", who, src->nx, src->ny);
  return 0;
}

int find_plan(const char* who, const void* plan, PlanInfo& pi) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_plans.find(plan);
  if (!plan || it == g_plans.end())
    return refuse(-105, "%s: not a plan noahmp_hip_regrid_conserve_plan has built", who);
  pi = it->second;
  return 0;
}

// the upper levels of one sum on `s`: p1 holds the level-1 partials [n][nchunk1]; `u` carries what the last level does
void launch_upper(const PlanInfo& pi, const int32_t* plan, int n, double* p1, double* p2, UpArgs u, hipStream_t s) {
  const int ngroup = (int)pi.l.ngroup;
  const int last = u.last_record;
  if (pi.levels == 3) {
    UpArgs m = u;
    m.in = p1; m.nin = pi.nchunk1; m.cstart = plan + pi.l.cstart2; m.nchunk = pi.nchunk2; m.out = p2; m.last_record = 0;
    hipLaunchKernelGGL(noahmp_regrid_conserve_upper_kernel, dim3((unsigned)((pi.nchunk2 + kWaves - 1) / kWaves), (unsigned)n), dim3(kBlock), 0, s, m);
    u.in = p2; u.nin = pi.nchunk2; u.cstart = plan + pi.l.choff2;
  } else {
    u.in = p1; u.nin = pi.nchunk1; u.cstart = plan + pi.l.choff1;
  }
  u.nchunk = ngroup; u.last_record = last;                          // the last level: chunk s = the partials of group s
  const int per_block = kWaves * 64;
  hipLaunchKernelGGL(noahmp_regrid_conserve_last_kernel, dim3((unsigned)((ngroup + per_block - 1) / per_block), (unsigned)n), dim3(kBlock), 0, s, u);
}

}  // namespace

namespace nmp_host {
void regrid_conserve_finalize() {
  std::lock_guard<std::mutex> pk(g_plan_mu);
  std::lock_guard<std::mutex> lk(g_mu);
  g_plans.clear();
  hipFree(sc.keys_in); hipFree(sc.keys_out); hipFree(sc.idx_in); hipFree(sc.tmp); hipFree(sc.part);
  if (sc.h_hdr) hipHostFree(sc.h_hdr);
  sc = Scratch();
}
}  // namespace nmp_host

extern "C" {

int noahmp_hip_regrid_conserve_plan_size(int ni, int nj, const noahmp_regrid_source* src, int64_t* words) {
  static const char* who = "noahmp_hip_regrid_conserve_plan_size";
  if (!words) return refuse(-105, "noahmp_hip_regrid_conserve_plan_size: words is required");
  int rc = check_source(who, src);
  if (rc) return rc;
  if (ni < 0 || nj < 0 || (long)ni * nj > kMaxCells) return refuse(-105, "noahmp_hip_regrid_conserve_plan_size: 0 .. 2^24 window cells");
  *words = layout_of(ni, nj, (long)src->nx * src->ny).words;
  return 0;
}

int noahmp_hip_regrid_conserve_plan(const int32_t* regrid_plan, int ni, int nj, const noahmp_regrid_source* src, const float* area,
                                    const int32_t* dst_index, int domain_edges, int32_t* cplan, int64_t cplan_words, int32_t* clipped,
                                    void* stream) {
  static const char* who = "noahmp_hip_regrid_conserve_plan";
  int64_t need_words = 0;
  int rc = noahmp_hip_regrid_conserve_plan_size(ni, nj, src, &need_words);
  if (rc) return rc;
  if (!regrid_plan || !cplan) return refuse(-105, "noahmp_hip_regrid_conserve_plan: regrid_plan and cplan are required");
  if ((uintptr_t)cplan & 7u) return refuse(-105, "noahmp_hip_regrid_conserve_plan: the plan workspace must be 8-byte aligned");
  if (domain_edges < 0 || domain_edges > 15) return refuse(-105, "noahmp_hip_regrid_conserve_plan: domain_edges is a set of NOAHMP_REGRID_EDGE_* bits (0..15)");
  if (cplan_words < need_words)
    return refuse(-105, "%s: the workspace has %lld words, noahmp_hip_regrid_conserve_plan_size asks for %lld", who, (long long)cplan_words, (long long)need_words);
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  hipStream_t s = stream_of(stream);
  const int ngroup = src->nx * src->ny;
  const Layout l = layout_of(ni, nj, ngroup);
  const long n = l.n;
  std::lock_guard<std::mutex> pk(g_plan_mu);
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_plans.erase(cplan);                                           // unusable until this call has succeeded
  }
  int* hdr = cplan;
  int* goff = cplan + l.goff; int* choff1 = cplan + l.choff1; int* choff2 = cplan + l.choff2;
  int* cstart1 = cplan + l.cstart1; int* cstart2 = cplan + l.cstart2;
  int* member = cplan + l.member; int* group = cplan + l.group; float* aw = (float*)(cplan + l.aw);
  int* gflag = cplan + l.gflag; double* dsum = (double*)(cplan + l.dsum);
  if (!sc.h_hdr) HIPCHK(hipHostMalloc((void**)&sc.h_hdr, H_WORDS * sizeof(int), hipHostMallocDefault));
  HIPCHK(hipMemsetAsync(hdr, 0, H_WORDS * sizeof(int), s));
  HIPCHK(hipMemsetAsync(gflag, 0, (size_t)ngroup * sizeof(int), s));
  if (n > 0) {
    if ((rc = nmp_host::ensure_bytes((void**)&sc.keys_in, &sc.keys_in_b, n * 4))) return rc;
    if ((rc = nmp_host::ensure_bytes((void**)&sc.keys_out, &sc.keys_out_b, n * 4))) return rc;
    if ((rc = nmp_host::ensure_bytes((void**)&sc.idx_in, &sc.idx_in_b, n * 4))) return rc;
    KeyArgs k;
    memset(&k, 0, sizeof k);
    k.base = regrid_plan; k.near = regrid_plan + n;
    for (int q = 0; q < 4; q++) k.w[q] = (const float*)(regrid_plan + (2 + q) * n);
    k.area = area; k.dst_index = dst_index; k.keys = sc.keys_in; k.idx = sc.idx_in; k.group = group; k.gflag = gflag; k.hdr = hdr;
    k.n = n; k.ni = ni; k.nj = nj; k.nx = src->nx; k.nxny = ngroup; k.periodic = src->periodic_x ? 1 : 0; k.edges = domain_edges;
    hipLaunchKernelGGL(conserve_key_kernel, grid_1d(n, kBlock), dim3(kBlock), 0, s, k);
    int bits = 1;
    while (bits < 32 && (1u << bits) <= (unsigned)ngroup) bits++;   // keys are 0 .. ngroup
    size_t need = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, need, sc.keys_in, sc.keys_out, sc.idx_in, member, (size_t)n, 0, bits, s));
    if ((rc = nmp_host::ensure_bytes(&sc.tmp, &sc.tmp_b, need))) return rc;
    HIPCHK(rocprim::radix_sort_pairs(sc.tmp, need, sc.keys_in, sc.keys_out, sc.idx_in, member, (size_t)n, 0, bits, s));   // LSD radix: stable
  }
  hipLaunchKernelGGL(region_offsets_kernel, grid_1d(ngroup + 1, kBlock), dim3(kBlock), 0, s, sc.keys_out, n, ngroup, goff);
  auto cnt = rocprim::make_counting_iterator<int>(0);
  for (int level = 1; level <= 2; level++) {
    const int* off = level == 1 ? goff : choff1;
    int* choff = level == 1 ? choff1 : choff2;
    auto in = rocprim::make_transform_iterator(cnt, ChunkCount{off, ngroup});
    size_t need = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, need, in, choff, 0, (size_t)ngroup + 1, rocprim::plus<int>(), s));
    if ((rc = nmp_host::ensure_bytes(&sc.tmp, &sc.tmp_b, need))) return rc;
    HIPCHK(rocprim::exclusive_scan(sc.tmp, need, in, choff, 0, (size_t)ngroup + 1, rocprim::plus<int>(), s));
    const long bound = level == 1 ? l.b1 : l.b2;
    hipLaunchKernelGGL(region_chunks_kernel, grid_1d(bound + 1, kBlock), dim3(kBlock), 0, s, off, choff, ngroup, bound,
                       level == 1 ? cstart1 : cstart2, level == 1 ? hdr + H_MAXC1 : (int*)nullptr);
  }
  if (n > 0 && area)
    hipLaunchKernelGGL(conserve_members_kernel, grid_1d(n, kBlock), dim3(kBlock), 0, s, member, goff, ngroup, area, aw);
  hipLaunchKernelGGL(conserve_clipped_kernel, grid_1d(ngroup, kBlock), dim3(kBlock), 0, s, gflag, ngroup, hdr);
  hipLaunchKernelGGL(conserve_header_kernel, dim3(1), dim3(1), 0, s, hdr, goff, choff1, choff2, ni, nj, ngroup, area ? 1 : 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sc.h_hdr, hdr, H_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (sc.h_hdr[H_BAD]) {
    hipMemsetAsync(hdr, 0, H_WORDS * sizeof(int), s);
    return refuse(-105, "%s: the area of a member is not finite and > 0", who);
  }
  PlanInfo pi;
  pi.ni = ni; pi.nj = nj; pi.nx = src->nx; pi.ny = src->ny; pi.periodic = src->periodic_x ? 1 : 0; pi.l = l;
  pi.nmember = sc.h_hdr[H_NMEMBER]; pi.nchunk1 = sc.h_hdr[H_NCHUNK1]; pi.nchunk2 = sc.h_hdr[H_NCHUNK2];
  pi.has_area = sc.h_hdr[H_AREA];
  pi.levels = sc.h_hdr[H_MAXC1] > kChunk ? 3 : 2;                   // 2^24 cells: at most 65 536 chunks, 256 partials of level 2, one of level 3
  // D_s: the same tree over the members' areas
  if ((rc = nmp_host::ensure_bytes((void**)&sc.part, &sc.part_b, sizeof(double) * (size_t)(pi.nchunk1 + pi.nchunk2 + 1)))) return rc;
  double* p1 = sc.part;
  double* p2 = p1 + pi.nchunk1;
  if (pi.nchunk1 > 0) {
    L1Args k;
    memset(&k, 0, sizeof k);
    k.cstart = cstart1; k.member = member; k.aw = pi.has_area ? aw : nullptr; k.out = p1;
    k.n = 1; k.nchunk = pi.nchunk1; k.area_only = 1; k.ncell = n;
    const int per_block = kWaves * kChunksPerWave;
    hipLaunchKernelGGL(noahmp_regrid_conserve_level1_kernel, grid_1d(pi.nchunk1, per_block), dim3(kBlock), 0, s, k);
  }
  UpArgs u;
  memset(&u, 0, sizeof u);
  u.out = dsum;
  launch_upper(pi, cplan, 1, p1, p2, u, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  if (clipped) *clipped = sc.h_hdr[H_CLIPPED];
  std::lock_guard<std::mutex> lk(g_mu);
  g_plans[cplan] = pi;
  return 0;
}

int noahmp_hip_regrid_conserve_scratch_size(const int32_t* cplan, int n, int64_t* bytes) {
  PlanInfo pi;
  int rc = find_plan("noahmp_hip_regrid_conserve_scratch_size", cplan, pi);
  if (rc) return rc;
  if (n < 1 || n > kMaxEntries) return refuse(-107, "noahmp_hip_regrid_conserve_scratch_size: 1..8 entries");
  if (!bytes) return refuse(-105, "noahmp_hip_regrid_conserve_scratch_size: bytes is required");
  *bytes = (int64_t)n * ((int64_t)sizeof(double) * ((int64_t)pi.nchunk1 + pi.nchunk2) + (int64_t)sizeof(GroupResult) * pi.l.ngroup);
  return 0;
}

int noahmp_hip_forcing_regrid_conserve(const int32_t* cplan, const int32_t* regrid_plan, const noahmp_regrid_source* src,
                                       const int32_t* dst_index, int64_t ndst, int n, const noahmp_regrid_conserve_entry* e,
                                       double* group_sum, void* scratch, void* stream) {
  static const char* who = "noahmp_hip_forcing_regrid_conserve";
  if (n < 1 || n > kMaxEntries) return refuse(-107, "%s: 1..%d entries per call (n = %d)", who, kMaxEntries, n);
  int rc = check_source(who, src);
  if (rc) return rc;
  if (!regrid_plan) return refuse(-105, "noahmp_hip_forcing_regrid_conserve: the regrid plan is NULL");
  if (!e) return refuse(-105, "noahmp_hip_forcing_regrid_conserve: entries are NULL");
  for (int f = 0; f < n; f++)
    if (!e[f].src || !e[f].dst) return refuse(-105, "%s: entry %d has a NULL plane", who, f);
  if (ndst < 0) return refuse(-105, "noahmp_hip_forcing_regrid_conserve: ndst < 0");
  PlanInfo pi;
  rc = find_plan(who, cplan, pi);
  if (rc) return rc;
  if (src->nx != pi.nx || src->ny != pi.ny || (src->periodic_x ? 1 : 0) != pi.periodic)
    return refuse(-105, "%s: the source grid is %d x %d, the plan's %d x %d (or periodic_x differs)", who, src->nx, src->ny, pi.nx, pi.ny);
  if (!scratch || ((uintptr_t)scratch & 7u)) return refuse(-105, "noahmp_hip_forcing_regrid_conserve: scratch is required, 8-byte aligned");
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  const long ncell = pi.l.n;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  const int ngroup = (int)pi.l.ngroup;
  double* p1 = (double*)scratch;
  double* p2 = p1 + (size_t)n * pi.nchunk1;
  GroupResult* res = (GroupResult*)(p2 + (size_t)n * pi.nchunk2);
  const float* wp[4];
  for (int q = 0; q < 4; q++) wp[q] = (const float*)(regrid_plan + (2 + q) * ncell);
  if (pi.nchunk1 > 0) {
    L1Args k;
    memset(&k, 0, sizeof k);
    for (int f = 0; f < n; f++) { k.src[f] = e[f].src; k.pattern[f] = e[f].pattern; }
    k.cstart = cplan + pi.l.cstart1; k.member = cplan + pi.l.member;
    k.aw = pi.has_area ? (const float*)(cplan + pi.l.aw) : nullptr;                               // absent: 1, and 4 bytes per member less
    k.base = regrid_plan;
    for (int q = 0; q < 4; q++) k.w[q] = wp[q];
    k.out = p1; k.n = n; k.nx = pi.nx; k.nxny = ngroup; k.periodic = pi.periodic; k.nchunk = pi.nchunk1; k.ncell = ncell;
    const int per_block = kWaves * kChunksPerWave;
    hipLaunchKernelGGL(noahmp_regrid_conserve_level1_kernel, grid_1d(pi.nchunk1, per_block), dim3(kBlock), 0, s, k);
  }
  UpArgs u;
  memset(&u, 0, sizeof u);
  for (int f = 0; f < n; f++) u.src[f] = e[f].src;
  u.last_record = 1; u.dsum = (const double*)(cplan + pi.l.dsum); u.goff = cplan + pi.l.goff; u.res = res; u.group_sum = group_sum;
  launch_upper(pi, cplan, n, p1, p2, u, s);
  ApplyArgs a;
  memset(&a, 0, sizeof a);
  for (int f = 0; f < n; f++) { a.src[f] = e[f].src; a.dst[f] = e[f].dst; a.pattern[f] = e[f].pattern; a.fill[f] = e[f].fill; }
  a.group = cplan + pi.l.group; a.dst_index = dst_index; a.base = regrid_plan;
  for (int q = 0; q < 4; q++) a.w[q] = wp[q];
  a.res = res; a.n = n; a.nx = pi.nx; a.nxny = ngroup; a.periodic = pi.periodic; a.ngroup = ngroup; a.ncell = ncell; a.ndst = ndst;
  hipLaunchKernelGGL(noahmp_regrid_conserve_apply_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, a);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
