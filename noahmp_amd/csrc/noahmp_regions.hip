// Region series of a device-resident run: per step, weighted sums / minima / maxima of fields of the step block over labelled regions
// (basins, counties, land-use zones).  No reference counterpart: hydrology users hold a basin mean of runoff, SWE, soil moisture or ET
// against a gauge, and a fetch of whole arrays every step (68 ms at 7 M columns) would run the model at PCIe speed.
//
// This is the one place where values of DIFFERENT columns are combined, so the order of summation is part of the result.  It is fixed
// by the TILE order of the cells (the contract is in include/noahmp_hip.h and INTEGRATION.md section 2e): the members of a region in
// ascending tile index are cut into chunks of 256 terms, a chunk is folded as a binary tree (h = 128 .. 1: v[i] += v[i+h]) and the
// partials of a region are summed the same way, level by level.  The column order of the block only decides WHERE a member's sample
// is read (plan: member -> position), never when it is added: the same bits in tile order, in any sorted layout, after any re-sort.
// No floating-point atomics anywhere.
//
// Plan (noahmp_hip_region_plan, on the device, into one caller-owned int32 workspace): a stable radix sort of the cells by region id
// with the tile index as value; region offsets by binary search; chunk offsets of each level by exclusive scans; the members' weights
// and positions in member order.  Step: level 1 is the only pass over the cells -- a wave owns a chunk, lane l holds elements l, l+64,
// l+128, l+192, so the folds at h = 128 and 64 stay in the lane and h = 32 .. 1 are cross-lane shuffles of float64; nothing in LDS.  Per
// member 16 bytes (position, weight, XLAND, XICE) + 4 per entry.  Levels 2 and 3 (one launch each, tiny) fold the partials; the last
// one writes the ring slot and the interval accumulators.
//
// A block in a sorted layout is read through the members' positions (random 4-byte reads); whether bringing the planes to tile order
// first would pay has not been measured (tools/region_bench.py times the direct read against a copy of the same bytes).
//
// The host keeps what it knows of a plan (sizes, levels) in a map keyed by the workspace's address: the workspace must stay where
// it was planned, a copy of it is no plan, and noahmp_hip_finalize forgets every plan.
#include <string.h>
#include <mutex>
#include <unordered_map>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "noahmp_hip.h"
#include "nmp_dev_regions.hpp"
#include "nmp_region_tree.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

// the chunk / offset kernels and the fold of a chunk: nmp_region_tree.hpp (shared with noahmp_regrid_conserve.hip)
using tree::kChunk; using tree::kBlock; using tree::kWaves;
using tree::region_offsets_kernel; using tree::region_chunks_kernel; using tree::ChunkCount; using tree::wave_fold;
constexpr int kMaxEntries = NOAHMP_REG_MAX_ENTRIES, kMaxLevels = 64;
constexpr int kChunksPerWave = 4;        // consecutive chunks of one wave (level 1)
constexpr int kBatch = 4;                // entries whose loads are issued before the first fold

// the plan's header words
enum { H_SPARE, H_NI, H_NJ, H_NREGION, H_NMEMBER, H_NCHUNK1, H_NCHUNK2, H_MAXC1, H_BAD, H_WEIGHT, H_WORDS = 16 };

struct Layout {                          // word offsets of the plan's sections, a function of (ni, nj, nregion) alone
  long n, nregion, b1, b2;
  long roff, choff1, choff2, cstart1, cstart2, tile, pos, w, words;
};
inline long even(long x) { return (x + 1) & ~1L; }
Layout layout_of(int ni, int nj, int nregion) {
  Layout l;
  l.n = (long)ni * nj; l.nregion = nregion;
  l.b1 = l.n / kChunk + nregion + 1;     // chunks of level 1: every region ends with at most one partial chunk
  l.b2 = l.b1 / kChunk + nregion + 1;
  long o = H_WORDS;
  l.roff = o; o += even(nregion + 1);
  l.choff1 = o; o += even(nregion + 1);
  l.choff2 = o; o += even(nregion + 1);
  l.cstart1 = o; o += even(l.b1 + 1);
  l.cstart2 = o; o += even(l.b2 + 1);
  l.tile = o; o += even(l.n);
  l.pos = o; o += even(l.n);
  l.w = o; o += even(l.n);
  l.words = o;
  return l;
}

// what the host knows about a plan it built (the step must not read the device to size its launches)
struct PlanInfo { int ni, nj, nregion, nmember, nchunk1, nchunk2, levels, has_w; Layout l; };
std::mutex g_mu;                         // g_plans
std::mutex g_plan_mu;                    // sc: one noahmp_hip_region_plan at a time
std::unordered_map<const void*, PlanInfo> g_plans;

struct Scratch {
  unsigned* keys_in = nullptr; unsigned* keys_out = nullptr; int* idx_in = nullptr; void* tmp = nullptr;
  size_t keys_in_b = 0, keys_out_b = 0, idx_in_b = 0, tmp_b = 0;
  int* h_hdr = nullptr;                  // pinned
} sc;

// ---------------------------------------------------------------------------------------------------------------- plan kernels
__global__ void __launch_bounds__(kBlock) region_key_kernel(const int* region, long n, int nregion, unsigned* keys, int* idx, int* hdr) {
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const int id = region[t];
  if (id >= nregion) hdr[H_BAD] = 1;     // every writer stores the same word
  keys[t] = (id < 0 || id >= nregion) ? (unsigned)nregion : (unsigned)id;      // non-members sort behind the last region
  idx[t] = (int)t;
}

// weights and positions in member order; weight NULL: positions only (noahmp_hip_region_plan_follow)
__global__ void __launch_bounds__(kBlock) region_members_kernel(const int* tile, const int* roff, int nregion, const float* weight, bool set_w,
                                                                const int* inv_perm, float* w, int* pos) {
  const long m = (long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= roff[nregion]) return;
  const int t = tile[m];
  if (set_w) w[m] = weight ? weight[t] : 1.f;
  pos[m] = inv_perm ? inv_perm[t] : t;
}

__global__ void region_header_kernel(int* hdr, const int* roff, const int* choff1, const int* choff2, int ni, int nj, int nregion, int has_w) {
  hdr[H_NI] = ni; hdr[H_NJ] = nj; hdr[H_NREGION] = nregion; hdr[H_WEIGHT] = has_w;
  hdr[H_NMEMBER] = roff[nregion]; hdr[H_NCHUNK1] = choff1[nregion]; hdr[H_NCHUNK2] = choff2[nregion];
}

// ---------------------------------------------------------------------------------------------------------------- step kernels
struct L1Args {                          // by value
  const float* src[kMaxEntries];
  int nlev[kMaxEntries], lev[kMaxEntries], op[kMaxEntries];
  const int* cstart; const int* pos; const float* w;
  const float* xland; const float* xice;
  double* out;                           // [n][nchunk]
  float xice_thres;
  int n, ni, nchunk;
  long ncol;
};

__global__ void __launch_bounds__(kBlock) noahmp_region_level1_kernel(const L1Args k) {
  const int lane = threadIdx.x & 63;
  const long c0 = ((long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kChunksPerWave;
  for (int u = 0; u < kChunksPerWave; u++) {
    const long c = c0 + u;
    if (c >= k.nchunk) return;                                      // the same for every lane of the wave
    const int s = k.cstart[c], e = min(s + kChunk, k.cstart[c + 1]);
    int p[4]; float w[4]; bool tk[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int m = s + lane + 64 * q;
      p[q] = m < e ? k.pos[m] : -1;
      if (p[q] < 0 || (long)p[q] >= k.ncol) p[q] = -1;              // padding, or a position outside the block (a wrong inv_perm is
                                                                    // not reported): reads nothing, contributes nothing
      w[q] = (p[q] >= 0 && k.w) ? k.w[m] : 1.f;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) tk[q] = p[q] >= 0 && hist_takes_part(k.xland[p[q]], k.xice[p[q]], k.xice_thres);
    for (int f0 = 0; f0 < k.n; f0 += kBatch) {
      float x[kBatch][4];
#pragma unroll
      for (int b = 0; b < kBatch; b++) {                            // the loads of a batch of entries before its first fold
        const int f = f0 + b;
        if (f >= k.n) break;
        const float* src = k.src[f];
        const int nk = k.nlev[f], lv = k.lev[f];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          x[b][q] = 1.f;
          if (!tk[q] || !src) continue;                             // a cell that takes no part contributes +0.0 whatever it holds
          const int c1 = p[q];
          size_t o = (size_t)c1;
          if (nk > 1) { const int row = c1 / k.ni; o = ((size_t)row * nk + lv) * k.ni + (c1 - row * k.ni); }        // (i,k,j) layout
          x[b][q] = src[o];
        }
      }
#pragma unroll
      for (int b = 0; b < kBatch; b++) {
        const int f = f0 + b;
        if (f >= k.n) break;
        const int op = k.op[f];
        const double r = wave_fold(op, reg_term(op, tk[0], w[0], x[b][0]), reg_term(op, tk[1], w[1], x[b][1]),
                                   reg_term(op, tk[2], w[2], x[b][2]), reg_term(op, tk[3], w[3], x[b][3]));
        if (lane == 0) k.out[(size_t)f * k.nchunk + c] = r;
      }
    }
  }
}

struct UpArgs {
  const double* in; long nin;            // [n][nin]: the partials of the level below
  const int* cstart; int nchunk;
  double* out;                           // [n][nchunk], or for the last level (chunk = region):
  double* series; double* acc;           // the ring slot [n][nregion]; the interval accumulators or NULL
  int last;
  int op[kMaxEntries];
};

// levels 2 and 3: a wave folds one chunk of partials of entry blockIdx.y
__global__ void __launch_bounds__(kBlock) noahmp_region_upper_kernel(const UpArgs k) {
  const int lane = threadIdx.x & 63, f = blockIdx.y;
  const long c = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (c >= k.nchunk) return;
  const int op = k.op[f];
  const int s = k.cstart[c], e = min(s + kChunk, k.cstart[c + 1]);
  const double* in = k.in + (size_t)f * k.nin;
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { const int m = s + lane + 64 * q; v[q] = m < e ? in[m] : reg_identity(op); }
  const double r = wave_fold(op, v[0], v[1], v[2], v[3]);
  if (lane != 0) return;
  const size_t o = (size_t)f * k.nchunk + c;
  if (!k.last) { k.out[o] = r; return; }
  k.series[o] = r;
  if (k.acc) k.acc[o] = reg_combine(op, k.acc[o], r);
}

}  // namespace

namespace nmp_host {
void regions_finalize() {
  std::lock_guard<std::mutex> pk(g_plan_mu);
  std::lock_guard<std::mutex> lk(g_mu);
  g_plans.clear();
  hipFree(sc.keys_in); hipFree(sc.keys_out); hipFree(sc.idx_in); hipFree(sc.tmp);
  if (sc.h_hdr) hipHostFree(sc.h_hdr);
  sc = Scratch();
}
}  // namespace nmp_host

extern "C" {

int noahmp_hip_region_plan_size(int ni, int nj, int nregion, int64_t* words) {
  if (!words) return refuse(-105, "noahmp_hip_region_plan_size: words is required");
  if (ni < 0 || nj < 0 || (long)ni * nj > NOAHMP_REG_MAX_CELLS) return refuse(-105, "noahmp_hip_region_plan_size: 0 .. 2^24 cells");
  if (nregion < 0 || nregion > NOAHMP_REG_MAX_CELLS) return refuse(-105, "noahmp_hip_region_plan_size: 0 .. 2^24 regions");
  *words = layout_of(ni, nj, nregion).words;
  return 0;
}

int noahmp_hip_region_plan(const int32_t* region_tile, const float* weight_tile, int ni, int nj, int nregion, const int32_t* inv_perm,
                           int32_t* plan, int64_t plan_words, void* stream) {
  static const char* who = "noahmp_hip_region_plan";
  int64_t need_words = 0;
  int rc = noahmp_hip_region_plan_size(ni, nj, nregion, &need_words);
  if (rc) return rc;
  if (!region_tile || !plan) return refuse(-105, "noahmp_hip_region_plan: region_tile and plan are required");
  if ((uintptr_t)plan & 7u) return refuse(-105, "noahmp_hip_region_plan: the plan workspace must be 8-byte aligned");
  if (plan_words < need_words)
    return refuse(-105, "%s: the workspace has %lld words, noahmp_hip_region_plan_size asks for %lld", who, (long long)plan_words, (long long)need_words);
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  hipStream_t s = stream_of(stream);
  const Layout l = layout_of(ni, nj, nregion);
  const long n = l.n;
  std::lock_guard<std::mutex> pk(g_plan_mu);
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_plans.erase(plan);                                            // unusable until this call has succeeded
  }
  int* hdr = plan;
  int* roff = plan + l.roff; int* choff1 = plan + l.choff1; int* choff2 = plan + l.choff2;
  int* cstart1 = plan + l.cstart1; int* cstart2 = plan + l.cstart2;
  int* tile = plan + l.tile; int* pos = plan + l.pos; float* w = (float*)(plan + l.w);
  if (!sc.h_hdr) HIPCHK(hipHostMalloc((void**)&sc.h_hdr, H_WORDS * sizeof(int), hipHostMallocDefault));
  HIPCHK(hipMemsetAsync(hdr, 0, H_WORDS * sizeof(int), s));
  if (n > 0) {
    if ((rc = nmp_host::ensure_bytes((void**)&sc.keys_in, &sc.keys_in_b, n * 4))) return rc;
    if ((rc = nmp_host::ensure_bytes((void**)&sc.keys_out, &sc.keys_out_b, n * 4))) return rc;
    if ((rc = nmp_host::ensure_bytes((void**)&sc.idx_in, &sc.idx_in_b, n * 4))) return rc;
    const dim3 nb = grid_1d(n, kBlock);
    hipLaunchKernelGGL(region_key_kernel, nb, dim3(kBlock), 0, s, region_tile, n, nregion, sc.keys_in, sc.idx_in, hdr);
    int bits = 1;
    while (bits < 32 && (1u << bits) <= (unsigned)nregion) bits++;  // keys are 0 .. nregion
    size_t need = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, need, sc.keys_in, sc.keys_out, sc.idx_in, tile, (size_t)n, 0, bits, s));
    if ((rc = nmp_host::ensure_bytes(&sc.tmp, &sc.tmp_b, need))) return rc;
    HIPCHK(rocprim::radix_sort_pairs(sc.tmp, need, sc.keys_in, sc.keys_out, sc.idx_in, tile, (size_t)n, 0, bits, s));   // LSD radix: stable
  }
  const dim3 rb = grid_1d(nregion + 1, kBlock);
  hipLaunchKernelGGL(region_offsets_kernel, rb, dim3(kBlock), 0, s, sc.keys_out, n, nregion, roff);
  auto cnt = rocprim::make_counting_iterator<int>(0);
  for (int level = 1; level <= 2; level++) {
    const int* off = level == 1 ? roff : choff1;
    int* choff = level == 1 ? choff1 : choff2;
    auto in = rocprim::make_transform_iterator(cnt, ChunkCount{off, nregion});
    size_t need = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, need, in, choff, 0, (size_t)nregion + 1, rocprim::plus<int>(), s));
    if ((rc = nmp_host::ensure_bytes(&sc.tmp, &sc.tmp_b, need))) return rc;
    HIPCHK(rocprim::exclusive_scan(sc.tmp, need, in, choff, 0, (size_t)nregion + 1, rocprim::plus<int>(), s));
    const long bound = level == 1 ? l.b1 : l.b2;
    hipLaunchKernelGGL(region_chunks_kernel, grid_1d(bound + 1, kBlock), dim3(kBlock), 0, s, off, choff, nregion, bound,
                       level == 1 ? cstart1 : cstart2, level == 1 ? hdr + H_MAXC1 : (int*)nullptr);
  }
  if (n > 0)
    hipLaunchKernelGGL(region_members_kernel, grid_1d(n, kBlock), dim3(kBlock), 0, s, tile, roff, nregion, weight_tile, true,
                       inv_perm, w, pos);
  hipLaunchKernelGGL(region_header_kernel, dim3(1), dim3(1), 0, s, hdr, roff, choff1, choff2, ni, nj, nregion, weight_tile ? 1 : 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sc.h_hdr, hdr, H_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (sc.h_hdr[H_BAD]) {
    hipMemsetAsync(hdr, 0, H_WORDS * sizeof(int), s);
    return refuse(-105, "%s: a cell has a region id >= nregion = %d", who, nregion);
  }
  PlanInfo pi;
  pi.ni = ni; pi.nj = nj; pi.nregion = nregion; pi.l = l;
  pi.nmember = sc.h_hdr[H_NMEMBER]; pi.nchunk1 = sc.h_hdr[H_NCHUNK1]; pi.nchunk2 = sc.h_hdr[H_NCHUNK2];
  pi.has_w = sc.h_hdr[H_WEIGHT];
  pi.levels = sc.h_hdr[H_MAXC1] > kChunk ? 3 : 2;                   // 2^24 cells: at most 65 536 chunks, 256 partials of level 2, one of level 3
  std::lock_guard<std::mutex> lk(g_mu);
  g_plans[plan] = pi;
  return 0;
}

static int find_plan(const char* who, const void* plan, PlanInfo& pi) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_plans.find(plan);
  if (!plan || it == g_plans.end())
    return refuse(-105, "%s: not a plan noahmp_hip_region_plan has built", who);
  pi = it->second;
  return 0;
}

int noahmp_hip_region_plan_follow(int32_t* plan, const int32_t* inv_perm, void* stream) {
  PlanInfo pi;
  int rc = find_plan("noahmp_hip_region_plan_follow", plan, pi);
  if (rc) return rc;
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  hipStream_t s = stream_of(stream);
  if (pi.nmember > 0)
    hipLaunchKernelGGL(region_members_kernel, grid_1d(pi.nmember, kBlock), dim3(kBlock), 0, s, plan + pi.l.tile,
                       plan + pi.l.roff, pi.nregion, (const float*)nullptr, false, inv_perm, (float*)nullptr, plan + pi.l.pos);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_region_scratch_size(const int32_t* plan, int n, int64_t* bytes) {
  PlanInfo pi;
  int rc = find_plan("noahmp_hip_region_scratch_size", plan, pi);
  if (rc) return rc;
  if (n < 0 || n > kMaxEntries || !bytes) return refuse(n > kMaxEntries ? -107 : -105, "noahmp_hip_region_scratch_size: 0..32 entries, bytes is required");
  const int64_t v = (int64_t)sizeof(double) * n * ((int64_t)pi.nchunk1 + pi.nchunk2);
  *bytes = v > 8 ? v : 8;
  return 0;
}

int noahmp_hip_region_step(const int32_t* plan, int n, const noahmp_region_entry* e, const noahmp_step_args* a, double* series, int nslot,
                           int slot, double* acc, void* scratch, void* stream) {
  static const char* who = "noahmp_hip_region_step";
  if (n < 0 || n > kMaxEntries) return refuse(-107, "%s: 0..%d entries per call (n = %d)", who, kMaxEntries, n);
  if (n > 0 && !e) return refuse(-105, "noahmp_hip_region_step: entries are NULL");
  for (int f = 0; f < n; f++) {
    if (e[f].op < NOAHMP_REG_SUM || e[f].op > NOAHMP_REG_MAX) return refuse(-105, "%s: entry %d has op %d (NOAHMP_REG_SUM .. NOAHMP_REG_MAX)", who, f, e[f].op);
    if (e[f].nlev < 1 || e[f].nlev > kMaxLevels || e[f].lev < 0 || e[f].lev >= e[f].nlev) {
      return refuse(-105, "%s: entry %d takes level %d of %d (1..%d levels)", who, f, e[f].lev, e[f].nlev, kMaxLevels);
    }
  }
  PlanInfo pi;
  int rc = find_plan(who, plan, pi);
  if (rc) return rc;
  if (!a || !a->xland || !a->xice) return refuse(-105, "noahmp_hip_region_step: the step block and its XLAND / XICE planes are required");
  if (a->ims != a->its || a->ime != a->ite || a->jms != a->jts || a->jme != a->jte) return refuse(-105, "noahmp_hip_region_step: the memory block must be the tile");
  if (a->ime - a->ims + 1 != pi.ni || a->jme - a->jms + 1 != pi.nj)
    return refuse(-105, "%s: the block is %d x %d, the plan's tile %d x %d", who, a->ime - a->ims + 1, a->jme - a->jms + 1, pi.ni, pi.nj);
  if (!series || nslot < 1 || slot < 0) return refuse(-105, "noahmp_hip_region_step: the series ring is required, with nslot >= 1 and slot >= 0");
  if (!scratch || ((uintptr_t)scratch & 7u)) return refuse(-105, "noahmp_hip_region_step: scratch is required, 8-byte aligned");
  rc = nmp_host::ensure_init();
  if (rc) return rc;
  if (n == 0 || pi.nregion == 0) return 0;
  hipStream_t s = stream_of(stream);
  double* p1 = (double*)scratch;
  double* p2 = p1 + (size_t)n * pi.nchunk1;
  if (pi.nchunk1 > 0) {
    L1Args k;
    memset(&k, 0, sizeof k);
    for (int f = 0; f < n; f++) {
      k.src[f] = e[f].src; k.nlev[f] = e[f].nlev; k.lev[f] = e[f].lev; k.op[f] = e[f].op;
    }
    k.pos = plan + pi.l.pos;
    k.xland = a->xland; k.xice = a->xice;
    k.cstart = plan + pi.l.cstart1; k.w = pi.has_w ? (const float*)(plan + pi.l.w) : nullptr;      // absent: 1, and 4 bytes per member less
    k.xice_thres = a->xice_thres;
    k.out = p1; k.n = n; k.ni = pi.ni; k.nchunk = pi.nchunk1; k.ncol = (long)pi.ni * pi.nj;
    const int per_block = kWaves * kChunksPerWave;
    hipLaunchKernelGGL(noahmp_region_level1_kernel, grid_1d(pi.nchunk1, per_block), dim3(kBlock), 0, s, k);
  }
  UpArgs u;
  memset(&u, 0, sizeof u);
  for (int f = 0; f < n; f++) u.op[f] = e[f].op;
  if (pi.levels == 3) {
    u.in = p1; u.nin = pi.nchunk1; u.cstart = plan + pi.l.cstart2; u.nchunk = pi.nchunk2; u.out = p2; u.last = 0;
    hipLaunchKernelGGL(noahmp_region_upper_kernel, dim3((unsigned)((pi.nchunk2 + kWaves - 1) / kWaves), (unsigned)n), dim3(kBlock), 0, s, u);
    u.in = p2; u.nin = pi.nchunk2; u.cstart = plan + pi.l.choff2;
  } else {
    u.in = p1; u.nin = pi.nchunk1; u.cstart = plan + pi.l.choff1;
  }
  u.nchunk = pi.nregion; u.out = nullptr; u.last = 1;               // the last level: chunk r = the partials of region r
  u.series = series + (size_t)(slot % nslot) * n * pi.nregion; u.acc = acc;
  hipLaunchKernelGGL(noahmp_region_upper_kernel, dim3((unsigned)((pi.nregion + kWaves - 1) / kWaves), (unsigned)n), dim3(kBlock), 0, s, u);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
