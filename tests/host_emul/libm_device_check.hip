// TEST INFRASTRUCTURE -- the libm forms of nmp_libm.hpp / nmp_dev_common.hpp run AS DEVICE CODE, built with the library's own flags
// (noahmp_amd.build.FLAGS): the unchecked forms against the checked ones over all 2^32 patterns (the device twin of
// libm_unchecked_check.hip), every form against the host's libm on structured and strided samples (the extension of libm_check.hip's
// libm_gpu_check), and the tables as libm_stage_tables() leaves them in LDS.  Never shipped.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <thread>
#include <vector>
#include "nmp_dev_common.hpp"

using namespace nmp;
using namespace nmp::libm;

#define HD __host__ __device__ static inline
HD bool same(float a, float b) { return (a != a && b != b) || asuint(a) == asuint(b); }
// an ordinary companion argument derived from the bits under test (positive normal, moderate exponent): fills the other slots of a batch
HD float companion(uint32_t bits, int q) { return asfloat(0x3e000000u + ((bits * 2654435761u * (uint32_t)(q + 1)) >> 7)); }
// TDFCND's batch of eight (bases TKICE / 0.57 alternating): the exponent under test at position pos.  rare = 0: the other exponents as
// libm_unchecked_check.hip's check_constbase (+0, -0, ordinary ones), 1: as rare_sites_check.hip (sign flip, +0, -0, derived patterns)
HD float cb_y(uint32_t bits, int pos, int n, int rare) {
  const int q = (n - pos) & 7;
  if (q == 0) return asfloat(bits);
  if (rare) return asfloat(q == 1 ? bits ^ 0x80000000u : (q == 2 ? 0u : (q == 3 ? 0x80000000u : bits * 2654435761u * (uint32_t)q)));
  return q == 1 ? 0.f : (q == 2 ? -0.f : companion(bits, n) - 0.5f);
}

// The two sides of every unchecked-against-checked comparison are called through functions that are not inlined: inlined into one
// kernel the unchecked form and the not-taken-branch path of the checked form are the same expressions, and the compiler folds the
// comparison to true without running it (libm_unchecked_check.hip).  The batch arrays go through scratch memory: fine in a test kernel.
#define NI __device__ __attribute__((noinline)) static
NI float c_expf(float x) { return expf_(x); }
NI float u_expf(float x, unsigned& s) { return expf_u_(x, s); }
NI float c_logf(float x) { return logf_(x); }
NI float u_logf(float x, unsigned& s) { return logf_u_(x, s); }
NI void c_expf4(const float* x, float* o) { expfN_<4>(x, o); }
NI void u_expf4(const float* x, float* o, unsigned& s) { expfN_u_<4>(x, o, s); }
NI void c_logf4(const float* x, float* o) { logfN_<4>(x, o); }
NI void u_logf4(const float* x, float* o, unsigned& s) { logfN_u_<4>(x, o, s); }
NI float c_powf(float x, float y) { return powf_(x, y); }
NI float u_powf(float x, float y, unsigned& s) { return powf_u_(x, y, s); }
NI void c_powf2(const float* x, const float* y, float* o) { powfN_<2>(x, y, o); }
NI void u_powf2(const float* x, const float* y, float* o, unsigned& s) { powfN_u_<2>(x, y, o, s); }
NI void c_powf4(const float* x, const float* y, float* o) { powfN_<4>(x, y, o); }
NI void u_powf4(const float* x, const float* y, float* o, unsigned& s) { powfN_u_<4>(x, y, o, s); }
NI void c_pair4(const float* x, float y1, float y2, float* o1, float* o2) { powf_pairN_<4>(x, y1, y2, o1, o2); }
NI void u_pair4(const float* x, float y1, float y2, float* o1, float* o2, unsigned& s) { powf_pairN_u_<4>(x, y1, y2, o1, o2, s); }
NI void c_cb8(const float* b, const double* l, const float* y, float* o) { nmp_powf_constbaseN<8>(b, l, y, o); }
NI void u_cb8(const double* l, const float* y, float* o, unsigned& s) { powf_constbaseN_u_<8>(l, y, o, s); }
NI float c_zero_base(float x) { return nmp_powf_zero_base(x, 0.667f); }
NI bool p_exp(float x) { return expf_is_special_(x); }
NI bool p_log(uint32_t ix) { return logf_is_special_(ix); }
NI bool p_pow(uint32_t ix, uint32_t iy, float y) { return powf_is_special_(ix, iy) || powf_range_special_((double)y * powf_log2_inline(ix)); }
// the wrappers the optimistic regions call (Libm<false>) and their checked twins (Libm<true>)
NI void c_quarter2(float a, float b, float& r1, float& r2) { Libm<true> m; m.pow_quarter2(a, b, r1, r2); }
NI void u_quarter2(float a, float b, float& r1, float& r2, unsigned& s) { Libm<false> m; m.pow_quarter2(a, b, r1, r2); s |= m.suspect; }
NI float c_half(float x) { Libm<true> m; return m.pow_half(x); }
NI float u_half(float x, unsigned& s) { Libm<false> m; const float r = m.pow_half(x); s |= m.suspect; return r; }
NI float c_negq(float x) { Libm<true> m; return m.pow_neg_quarter(x); }
NI float u_negq(float x, unsigned& s) { Libm<false> m; const float r = m.pow_neg_quarter(x); s |= m.suspect; return r; }

// failures of one form: their number and the smallest failing key (a bit pattern, or the index of a sample)
struct Fail { unsigned long long n; unsigned int first; unsigned int pad; };
__device__ static inline void note(Fail* f, uint32_t key) { atomicAdd(&f->n, 1ull); atomicMin(&f->first, key); }

// ---- 1a: unchecked against checked, and the exactness of `suspect` (the properties of libm_unchecked_check.hip)
// one argument (what 0: expf, 1: logf) in the scalar form and at position pos of a batch of four
__device__ static bool check_explog(int what, uint32_t bits, int pos) {
  const float x = asfloat(bits);
  bool ok = true;
  unsigned sus = 0, susN = 0;
  float xs[4], ou[4], oc[4];
  for (int n = 0; n < 4; n++) xs[n] = (n == pos) ? x : (what == 0 ? companion(bits, n) - 2.0f : companion(bits, n));
  if (what == 0) {
    const float u = u_expf(x, sus);
    ok = ok && (sus != 0) == p_exp(x);
    if (!sus) ok = ok && same(u, c_expf(x));
    u_expf4(xs, ou, susN); c_expf4(xs, oc);
  } else {
    const float u = u_logf(x, sus);
    ok = ok && (sus != 0) == p_log(bits);
    if (!sus) ok = ok && same(u, c_logf(x));
    u_logf4(xs, ou, susN); c_logf4(xs, oc);
  }
  ok = ok && (susN != 0) == (sus != 0);
  if (!susN) for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]);
  return ok;
}
// TDFCND's form: the exponent under test at position pos of a batch of eight
__device__ static bool check_constbase(uint32_t ybits, int pos) {
  float b[8], y[8], ou[8], oc[8]; double l[8];
  bool ok = true, expect = false;
  for (int n = 0; n < 8; n++) {
    b[n] = (n & 1) ? 0.57f : TKICE;
    l[n] = (n & 1) ? NMP_LOG2K(0.57f) : NMP_LOG2K(TKICE);
    y[n] = cb_y(ybits, pos, n, 0);
    expect = expect || powf_infnan(asuint(y[n])) || powf_range_special_((double)y[n] * l[n]);
  }
  unsigned sus = 0;
  u_cb8(l, y, ou, sus); c_cb8(b, l, y, oc);
  ok = ok && (sus != 0) == expect;
  if (!sus) for (int n = 0; n < 8; n++) ok = ok && same(ou[n], oc[n]);
  return ok;
}
// Four consecutive bases x0..x0+3 to both exponents through every form: the scalar form per base and exponent (with the exactness of
// `suspect`), the four as one pair batch, as batches of four and of two per exponent.  A batch that raised `suspect` is not compared:
// its elements are covered by the scalar form; a batch that holds a suspect element must have raised it.
__device__ static bool check_pow_block(uint32_t x0, uint32_t ybits, uint32_t y2bits) {
  const float y = asfloat(ybits), y2 = asfloat(y2bits);
  float xs[4], ou[4], oc[4], ou2[4], oc2[4];
  bool ok = true;
  unsigned any[2] = {0, 0}, el[2][4];
  for (int n = 0; n < 4; n++) {
    const uint32_t xb = x0 + (uint32_t)n;
    xs[n] = asfloat(xb);
    for (int e = 0; e < 2; e++) {
      const float yy = e ? y2 : y;
      unsigned sus = 0;
      const float u = u_powf(xs[n], yy, sus);
      ok = ok && (sus != 0) == p_pow(xb, e ? y2bits : ybits, yy);
      if (!sus) ok = ok && same(u, c_powf(xs[n], yy));
      el[e][n] = sus; any[e] |= sus;
    }
  }
  {
    unsigned sp = 0;
    u_pair4(xs, y, y2, ou, ou2, sp);
    ok = ok && (sp != 0 || !(any[0] | any[1]));
    if (!sp) { c_pair4(xs, y, y2, oc, oc2); for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]) && same(ou2[n], oc2[n]); }
  }
  for (int e = 0; e < 2; e++) {
    const float yy = e ? y2 : y;
    const float ys[4] = {yy, yy, yy, yy};
    unsigned s4 = 0;
    u_powf4(xs, ys, ou, s4);
    ok = ok && (s4 != 0 || !any[e]);
    if (!s4) { c_powf4(xs, ys, oc); for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]); }
    for (int h = 0; h < 4; h += 2) {
      unsigned s2 = 0;
      u_powf2(xs + h, ys, ou, s2);
      ok = ok && (s2 != 0 || !(el[e][h] | el[e][h + 1]));
      if (!s2) { c_powf2(xs + h, ys, oc); ok = ok && same(ou[0], oc[0]) && same(ou[1], oc[1]); }
    }
  }
  return ok;
}
// Libm<false>'s pow_quarter2 (the base at both positions), pow_half and pow_neg_quarter against Libm<true>'s
__device__ static bool check_wrappers(uint32_t bits) {
  const float x = asfloat(bits), c = companion(bits, 0);
  bool ok = true;
  const bool sq = p_pow(bits, asuint(0.25f), 0.25f);
  for (int p = 0; p < 2; p++) {
    unsigned s = 0;
    float u1, u2, c1, c2;
    u_quarter2(p ? c : x, p ? x : c, u1, u2, s);
    ok = ok && (s != 0) == sq;                     // the companion is never suspect
    if (!s) { c_quarter2(p ? c : x, p ? x : c, c1, c2); ok = ok && same(u1, c1) && same(u2, c2); }
  }
  unsigned sh = 0, sn = 0;
  const float uh = u_half(x, sh), un = u_negq(x, sn);
  ok = ok && (sh != 0) == p_pow(bits, asuint(0.5f), 0.5f) && (sn != 0) == p_pow(bits, asuint(-0.25f), -0.25f);
  if (!sh) ok = ok && same(uh, c_half(x));
  if (!sn) ok = ok && same(un, c_negq(x));
  return ok;
}

// what: 0 expf, 1 logf (every batch position), 2 powf family (item i = the four bases lo + 4 i stride ..+3), 3 constant-base form (every
// batch position), 4 Libm<false>'s wrappers.  Item i of 0, 1, 3, 4 is the pattern lo + i stride.
constexpr int kPer = 16;
__global__ void __launch_bounds__(256) sweep_kernel(int what, uint32_t lo, unsigned long long count, uint32_t stride, uint32_t ybits,
                                                    uint32_t y2bits, Fail* f) {
  libm_stage_tables();
  for (int j = 0; j < kPer; j++) {
    const unsigned long long i = ((unsigned long long)blockIdx.x * kPer + j) * 256 + threadIdx.x;
    if (i >= count) return;
    const uint32_t bits = lo + (uint32_t)i * stride * (what == 2 ? 4u : 1u);
    bool ok = true;
    if (what <= 1) { for (int pos = 0; pos < 4; pos++) ok = check_explog(what, bits, pos) && ok; }
    else if (what == 2) ok = check_pow_block(bits, ybits, y2bits);
    else if (what == 3) { for (int pos = 0; pos < 8; pos++) ok = check_constbase(bits, pos) && ok; }
    else ok = check_wrappers(bits);
    if (!ok) note(f, bits);
  }
}

// ---- 1b: every form against the host's libm.  The host half evaluates ::powf / ::expf / ::logf, the device compares its own results
// with them (values from memory: nothing to fold) and counts per form; the key of a failure is the index of its sample.
enum { P_POWF, P_POWF2, P_POWF4, P_PAIR4, P_POWF_U, P_POWF2_U, P_POWF4_U, P_PAIR4_U, P_NFORM };
__global__ void __launch_bounds__(256) pow_vs_host_kernel(const uint32_t* __restrict__ xb, const uint32_t* __restrict__ yb,
                                                          const uint32_t* __restrict__ y2b, const float* __restrict__ e1,
                                                          const float* __restrict__ e2, long n, int allpos, Fail* f) {
  libm_stage_tables();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t xbits = xb[i];
  const float x = asfloat(xbits), ys2[2] = {asfloat(yb[i]), asfloat(y2b[i])}, ex[2] = {e1[i], e2[i]};
  for (int e = 0; e < 2; e++) {
    const float y = ys2[e];
    unsigned s = 0;
    if (!same(c_powf(x, y), ex[e])) note(f + P_POWF, (uint32_t)i);
    const float u = u_powf(x, y, s);
    if (!s && !same(u, ex[e])) note(f + P_POWF_U, (uint32_t)i);
  }
  for (int pos = allpos ? 0 : (int)(i & 3); pos < (allpos ? 4 : (int)(i & 3) + 1); pos++) {
    float xs[4], ys[4], o[4], o2[4];
    for (int q = 0; q < 4; q++) xs[q] = q == pos ? x : companion(xbits, q);
    for (int e = 0; e < 2; e++) {
      for (int q = 0; q < 4; q++) ys[q] = ys2[e];
      unsigned s = 0;
      c_powf4(xs, ys, o);
      if (!same(o[pos], ex[e])) note(f + P_POWF4, (uint32_t)i);
      u_powf4(xs, ys, o, s);
      if (!s && !same(o[pos], ex[e])) note(f + P_POWF4_U, (uint32_t)i);
      const float x2[2] = {pos & 1 ? companion(xbits, 0) : x, pos & 1 ? x : companion(xbits, 0)};
      s = 0;
      c_powf2(x2, ys, o);
      if (!same(o[pos & 1], ex[e])) note(f + P_POWF2, (uint32_t)i);
      u_powf2(x2, ys, o, s);
      if (!s && !same(o[pos & 1], ex[e])) note(f + P_POWF2_U, (uint32_t)i);
    }
    unsigned s = 0;
    c_pair4(xs, ys2[0], ys2[1], o, o2);
    if (!same(o[pos], ex[0]) || !same(o2[pos], ex[1])) note(f + P_PAIR4, (uint32_t)i);
    u_pair4(xs, ys2[0], ys2[1], o, o2, s);
    if (!s && (!same(o[pos], ex[0]) || !same(o2[pos], ex[1]))) note(f + P_PAIR4_U, (uint32_t)i);
  }
}

enum { E_EXPF, E_EXPF4, E_LOGF, E_LOGF4, E_EXPF_U, E_EXPF4_U, E_LOGF_U, E_LOGF4_U, E_NFORM };
__global__ void __launch_bounds__(256) explog_vs_host_kernel(const uint32_t* __restrict__ xb, const float* __restrict__ ee,
                                                             const float* __restrict__ el, long n, int allpos, Fail* f) {
  libm_stage_tables();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t bits = xb[i];
  const float x = asfloat(bits);
  unsigned s = 0;
  if (!same(c_expf(x), ee[i])) note(f + E_EXPF, (uint32_t)i);
  if (!same(c_logf(x), el[i])) note(f + E_LOGF, (uint32_t)i);
  float u = u_expf(x, s);
  if (!s && !same(u, ee[i])) note(f + E_EXPF_U, (uint32_t)i);
  s = 0;
  u = u_logf(x, s);
  if (!s && !same(u, el[i])) note(f + E_LOGF_U, (uint32_t)i);
  for (int pos = allpos ? 0 : (int)(i & 3); pos < (allpos ? 4 : (int)(i & 3) + 1); pos++) {
    float xs[4], o[4];
    for (int q = 0; q < 4; q++) xs[q] = q == pos ? x : companion(bits, q) - 2.0f;
    c_expf4(xs, o);
    if (!same(o[pos], ee[i])) note(f + E_EXPF4, (uint32_t)i);
    s = 0;
    u_expf4(xs, o, s);
    if (!s && !same(o[pos], ee[i])) note(f + E_EXPF4_U, (uint32_t)i);
    for (int q = 0; q < 4; q++) xs[q] = q == pos ? x : companion(bits, q);
    c_logf4(xs, o);
    if (!same(o[pos], el[i])) note(f + E_LOGF4, (uint32_t)i);
    s = 0;
    u_logf4(xs, o, s);
    if (!s && !same(o[pos], el[i])) note(f + E_LOGF4_U, (uint32_t)i);
  }
}

// the two rare sites (rare_sites_check.hip): TDFCND's batch with y = +-0 among it, checked and unchecked, and CANWATER's zero base
enum { R_CONSTBASE, R_CONSTBASE_U, R_ZERO_BASE, R_NFORM };
__global__ void __launch_bounds__(256) rare_vs_host_kernel(const uint32_t* __restrict__ yb, const uint8_t* __restrict__ posb,
                                                           const float* __restrict__ e8, const float* __restrict__ ez, long n, Fail* f) {
  libm_stage_tables();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t bits = yb[i];
  float b[8], y[8], o[8]; double l[8];
  for (int q = 0; q < 8; q++) {
    b[q] = (q & 1) ? 0.57f : TKICE;
    l[q] = (q & 1) ? NMP_LOG2K(0.57f) : NMP_LOG2K(TKICE);
    y[q] = cb_y(bits, posb[i], q, 1);
  }
  bool ok = true;
  c_cb8(b, l, y, o);
  for (int q = 0; q < 8; q++) ok = ok && same(o[q], e8[8 * i + q]);
  if (!ok) note(f + R_CONSTBASE, (uint32_t)i);
  unsigned s = 0;
  ok = true;
  u_cb8(l, y, o, s);
  if (!s) for (int q = 0; q < 8; q++) ok = ok && same(o[q], e8[8 * i + q]);
  if (!ok) note(f + R_CONSTBASE_U, (uint32_t)i);
  if (!same(c_zero_base(asfloat(bits)), ez[i])) note(f + R_ZERO_BASE, (uint32_t)i);
}

// the three tables as the routines read them after libm_stage_tables() (the LDS copies in the default build)
__global__ void __launch_bounds__(256) tables_kernel(uint64_t* out) {
  libm_stage_tables();
  const int t = threadIdx.x;
  if (t < 32) {
    out[t] = NMP_T_EXP2F[t];
    out[32 + t] = asuint64(NMP_T_LOGF[t]);
    out[64 + t] = asuint64(NMP_T_POWLOG2[t]);
  }
}

// ---- host half
namespace {
struct DevBuf {                                   // device memory of one call, released on every way out
  std::vector<void*> p;
  ~DevBuf() { for (void* q : p) hipFree(q); }
  template <class T> T* up(const T* h, size_t n) {
    void* d = nullptr;
    if (hipMalloc(&d, n * sizeof(T) + 16) != hipSuccess) return nullptr;
    p.push_back(d);
    if (h && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return (T*)d;
  }
};
Fail* fresh_fails(DevBuf& m, int nform) {
  std::vector<Fail> f(nform);
  for (auto& x : f) { x.n = 0; x.first = 0xffffffffu; x.pad = 0; }
  return m.up(f.data(), (size_t)nform);
}
long fetch_fails(const Fail* d, int nform, long* counts, uint32_t* first) {
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
  std::vector<Fail> f(nform);
  if (hipMemcpy(f.data(), d, nform * sizeof(Fail), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  long total = 0;
  for (int i = 0; i < nform; i++) { counts[i] = (long)f[i].n; first[i] = f[i].first; total += (long)f[i].n; }
  return total;
}
template <class F> void parallel_for(long n, int nthreads, F fn) {
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; t++) th.emplace_back([=]() { for (long i = n * t / nthreads; i < n * (t + 1) / nthreads; i++) fn(i); });
  for (auto& x : th) x.join();
}
}  // namespace

// failing items of the sweep (what as sweep_kernel), *first_bad = the smallest failing pattern; -1 on a HIP error
extern "C" long libm_dev_sweep(int what, uint32_t lo, unsigned long long count, uint32_t stride, uint32_t ybits, uint32_t y2bits,
                               uint32_t* first_bad) {
  DevBuf m;
  Fail* f = fresh_fails(m, 1);
  if (!f) return -1;
  const unsigned long long per_block = 256ull * kPer, nb = (count + per_block - 1) / per_block;
  if (nb == 0 || nb > 0x7fffffffull) return -1;
  hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)nb), dim3(256), 0, 0, what, lo, count, stride, ybits, y2bits, f);
  long c = 0;
  return fetch_fails(f, 1, &c, first_bad);
}

// n samples (x, y, y2): every powf form on the device against ::powf.  counts / first: P_NFORM entries (first = sample index)
extern "C" long libm_dev_pow_vs_host(const uint32_t* xb, const uint32_t* yb, const uint32_t* y2b, long n, int allpos, int nthreads,
                                     long* counts, uint32_t* first) {
  std::vector<float> e1(n), e2(n);
  parallel_for(n, nthreads, [&](long i) { e1[i] = ::powf(asfloat(xb[i]), asfloat(yb[i])); e2[i] = ::powf(asfloat(xb[i]), asfloat(y2b[i])); });
  DevBuf m;
  Fail* f = fresh_fails(m, P_NFORM);
  const uint32_t *dx = m.up(xb, n), *dy = m.up(yb, n), *dy2 = m.up(y2b, n);
  const float *d1 = m.up(e1.data(), n), *d2 = m.up(e2.data(), n);
  if (!f || !dx || !dy || !dy2 || !d1 || !d2) return -1;
  hipLaunchKernelGGL(pow_vs_host_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, dy2, d1, d2, n, allpos, f);
  return fetch_fails(f, P_NFORM, counts, first);
}

// n arguments: every expf / logf form on the device against ::expf / ::logf.  pin: npin pairs (x bits, result bits) that stand for
// ::expf at those arguments (the pinned build's results where glibc's two builds differ, tests/test_libm.py).  E_NFORM entries.
extern "C" long libm_dev_explog_vs_host(const uint32_t* xb, long n, int allpos, int nthreads, const uint32_t* pin, int npin,
                                        long* counts, uint32_t* first) {
  std::vector<float> ee(n), el(n);
  parallel_for(n, nthreads, [&](long i) {
    ee[i] = ::expf(asfloat(xb[i])); el[i] = ::logf(asfloat(xb[i]));
    for (int q = 0; q < npin; q++) if (xb[i] == pin[2 * q]) ee[i] = asfloat(pin[2 * q + 1]);
  });
  DevBuf m;
  Fail* f = fresh_fails(m, E_NFORM);
  const uint32_t* dx = m.up(xb, n);
  const float *de = m.up(ee.data(), n), *dl = m.up(el.data(), n);
  if (!f || !dx || !de || !dl) return -1;
  hipLaunchKernelGGL(explog_vs_host_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, de, dl, n, allpos, f);
  return fetch_fails(f, E_NFORM, counts, first);
}

// n samples (exponent bits, batch position): the rare-site forms against ::powf.  R_NFORM entries.
extern "C" long libm_dev_rare_vs_host(const uint32_t* yb, const uint8_t* pos, long n, int nthreads, long* counts, uint32_t* first) {
  std::vector<float> e8(8 * n), ez(n);
  parallel_for(n, nthreads, [&](long i) {
    for (int q = 0; q < 8; q++) e8[8 * i + q] = ::powf((q & 1) ? 0.57f : TKICE, cb_y(yb[i], pos[i], q, 1));
    ez[i] = ::powf(asfloat(yb[i]), 0.667f);
  });
  DevBuf m;
  Fail* f = fresh_fails(m, R_NFORM);
  const uint32_t* dy = m.up(yb, n);
  const uint8_t* dp = m.up(pos, n);
  const float *d8 = m.up(e8.data(), 8 * n), *dz = m.up(ez.data(), n);
  if (!f || !dy || !dp || !d8 || !dz) return -1;
  hipLaunchKernelGGL(rare_vs_host_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dy, dp, d8, dz, n, f);
  return fetch_fails(f, R_NFORM, counts, first);
}

// the 96 table words the device routines read, and the committed constants they must be
extern "C" long libm_dev_tables(uint64_t* staged, uint64_t* committed) {
  for (int t = 0; t < 32; t++) { committed[t] = kExp2fTab[t]; committed[32 + t] = asuint64(kLogfTab[t]); committed[64 + t] = asuint64(kPowfLog2Tab[t]); }
  DevBuf m;
  uint64_t* d = m.up((const uint64_t*)nullptr, 96);
  if (!d) return -1;
  hipLaunchKernelGGL(tables_kernel, dim3(1), dim3(256), 0, 0, d);
  if (hipGetLastError() != hipSuccess || hipMemcpy(staged, d, 96 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return 0;
}
extern "C" double libm_dev_log2(uint32_t xbits) { return powf_log2_inline(xbits); }
extern "C" double libm_dev_log2base(int which) { return which ? NMP_LOG2K(0.57f) : NMP_LOG2K(TKICE); }
