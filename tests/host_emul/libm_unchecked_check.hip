// TEST INFRASTRUCTURE -- the unchecked libm forms (nmp_libm.hpp: expf_u_, logf_u_, powf_u_ and the batched / pair / constant-base
// forms) against the checked ones: wherever an unchecked form leaves `suspect` 0 its bits are the checked form's (NaN = NaN), and
// `suspect` is raised exactly where the checked form's own test is true.  Host compilation of the device source.  Never shipped.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <thread>
#include <vector>
#include "nmp_dev_common.hpp"

using namespace nmp;
using namespace nmp::libm;

static inline bool same(float a, float b) {
  if (isnan(a) && isnan(b)) return true;
  return asuint(a) == asuint(b);
}
// an ordinary companion argument derived from the bits under test (positive normal, moderate exponent): fills the other slots of a batch
static inline float companion(uint32_t bits, int q) { return asfloat(0x3e000000u + ((bits * 2654435761u * (uint32_t)(q + 1)) >> 7)); }

// The two sides of every comparison are called through functions that are not inlined: inlined into one function the unchecked form and
// the not-taken-branch path of the checked form are the same expressions, and the compiler folds the comparison to true without running it.
#define NI __attribute__((noinline)) static
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
NI void c_cb8(const float* b, const double* l, const float* y, float* o) { powf_constbaseN_<8>(b, l, y, o); }
NI void u_cb8(const double* l, const float* y, float* o, unsigned& s) { powf_constbaseN_u_<8>(l, y, o, s); }
NI bool p_exp(float x) { return expf_is_special_(x); }
NI bool p_log(uint32_t ix) { return logf_is_special_(ix); }
NI bool p_pow(uint32_t ix, uint32_t iy, float y) { return powf_is_special_(ix, iy) || powf_range_special_((double)y * powf_log2_inline(ix)); }

// one argument (what 0: expf, 1: logf) in the scalar form and at position pos of a batch of four
static bool check_explog(int what, uint32_t bits, int pos) {
  const float x = asfloat(bits);
  bool ok = true;
  unsigned sus = 0;
  float xs[4], ou[4], oc[4];
  for (int n = 0; n < 4; n++) xs[n] = (n == pos) ? x : (what == 0 ? companion(bits, n) - 2.0f : companion(bits, n));
  if (what == 0) {
    const float u = u_expf(x, sus);
    ok = ok && (sus != 0) == p_exp(x);
    if (!sus) ok = ok && same(u, c_expf(x));
    unsigned susN = 0;
    u_expf4(xs, ou, susN); c_expf4(xs, oc);
    ok = ok && (susN != 0) == (sus != 0);
    if (!susN) for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]);
  } else {
    const float u = u_logf(x, sus);
    ok = ok && (sus != 0) == p_log(bits);
    if (!sus) ok = ok && same(u, c_logf(x));
    unsigned susN = 0;
    u_logf4(xs, ou, susN); c_logf4(xs, oc);
    ok = ok && (susN != 0) == (sus != 0);
    if (!susN) for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]);
  }
  return ok;
}

// x ** y and x ** y2 in every form the kernels use: powf_u_, powfN_u_<2> (pow_quarter2's form), powfN_u_<4>, powf_pairN_u_<4>
static bool check_pow(uint32_t xbits, uint32_t ybits, uint32_t y2bits, int pos) {
  const float x = asfloat(xbits), y = asfloat(ybits), y2 = asfloat(y2bits);
  bool ok = true;
  unsigned sus = 0;
  const float u = u_powf(x, y, sus);
  ok = ok && (sus != 0) == p_pow(xbits, ybits, y);
  if (!sus) ok = ok && same(u, c_powf(x, y)) && same(u, ::powf(x, y));
  {
    const float xs[2] = {pos & 1 ? companion(xbits, 0) : x, pos & 1 ? x : companion(xbits, 0)}, ys[2] = {y, y};
    float ou[2], oc[2]; unsigned s2 = 0;
    u_powf2(xs, ys, ou, s2); c_powf2(xs, ys, oc);
    if (!s2) ok = ok && same(ou[0], oc[0]) && same(ou[1], oc[1]);
    else ok = ok && (sus != 0 || powf_range_special_((double)y * powf_log2_inline(asuint(companion(xbits, 0)))));
  }
  float xs[4], ys[4], ou[4], oc[4], ou2[4], oc2[4];
  for (int n = 0; n < 4; n++) { xs[n] = (n == (pos & 3)) ? x : companion(xbits, n); ys[n] = (n & 1) ? y2 : y; }
  {
    unsigned s4 = 0;
    u_powf4(xs, ys, ou, s4); c_powf4(xs, ys, oc);
    if (!s4) for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]);
  }
  {
    unsigned sp = 0;
    u_pair4(xs, y, y2, ou, ou2, sp); c_pair4(xs, y, y2, oc, oc2);
    if (!sp) for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]) && same(ou2[n], oc2[n]);
    if (sus) ok = ok && sp != 0;                     // the element under test is in the batch with exponent y
  }
  return ok;
}

// TDFCND's form: compile-time bases TKICE and 0.57, the exponent under test at position pos of a batch of eight
static bool check_constbase(uint32_t ybits, int pos) {
  float b[8], y[8], ou[8], oc[8]; double l[8];
  bool ok = true, expect = false;
  for (int n = 0; n < 8; n++) {
    b[n] = (n & 1) ? 0.57f : TKICE;
    l[n] = (n & 1) ? NMP_LOG2K(0.57f) : NMP_LOG2K(TKICE);
    const int q = (n - pos) & 7;
    y[n] = q == 0 ? asfloat(ybits) : (q == 1 ? 0.f : (q == 2 ? -0.f : companion(ybits, n) - 0.5f));
    expect = expect || powf_infnan(asuint(y[n])) || powf_range_special_((double)y[n] * l[n]);
  }
  unsigned sus = 0;
  u_cb8(l, y, ou, sus); c_cb8(b, l, y, oc);
  ok = ok && (sus != 0) == expect;
  if (!sus) for (int n = 0; n < 8; n++) ok = ok && same(ou[n], oc[n]);
  return ok;
}

// Four consecutive bases x0..x0+3 to both exponents through every form, sized for the exhaustive sweep: the scalar form per base and
// exponent (with the exactness of `suspect`), the four as one pair batch, as batches of four and of two per exponent.  A batch that
// raised `suspect` is not compared (its checked twin is not evaluated): its elements are covered by the scalar form.
static bool check_pow_block(uint32_t x0, uint32_t ybits, uint32_t y2bits) {
  const float y = asfloat(ybits), y2 = asfloat(y2bits);
  float xs[4], ou[4], oc[4], ou2[4], oc2[4];
  bool ok = true;
  for (int n = 0; n < 4; n++) {
    const uint32_t xb = x0 + (uint32_t)n;
    xs[n] = asfloat(xb);
    for (int e = 0; e < 2; e++) {
      const float yy = e ? y2 : y;
      unsigned sus = 0;
      const float u = u_powf(xs[n], yy, sus);
      ok = ok && (sus != 0) == p_pow(xb, e ? y2bits : ybits, yy);
      if (!sus) ok = ok && same(u, c_powf(xs[n], yy));
    }
  }
  {
    unsigned sp = 0;
    u_pair4(xs, y, y2, ou, ou2, sp);
    if (!sp) { c_pair4(xs, y, y2, oc, oc2); for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]) && same(ou2[n], oc2[n]); }
  }
  for (int e = 0; e < 2; e++) {
    const float yy = e ? y2 : y;
    const float ys[4] = {yy, yy, yy, yy};
    unsigned s4 = 0;
    u_powf4(xs, ys, ou, s4);
    if (!s4) { c_powf4(xs, ys, oc); for (int n = 0; n < 4; n++) ok = ok && same(ou[n], oc[n]); }
    for (int h = 0; h < 4; h += 2) {
      unsigned s2 = 0;
      u_powf2(xs + h, ys, ou, s2);
      if (!s2) { c_powf2(xs + h, ys, oc); ok = ok && same(ou[0], oc[0]) && same(ou[1], oc[1]); }
    }
  }
  return ok;
}

// what: 0 expf, 1 logf (argument swept), 2 powf family (base swept, exponents ybits / y2bits), 3 constant-base form (exponent swept).
// Walks the bit patterns 0, stride, 2 stride, ... of the whole 2^32 space; stride 1 is every pattern (the powf family then takes the
// patterns four at a time).
extern "C" long libm_unchecked_sweep(int what, uint32_t stride, int nthreads, uint32_t ybits, uint32_t y2bits, uint32_t* first_bad) {
  std::vector<long> bad(nthreads, 0);
  std::vector<uint32_t> fb(nthreads, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; t++)
    th.emplace_back([&, t]() {
      const uint64_t lo = ((uint64_t)t * (1ull << 32) / nthreads) & ~3ull, hi = ((uint64_t)(t + 1) * (1ull << 32) / nthreads) & ~3ull;
      if (what == 2 && stride == 1) {
        for (uint64_t u = lo; u < hi; u += 4)
          if (!check_pow_block((uint32_t)u, ybits, y2bits)) { if (!bad[t]) fb[t] = (uint32_t)u; bad[t]++; }
        return;
      }
      for (uint64_t u = lo + (stride - lo % stride) % stride; u < hi; u += stride) {
        const uint32_t bits = (uint32_t)u; const int pos = (int)(u / stride % 8);
        const bool ok = what <= 1 ? check_explog(what, bits, pos & 3) : (what == 2 ? check_pow(bits, ybits, y2bits, pos) : check_constbase(bits, pos));
        if (!ok) { if (!bad[t]) fb[t] = bits; bad[t]++; }
      }
    });
  for (auto& x : th) x.join();
  long n = 0;
  for (int t = 0; t < nthreads; t++) { if (bad[t] && !n) *first_bad = fb[t]; n += bad[t]; }
  return n;
}

// the structured set: every x of xs with every y of ys (powf family, at every batch position), every pattern of xs through expf / logf
// and the constant-base form.  Returns the number of failing combinations; first_bad = {x bits, y bits} of the first.
extern "C" long libm_unchecked_pairs(const uint32_t* xs, int nx, const uint32_t* ys, int ny, uint32_t* first_bad) {
  long n = 0;
  auto note = [&](uint32_t a, uint32_t b) { if (!n) { first_bad[0] = a; first_bad[1] = b; } n++; };
  for (int i = 0; i < nx; i++) {
    for (int pos = 0; pos < 4; pos++) {
      if (!check_explog(0, xs[i], pos)) note(xs[i], 0);
      if (!check_explog(1, xs[i], pos)) note(xs[i], 1);
    }
    for (int pos = 0; pos < 8; pos++) if (!check_constbase(xs[i], pos)) note(xs[i], 3);
    for (int j = 0; j < ny; j++)
      for (int pos = 0; pos < 4; pos++)
        if (!check_pow(xs[i], ys[j], ys[(j + 1) % ny], pos)) note(xs[i], ys[j]);
  }
  return n;
}
extern "C" double libm_unchecked_log2(uint32_t xbits) { return powf_log2_inline(xbits); }
