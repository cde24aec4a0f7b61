// TEST INFRASTRUCTURE -- the two call sites whose "rare" libm arguments are in fact the common case of a run (TDFCND's
// BASE ** 0, CANWATER's 0 ** 0.667): the forms that keep those arguments out of powf's cold blocks, against the live libm of
// this machine, bit for bit.  Host compilation of the device source.  Never shipped.
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

// what: 0 = powf_constbaseN_<8> as TDFCND calls it (bases TKICE, 0.57 alternating, log2 from NMP_LOG2K), the exponent under test at
// every position of the batch in turn, the other positions holding exponents derived from its bits; 1 = nmp_powf_zero_base(x, 0.667f).
// Walks the bit patterns stride, 2 stride, ... of the whole 2^32 space plus every pattern of `extra`.
static long sweep(int what, uint32_t stride, int nthreads, const uint32_t* extra, int nextra, uint32_t* first_bad) {
  std::vector<long> bad(nthreads, 0);
  std::vector<uint32_t> fb(nthreads, 0);
  std::vector<std::thread> th;
  auto one = [&](int t, uint32_t bits, int pos) {
    bool ok = true;
    if (what == 0) {
      float b[8], y[8], o[8]; double l[8];
      for (int n = 0; n < 8; n++) {
        b[n] = (n & 1) ? 0.57f : TKICE;
        l[n] = (n & 1) ? NMP_LOG2K(0.57f) : NMP_LOG2K(TKICE);
        const int q = (n - pos) & 7;
        y[n] = asfloat(q == 0 ? bits : (q == 1 ? bits ^ 0x80000000u : (q == 2 ? 0u : (q == 3 ? 0x80000000u : bits * 2654435761u * (uint32_t)q))));
      }
      nmp_powf_constbaseN<8>(b, l, y, o);
      for (int n = 0; n < 8; n++) ok = ok && same(o[n], ::powf(b[n], y[n]));
    } else {
      const float x = asfloat(bits);
      ok = same(nmp_powf_zero_base(x, 0.667f), ::powf(x, 0.667f));
    }
    if (!ok) { if (!bad[t]) fb[t] = bits; bad[t]++; }
  };
  for (int t = 0; t < nthreads; t++)
    th.emplace_back([&, t]() {
      const uint64_t lo = (uint64_t)t * (1ull << 32) / nthreads, hi = (uint64_t)(t + 1) * (1ull << 32) / nthreads;
      for (uint64_t u = lo + (stride - lo % stride) % stride; u < hi; u += stride) one(t, (uint32_t)u, (int)(u / stride % 8));
      if (t == 0)
        for (int e = 0; e < nextra; e++)
          for (int pos = 0; pos < (what == 0 ? 8 : 1); pos++) one(t, extra[e], pos);     // the batch position means something to form 0 only
    });
  for (auto& x : th) x.join();
  long n = 0;
  for (int t = 0; t < nthreads; t++) { if (bad[t] && !n) *first_bad = fb[t]; n += bad[t]; }
  return n;
}

extern "C" long rare_sites_check(int what, uint32_t stride, int nthreads, const uint32_t* extra, int nextra, uint32_t* first_bad) {
  return sweep(what, stride, nthreads, extra, nextra, first_bad);
}
// |y log2 BASE| of the two TDFCND bases, for the test to place exponents on both sides of the range ends
extern "C" double rare_sites_log2base(int which) { return which ? NMP_LOG2K(0.57f) : NMP_LOG2K(TKICE); }
