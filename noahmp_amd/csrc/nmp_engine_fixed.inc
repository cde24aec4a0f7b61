// Option-specialised column kernels: this file is the body of a translation unit that defines NMP_FIXED_DVEG and NMP_FIXED_RUN first.
// The physics headers are compiled once more with `struct Opt` made of compile-time constants -- the values of the reference's
// namelist (run/namelist.hrldas: CRS 1, BTR 1, SFC 1, FRZ 1, INF 1, RAD 3, ALB 2, SNF 1, TBOT 2, STC 1; DVEG and RUN per unit) -- so that the
// code of every other OPT_* alternative is not in the kernel: the land-only kernel then needs 2 spilled registers instead of
// 136 and runs ~20 % faster.  Same source, same arithmetic, same results (tests compare the two kernels bit for bit); the host
// (noahmp_engine.hip, fixed_level) uses it only for calls whose twelve options have exactly these values.
// The namespace of the physics is renamed for this unit so that its host-side inline functions are distinct symbols.
#define NMP_CAT2(a, b) a##b
#define NMP_CAT(a, b) NMP_CAT2(a, b)
#define NMP_FIXED_TAG NMP_CAT(NMP_CAT(d, NMP_FIXED_DVEG), NMP_CAT(_r, NMP_FIXED_RUN))
#define nmp NMP_CAT(nmp_fixed_, NMP_FIXED_TAG)
#include "nmp_kernel.hpp"

namespace nmp_host {

static void NMP_CAT(fill_fixed_, NMP_FIXED_TAG)(KArgs& k, const LaunchDesc& d) {
  memset(&k, 0, sizeof(k));
  k.a = d.a;
  k.c.T = d.tables; k.c.D = derived_of(d.tables); k.c.dt = d.dt; k.c.isurban = d.isurban;
  k.c.ts = tab_scalars_unpack(d.ts_i, d.ts_f);
  for (int l = 0; l < NL; l++) k.c.zsoil[l] = d.zsoil[l];
  ctx_fill_uniform(k.c);
  k.ni = d.ni; k.nka = d.nka; k.nti = d.nti; k.ntj = d.ntj; k.k1 = d.k1; k.kp_lo = d.kp_lo; k.kp_hi = d.kp_hi; k.yearlen = d.yearlen;
  k.c.cost = d.cost; k.c.force_checked = d.force_checked;
  k.r_land = d.r_land; k.r_ice = d.r_ice; k.r_skip = d.r_skip;
  k.err = d.err; k.counts = d.counts; k.err_base = d.err_base; k.t_offset = d.t_offset; k.t_first = d.t_first; k.t_count = d.t_count;
}

#ifdef NMP_FIXED_EXPORT_PACK
// the kernel-argument block of ANY option-constant compilation of the kernel (Opt has no data members there, so the layout does
// not depend on the option values): used to launch kernels compiled at run time (noahmp_jit.hip)
size_t pack_fixed_kargs(const LaunchDesc& d, void* buf, size_t cap) {
  if (cap < sizeof(KArgs)) return 0;
  NMP_CAT(fill_fixed_, NMP_FIXED_TAG)(*reinterpret_cast<KArgs*>(buf), d);
  return sizeof(KArgs);
}
#endif

// mode 0: the tile as it is; 4: the three class ranges of a sorted layout in one launch (noahmp_ranges_kernel).  ev0 / ev1 (may be NULL): the
// kernel's own start / stop time, attached to the dispatch itself (hipExtLaunchKernel) -- no event packet stands between two kernels.
void NMP_CAT(launch_fixed_, NMP_FIXED_TAG)(const LaunchDesc& d, int mode, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  KArgs k;
  NMP_CAT(fill_fixed_, NMP_FIXED_TAG)(k, d);
  // workgroup size (nmp_kernel.hpp: NMP_FIXED_BLOCK) / layer-array storage of the specialised kernels: build-time knobs
#ifndef NMP_FIXED_USE_LDS
#define NMP_FIXED_USE_LDS true
#endif
  constexpr long B = NMP_FIXED_BLOCK;
  if (mode == 4) {
    const long nb = (k.r_ice + B - 1) / B + (k.r_land + B - 1) / B + (k.r_skip + B - 1) / B;
    if (nb <= 0) return;
    hipExtLaunchKernelGGL((noahmp_ranges_kernel<NMP_FIXED_BLOCK>), dim3((unsigned)nb), dim3(NMP_FIXED_BLOCK), 0, s, ev0, ev1, 0, k);
    return;
  }
  const long n = (long)k.nti * k.ntj;
  if (n <= 0) return;
  hipExtLaunchKernelGGL((noahmp_column_kernel<NMP_FIXED_BLOCK, NMP_FIXED_USE_LDS, 0>), dim3((unsigned)((n + B - 1) / B)), dim3(NMP_FIXED_BLOCK), 0, s, ev0, ev1, 0, k);
}

#ifdef NMP_PHASE_TIMERS
// profiling build only: add this unit's phase tick counters (its own copy of g_nmp_prof) to acc[0..n) and clear them
void NMP_CAT(prof_fixed_, NMP_FIXED_TAG)(unsigned long long* acc, int n) {
  std::vector<unsigned long long> h(nmp::NMP_NPHASE * 256);
  if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(nmp::g_nmp_prof), h.size() * 8) != hipSuccess) return;
  for (int p = 0; p < n && p < nmp::NMP_NPHASE; p++)
    for (int s2 = 0; s2 < 256; s2++) acc[p] += h[p * 256 + s2];
  std::fill(h.begin(), h.end(), 0ull);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(nmp::g_nmp_prof), h.data(), h.size() * 8);
}
#endif

}  // namespace nmp_host
