// TEST INFRASTRUCTURE: the per-cell and per-group functions of the budget-preserving regrid (noahmp_amd/csrc/nmp_dev_regrid_conserve.hpp)
// compiled for the host and composed as the kernels compose them.  tests/test_regrid_conserve.py builds this file on demand
// (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "nmp_dev_regrid_conserve.hpp"
#include "nmp_dev_regions.hpp"

namespace {

// S of include/noahmp_hip.h with the library's own node (reg_combine): chunks of 256, folded h = 128 .. 1, again on the partials
double tree_sum(std::vector<double> t) {
  if (t.empty()) return 0.0;
  for (;;) {
    std::vector<double> part;
    for (size_t s = 0; s < t.size(); s += 256) {
      double v[256];
      for (int i = 0; i < 256; i++) v[i] = s + i < t.size() ? t[s + i] : 0.0;
      for (int h = 128; h > 0; h >>= 1)
        for (int i = 0; i < h; i++) v[i] = nmp::reg_combine(NOAHMP_REG_SUM, v[i], v[i + h]);
      part.push_back(v[0]);
    }
    if (part.size() == 1) return part[0];
    t.swap(part);
  }
}

}  // namespace

extern "C" {

// group[c] <- the owner of window cell c or -1
void conserve_groups(const int32_t* plan, long ncell, const noahmp_regrid_source* g, int32_t* group) {
  const int nxny = g->nx * g->ny;
  for (long c = 0; c < ncell; c++) {
    float w[4];
    int idx[4];
    for (int q = 0; q < 4; q++) memcpy(&w[q], &plan[(2 + q) * ncell + c], 4);
    group[c] = nmp::rc_group(plan[c], plan[ncell + c], w, g->nx, nxny, g->periodic_x ? 1 : 0, idx);
  }
}

// One entry over a window: out[c] for every cell (non-members: fill), nsum[s] = N_s for the groups that have members (others untouched),
// dsum[s] likewise.  area / pattern may be NULL.  `reads` (may be NULL) counts the corner reads of each source cell in ONE pass of v.
// Returns the number of members whose area is not finite and > 0.
long conserve_run(const int32_t* plan, long ncell, const noahmp_regrid_source* g, const float* src, const float* area, const float* pattern,
                  float fill, float* out, double* nsum, double* dsum, int32_t* reads) {
  const int nxny = g->nx * g->ny;
  std::vector<int> group(ncell);
  std::vector<float> v(ncell, 0.f);
  conserve_groups(plan, ncell, g, group.data());
  std::vector<std::vector<double>> tn(nxny), td(nxny);
  long bad = 0;
  for (long c = 0; c < ncell; c++) {
    if (group[c] < 0) continue;
    float w[4], s[4] = {0.f, 0.f, 0.f, 0.f};
    int idx[4];
    for (int q = 0; q < 4; q++) memcpy(&w[q], &plan[(2 + q) * ncell + c], 4);
    nmp::regrid_corners(plan[c], w, g->nx, nxny, g->periodic_x ? 1 : 0, idx);
    for (int q = 0; q < 4; q++)
      if (w[q] != 0.f) { s[q] = src[idx[q]]; if (reads) reads[idx[q]]++; }
    v[c] = nmp::rc_value(nmp::regrid_bilinear(w, s), pattern != nullptr, pattern ? pattern[c] : 1.f);
    const float a = area ? area[c] : 1.f;
    if (!nmp::rc_area_ok(a)) bad++;
    tn[group[c]].push_back(nmp::rc_term(a, v[c]));
    td[group[c]].push_back(nmp::rc_term(a, 1.f));
  }
  std::vector<float> val(nxny, 0.f);
  std::vector<int> kind(nxny, 0);
  for (int s = 0; s < nxny; s++) {
    if (tn[s].empty()) continue;
    const double N = tree_sum(tn[s]), D = tree_sum(td[s]);
    nsum[s] = N;
    dsum[s] = D;
    kind[s] = nmp::rc_group_result(src[s], D, N, &val[s]);
  }
  for (long c = 0; c < ncell; c++) out[c] = group[c] < 0 ? fill : nmp::rc_out(kind[group[c]], val[group[c]], v[c]);
  return bad;
}

}  // extern "C"
