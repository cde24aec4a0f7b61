// TEST INFRASTRUCTURE: the per-element functions of the device-side history (noahmp_amd/csrc/nmp_dev_history.hpp) compiled for the host,
// applied to whole arrays.  tests/test_history.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_history.hpp"

extern "C" {

// acc[i] <- one sample x[i]; part (may be NULL): only the elements with part[i] != 0 take the sample
void history_apply(int op, float* acc, const float* x, float scale, const unsigned char* part, long n) {
  for (long i = 0; i < n; i++)
    if (!part || part[i]) acc[i] = nmp::hist_apply(op, acc[i], x[i], scale);
}

void history_takes_part(const float* xland, const float* xice, float xice_thres, unsigned char* out, long n) {
  for (long i = 0; i < n; i++) out[i] = nmp::hist_takes_part(xland[i], xice[i], xice_thres) ? 1 : 0;
}

// dst[i] <- finished acc[i]; acc[i] <- its identity when reset != 0
void history_finish(int op, float* acc, const int32_t* count, int mean, int reset, float fill, float* dst, long n) {
  for (long i = 0; i < n; i++) {
    dst[i] = nmp::hist_finish(acc[i], count[i], mean != 0, fill);
    if (reset) acc[i] = nmp::hist_identity(op, acc[i]);
  }
}

}  // extern "C"
