// The scalar rules of csrc/fold.hip, executed on the host: the float64 BatchNorm scale / folded weight / bias, the row-scale exponent
// taken from the bits of the row maximum, the hi / lo half split and the packed index of both layouts are plain scalar C++ behind
// `__device__`.  tests/test_fold_host.py cuts their text out of fold.hip into fold_cut.inc; with `__device__` mapped to host functions
// the SAME TEXT is compiled for x86 and held bit for bit to `_fold`, `_row_scales`, `_h8l8`, `_h4l4` and `pack_weight_khwc` of
// ssg_amd/resnet.py.  Test infrastructure: nothing here is linked into the product.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#undef __device__
#undef __forceinline__
#define __device__
#define __forceinline__ inline
static inline long long hx_double_as_longlong(double x) { long long r; memcpy(&r, &x, 8); return r; }
#define __double_as_longlong hx_double_as_longlong          // ssg_common.h's d2h
#include "../../self-similarity-grouping_amd/csrc/ssg_common.h"
namespace ssg {
#include "fold_cut.inc"
}
using namespace ssg;

extern "C" {
// per channel: scale (float64), bias (float32)
void hx_fold_channel(const float* gamma, const float* beta, const float* mean, const float* var, double eps, long n, double* scale, float* bias) {
  for (long i = 0; i < n; i++) {
    scale[i] = fold_scale(gamma[i], var[i], eps);
    bias[i] = fold_bias(beta[i], mean[i], scale[i]);
  }
}
// w [rows][k] with one scale per row -> w' float32
void hx_fold_weight(const float* w, const double* scale, long rows, long k, float* out) {
  for (long r = 0; r < rows; r++)
    for (long i = 0; i < k; i++) out[r * k + i] = fold_weight(w[r * k + i], scale[r]);
}
// row maxima (float32, not negative) -> exponent e, 2^e and 2^-e
void hx_fold_row_scale(const float* mx, long n, int* e, float* sc, float* inv) {
  for (long i = 0; i < n; i++) {
    uint32_t b;
    memcpy(&b, &mx[i], 4);
    e[i] = fold_row_exponent(b & 0x7fffffffu);
    sc[i] = fold_pow2(e[i]);
    inv[i] = fold_pow2(-e[i]);
  }
}
void hx_fold_split(const float* w, const float* sc, long rows, long k, uint16_t* hi, uint16_t* lo) {
  for (long r = 0; r < rows; r++)
    for (long i = 0; i < k; i++) fold_split(w[r * k + i], sc[r], hi[r * k + i], lo[r * k + i]);
}
// index[c][tap] of one row: the Cin % 32 == 0 order, or the stem's (cin == 3)
void hx_fold_index(int cin, int taps, int* out) {
  for (int c = 0; c < cin; c++)
    for (int t = 0; t < taps; t++) out[c * taps + t] = cin == 3 ? fold_stem_index(c, t) : fold_packed_index(c, t, taps);
}
}
