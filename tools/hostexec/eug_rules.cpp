// The scalar rules of csrc/eug.hip, executed on the host: the leaf program of numpy's pairwise sum (eug_build_program), the np.argmin
// order (eug_better) and the np.argsort(-score) key (eug_score_key) are plain scalar C++ behind `__device__`.
// tests/test_eug_range_host.py cuts their text and the EUG_* constants out of eug.hip into eug_cut.inc; with `__device__` mapped to
// host functions and int4 / make_int4 / min / __double_as_longlong given their plain meaning the SAME TEXT is compiled for x86 and
// held to numpy.  Test infrastructure: nothing here is linked into the product.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#define __device__
#define __forceinline__ inline
struct int4 { int x, y, z, w; };
static inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
static inline long long __double_as_longlong(double x) { long long b; std::memcpy(&b, &x, sizeof b); return b; }
using std::min;
namespace ssg {
#include "eug_cut.inc"
}
using namespace ssg;

extern "C" {
// out[0..6] = EUG_TU, EUG_TL, EUG_KW, EUG_MAXD, EUG_CHUNK, EUG_MAXLEAF, EUG_CM_CHUNKS
void hx_eug_constants(int* out) {
  const int c[7] = {EUG_TU, EUG_TL, EUG_KW, EUG_MAXD, EUG_CHUNK, EUG_MAXLEAF, EUG_CM_CHUNKS};
  for (int i = 0; i < 7; i++) out[i] = c[i];
}
// prog = room for d + 1 rows of (start, length, pops, chunk end): a leaf holds at least one column, so no program is longer
int hx_eug_build_program(int d, int* prog) { return eug_build_program(d, reinterpret_cast<int4*>(prog)); }
int hx_eug_better(float v, int i, float m, int j) { return eug_better(v, i, m, j) ? 1 : 0; }
// the arg-min of vals[idx[0]], vals[idx[1]], ... folded in that order from the kernel's start value (+inf, 0x7fffffff)
int hx_eug_fold(const float* vals, const int* idx, long n, float* best) {
  float bv = INFINITY; int bi = 0x7fffffff;
  for (long q = 0; q < n; q++)
    if (eug_better(vals[idx[q]], idx[q], bv, bi)) { bv = vals[idx[q]]; bi = idx[q]; }
  *best = bv;
  return bi;
}
void hx_eug_score_key(const double* x, long n, uint64_t* key) {
  for (long i = 0; i < n; i++) key[i] = eug_score_key(x[i]);
}
}
