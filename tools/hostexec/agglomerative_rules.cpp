// The scalar rules of csrc/agglomerative.hip, executed on the host: the better-than order of a scan's arg-min, the "previous element keeps
// ties" rule, the complete and average updates and the single-linkage min-update are plain scalar C++ behind `__device__`.
// tests/test_agglomerative_host.py cuts their text out of agglomerative.hip into agglomerative_cut.inc; with `__device__` mapped to host
// functions and the three rounding intrinsics to one IEEE operation each (the build passes -ffp-contract=off) the SAME TEXT is compiled
// for x86 and held bit for bit to numpy and to scipy's loop.  Test infrastructure: nothing here is linked into the product.
#include <cmath>
#include <cstring>
#define __device__
#define __forceinline__ inline
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline double __dadd_rn(double a, double b) { return a + b; }
static inline double __ddiv_rn(double a, double b) { return a / b; }
namespace ssg {
#include "agglomerative_cut.inc"
}
using namespace ssg;

extern "C" {
void hx_agglo_average(const double* da, const double* db, const int* na, const int* nb, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = agglo_average(da[i], db[i], na[i], nb[i]);
}
void hx_agglo_complete(const double* da, const double* db, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = agglo_complete(da[i], db[i]);
}
void hx_agglo_min_update(const double* m, const double* d, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = agglo_min_update(m[i], d[i]);
}
// One scan as the kernel runs it: row [n] of slot x, size [n] (0 = dead), p = chain[-2] or -1.  Folds the slots in ascending or
// descending index order -- the rule must not depend on it -- then applies the previous-element rule once.  -> y, *cur = its distance
long hx_agglo_scan(const double* row, const int* size, long n, long x, long p, int descending, double* cur) {
  double bs = __builtin_inf(); int bj = 0x7fffffff;
  for (long q = 0; q < n; q++) {
    const long j = descending ? n - 1 - q : q;
    if (size[j] > 0 && j != x && agglo_better(row[j], (int)j, bs, bj)) { bs = row[j]; bj = (int)j; }
  }
  if (p >= 0 && agglo_prev_keeps(bs, row[p])) { *cur = row[p]; return p; }
  *cur = bs;
  return bj == 0x7fffffff ? -1 : bj;
}
}
