// The scalar rules of csrc/hdbscan.hip, executed on the host: the three-way max of the mutual reachability, the min-update, the
// better-than order of the arg-min and the allclose predicate are plain scalar C++ behind `__device__`.  tests/test_hdbscan_host.py cuts
// their text out of hdbscan.hip into hdbscan_cut.inc; with `__device__` mapped to host functions the SAME TEXT is compiled for x86 and held
// bit for bit to numpy.  Test infrastructure: nothing here is linked into the product.
#include <cmath>
#include <cstring>
#define __device__
#define __forceinline__ inline
namespace ssg {
#include "hdbscan_cut.inc"
}
using namespace ssg;

extern "C" {
void hx_hdbscan_mreach(const double* cc, const double* cj, const double* d, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = hdbscan_mreach(cc[i], cj[i], d[i]);
}
void hx_hdbscan_min_update(const double* m, const double* r, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = hdbscan_min_update(m[i], r[i]);
}
void hx_hdbscan_close(const double* x, const double* y, long n, unsigned char* out) {
  for (long i = 0; i < n; i++) out[i] = hdbscan_close(x[i], y[i]) ? 1 : 0;
}
// One Prim step as the kernel runs it: S[j] is m[j], NaN once j is in the tree; row d [n] of the current node c (already divided by
// alpha), cc = core[c].  Folds the nodes in ascending or descending index order -- the rule must not depend on it.  -> the next node
long hx_hdbscan_step(const double* d, const double* core, double cc, long n, int descending, double* S, double* best) {
  double bs = __builtin_inf(); int bj = 0x7fffffff;
  for (long q = 0; q < n; q++) {
    const long j = descending ? n - 1 - q : q;
    const double s = S[j];
    if (s != s) continue;
    const double m = hdbscan_min_update(s, hdbscan_mreach(cc, core[j], d[j]));
    S[j] = m;
    if (hdbscan_better(m, (int)j, bs, bj)) { bs = m; bj = (int)j; }
  }
  *best = bs;
  return bj == 0x7fffffff ? -1 : bj;
}
}
