// The scalar rules of csrc/optics.hip, executed on the host: around15, the core-distance finish, the reachability update of one
// neighbour, the arg-min tie rule and the order-preserving key are plain scalar C++ behind `__device__`.  tests/test_optics_host.py cuts
// their text out of optics.hip into optics_cut.inc; with `__device__` mapped to host functions the SAME TEXT is compiled for x86 and held
// bit for bit to numpy.  Test infrastructure: nothing here is linked into the product.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#undef __device__
#undef __forceinline__
#define __device__
#define __forceinline__ inline
static inline long long hx_double_as_longlong(double x) { long long r; memcpy(&r, &x, 8); return r; }
static inline double hx_longlong_as_double(long long x) { double r; memcpy(&r, &x, 8); return r; }
#define __double_as_longlong hx_double_as_longlong
#define __longlong_as_double hx_longlong_as_double
#include "../../self-similarity-grouping_amd/csrc/ssg_common.h"
namespace ssg {
#include "optics_cut.inc"
}
using namespace ssg;

extern "C" {
void hx_optics_around15(const double* x, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = optics_around15(x[i]);
}
void hx_optics_core_finish(const double* kth, long n, double max_eps, double* out) {
  for (long i = 0; i < n; i++) out[i] = optics_core_finish(kth[i], max_eps);
}
// one step's update of reach [n] from row d [n] of point p (skip[j] != 0: processed); pred[j] = p where reach improved
void hx_optics_update_row(const double* d, const unsigned char* skip, long n, double cp, double max_eps, long p, double* reach, long long* pred) {
  for (long j = 0; j < n; j++) {
    if (skip[j]) continue;
    double s = reach[j];
    if (optics_update(d[j], cp, max_eps, s)) { reach[j] = s; pred[j] = p; }
  }
}
// the arg-min over the unprocessed points, folded in two orders (ascending and descending index): the rule must not depend on it
long hx_optics_argmin(const double* reach, const unsigned char* skip, long n, int descending) {
  double bs = __builtin_inf(); int bj = 0x7fffffff;
  for (long q = 0; q < n; q++) {
    const long j = descending ? n - 1 - q : q;
    if (skip[j]) continue;
    if (optics_better(reach[j], (int)j, bs, bj)) { bs = reach[j]; bj = (int)j; }
  }
  return bj == 0x7fffffff ? -1 : bj;
}
void hx_optics_key(const double* x, long n, unsigned long long* key, double* back) {
  for (long i = 0; i < n; i++) { key[i] = optics_key(x[i]); back[i] = optics_unkey(key[i]); }
}
}
