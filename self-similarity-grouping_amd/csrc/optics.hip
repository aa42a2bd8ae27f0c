// optics.hip -- OPTICS on a precomputed distance matrix: core distances and the ordering loop.
//
// Replaces sklearn 1.7.2 compute_optics_graph(metric='precomputed') bit for bit (ssg_amd/optics.py holds the estimator and the two label
// extractions, which work on four N-long arrays and stay on the host):
//   core[i]  = around15(the min_samples-th smallest entry of row i, the diagonal counted as it stands; > max_eps -> +inf)
//   the loop = N strictly sequential steps: p = the unprocessed point of smallest reachability (ties: smallest index), and, when core[p]
//              is finite, every unprocessed j with X[p,j] <= max_eps takes r = around15(max(X[p,j], core[p])) when r < reach[j].
// sklearn widens every matrix to float64 first; the matrix is read through MatView / load_vals (matview.h), so a re-rank handle (mode 0)
// and a half matrix (mode 1) are widened element by element and never materialised.
//
// The loop runs in ONE workgroup: a step is one stream of row p, with the next step's arg-min folded into the same pass, and one
// workgroup reduction.  There is no synchronisation between workgroups, no spin loop and no atomic: every loop below is bounded by N.
// The state is one double per point -- its reachability while it is unprocessed, NaN once it is processed (a reachability is never NaN:
// an entry that is NaN fails `<= max_eps` and is skipped) -- in LDS while 8 N bytes fit, else in a workspace in global memory.
#include "kth_select.h"

namespace ssg {

// ------------------------------------------------------------------ the scalar rules (tests/test_optics_host.py compiles this text for x86)
// np.around(x, 15): product, round-half-even and division each rounded on their own; the division is applied whatever the size of the
// product (numpy does so: past 2^53 the result can differ from x); +inf stays +inf
__device__ __forceinline__ double optics_around15(double x) {
  const double s = x * 1e15;
  const double r = rint(s);
  return r / 1e15;
}
// core distance from the min_samples-th smallest entry of the row
__device__ __forceinline__ double optics_core_finish(double kth, double max_eps) { return optics_around15(kth > max_eps ? __builtin_inf() : kth); }
// _set_reach_dist for one unprocessed j: d = X[p,j], cp = core[p] (finite), s = reach[j]; true when s was improved
__device__ __forceinline__ bool optics_update(double d, double cp, double max_eps, double& s) {
  if (!(d <= max_eps)) return false;                       // radius_neighbors(radius=max_eps) on the precomputed row
  const double m = d > cp ? d : cp;                        // np.maximum
  // around15(m) >= m (1 - 2^-52) - 0.5e-15 (1 + 2^-52) for m > 0 (product and quotient lose at most 2^-53 each, rint at most 0.5): a
  // candidate that lies above s by more than that margin cannot improve it.  The loop is bound by this arithmetic (sixteen waves on the
  // four SIMDs of one CU) and most candidates are far above s: they skip the division.
  if (m > 0.0 && m - m * 1e-15 - 1e-15 >= s) return false;
  const double r = optics_around15(m);                     // np.around
  if (r < s) { s = r; return true; }
  return false;
}
// the arg-min of the next step: smaller reachability first, then the smaller index (np.argmin over the ascending unprocessed indices;
// +inf == +inf, so a step on which nothing is reachable restarts at the smallest unprocessed index)
__device__ __forceinline__ bool optics_better(double s, int j, double bs, int bj) { return s < bs || (s == bs && j < bj); }
// order-preserving 64-bit key of a double (any sign) and its inverse
__device__ __forceinline__ uint64_t optics_key(double d) {
  const uint64_t b = (uint64_t)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double optics_unkey(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
  return __longlong_as_double((long long)b);
}
// ------------------------------------------------------------------ end of the scalar rules

// One wave per row: the min_samples-th smallest entry by the radix select of kth_select.h.  The four waves of a workgroup walk the same
// number of rows (a wave past the end repeats the last row and writes nothing), so the barriers match.
template <int MODE>
__global__ __launch_bounds__(256) void optics_core_kernel(MatView mv, int k, double max_eps, double* __restrict__ core) {
  __shared__ int hist[4][256];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  for (int base = (int)blockIdx.x * 4; base < mv.nrows; base += (int)gridDim.x * 4) {
    const bool live = base + wave < mv.nrows;
    const int il = live ? base + wave : mv.nrows - 1;
    const double kth = row_kth_smallest<MODE>(mv, il, k, hist[wave]);
    if (live && lane == 0) core[il] = optics_core_finish(kth, max_eps);
  }
}

// The ordering loop.  blockDim = 64 * (waves that a row has 512-entry chunks for, at most 16).  Chunk c of row p goes to wave c % waves,
// eight columns per lane; which thread sees column j changes with the row's alignment, and the barrier between two steps orders the
// accesses to S[j].  Two barriers per step: S[p] = NaN before the pass, the wave minima before the next p is read.
constexpr int OPTICS_MAX_WAVES = 16;
template <int MODE, bool LDS>
__global__ __launch_bounds__(64 * OPTICS_MAX_WAVES) void optics_order_kernel(MatView mv, const double* __restrict__ core, double max_eps, double* __restrict__ gstate,
                                                                           int64_t* __restrict__ ordering, double* __restrict__ reach, int64_t* __restrict__ pred) {
  extern __shared__ double optics_lds[];
  __shared__ double wred_s[OPTICS_MAX_WAVES];
  __shared__ int wred_j[OPTICS_MAX_WAVES];
  double* S = LDS ? optics_lds : gstate;
  const int N = mv.N, tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = lane_id(), wave = tid >> 6, nwaves = nthr >> 6;
  const double inf = __builtin_inf();
  for (int j = tid; j < N; j += nthr) { S[j] = inf; pred[j] = -1; }
  __syncthreads();
  int p = 0;                                               // every reachability is +inf: the smallest index
  for (int t = 0; t < N; t++) {
    if ((unsigned)p >= (unsigned)N) break;                 // (the same p in every thread; cannot happen while t < N points are processed)
    if (tid == 0) { ordering[t] = p; reach[p] = S[p]; S[p] = __builtin_nan(""); }
    const double cp = core[p];
    __syncthreads();
    double bs = inf; int bj = 0x7fffffff;
    if (cp < inf) {
      RowStream rs(p, N, N);
      for (int c = wave; c < rs.nchunks; c += nwaves) {
        double d[8];
        load_vals<MODE>(mv, rs, c, lane, p, d);
        const int j0 = rs.col0(c, lane);
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int j = j0 + e;
          if (j < 0 || j >= N) continue;
          double s = S[j];
          if (s != s) continue;                            // processed
          if (optics_update(d[e], cp, max_eps, s)) { S[j] = s; pred[j] = p; }
          if (optics_better(s, j, bs, bj)) { bs = s; bj = j; }
        }
      }
    } else {
      for (int j = tid; j < N; j += nthr) {
        const double s = S[j];
        if (s == s && optics_better(s, j, bs, bj)) { bs = s; bj = j; }
      }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      const double os = __shfl_xor(bs, x, 64); const int oj = __shfl_xor(bj, x, 64);
      if (optics_better(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    if (lane == 0) { wred_s[wave] = bs; wred_j[wave] = bj; }
    __syncthreads();
    bs = wred_s[0]; bj = wred_j[0];
    for (int w = 1; w < nwaves; w++) {
      const double os = wred_s[w]; const int oj = wred_j[w];
      if (optics_better(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    p = bj;
  }
}

}  // namespace ssg

using namespace ssg;

// the state of the ordering loop in LDS: 8 N bytes beside the reduction words, inside the 160 KB a workgroup may hold
constexpr size_t OPTICS_LDS_LIMIT = 160 * 1024;
constexpr size_t OPTICS_LDS_STATIC = 256;
extern "C" int ssg_optics_lds_max_n(void) { return (int)((OPTICS_LDS_LIMIT - OPTICS_LDS_STATIC) / 8); }

static int optics_check_matrix(const char* fn, const void* M, const uint16_t* v, int N, int mode) {
  if (!M || N < 2 || mode < 0 || mode > 2 || (mode == 0 && !v)) {
    ssg_set_error("%s: bad matrix (M=%p N=%d mode=%d%s); N >= 2, mode 0 needs v", fn, M, N, mode, (mode == 0 && !v) ? " v=NULL" : "");
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

extern "C" int ssg_optics_core_dist(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int min_samples, double max_eps, double* core,
                                    hipStream_t stream) {
  int rc = optics_check_matrix("ssg_optics_core_dist", M, v, N, mode); if (rc) return rc;
  if (!core) { ssg_set_error("ssg_optics_core_dist: null output"); return SSG_ERR_INVALID; }
  if (min_samples < 2 || min_samples > N) { ssg_set_error("ssg_optics_core_dist: min_samples=%d outside [2, N=%d]", min_samples, N); return SSG_ERR_INVALID; }
  if (!(max_eps >= 0.0)) { ssg_set_error("ssg_optics_core_dist: max_eps=%g must be >= 0", max_eps); return SSG_ERR_INVALID; }
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
#define SSG_OC(MD) hipLaunchKernelGGL(optics_core_kernel<MD>, dim3(stream_grid(N)), dim3(256), 0, stream, mv, min_samples, max_eps, core)
  if (mode == 0) SSG_OC(0); else if (mode == 1) SSG_OC(1); else SSG_OC(2);
#undef SSG_OC
  SSG_LAUNCH_CHECK("optics_core_kernel");
  return SSG_OK;
}

extern "C" int ssg_optics_order(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const double* core, double max_eps, int state,
                                void* ws, size_t ws_bytes, int64_t* ordering, double* reachability, int64_t* predecessor, hipStream_t stream) {
  int rc = optics_check_matrix("ssg_optics_order", M, v, N, mode); if (rc) return rc;
  if (!core || !ordering || !reachability || !predecessor) { ssg_set_error("ssg_optics_order: null core / ordering / reachability / predecessor"); return SSG_ERR_INVALID; }
  if (!(max_eps >= 0.0)) { ssg_set_error("ssg_optics_order: max_eps=%g must be >= 0", max_eps); return SSG_ERR_INVALID; }
  if (state < 0 || state > 2) { ssg_set_error("ssg_optics_order: state=%d must be 0 (auto), 1 (LDS) or 2 (global)", state); return SSG_ERR_INVALID; }
  const bool fits = N <= ssg_optics_lds_max_n();
  if (state == 1 && !fits) { ssg_set_error("ssg_optics_order: state=1 (LDS) holds at most N=%d points, got N=%d", ssg_optics_lds_max_n(), N); return SSG_ERR_INVALID; }
  const bool lds = state == 1 || (state == 0 && fits);
  if (!lds && (!ws || ws_bytes < (size_t)N * 8 || ((uintptr_t)ws & 7))) {
    ssg_set_error("ssg_optics_order: the global state needs an 8-byte aligned workspace of %zu bytes, got %zu", (size_t)N * 8, ws ? ws_bytes : (size_t)0);
    return SSG_ERR_INVALID;
  }
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
  const int chunks = (N + 7 + 511) / 512;
  const int waves = chunks < 1 ? 1 : chunks > OPTICS_MAX_WAVES ? OPTICS_MAX_WAVES : chunks;
  const size_t dyn = lds ? (size_t)N * 8 : 0;
#define SSG_OO(MD, L) do { \
    if (dyn > 48 * 1024) SSG_HIP(hipFuncSetAttribute((const void*)optics_order_kernel<MD, L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn)); \
    hipLaunchKernelGGL((optics_order_kernel<MD, L>), dim3(1), dim3(64 * waves), dyn, stream, mv, core, max_eps, (double*)ws, ordering, reachability, predecessor); \
  } while (0)
  if (lds) { if (mode == 0) SSG_OO(0, true); else if (mode == 1) SSG_OO(1, true); else SSG_OO(2, true); }
  else { if (mode == 0) SSG_OO(0, false); else if (mode == 1) SSG_OO(1, false); else SSG_OO(2, false); }
#undef SSG_OO
  SSG_LAUNCH_CHECK("optics_order_kernel");
  return SSG_OK;
}
