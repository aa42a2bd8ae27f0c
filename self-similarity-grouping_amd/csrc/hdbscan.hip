// hdbscan.hip -- HDBSCAN on a precomputed distance matrix: the symmetry / NaN check, the core distances and Prim's spanning tree.
//
// Replaces the matrix stages of sklearn 1.7.2 HDBSCAN(metric='precomputed', algorithm brute) bit for bit (ssg_amd/hdbscan.py holds the
// estimator and everything that works on N-long arrays: the sort of the edges, single linkage, the condensed tree, the selection):
//   the check = how many entries are NaN, and how many ordered pairs (i, j) fail np.isclose(X[i,j], X[j,i], rtol=1e-7, atol=1e-9);
//   core[i]   = (the min_samples-th smallest entry of row i, the diagonal counted as it stands) / alpha;
//   the tree  = Prim from node 0 on the mutual reachability max(core[c], core[j], X[c,j] / alpha): N - 1 strictly sequential steps, each
//               the min-update of m[j] over the nodes outside the tree and the first arg-min of m.  The edge recorded is (the node the
//               step started from, the new node, m[new]) -- sklearn's mst_from_mutual_reachability, not the textbook (source, new).
// sklearn widens the matrix to float64, divides it by alpha and overwrites it with the mutual reachability graph (8 N^2 bytes); here the
// matrix is read through MatView / load_vals (matview.h) -- a re-rank handle (mode 0) and a half matrix (mode 1) are widened element by
// element -- and nothing N x N is ever written.  Dividing by alpha > 0 is monotone, so the select runs on the raw row.
//
// The tree runs in ONE workgroup, like the ordering loop of optics.hip: a step is one stream of row c with the min-update and the next
// arg-min in the same pass, then one workgroup reduction.  No synchronisation between workgroups, no spin loop, no atomic: every loop is
// bounded by N.  The state is one double per node -- m[j] while j is outside the tree, NaN once it is inside (NaN input is refused
// before, by the check) -- in LDS while 8 N bytes fit, else in a workspace in global memory.
//
// core[] is read from global memory (8 N bytes, read in full at every step: it stays in L2 and in the CU's vector cache), not copied into
// LDS beside the state.  Measured on one MI355X (profiles/hdbscan_times.txt; building with -DSSG_HDBSCAN_CORE_LDS=1 puts the copy into
// LDS, tools/time_hdbscan.py times both builds): the copy makes a step 3 to 4 % faster where both fit (3.2 against 3.3 us at N = 4 000, 5.2
// against 5.4 us at N = 10 000), and it halves the N the LDS placement holds, to 10 223 -- the sizes this is built for (a re-rank
// distance of 12 000 to 16 000 images) would fall to the state in global memory, which costs 14 % there (8.4 against 7.4 us per step at
// N = 16 000).  In the same rounds, on the same matrix, the loop is faster per step than optics_order_kernel in both placements (7.4
// against 8.1 us and 8.4 against 10.4 us at N = 16 000): it does less arithmetic per element and reads its state in 16-byte pairs.
#include "kth_select.h"

#ifndef SSG_HDBSCAN_CORE_LDS
#define SSG_HDBSCAN_CORE_LDS 0
#endif

namespace ssg {

// ------------------------------------------------------------------ the scalar rules (tests/test_hdbscan_host.py compiles this text for x86)
// mutual reachability max(core[c], core[j], d): the first of equal values is kept, as the three-way max of sklearn's compiled loop does
// (it matters for the sign of a zero only)
__device__ __forceinline__ double hdbscan_mreach(double cc, double cj, double d) {
  double r = cc;
  if (cj > r) r = cj;
  if (d > r) r = d;
  return r;
}
// np.minimum(m, r) without NaN: the second of equal values
__device__ __forceinline__ double hdbscan_min_update(double m, double r) { return m < r ? m : r; }
// the arg-min of a step: the smaller value first, then the smaller index (np.argmin over the ascending remaining nodes; +inf == +inf, so
// a step on which nothing is reachable takes the smallest remaining index)
__device__ __forceinline__ bool hdbscan_better(double s, int j, double bs, int bj) { return s < bs || (s == bs && j < bj); }
// np.isclose(x, y, rtol=1e-7, atol=1e-9), equal_nan=False: |x - y| <= atol + rtol |y| with y finite, or x == y (equal infinities)
__device__ __forceinline__ bool hdbscan_close(double x, double y) {
  const double tol = 1e-9 + 1e-7 * __builtin_fabs(y);
  const bool yfin = __builtin_fabs(y) < __builtin_inf();
  return (__builtin_fabs(x - y) <= tol && yfin) || x == y;
}
// ------------------------------------------------------------------ end of the scalar rules

// The check.  Workgroup (bi <= bj) holds the pair of 64 x 64 tiles A = X[I, J] and B = X[J, I].  Both are read row-wise: a row of a tile
// is the (at most nine) aligned 8-entry groups of load_vals that overlap its 64 columns, one group per lane, sixteen lanes per row, so a
// wave reads four rows of 128 to 144 contiguous bytes (half) each.  B goes to LDS, A meets it transposed there.  The LDS rows are padded
// to 65 doubles: the lanes of a wave touch B at a stride of 8 rows, which without the pad is one bank for all nine groups of a row and
// with it is four banks (a three-way conflict; the pass is bound by the matrix read).  Ragged last tiles are masked by row and column.
constexpr int HDB_TILE = 64;
template <int MODE>
__global__ __launch_bounds__(256) void hdbscan_check_kernel(MatView mv, unsigned long long* __restrict__ counts) {
  const int bi = (int)blockIdx.y, bj = (int)blockIdx.x;
  if (bi > bj) return;
  __shared__ double Bt[HDB_TILE][HDB_TILE + 1];
  __shared__ unsigned red[2][4];
  const int N = mv.N, tid = (int)threadIdx.x, q = tid & 15, rsub = tid >> 4;
  const int i0 = bi * HDB_TILE, j0 = bj * HDB_TILE;
  unsigned nan = 0, bad = 0;
  for (int rr = 0; rr < HDB_TILE; rr += 16) {              // B = X[j0 + r, i0 + c]
    const int r = rr + rsub, row = j0 + r;
    if (row >= N) continue;
    RowStream rs(row, N, N);
    const int g = ((i0 + rs.first) >> 3) + q, c0 = g * 8 - rs.first;
    if (c0 >= i0 + HDB_TILE || c0 >= N) continue;
    double d[8];
    load_vals<MODE>(mv, rs, g >> 6, g & 63, row, d);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int c = c0 + e;
      if (c < i0 || c >= i0 + HDB_TILE || c >= N) continue;
      Bt[r][c - i0] = d[e];
      if (bi != bj && d[e] != d[e]) nan++;
    }
  }
  __syncthreads();
  for (int rr = 0; rr < HDB_TILE; rr += 16) {              // A = X[i0 + r, j0 + c] against B[c][r]
    const int r = rr + rsub, row = i0 + r;
    if (row >= N) continue;
    RowStream rs(row, N, N);
    const int g = ((j0 + rs.first) >> 3) + q, c0 = g * 8 - rs.first;
    if (c0 >= j0 + HDB_TILE || c0 >= N) continue;
    double d[8];
    load_vals<MODE>(mv, rs, g >> 6, g & 63, row, d);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int c = c0 + e;
      if (c < j0 || c >= j0 + HDB_TILE || c >= N) continue;
      const double x = d[e], y = Bt[c - j0][r];
      if (x != x) nan++;
      if (!hdbscan_close(x, y)) bad++;                      // the ordered pair (row, c)
      if (bi != bj && !hdbscan_close(y, x)) bad++;          // and (c, row): off the diagonal tiles nobody else sees it
    }
  }
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) { nan += __shfl_xor(nan, x, 64); bad += __shfl_xor(bad, x, 64); }
  if ((tid & 63) == 0) { red[0][tid >> 6] = nan; red[1][tid >> 6] = bad; }
  __syncthreads();
  if (tid == 0) {
    const unsigned tn = red[0][0] + red[0][1] + red[0][2] + red[0][3], tb = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (tn) atomicAdd(&counts[0], (unsigned long long)tn);
    if (tb) atomicAdd(&counts[1], (unsigned long long)tb);
  }
}

// Core distances: the select of kth_select.h (shared with optics.hip), finished with the division by alpha.
template <int MODE>
__global__ __launch_bounds__(256) void hdbscan_core_kernel(MatView mv, int k, double alpha, double* __restrict__ core) {
  __shared__ int hist[4][256];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  for (int base = (int)blockIdx.x * 4; base < mv.nrows; base += (int)gridDim.x * 4) {
    const bool live = base + wave < mv.nrows;
    const int il = live ? base + wave : mv.nrows - 1;
    const double kth = row_kth_smallest<MODE>(mv, il, k, hist[wave]);
    if (live && lane == 0) core[il] = kth / alpha;
  }
}

// Prim.  blockDim = 64 * (waves that a row has 512-entry chunks for, at most 16), chunk c of the row goes to wave c % waves, eight columns
// per lane.  Two barriers per step: S[c] = NaN before the pass, the wave minima before the next c is read.  Where a lane's eight columns
// start on an even index inside the row (every chunk of every row when N is even) the state and the core distances are read as four
// 16-byte pairs; the entry-by-entry path reads the same values.
constexpr int HDB_MAX_WAVES = 16;
template <int MODE, bool LDS>
__global__ __launch_bounds__(64 * HDB_MAX_WAVES) void hdbscan_mst_kernel(MatView mv, const double* __restrict__ core, double alpha, double* __restrict__ gstate,
                                                                       int64_t* __restrict__ current, int64_t* __restrict__ next, double* __restrict__ distance) {
  extern __shared__ __align__(16) double hdbscan_lds[];
  __shared__ double wred_s[HDB_MAX_WAVES];
  __shared__ int wred_j[HDB_MAX_WAVES];
  double* S = LDS ? hdbscan_lds : gstate;
  const int N = mv.N, tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = lane_id(), wave = tid >> 6, nwaves = nthr >> 6;
  const double inf = __builtin_inf();
#if SSG_HDBSCAN_CORE_LDS
  double* Cl = hdbscan_lds + (LDS ? ((N + 1) & ~1) : 0);
  for (int j = tid; j < N; j += nthr) Cl[j] = core[j];
  const double* C = Cl;
  const bool pairs = (!LDS && ((uintptr_t)gstate & 15)) ? false : true;
#else
  const double* C = core;
  const bool pairs = !(((uintptr_t)core & 15) || (!LDS && ((uintptr_t)gstate & 15)));
#endif
  const bool unit = alpha == 1.0;                          // x / 1.0 is x: the common case skips N - 1 rows of divisions
  for (int j = tid; j < N; j += nthr) S[j] = inf;
  __syncthreads();
  int c = 0;
  for (int t = 0; t < N - 1; t++) {
    if ((unsigned)c >= (unsigned)N) break;                 // (the same c in every thread; cannot happen while nodes remain outside the tree)
    if (tid == 0) { current[t] = c; S[c] = __builtin_nan(""); }
    const double cc = C[c];
    __syncthreads();
    double bs = inf; int bj = 0x7fffffff;
    RowStream rs(c, N, N);
    for (int ch = wave; ch < rs.nchunks; ch += nwaves) {
      double d[8], s[8], cj[8];
      load_vals<MODE>(mv, rs, ch, lane, c, d);
      const int j0 = rs.col0(ch, lane);
      if (pairs && j0 >= 0 && j0 + 8 <= N && !(j0 & 1)) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const double2 a = *reinterpret_cast<const double2*>(S + j0 + 2 * q), b = *reinterpret_cast<const double2*>(C + j0 + 2 * q);
          s[2 * q] = a.x; s[2 * q + 1] = a.y; cj[2 * q] = b.x; cj[2 * q + 1] = b.y;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int j = j0 + e;
          const bool in = j >= 0 && j < N;
          s[e] = in ? S[j] : __builtin_nan("");
          cj[e] = in ? C[j] : 0.0;
        }
      }
      if (!unit) {
#pragma unroll
        for (int e = 0; e < 8; e++) d[e] = d[e] / alpha;
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        if (s[e] != s[e]) continue;                        // in the tree, or outside the row
        const double m = hdbscan_min_update(s[e], hdbscan_mreach(cc, cj[e], d[e]));
        if (__double_as_longlong(m) != __double_as_longlong(s[e])) S[j0 + e] = m;
        if (hdbscan_better(m, j0 + e, bs, bj)) { bs = m; bj = j0 + e; }
      }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      const double os = __shfl_xor(bs, x, 64); const int oj = __shfl_xor(bj, x, 64);
      if (hdbscan_better(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    if (lane == 0) { wred_s[wave] = bs; wred_j[wave] = bj; }
    __syncthreads();
    bs = wred_s[0]; bj = wred_j[0];
    for (int w = 1; w < nwaves; w++) {
      const double os = wred_s[w]; const int oj = wred_j[w];
      if (hdbscan_better(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    if (tid == 0 && (unsigned)bj < (unsigned)N) { next[t] = bj; distance[t] = bs; }
    c = bj;
  }
}

}  // namespace ssg

using namespace ssg;

// the state of the tree in LDS (and, in the measuring build, the core distances beside it) inside the 160 KB a workgroup may hold
constexpr size_t HDB_LDS_LIMIT = 160 * 1024;
constexpr size_t HDB_LDS_STATIC = 256;
extern "C" int ssg_hdbscan_lds_max_n(void) { return (int)((HDB_LDS_LIMIT - HDB_LDS_STATIC) / (SSG_HDBSCAN_CORE_LDS ? 16 : 8)) - (SSG_HDBSCAN_CORE_LDS ? 1 : 0); }

static int hdbscan_check_matrix(const char* fn, const void* M, const uint16_t* v, int N, int mode) {
  if (!M || N < 2 || mode < 0 || mode > 2 || (mode == 0 && !v)) {
    ssg_set_error("%s: bad matrix (M=%p N=%d mode=%d%s); N >= 2, mode 0 needs v", fn, M, N, mode, (mode == 0 && !v) ? " v=NULL" : "");
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}
static int hdbscan_check_alpha(const char* fn, double alpha) {
  if (!(alpha > 0.0) || !(alpha < __builtin_inf())) { ssg_set_error("%s: alpha=%g must be positive and finite", fn, alpha); return SSG_ERR_INVALID; }
  return SSG_OK;
}

extern "C" int ssg_hdbscan_check(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int64_t* counts, hipStream_t stream) {
  int rc = hdbscan_check_matrix("ssg_hdbscan_check", M, v, N, mode); if (rc) return rc;
  if (!counts || ((uintptr_t)counts & 7)) { ssg_set_error("ssg_hdbscan_check: counts must be two 8-byte aligned int64 words, got %p", (void*)counts); return SSG_ERR_INVALID; }
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
  const int T = (N + HDB_TILE - 1) / HDB_TILE;
  SSG_HIP(hipMemsetAsync(counts, 0, 16, stream));
#define SSG_HC(MD) hipLaunchKernelGGL(hdbscan_check_kernel<MD>, dim3(T, T), dim3(256), 0, stream, mv, (unsigned long long*)counts)
  if (mode == 0) SSG_HC(0); else if (mode == 1) SSG_HC(1); else SSG_HC(2);
#undef SSG_HC
  SSG_LAUNCH_CHECK("hdbscan_check_kernel");
  return SSG_OK;
}

extern "C" int ssg_hdbscan_core_dist(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int min_samples, double alpha, double* core,
                                     hipStream_t stream) {
  int rc = hdbscan_check_matrix("ssg_hdbscan_core_dist", M, v, N, mode); if (rc) return rc;
  if (!core) { ssg_set_error("ssg_hdbscan_core_dist: null output"); return SSG_ERR_INVALID; }
  if (min_samples < 1 || min_samples > N) { ssg_set_error("ssg_hdbscan_core_dist: min_samples=%d outside [1, N=%d]", min_samples, N); return SSG_ERR_INVALID; }
  rc = hdbscan_check_alpha("ssg_hdbscan_core_dist", alpha); if (rc) return rc;
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
#define SSG_HK(MD) hipLaunchKernelGGL(hdbscan_core_kernel<MD>, dim3(stream_grid(N)), dim3(256), 0, stream, mv, min_samples, alpha, core)
  if (mode == 0) SSG_HK(0); else if (mode == 1) SSG_HK(1); else SSG_HK(2);
#undef SSG_HK
  SSG_LAUNCH_CHECK("hdbscan_core_kernel");
  return SSG_OK;
}

extern "C" int ssg_hdbscan_mst(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const double* core, double alpha, int state, void* ws,
                               size_t ws_bytes, int64_t* current, int64_t* next, double* distance, hipStream_t stream) {
  int rc = hdbscan_check_matrix("ssg_hdbscan_mst", M, v, N, mode); if (rc) return rc;
  if (!core || !current || !next || !distance) { ssg_set_error("ssg_hdbscan_mst: null core / current / next / distance"); return SSG_ERR_INVALID; }
  if (((uintptr_t)core & 7) || ((uintptr_t)current & 7) || ((uintptr_t)next & 7) || ((uintptr_t)distance & 7)) {
    ssg_set_error("ssg_hdbscan_mst: core / current / next / distance must be 8-byte aligned"); return SSG_ERR_INVALID;
  }
  rc = hdbscan_check_alpha("ssg_hdbscan_mst", alpha); if (rc) return rc;
  if (state < 0 || state > 2) { ssg_set_error("ssg_hdbscan_mst: state=%d must be 0 (auto), 1 (LDS) or 2 (global)", state); return SSG_ERR_INVALID; }
  const bool fits = N <= ssg_hdbscan_lds_max_n();
  if (state == 1 && !fits) { ssg_set_error("ssg_hdbscan_mst: state=1 (LDS) holds at most N=%d nodes, got N=%d", ssg_hdbscan_lds_max_n(), N); return SSG_ERR_INVALID; }
  const bool lds = state == 1 || (state == 0 && fits);
  if (!lds && (!ws || ws_bytes < (size_t)N * 8 || ((uintptr_t)ws & 7))) {
    ssg_set_error("ssg_hdbscan_mst: the global state needs an 8-byte aligned workspace of %zu bytes, got %zu", (size_t)N * 8, ws ? ws_bytes : (size_t)0);
    return SSG_ERR_INVALID;
  }
#if SSG_HDBSCAN_CORE_LDS
  if (!fits) { ssg_set_error("ssg_hdbscan_mst: the measuring build (core distances in LDS) holds at most N=%d nodes, got N=%d", ssg_hdbscan_lds_max_n(), N); return SSG_ERR_INVALID; }
#endif
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
  const int chunks = (N + 7 + 511) / 512;
  const int waves = chunks < 1 ? 1 : chunks > HDB_MAX_WAVES ? HDB_MAX_WAVES : chunks;
  const size_t n2 = ((size_t)N + 1) & ~(size_t)1;
  const size_t dyn = (lds ? n2 * 8 : 0) + (SSG_HDBSCAN_CORE_LDS ? n2 * 8 : 0);
#define SSG_HM(MD, L) do { \
    if (dyn > 48 * 1024) SSG_HIP(hipFuncSetAttribute((const void*)hdbscan_mst_kernel<MD, L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn)); \
    hipLaunchKernelGGL((hdbscan_mst_kernel<MD, L>), dim3(1), dim3(64 * waves), dyn, stream, mv, core, alpha, (double*)ws, current, next, distance); \
  } while (0)
  if (lds) { if (mode == 0) SSG_HM(0, true); else if (mode == 1) SSG_HM(1, true); else SSG_HM(2, true); }
  else { if (mode == 0) SSG_HM(0, false); else if (mode == 1) SSG_HM(1, false); else SSG_HM(2, false); }
#undef SSG_HM
  SSG_LAUNCH_CHECK("hdbscan_mst_kernel");
  return SSG_OK;
}
