// agglomerative.hip -- bottom-up clustering of a precomputed distance matrix: the NaN / inf check, the float64 working square and the
// merge loop of average, complete and single linkage.
//
// Replaces scipy 1.15.3's `linkage(y, method)` on the condensed upper triangle -- what sklearn 1.7.2's AgglomerativeClustering(
// metric='precomputed', connectivity=None) calls -- bit for bit (ssg_amd/agglomerative.py holds the estimator and everything that works
// on N-long arrays: the stable sort of the merges, scipy's `label` pass, the cut):
//   the check  = how many entries of the whole matrix are NaN and how many are +-inf (sklearn's validate_data refuses both);
//   the expand = W[i,j] = W[j,i] = d(i,j) = X[min(i,j), max(i,j)] widened to float64: only the strict upper triangle is read, the
//                diagonal of W is 0 and is never looked at.  W is the ONLY N x N write and the input is never modified; in return a scan
//                from slot x is one contiguous row.  Rows of W are `ld` doubles apart, ld % 4 == 0, so every row starts on 32 bytes;
//   the loop   = average / complete: scipy's nn_chain.  A SCAN from x = chain[-1]: the live slot i != x of smallest W[x,i], the lowest
//                index on ties, except that p = chain[-2] keeps every tie with the minimum (the rule that prevents cycling).  y == p
//                ends the chain walk, else y is pushed.  A MERGE pops two slots, orders them a < b, records (a, b, W[a,b],
//                size[a] + size[b]), kills slot a and rewrites row b and column b:  complete max(W[i,a], W[i,b]);  average
//                (na * W[i,a] + nb * W[i,b]) / (na + nb) -- two products, one sum, one quotient, each rounded once, never fused.
//                single: scipy's mst_single_linkage, Prim from node 0 on W with m[j] = min(m[j], W[c,j]), the next node the unmerged
//                node of smallest m, lowest index on ties; a step records (c, next, m[next]).
//
// The loop runs in ONE workgroup like the spanning tree of hdbscan.hip and the ordering of optics.hip: no synchronisation between
// workgroups, no spin loop, no atomic.  Every loop is bounded: nn_chain makes at most 3 (N - 1) scans (every scan pushes or merges, and
// starts + pushes = 2 (N - 1)); the kernel counts them, stops at the bound and raises flag[0].  It reads the check's counts first and
// returns at once when the matrix holds a NaN or an infinity, so every comparison below is between finite values.  The state -- size[]
// and chain[] (int32 each), or m[] (float64) for single linkage, 8 bytes per slot -- lives in LDS while it fits, else in a workspace.
#include "matview.h"

namespace ssg {

// ------------------------------------------------------------------ the scalar rules (tests/test_agglomerative_host.py compiles this text for x86)
// the arg-min of a scan: the smaller value first, then the smaller index -- the same answer in any fold order
__device__ __forceinline__ bool agglo_better(double s, int j, double bs, int bj) { return s < bs || (s == bs && j < bj); }
// scipy starts a scan at (p, W[x,p]) and moves only on a strictly smaller value: p keeps every tie with the minimum
__device__ __forceinline__ bool agglo_prev_keeps(double best, double dp) { return !(best < dp); }
// complete linkage: Cython's max(d_xi, d_yi), the first of equal values
__device__ __forceinline__ double agglo_complete(double da, double db) { return db > da ? db : da; }
// average linkage: (na * d_xi + nb * d_yi) / (na + nb), four roundings
__device__ __forceinline__ double agglo_average(double da, double db, int na, int nb) {
  return __ddiv_rn(__dadd_rn(__dmul_rn((double)na, da), __dmul_rn((double)nb, db)), (double)(na + nb));
}
// single linkage: `if D[k] > dist: D[k] = dist`, the first of equal values
__device__ __forceinline__ double agglo_min_update(double m, double d) { return m > d ? d : m; }
// ------------------------------------------------------------------ end of the scalar rules

// The check: one wave per row through load_vals, the rows dealt over a persistent grid; one atomic pair per workgroup.
template <int MODE>
__global__ __launch_bounds__(256) void agglo_check_kernel(MatView mv, unsigned long long* __restrict__ counts) {
  __shared__ unsigned red[2][4];
  const int N = mv.N, lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  const double inf = __builtin_inf();
  unsigned nan = 0, ninf = 0;
  for (int row = (int)blockIdx.x * 4 + wave; row < N; row += (int)gridDim.x * 4) {
    RowStream rs(row, N, N);
    for (int ch = 0; ch < rs.nchunks; ch++) {
      double d[8];
      load_vals<MODE>(mv, rs, ch, lane, row, d);
      const int j0 = rs.col0(ch, lane);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int j = j0 + e;
        if (j < 0 || j >= N) continue;
        if (d[e] != d[e]) nan++;
        else if (__builtin_fabs(d[e]) == inf) ninf++;
      }
    }
  }
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) { nan += __shfl_xor(nan, x, 64); ninf += __shfl_xor(ninf, x, 64); }
  if (lane == 0) { red[0][wave] = nan; red[1][wave] = ninf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned tn = red[0][0] + red[0][1] + red[0][2] + red[0][3], ti = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (tn) atomicAdd(&counts[0], (unsigned long long)tn);
    if (ti) atomicAdd(&counts[1], (unsigned long long)ti);
  }
}

// The expand.  Workgroup (bi <= bj) reads the 64 x 64 tile A = X[I, J] row-wise as hdbscan_check_kernel reads its tiles (the aligned
// 8-entry groups of load_vals that overlap the 64 columns, sixteen lanes per row), parks it in LDS (rows padded to 65 doubles) and
// writes W[I, J] = A and W[J, I] = A^T, both in rows of 512 contiguous bytes per wave.  The diagonal tile takes its lower half from its
// own upper half.  Tiles below the diagonal are never read.  Ragged last tiles are masked by row and column.
constexpr int AGG_TILE = 64;
template <int MODE>
__global__ __launch_bounds__(256) void agglo_expand_kernel(MatView mv, double* __restrict__ W, size_t ld) {
  const int bi = (int)blockIdx.y, bj = (int)blockIdx.x;
  if (bi > bj) return;
  __shared__ double At[AGG_TILE][AGG_TILE + 1];
  const int N = mv.N, tid = (int)threadIdx.x, q = tid & 15, rsub = tid >> 4;
  const int i0 = bi * AGG_TILE, j0 = bj * AGG_TILE;
  for (int rr = 0; rr < AGG_TILE; rr += 16) {
    const int r = rr + rsub, row = i0 + r;
    if (row >= N) continue;
    RowStream rs(row, N, N);
    const int g = ((j0 + rs.first) >> 3) + q, c0 = g * 8 - rs.first;
    if (c0 >= j0 + AGG_TILE || c0 >= N) continue;
    double d[8];
    load_vals<MODE>(mv, rs, g >> 6, g & 63, row, d);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int c = c0 + e;
      if (c < j0 || c >= j0 + AGG_TILE || c >= N) continue;
      At[r][c - j0] = d[e];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < AGG_TILE * AGG_TILE; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    if (bi != bj) {
      if (i0 + r < N && j0 + c < N) W[(size_t)(i0 + r) * ld + (j0 + c)] = At[r][c];
      if (j0 + r < N && i0 + c < N) W[(size_t)(j0 + r) * ld + (i0 + c)] = At[c][r];
    } else if (i0 + r < N && i0 + c < N) {
      W[(size_t)(i0 + r) * ld + (i0 + c)] = r < c ? At[r][c] : r > c ? At[c][r] : 0.0;
    }
  }
}

// nn_chain.  blockDim = 64 * (waves that a row has 256-entry pieces for, at most 16); a thread takes four consecutive slots per piece:
// 32 bytes of the row and 16 bytes of size[].  One barrier per scan (the wave minima are double-buffered), two per merge.  x, p and
// the chain length are the same in every thread: they follow from the reduced minima, which every thread folds in the same order.
constexpr int AGG_MAX_WAVES = 16;
template <int METHOD, bool LDS>
__global__ __launch_bounds__(64 * AGG_MAX_WAVES) void agglo_nn_chain_kernel(double* __restrict__ W, int N, size_t ld, const int64_t* __restrict__ counts,
                                                                          int* __restrict__ gstate, int64_t* __restrict__ ox, int64_t* __restrict__ oy,
                                                                          double* __restrict__ od, int64_t* __restrict__ osz, int64_t* __restrict__ flag) {
  extern __shared__ __align__(16) int agglo_lds[];
  __shared__ double wred_s[2][AGG_MAX_WAVES];
  __shared__ int wred_j[2][AGG_MAX_WAVES];
  if (counts[0] != 0 || counts[1] != 0) return;              // NaN or inf: the outputs keep what the caller put there
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = lane_id(), wave = tid >> 6, nwaves = nthr >> 6;
  const int n4 = (N + 3) & ~3;
  int* size = LDS ? agglo_lds : gstate;
  int* chain = size + n4;
  const double inf = __builtin_inf();
  for (int j = tid; j < n4; j += nthr) size[j] = j < N ? 1 : 0;
  __syncthreads();
  const long long bound = 3ll * (N - 1);
  long long scans = 0;
  int clen = 0, lowest = 0, x = 0, p = 0, par = 0;
  for (int k = 0; k < N - 1; k++) {
    if (clen == 0) {
      while (lowest < N && size[lowest] == 0) lowest++;
      if (lowest >= N) { if (tid == 0) { flag[0] = 2; flag[1] = scans; } return; }
      if (tid == 0) chain[0] = lowest;
      x = lowest; clen = 1;
    }
    int y; double cur;
    while (true) {
      if (scans >= bound) { if (tid == 0) { flag[0] = 1; flag[1] = scans; } return; }
      scans++;
      double bs = inf; int bj = 0x7fffffff;
      const double* row = W + (size_t)x * ld;
      for (int j0 = 4 * tid; j0 < N; j0 += 4 * nthr) {
        const double2 a = *reinterpret_cast<const double2*>(row + j0), b = *reinterpret_cast<const double2*>(row + j0 + 2);
        const int4 s = *reinterpret_cast<const int4*>(size + j0);
        const double d[4] = {a.x, a.y, b.x, b.y};
        const int sz[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int j = j0 + e;
          if (sz[e] > 0 && j != x && agglo_better(d[e], j, bs, bj)) { bs = d[e]; bj = j; }
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(bs, m, 64); const int oj = __shfl_xor(bj, m, 64);
        if (agglo_better(os, oj, bs, bj)) { bs = os; bj = oj; }
      }
      if (lane == 0) { wred_s[par][wave] = bs; wred_j[par][wave] = bj; }
      __syncthreads();
      bs = wred_s[par][0]; bj = wred_j[par][0];
      for (int w = 1; w < nwaves; w++) {
        const double os = wred_s[par][w]; const int oj = wred_j[par][w];
        if (agglo_better(os, oj, bs, bj)) { bs = os; bj = oj; }
      }
      par ^= 1;
      if ((unsigned)bj >= (unsigned)N) { if (tid == 0) { flag[0] = 2; flag[1] = scans; } return; }   // (no live slot beside x: cannot happen before merge N - 1)
      if (clen > 1) {
        const double dp = row[p];
        if (agglo_prev_keeps(bs, dp)) { y = p; cur = dp; break; }
      }
      if (clen >= N) { if (tid == 0) { flag[0] = 2; flag[1] = scans; } return; }                   // (the chain holds distinct live slots)
      if (tid == 0) chain[clen] = bj;
      clen++; p = x; x = bj;
    }
    // the merge
    clen -= 2;
    const int a = x < y ? x : y, b = x < y ? y : x;
    const int na = size[a], nb = size[b];
    const double* ra = W + (size_t)a * ld;
    double* rb = W + (size_t)b * ld;
    for (int j0 = 4 * tid; j0 < N; j0 += 4 * nthr) {
      const double2 a0 = *reinterpret_cast<const double2*>(ra + j0), a1 = *reinterpret_cast<const double2*>(ra + j0 + 2);
      const double2 b0 = *reinterpret_cast<const double2*>(rb + j0), b1 = *reinterpret_cast<const double2*>(rb + j0 + 2);
      const int4 s = *reinterpret_cast<const int4*>(size + j0);
      const double da[4] = {a0.x, a0.y, a1.x, a1.y}, db[4] = {b0.x, b0.y, b1.x, b1.y};
      const int sz[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int j = j0 + e;
        if (sz[e] <= 0 || j == a || j == b) continue;
        const double v = METHOD == 1 ? agglo_complete(da[e], db[e]) : agglo_average(da[e], db[e], na, nb);
        rb[j] = v;
        W[(size_t)j * ld + b] = v;
      }
    }
    __syncthreads();                                          // every thread has read size[a], size[b] and its part of the two rows
    if (tid == 0) {
      size[a] = 0; size[b] = na + nb;
      ox[k] = a; oy[k] = b; od[k] = cur; osz[k] = na + nb;
    }
    if (clen >= 1) x = chain[clen - 1];
    if (clen >= 2) p = chain[clen - 2];
    __syncthreads();                                          // the new sizes, row b and column b before the next scan
  }
  if (tid == 0) flag[1] = scans;
}

// single linkage: Prim on W.  The state is m[j] while j is unmerged and NaN once it is merged (the check refused NaN input).  Two
// barriers per step, as in hdbscan_mst_kernel.  (ssg_hdbscan_mst with core = -inf and alpha = 1 is the same loop on a symmetric matrix
// without zeros of both signs; it reads X[c,j] on both sides of the diagonal and its min-update keeps the SECOND of equal values, scipy's
// the first, so on an asymmetric matrix or on -0.0 against +0.0 its bits differ: hence this variant on W.)
template <bool LDS>
__global__ __launch_bounds__(64 * AGG_MAX_WAVES) void agglo_single_kernel(const double* __restrict__ W, int N, size_t ld, const int64_t* __restrict__ counts,
                                                                        double* __restrict__ gstate, int64_t* __restrict__ ox, int64_t* __restrict__ oy,
                                                                        double* __restrict__ od, int64_t* __restrict__ flag) {
  extern __shared__ __align__(16) int agglo_lds[];
  __shared__ double wred_s[AGG_MAX_WAVES];
  __shared__ int wred_j[AGG_MAX_WAVES];
  if (counts[0] != 0 || counts[1] != 0) return;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = lane_id(), wave = tid >> 6, nwaves = nthr >> 6;
  const int n4 = (N + 3) & ~3;
  double* S = LDS ? reinterpret_cast<double*>(agglo_lds) : gstate;
  const double inf = __builtin_inf();
  for (int j = tid; j < n4; j += nthr) S[j] = j < N ? inf : __builtin_nan("");
  __syncthreads();
  int c = 0;
  for (int t = 0; t < N - 1; t++) {
    if (tid == 0) { ox[t] = c; S[c] = __builtin_nan(""); }
    __syncthreads();
    double bs = inf; int bj = 0x7fffffff;
    const double* row = W + (size_t)c * ld;
    for (int j0 = 4 * tid; j0 < N; j0 += 4 * nthr) {
      const double2 a = *reinterpret_cast<const double2*>(row + j0), b = *reinterpret_cast<const double2*>(row + j0 + 2);
      const double2 s0 = *reinterpret_cast<const double2*>(S + j0), s1 = *reinterpret_cast<const double2*>(S + j0 + 2);
      const double d[4] = {a.x, a.y, b.x, b.y}, s[4] = {s0.x, s0.y, s1.x, s1.y};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        if (s[e] != s[e]) continue;                          // merged, or past the row
        const double m = agglo_min_update(s[e], d[e]);
        if (__double_as_longlong(m) != __double_as_longlong(s[e])) S[j0 + e] = m;
        if (agglo_better(m, j0 + e, bs, bj)) { bs = m; bj = j0 + e; }
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double os = __shfl_xor(bs, m, 64); const int oj = __shfl_xor(bj, m, 64);
      if (agglo_better(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    if (lane == 0) { wred_s[wave] = bs; wred_j[wave] = bj; }
    __syncthreads();
    bs = wred_s[0]; bj = wred_j[0];
    for (int w = 1; w < nwaves; w++) {
      const double os = wred_s[w]; const int oj = wred_j[w];
      if (agglo_better(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    if ((unsigned)bj >= (unsigned)N) { if (tid == 0) flag[0] = 2; return; }   // (cannot happen while nodes remain unmerged)
    if (tid == 0) { oy[t] = bj; od[t] = bs; }
    c = bj;
  }
  if (tid == 0) flag[1] = N - 1;
}

}  // namespace ssg

using namespace ssg;

// the loop's state (8 bytes per slot, rounded up to four slots) inside the 160 KB a workgroup may hold
constexpr size_t AGG_LDS_LIMIT = 160 * 1024;
constexpr size_t AGG_LDS_STATIC = 1024;
extern "C" int ssg_agglo_lds_max_n(void) { return (int)(((AGG_LDS_LIMIT - AGG_LDS_STATIC) / 8) & ~(size_t)3); }

static int agglo_check_matrix(const char* fn, const void* M, const uint16_t* v, int N, int mode) {
  if (!M || N < 2 || mode < 0 || mode > 2 || (mode == 0 && !v) || ((uintptr_t)M & (mode == 2 ? 7 : 1)) || (v && ((uintptr_t)v & 1))) {
    ssg_set_error("%s: bad matrix (M=%p N=%d mode=%d%s); N >= 2, mode 0 needs v, pointers aligned to their element", fn, M, N, mode,
                  (mode == 0 && !v) ? " v=NULL" : "");
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}
static int agglo_check_square(const char* fn, const double* W, int N, int64_t ld) {
  if (!W || ((uintptr_t)W & 31) || N < 2 || ld < N || (ld & 3)) {
    ssg_set_error("%s: the working square must be 32-byte aligned with N >= 2 and a row pitch ld >= N, ld %% 4 == 0 (W=%p N=%d ld=%lld)", fn, (const void*)W, N,
                  (long long)ld);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

extern "C" int ssg_agglo_check(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int64_t* counts, hipStream_t stream) {
  int rc = agglo_check_matrix("ssg_agglo_check", M, v, N, mode); if (rc) return rc;
  if (!counts || ((uintptr_t)counts & 7)) { ssg_set_error("ssg_agglo_check: counts must be two 8-byte aligned int64 words, got %p", (void*)counts); return SSG_ERR_INVALID; }
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
  SSG_HIP(hipMemsetAsync(counts, 0, 16, stream));
#define SSG_AC(MD) hipLaunchKernelGGL(agglo_check_kernel<MD>, dim3(stream_grid(N)), dim3(256), 0, stream, mv, (unsigned long long*)counts)
  if (mode == 0) SSG_AC(0); else if (mode == 1) SSG_AC(1); else SSG_AC(2);
#undef SSG_AC
  SSG_LAUNCH_CHECK("agglo_check_kernel");
  return SSG_OK;
}

extern "C" int ssg_agglo_expand(const void* M, const uint16_t* v, int N, int mode, double lambda_value, double* W, int64_t ld, hipStream_t stream) {
  int rc = agglo_check_matrix("ssg_agglo_expand", M, v, N, mode); if (rc) return rc;
  rc = agglo_check_square("ssg_agglo_expand", W, N, ld); if (rc) return rc;
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
  const int T = (N + AGG_TILE - 1) / AGG_TILE;
#define SSG_AE(MD) hipLaunchKernelGGL(agglo_expand_kernel<MD>, dim3(T, T), dim3(256), 0, stream, mv, W, (size_t)ld)
  if (mode == 0) SSG_AE(0); else if (mode == 1) SSG_AE(1); else SSG_AE(2);
#undef SSG_AE
  SSG_LAUNCH_CHECK("agglo_expand_kernel");
  return SSG_OK;
}

extern "C" int ssg_agglo_nn_chain(double* W, int N, int64_t ld, int method, int state, const int64_t* counts, void* ws, size_t ws_bytes, int64_t* x, int64_t* y,
                                  double* distance, int64_t* size, int64_t* flag, hipStream_t stream) {
  int rc = agglo_check_square("ssg_agglo_nn_chain", W, N, ld); if (rc) return rc;
  if (method < 0 || method > 2) { ssg_set_error("ssg_agglo_nn_chain: method=%d must be 0 (average), 1 (complete) or 2 (single)", method); return SSG_ERR_INVALID; }
  if (!counts || !x || !y || !distance || !flag || (method != 2 && !size)) { ssg_set_error("ssg_agglo_nn_chain: null counts / x / y / distance / size / flag"); return SSG_ERR_INVALID; }
  if (((uintptr_t)counts & 7) || ((uintptr_t)x & 7) || ((uintptr_t)y & 7) || ((uintptr_t)distance & 7) || ((uintptr_t)size & 7) || ((uintptr_t)flag & 7)) {
    ssg_set_error("ssg_agglo_nn_chain: counts / x / y / distance / size / flag must be 8-byte aligned"); return SSG_ERR_INVALID;
  }
  if (state < 0 || state > 2) { ssg_set_error("ssg_agglo_nn_chain: state=%d must be 0 (auto), 1 (LDS) or 2 (global)", state); return SSG_ERR_INVALID; }
  const bool fits = N <= ssg_agglo_lds_max_n();
  if (state == 1 && !fits) { ssg_set_error("ssg_agglo_nn_chain: state=1 (LDS) holds at most N=%d slots, got N=%d", ssg_agglo_lds_max_n(), N); return SSG_ERR_INVALID; }
  const bool lds = state == 1 || (state == 0 && fits);
  const size_t n4 = ((size_t)N + 3) & ~(size_t)3, need = n4 * 8;
  if (!lds && (!ws || ws_bytes < need || ((uintptr_t)ws & 15))) {
    ssg_set_error("ssg_agglo_nn_chain: the global state needs a 16-byte aligned workspace of %zu bytes, got %zu", need, ws ? ws_bytes : (size_t)0);
    return SSG_ERR_INVALID;
  }
  const int pieces = (N + 255) / 256;
  const int waves = pieces > AGG_MAX_WAVES ? AGG_MAX_WAVES : pieces;
  const size_t dyn = lds ? need : 0;
  SSG_HIP(hipMemsetAsync(flag, 0, 16, stream));
#define SSG_AN(KERNEL, ...) do { \
    if (dyn > 48 * 1024) SSG_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn)); \
    hipLaunchKernelGGL(KERNEL, dim3(1), dim3(64 * waves), dyn, stream, __VA_ARGS__); \
  } while (0)
  if (method == 2) {
    if (lds) SSG_AN((agglo_single_kernel<true>), W, N, (size_t)ld, counts, (double*)ws, x, y, distance, flag);
    else SSG_AN((agglo_single_kernel<false>), W, N, (size_t)ld, counts, (double*)ws, x, y, distance, flag);
  } else if (method == 1) {
    if (lds) SSG_AN((agglo_nn_chain_kernel<1, true>), W, N, (size_t)ld, counts, (int*)ws, x, y, distance, size, flag);
    else SSG_AN((agglo_nn_chain_kernel<1, false>), W, N, (size_t)ld, counts, (int*)ws, x, y, distance, size, flag);
  } else {
    if (lds) SSG_AN((agglo_nn_chain_kernel<0, true>), W, N, (size_t)ld, counts, (int*)ws, x, y, distance, size, flag);
    else SSG_AN((agglo_nn_chain_kernel<0, false>), W, N, (size_t)ld, counts, (int*)ws, x, y, distance, size, flag);
  }
#undef SSG_AN
  SSG_LAUNCH_CHECK("agglo_nn_chain_kernel");
  return SSG_OK;
}
