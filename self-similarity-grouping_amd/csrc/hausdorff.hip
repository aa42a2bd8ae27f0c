// hausdorff.hip -- the Hausdorff re-ranking variant (reid/rerank_hausdorff.py:7-65 re_ranking).
//
// After the steps it shares with the other two variants (half original distance :22-41 -- csrc/gram_i8.hip, pairwise.hip; kNN sets
// :43-49 -- csrc/topk.hip, rerank_plain.hip) the reference computes, all in float64:
//   vec[i]  = min_s |tgt_i - src_s|, vec /= max(vec)                                              (:13-15, scipy cdist)
//   H[i,j]  = max( max_{a in S_i} min_{b in S_j} |a - b|, max_{b in S_j} min_{a in S_i} |a - b| )  (:52-58, scipy directed_hausdorff)
//   H      /= max(H);  final = H * (1 - lambda) + (vec[j] + vec[i]) * lambda                       (:60-62)
// Both scipy routines evaluate |a - b| as sqrt(s) with s = 0; for c = 0 .. d-1: t = a[c] - b[c]; s = s + t * t on float64 copies of the
// features, product and sum rounded separately.  That order is kept here (one accumulator per pair, walked c = 0 .. d-1, no fma), so
// every value is the reference's bit for bit -- a matrix-core GEMM form |a|^2 + |b|^2 - 2 a.b is off by ~1e-6.
//
// The Hausdorff rows need no per-pair sub-block.  With E[a,b] = |tgt_a - tgt_b| (all N x N, exactly symmetric) and
//   P_i[b]  = min_{a in S_i} E[a,b]          (column minima of the panel E[S_i, :]: |S_i| contiguous rows, read coalesced)
//   G[i,j]  = max_{b in S_j} P_i[b]          (directed distance S_j -> S_i: |S_j| gathers out of one cached row of N doubles)
// the other direction is max_{a in S_i} min_{b in S_j} E[a,b] = max_{a in S_i} P_j[a] = G[j,i], so H = max(G, G^T): N |S| coalesced
// row reads and N^2 |S| gathers from a row that stays in cache instead of N^2/2 |S|^2 scattered 8-byte loads.  min and max only select,
// so the values do not depend on the order they are taken in.
#include "ssg_common.h"

namespace ssg {

constexpr int HD_T = 64;    // pairs tile edge: 256 threads x (4 x 4) accumulators
constexpr int HD_KC = 32;   // features per LDS strip

__device__ __forceinline__ double hd_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
// non-negative doubles order like their bit patterns: integer atomics give one result whatever order they arrive in
__device__ __forceinline__ void hd_atomic_min(double* p, double v) { atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v)); }
__device__ __forceinline__ void hd_atomic_max(double* p, double v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v)); }

// MODE 0: out[i, j] for an m x n block.  MODE 1: y == x, tiles on or above the diagonal only, mirrored ((a-b)^2 == (b-a)^2 bit for bit).
// MODE 2: out[i] = min(out[i], min_j s[i, j]) over the column tiles of blockIdx.y's slice (out preset to +inf), nothing else is written.
template <int MODE>
__global__ __launch_bounds__(256) void hd_seqdist_kernel(const float* __restrict__ x, int m, const float* __restrict__ y, int n, int d, int take_sqrt,
                                                         double* __restrict__ out, int64_t ld, int tiles_per_slice) {
  __shared__ float xs[HD_KC][HD_T + 1];
  __shared__ float ys[HD_KC][HD_T + 1];
  __shared__ double red[HD_T][17];
  __shared__ double tile[MODE == 1 ? HD_T : 1][HD_T + 1];   // self form: the tile on its way to the mirrored position
  const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int lc = tid & (HD_KC - 1), lr = tid >> 5;      // loader: 32 consecutive features of 8 rows per pass
  int bi, jt0, jt1;
  if (MODE == 2) {
    bi = (int)blockIdx.x;
    jt0 = (int)blockIdx.y * tiles_per_slice;
    const int ntile = (n + HD_T - 1) / HD_T;
    jt1 = jt0 + tiles_per_slice < ntile ? jt0 + tiles_per_slice : ntile;
  } else {
    bi = (int)blockIdx.y; jt0 = (int)blockIdx.x; jt1 = jt0 + 1;
    if (MODE == 1 && jt0 < bi) return;
  }
  const int i0 = bi * HD_T;
  double rmin[4];
#pragma unroll
  for (int r = 0; r < 4; r++) rmin[r] = hd_inf();

  for (int jt = jt0; jt < jt1; jt++) {
    const int j0 = jt * HD_T;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int q = 0; q < 4; q++) acc[r][q] = 0.0;
    for (int c0 = 0; c0 < d; c0 += HD_KC) {
      __syncthreads();
      // a feature past d or a row past the block is staged as 0 in BOTH strips: t = 0 adds +0.0, which changes no sum
      const bool cok = c0 + lc < d;
#pragma unroll
      for (int p = 0; p < HD_T / 8; p++) {
        const int r = lr + 8 * p;
        xs[lc][r] = (cok && i0 + r < m) ? x[(int64_t)(i0 + r) * d + c0 + lc] : 0.f;
        ys[lc][r] = (cok && j0 + r < n) ? y[(int64_t)(j0 + r) * d + c0 + lc] : 0.f;
      }
      __syncthreads();
#pragma unroll 4
      for (int c = 0; c < HD_KC; c++) {
        double xa[4], yb[4];
#pragma unroll
        for (int r = 0; r < 4; r++) { xa[r] = (double)xs[c][ty + 16 * r]; yb[r] = (double)ys[c][tx + 16 * r]; }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const double t = xa[r] - yb[q];
            acc[r][q] = acc[r][q] + t * t;
          }
      }
    }
    if (MODE == 2) {
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (j0 + tx + 16 * q < n) rmin[r] = acc[r][q] < rmin[r] ? acc[r][q] : rmin[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * q;
          if (i < m && j < n) {
            const double v = take_sqrt ? __dsqrt_rn(acc[r][q]) : acc[r][q];
            out[(int64_t)i * ld + j] = v;
            if (MODE == 1) tile[ty + 16 * r][tx + 16 * q] = v;
          }
        }
      if (MODE == 1 && jt0 != bi) {      // the mirror image row by row: lanes walk i, so the stores are as coalesced as the ones above
        __syncthreads();
        const int ci = tid & 63;
        for (int rj = tid >> 6; rj < HD_T; rj += 4)
          if (i0 + ci < m && j0 + rj < n) out[(int64_t)(j0 + rj) * ld + i0 + ci] = tile[ci][rj];
      }
    }
  }
  if (MODE == 2) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) red[ty + 16 * r][tx] = rmin[r];
    __syncthreads();
    if (tid < HD_T && i0 + tid < m) {
      double mn = red[tid][0];
      for (int q = 1; q < 16; q++) mn = red[tid][q] < mn ? red[tid][q] : mn;
      hd_atomic_min(out + i0 + tid, mn);
    }
  }
}

__global__ void hd_fill_kernel(double* p, int n, double v) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) p[i] = v;
}

__device__ __forceinline__ double hd_block_max(double v, double* sh) {
  const int tid = (int)threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int s = (int)blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = sh[tid + s] > sh[tid] ? sh[tid + s] : sh[tid];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// one workgroup: vec = sqrt(rowmin); *vmax = max(vec); vec /= max(vec)   (rerank_hausdorff.py:14-15)
__global__ __launch_bounds__(1024) void hd_source_finish_kernel(const double* __restrict__ rowmin, int N, double* __restrict__ vec, double* __restrict__ vmax) {
  __shared__ double sh[1024];
  double mx = 0.0;
  for (int i = (int)threadIdx.x; i < N; i += 1024) {
    const double v = __dsqrt_rn(rowmin[i]);
    vec[i] = v;
    mx = v > mx ? v : mx;
  }
  mx = hd_block_max(mx, sh);
  for (int i = (int)threadIdx.x; i < N; i += 1024) vec[i] = vec[i] / mx;
  if (threadIdx.x == 0) *vmax = mx;
}

// One workgroup per row i (grid stride): P_i into this workgroup's N doubles of workspace, then G[i, :].
__global__ __launch_bounds__(256) void hd_directed_rows_kernel(const double* __restrict__ E, const int32_t* __restrict__ a_idx, const int32_t* __restrict__ a_nnz,
                                                               int cap, int N, int row0, int nrows, double* __restrict__ ws, double* __restrict__ G) {
  double* P = ws + (int64_t)blockIdx.x * N;
  for (int il = (int)blockIdx.x; il < nrows; il += (int)gridDim.x) {
    const int i = row0 + il;
    const int ni = a_nnz[i] < cap ? a_nnz[i] : cap;
    const int32_t* si = a_idx + (int64_t)i * cap;
    for (int b = (int)threadIdx.x; b < N; b += 256) {
      double mn = hd_inf();
      for (int p = 0; p < ni; p++) {
        const int a = si[p];
        if ((unsigned)a >= (unsigned)N) continue;
        const double e = E[(int64_t)a * N + b];
        mn = e < mn ? e : mn;
      }
      P[b] = mn;
    }
    __syncthreads();
    for (int j = (int)threadIdx.x; j < N; j += 256) {
      const int nj = a_nnz[j] < cap ? a_nnz[j] : cap;
      const int32_t* sj = a_idx + (int64_t)j * cap;
      double mx = 0.0;
      for (int q = 0; q < nj; q++) {
        const int b = sj[q];
        if ((unsigned)b >= (unsigned)N) continue;
        const double e = P[b];
        mx = e > mx ? e : mx;
      }
      G[(int64_t)i * N + j] = j == i ? 0.0 : mx;
    }
    __syncthreads();
  }
}

// H = max(G, G^T) in place, one workgroup per pair of mirrored 32 x 32 tiles; *hmax = max(H) (preset to 0)
__global__ __launch_bounds__(256) void hd_symmetrize_kernel(double* __restrict__ G, int N, double* __restrict__ hmax) {
  const int bi = (int)blockIdx.y, bj = (int)blockIdx.x;
  if (bj < bi) return;
  __shared__ double ta[32][33], tb[32][33], sh[256];
  const int c = (int)threadIdx.x & 31, r0 = (int)threadIdx.x >> 5;
  for (int r = r0; r < 32; r += 8) {
    const int ia = bi * 32 + r, ja = bj * 32 + c, ib = bj * 32 + r, jb = bi * 32 + c;
    ta[r][c] = (ia < N && ja < N) ? G[(int64_t)ia * N + ja] : 0.0;
    tb[r][c] = (ib < N && jb < N) ? G[(int64_t)ib * N + jb] : 0.0;
  }
  __syncthreads();
  double mx = 0.0;
  for (int r = r0; r < 32; r += 8) {
    const int ia = bi * 32 + r, ja = bj * 32 + c, ib = bj * 32 + r, jb = bi * 32 + c;
    if (ia < N && ja < N) {
      const double h = ta[r][c] > tb[c][r] ? ta[r][c] : tb[c][r];
      G[(int64_t)ia * N + ja] = h;
      mx = h > mx ? h : mx;
    }
    if (bi != bj && ib < N && jb < N) G[(int64_t)ib * N + jb] = tb[r][c] > ta[c][r] ? tb[r][c] : ta[c][r];
  }
  mx = hd_block_max(mx, sh);
  if (threadIdx.x == 0) hd_atomic_max(hmax, mx);
}

// final = (H / hmax) * (1 - lambda) + (vec[j] + vec[i]) * lambda, every operation rounded on its own (rerank_hausdorff.py:60-62);
// out may be H itself (each thread reads the entry it overwrites)
__global__ __launch_bounds__(256) void hd_blend_kernel(const double* H, const double* __restrict__ hmax, const double* __restrict__ vec, int N,
                                                       int row0, int nrows, double om, double lam, double* out) {
  const double hm = *hmax;
  const int64_t total = (int64_t)nrows * N;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int il = (int)(e / N), j = (int)(e - (int64_t)il * N);
    const double q = H[e] / hm;
    out[e] = q * om + (vec[j] + vec[row0 + il]) * lam;
  }
}

// euclid = D / max(D) in numpy's half arithmetic (rerank_hausdorff.py:41).  The row maxima are non-negative halves (bit order = value
// order): their maximum is collected once with integer atomics into the four bytes the word *gmax (preset 0).
__global__ __launch_bounds__(256) void hd_half_max_kernel(const uint32_t* __restrict__ rowmax, int N, unsigned* __restrict__ gmax) {
  __shared__ unsigned sh[256];
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  sh[threadIdx.x] = i < N ? rowmax[i] : 0u;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x + s] > sh[threadIdx.x] ? sh[threadIdx.x + s] : sh[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(gmax, sh[0]);
}

__global__ __launch_bounds__(256) void hd_half_normalize_kernel(const hbits* __restrict__ D, const unsigned* __restrict__ gmax, int64_t total,
                                                                hbits* __restrict__ out) {
  const hbits gm = (hbits)*gmax;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) out[e] = h_div(D[e], gm);
}

static int hd_grid(int64_t total) {
  const int64_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

}  // namespace ssg

using namespace ssg;

extern "C" int ssg_seqdist_f64(const float* x, int m, const float* y, int n, int d, int take_sqrt, double* out, int64_t ld, hipStream_t stream) {
  if (m <= 0 || n <= 0 || d <= 0 || ld < n) { ssg_set_error("ssg_seqdist_f64: bad shape m=%d n=%d d=%d ld=%lld", m, n, d, (long long)ld); return SSG_ERR_INVALID; }
  if (!x || !y || !out) { ssg_set_error("ssg_seqdist_f64: null pointer"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(hd_seqdist_kernel<0>, dim3((n + HD_T - 1) / HD_T, (m + HD_T - 1) / HD_T), dim3(256), 0, stream, x, m, y, n, d, take_sqrt, out, ld, 1);
  SSG_LAUNCH_CHECK("hd_seqdist_kernel<0>");
  return SSG_OK;
}

extern "C" int ssg_seqdist_self_f64(const float* x, int n, int d, int take_sqrt, double* out, int64_t ld, hipStream_t stream) {
  if (n <= 0 || d <= 0 || ld < n) { ssg_set_error("ssg_seqdist_self_f64: bad shape n=%d d=%d ld=%lld", n, d, (long long)ld); return SSG_ERR_INVALID; }
  if (!x || !out) { ssg_set_error("ssg_seqdist_self_f64: null pointer"); return SSG_ERR_INVALID; }
  const int t = (n + HD_T - 1) / HD_T;
  hipLaunchKernelGGL(hd_seqdist_kernel<1>, dim3(t, t), dim3(256), 0, stream, x, n, x, n, d, take_sqrt, out, ld, 1);
  SSG_LAUNCH_CHECK("hd_seqdist_kernel<1>");
  return SSG_OK;
}

extern "C" int ssg_seqdist_rowmin_f64(const float* x, int m, const float* y, int n, int d, double* rowmin, hipStream_t stream) {
  if (m <= 0 || n <= 0 || d <= 0) { ssg_set_error("ssg_seqdist_rowmin_f64: bad shape m=%d n=%d d=%d", m, n, d); return SSG_ERR_INVALID; }
  if (!x || !y || !rowmin) { ssg_set_error("ssg_seqdist_rowmin_f64: null pointer"); return SSG_ERR_INVALID; }
  const int mt = (m + HD_T - 1) / HD_T, nt = (n + HD_T - 1) / HD_T;
  int slices = 2048 / mt;                      // enough workgroups for 256 CUs when there are few row tiles
  slices = slices < 1 ? 1 : slices > nt ? nt : slices;
  const int per = (nt + slices - 1) / slices;
  slices = (nt + per - 1) / per;
  hipLaunchKernelGGL(hd_fill_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, rowmin, m, __builtin_inf());
  SSG_LAUNCH_CHECK("hd_fill_kernel");
  hipLaunchKernelGGL(hd_seqdist_kernel<2>, dim3(mt, slices), dim3(256), 0, stream, x, m, y, n, d, 0, rowmin, (int64_t)0, per);
  SSG_LAUNCH_CHECK("hd_seqdist_kernel<2>");
  return SSG_OK;
}

extern "C" int ssg_hausdorff_source_finish(const double* rowmin, int N, double* vec, double* vmax, hipStream_t stream) {
  if (N <= 0) { ssg_set_error("ssg_hausdorff_source_finish: bad shape N=%d", N); return SSG_ERR_INVALID; }
  if (!rowmin || !vec || !vmax) { ssg_set_error("ssg_hausdorff_source_finish: null pointer"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(hd_source_finish_kernel, dim3(1), dim3(1024), 0, stream, rowmin, N, vec, vmax);
  SSG_LAUNCH_CHECK("hd_source_finish_kernel");
  return SSG_OK;
}

static int hd_rows_grid(int nrows) { return nrows < 1024 ? nrows : 1024; }

extern "C" size_t ssg_hausdorff_workspace_bytes(int N, int nrows) {
  if (N <= 0 || nrows <= 0) return 0;
  return (size_t)hd_rows_grid(nrows) * (size_t)N * sizeof(double);
}

extern "C" int ssg_hausdorff_directed_rows(const double* E, const int32_t* a_idx, const int32_t* a_nnz, int cap, int N, int row0, int nrows, double* G,
                                           void* ws, size_t ws_bytes, hipStream_t stream) {
  if (N <= 0 || nrows <= 0 || row0 < 0 || row0 > N - nrows || cap <= 0 || (int64_t)N * N >= (1LL << 31)) {
    ssg_set_error("ssg_hausdorff_directed_rows: bad shape N=%d row0=%d nrows=%d cap=%d (need N * N < 2^31)", N, row0, nrows, cap);
    return SSG_ERR_INVALID;
  }
  if (!E || !a_idx || !a_nnz || !G || !ws) { ssg_set_error("ssg_hausdorff_directed_rows: null pointer"); return SSG_ERR_INVALID; }
  if (ws_bytes < ssg_hausdorff_workspace_bytes(N, nrows)) { ssg_set_error("ssg_hausdorff_directed_rows: workspace too small"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(hd_directed_rows_kernel, dim3(hd_rows_grid(nrows)), dim3(256), 0, stream, E, a_idx, a_nnz, cap, N, row0, nrows, (double*)ws, G);
  SSG_LAUNCH_CHECK("hd_directed_rows_kernel");
  return SSG_OK;
}

extern "C" int ssg_hausdorff_symmetrize(double* G, int N, double* hmax, hipStream_t stream) {
  if (N <= 0 || (int64_t)N * N >= (1LL << 31)) { ssg_set_error("ssg_hausdorff_symmetrize: bad shape N=%d (need N * N < 2^31)", N); return SSG_ERR_INVALID; }
  if (!G || !hmax) { ssg_set_error("ssg_hausdorff_symmetrize: null pointer"); return SSG_ERR_INVALID; }
  SSG_HIP(hipMemsetAsync(hmax, 0, sizeof(double), stream));
  const int t = (N + 31) / 32;
  hipLaunchKernelGGL(hd_symmetrize_kernel, dim3(t, t), dim3(256), 0, stream, G, N, hmax);
  SSG_LAUNCH_CHECK("hd_symmetrize_kernel");
  return SSG_OK;
}

extern "C" int ssg_hausdorff_blend(const double* H, const double* hmax, const double* vec, int N, int row0, int nrows, double one_minus_lambda,
                                   double lambda_value, double* out, hipStream_t stream) {
  if (N <= 0 || nrows <= 0 || row0 < 0 || row0 > N - nrows) { ssg_set_error("ssg_hausdorff_blend: bad shape N=%d row0=%d nrows=%d", N, row0, nrows); return SSG_ERR_INVALID; }
  if (!H || !hmax || !vec || !out) { ssg_set_error("ssg_hausdorff_blend: null pointer"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(hd_blend_kernel, dim3(hd_grid((int64_t)nrows * N)), dim3(256), 0, stream, H, hmax, vec, N, row0, nrows, one_minus_lambda, lambda_value, out);
  SSG_LAUNCH_CHECK("hd_blend_kernel");
  return SSG_OK;
}

extern "C" int ssg_half_div_max(const uint16_t* D, const uint32_t* rowmax, int N, uint16_t* out, uint32_t* gmax, hipStream_t stream) {
  if (N <= 0) { ssg_set_error("ssg_half_div_max: bad shape N=%d", N); return SSG_ERR_INVALID; }
  if (!D || !rowmax || !out || !gmax) { ssg_set_error("ssg_half_div_max: null pointer"); return SSG_ERR_INVALID; }
  SSG_HIP(hipMemsetAsync(gmax, 0, sizeof(uint32_t), stream));
  hipLaunchKernelGGL(hd_half_max_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, rowmax, N, gmax);
  SSG_LAUNCH_CHECK("hd_half_max_kernel");
  hipLaunchKernelGGL(hd_half_normalize_kernel, dim3(hd_grid((int64_t)N * N)), dim3(256), 0, stream, D, gmax, (int64_t)N * N, out);
  SSG_LAUNCH_CHECK("hd_half_normalize_kernel");
  return SSG_OK;
}
