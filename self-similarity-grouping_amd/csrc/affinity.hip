// affinity.hip -- affinity propagation on a precomputed similarity matrix (sklearn 1.7.2 _affinity_propagation, float64), gfx950.
//
// Everything is float64, row-major [N,N], indexed with size_t.  The contract is "the bits of the numpy loop":
//   * every damped update rounds twice (R*d, then + tmp; tmp = x*(1-d) rounded before): contraction is off in this library;
//   * np.sum(tmp, axis=0) adds the rows in ascending order, one running sum per column -> ap_colwalk_kernel keeps exactly that chain
//     (the columns are the only parallelism; spare lanes stage the next rows in LDS so that the chain never waits for HBM);
//   * np.argmax takes the first maximum.
// No float atomics anywhere (the integer ones count histogram bins, the minimum / maximum of order-preserving keys and flags).
//
// One iteration `it` = row kernel [A update of it-1, then R update of it] -> column walk cs(it) -> check(it).  The check computes
// E[k] = (A'[k,k] + R[k,k] > 0) from the diagonals and cs alone (A' = what the next row kernel will store: the same expression, the same
// bits), keeps the [N, convergence_iter] window and applies sklearn's stopping rule; when it fires it writes ctrl[0] = 1 and
// ctrl[1] = it + 1.  Every later kernel reads ctrl: the row kernel right behind the firing check still applies that iteration's A
// update (ctrl[1] == its `it`) and nothing else; all others leave A, R, cs and the window untouched.  The host can therefore queue
// iterations blindly and read ctrl once per chunk.
#include "ssg_common.h"
#include <float.h>

namespace ssg {
namespace ap {

constexpr int ROW_THREADS = 256;
constexpr int CW_BIG_MAX_WGS = 512, CW_SMALL_CFG = 1;      // column walk: tile 0 up to 512 workgroups (N <= 8192), tile 1 above (profiles/affinity_times.txt)
constexpr int SEL_BINS = 8192;                                                              // radix select: 13-bit digits

__device__ __forceinline__ uint64_t key_of(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double unkey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
  return __longlong_as_double((long long)u);
}
__device__ __forceinline__ bool finite64(double x) { return (((uint64_t)__double_as_longlong(x) >> 52) & 0x7ff) != 0x7ff; }

// -tmp of sklearn's availability step for one entry: clip(max(R,0) - cs, 0, inf) off the diagonal, R - cs on it
__device__ __forceinline__ double avail_term(double r, double cs, bool diag) {
  if (diag) return r - cs;
  const double rp = r > 0.0 ? r : 0.0;
  const double x = rp - cs;
  return x > 0.0 ? x : 0.0;
}
// A *= d; A -= tmp * (1 - d)
__device__ __forceinline__ double damp_a(double a, double t, double d, double omd) { return a * d - t * omd; }

struct Top2 { double y1; int i1; double y2; };
__device__ __forceinline__ void top2_push(Top2& t, double v, int k) {
  if (v > t.y1 || (v == t.y1 && k < t.i1)) { t.y2 = t.y1; t.y1 = v; t.i1 = k; }
  else if (v > t.y2) t.y2 = v;
}
__device__ __forceinline__ void top2_merge(Top2& a, const Top2& b) {
  if (b.y1 > a.y1 || (b.y1 == a.y1 && b.i1 < a.i1)) {
    const double l = a.y1;
    a.y1 = b.y1; a.i1 = b.i1; a.y2 = l > b.y2 ? l : b.y2;
  } else if (b.y1 > a.y2) a.y2 = b.y1;
}

// ---- row kernel: A update of iteration it-1 fused with the R update of iteration it; one workgroup per row, 16-byte accesses when N is even
template <int VEC>
__global__ __launch_bounds__(ROW_THREADS) void ap_row_kernel(const double* __restrict__ S, double* __restrict__ A, double* __restrict__ R,
                                                             const double* __restrict__ cs, int N, double d, double omd, int it, int do_r,
                                                             const int64_t* __restrict__ ctrl) {
  const int64_t done = ctrl[0], nit = ctrl[1];
  const bool doA = it > 0 && (!done || nit == (int64_t)it);
  const bool doR = do_r && !done;
  if (!doA && !doR) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)i * (size_t)N;
  Top2 t = {-INFINITY, 0x7fffffff, -INFINITY};
  for (int k = tid * VEC; k < N; k += ROW_THREADS * VEC) {
    double a[VEC], s[VEC], r[VEC], c[VEC];
    if (VEC == 2) {
      const double2 av = *reinterpret_cast<const double2*>(A + base + k);
      a[0] = av.x; a[VEC - 1] = av.y;
      if (doR) { const double2 sv = *reinterpret_cast<const double2*>(S + base + k); s[0] = sv.x; s[VEC - 1] = sv.y; }
      if (doA) {
        const double2 rv = *reinterpret_cast<const double2*>(R + base + k);
        const double2 cv = *reinterpret_cast<const double2*>(cs + k);
        r[0] = rv.x; r[VEC - 1] = rv.y; c[0] = cv.x; c[VEC - 1] = cv.y;
      }
    } else {
      a[0] = A[base + k];
      if (doR) s[0] = S[base + k];
      if (doA) { r[0] = R[base + k]; c[0] = cs[k]; }
    }
    if (doA) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) a[v] = damp_a(a[v], avail_term(r[v], c[v], k + v == i), d, omd);
      if (VEC == 2) *reinterpret_cast<double2*>(A + base + k) = make_double2(a[0], a[VEC - 1]);
      else A[base + k] = a[0];
    }
    if (doR) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) top2_push(t, a[v] + s[v], k + v);
    }
  }
  if (!doR) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Top2 b;
    b.y1 = __shfl_xor(t.y1, o); b.i1 = __shfl_xor(t.i1, o); b.y2 = __shfl_xor(t.y2, o);
    top2_merge(t, b);
  }
  __shared__ Top2 s_t[ROW_THREADS / 64];
  if ((tid & 63) == 0) s_t[tid >> 6] = t;
  __syncthreads();
  t = s_t[0];
#pragma unroll
  for (int w = 1; w < ROW_THREADS / 64; ++w) top2_merge(t, s_t[w]);
  const double Y = t.y1, Y2 = t.y2;
  const int I = t.i1;
  // R *= d; R += (S - Y) * (1 - d), with Y2 at the argmax
  for (int k = tid * VEC; k < N; k += ROW_THREADS * VEC) {
    if (VEC == 2) {
      double2 rv = *reinterpret_cast<const double2*>(R + base + k);
      const double2 sv = *reinterpret_cast<const double2*>(S + base + k);
      rv.x = rv.x * d + (sv.x - (k == I ? Y2 : Y)) * omd;
      rv.y = rv.y * d + (sv.y - (k + 1 == I ? Y2 : Y)) * omd;
      *reinterpret_cast<double2*>(R + base + k) = rv;
    } else {
      R[base + k] = R[base + k] * d + (S[base + k] - (k == I ? Y2 : Y)) * omd;
    }
  }
}

// ---- column walk: out[j] = sum over i ascending of f(M[i,j]), ONE running sum per column.
// MODE 0: f = max(R,0) off the diagonal, R on it (sklearn's Rp); skipped once ctrl[0] is set.
// MODE 1: f = S[i,j] where cl[i] == cl[j], nothing otherwise (the exemplar refinement's np.sum(S[ii][:, ii], axis=0) for every cluster at once).
// One adder wave + CW_COLS x CW_LANES loader threads.  The adder wave (its first CW_COLS lanes) adds the CW_ROWS staged rows of tile t from
// LDS in order and does nothing else, so the chain never waits for memory; meanwhile the loaders write tile t+1 (loaded one period
// earlier, CW_UNROLL independent loads per thread) into the other LDS buffer and issue the loads of tile t+2.  One barrier per tile.
// Tiles (columns, row lanes, rows per lane): few workgroups want many loaders each (16 x 32 x 4), many workgroups want fewer threads in
// the same 32 KB of LDS so that more of them are resident (16 x 16 x 8); ssg_ap_colsum_cfg_f64 picks one by index (tools/time_affinity.py --sweep), -1 = by the number of workgroups.
template <int MODE, int CW_COLS, int CW_LANES, int CW_UNROLL>
__global__ __launch_bounds__(64 + CW_COLS * CW_LANES) void ap_colwalk_kernel(const double* __restrict__ M, int N, const int32_t* __restrict__ cl,
                                                                             double* __restrict__ out, const int64_t* __restrict__ ctrl) {
  constexpr int CW_ROWS = CW_LANES * CW_UNROLL;
  static_assert((CW_COLS & (CW_COLS - 1)) == 0 && CW_COLS <= 64 && 64 + CW_COLS * CW_LANES <= 1024 && 2 * CW_ROWS * CW_COLS * 8 <= 65536, "column walk tile");
  if (MODE == 0 && ctrl[0]) return;
  __shared__ double buf[2][CW_ROWS][CW_COLS];
  const bool adder = threadIdx.x < 64;
  const int lt = adder ? (int)threadIdx.x : (int)threadIdx.x - 64;
  const int c = lt & (CW_COLS - 1), r = lt / CW_COLS;      // (adder wave: r == 0 marks the lanes that own a column)
  const int col = blockIdx.x * CW_COLS + c;
  const bool cok = col < N;
  const int mycl = (MODE == 1 && cok && !adder) ? cl[col] : 0;
  const int ntiles = (N + CW_ROWS - 1) / CW_ROWS;
  double v[CW_UNROLL];
  auto load = [&](int tile) {
#pragma unroll
    for (int u = 0; u < CW_UNROLL; ++u) {
      const int i = tile * CW_ROWS + u * CW_LANES + r;
      double x = 0.0;
      if (cok && i < N) {
        x = M[(size_t)i * (size_t)N + (size_t)col];
        if (MODE == 0) { if (i != col) x = x > 0.0 ? x : 0.0; }
        else if (cl[i] != mycl) x = 0.0;
      }
      v[u] = x;
    }
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int u = 0; u < CW_UNROLL; ++u) buf[b][u * CW_LANES + r][c] = v[u];
  };
  if (!adder) {
    load(0);
    stash(0);
    if (ntiles > 1) load(1);
  }
  __syncthreads();
  double s = -0.0;      // the identity of +: the sum starts from the first row's value, as numpy's reduction does
  for (int tile = 0; tile < ntiles; ++tile) {
    if (adder) {
      if (r == 0) {
        const int nr = min(CW_ROWS, N - tile * CW_ROWS);
        const int b = tile & 1;
        if (nr == CW_ROWS) {
#pragma unroll
          for (int q = 0; q < CW_ROWS; ++q) s += buf[b][q][c];
        } else {
          for (int q = 0; q < nr; ++q) s += buf[b][q][c];
        }
      }
    } else {
      if (tile + 1 < ntiles) stash((tile + 1) & 1);
      if (tile + 2 < ntiles) load(tile + 2);
    }
    __syncthreads();
  }
  if (adder && r == 0 && cok) out[col] = s;
}

// ---- convergence: E, the window, sklearn's stopping rule.  One workgroup.
__global__ __launch_bounds__(1024) void ap_check_kernel(const double* __restrict__ A, const double* __restrict__ R, const double* __restrict__ cs,
                                                        int N, double d, double omd, int it, int ci, uint8_t* __restrict__ window,
                                                        uint8_t* __restrict__ E, int64_t* __restrict__ ctrl) {
  if (ctrl[0]) return;
  __shared__ int s_bad, s_K;
  if (threadIdx.x == 0) { s_bad = 0; s_K = 0; }
  __syncthreads();
  int bad = 0, K = 0;
  const int slot = it % ci;
  for (int k = threadIdx.x; k < N; k += 1024) {
    const size_t dg = (size_t)k * (size_t)N + (size_t)k;
    const double r = R[dg];
    const double a = damp_a(A[dg], avail_term(r, cs[k], true), d, omd);
    const int e = (a + r) > 0.0;
    E[k] = (uint8_t)e;
    uint8_t* w = window + (size_t)k * (size_t)ci;
    w[slot] = (uint8_t)e;
    K += e;
    if (it >= ci) {
      int se = 0;
      for (int q = 0; q < ci; ++q) se += w[q];
      if (se != ci && se != 0) bad = 1;
    }
  }
  if (bad) atomicOr(&s_bad, 1);
  if (K) atomicAdd(&s_K, K);
  __syncthreads();
  if (threadIdx.x == 0) {
    ctrl[2] = s_K;
    if (it >= ci && !s_bad && s_K > 0) { ctrl[1] = (int64_t)it + 1; ctrl[0] = 1; }
  }
}

// ---- prepare: the finite check and the extrema (device form of _equal_similarities_and_preferences), then preference + noise
// stats: [0] non-finite entries of S, [1]/[2] min / max key off the diagonal, [3]/[4] min / max key of the preference,
//        [5] non-finite preferences, [6] bits of S[0,N-1], [7] bits of preference[0]
__global__ void ap_stats_init_kernel(uint64_t* __restrict__ stats) {
  const int t = threadIdx.x;
  if (t < 8) stats[t] = (t == 1 || t == 3) ? ~0ULL : 0ULL;
}

__global__ __launch_bounds__(256) void ap_stats_kernel(const double* __restrict__ S, int N, const double* __restrict__ pref, int pref_n,
                                                       uint64_t* __restrict__ stats) {
  const size_t total = (size_t)N * (size_t)N;
  uint64_t mn = ~0ULL, mx = 0ULL;
  unsigned bad = 0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const double x = S[e];
    if (!finite64(x)) { ++bad; continue; }
    if (e / (size_t)N == e % (size_t)N) continue;
    const uint64_t k = key_of(x);
    mn = k < mn ? k : mn;
    mx = k > mx ? k : mx;
  }
  uint64_t pmn = ~0ULL, pmx = 0ULL;
  unsigned pbad = 0;
  if (blockIdx.x == 0) {
    for (int e = threadIdx.x; e < pref_n; e += 256) {
      const double x = pref[e];
      if (!finite64(x)) { ++pbad; continue; }
      const uint64_t k = key_of(x);
      pmn = k < pmn ? k : pmn;
      pmx = k > pmx ? k : pmx;
    }
    if (threadIdx.x == 0) {
      stats[6] = (uint64_t)__double_as_longlong(S[(size_t)N - 1]);
      stats[7] = (uint64_t)__double_as_longlong(pref[0]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t a = __shfl_xor(mn, o), b = __shfl_xor(mx, o), pa = __shfl_xor(pmn, o), pb = __shfl_xor(pmx, o);
    mn = a < mn ? a : mn; mx = b > mx ? b : mx; pmn = pa < pmn ? pa : pmn; pmx = pb > pmx ? pb : pmx;
    bad += __shfl_xor(bad, o); pbad += __shfl_xor(pbad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd((unsigned long long*)&stats[0], (unsigned long long)bad);
    if (mn != ~0ULL) atomicMin((unsigned long long*)&stats[1], (unsigned long long)mn);
    if (mx != 0ULL) atomicMax((unsigned long long*)&stats[2], (unsigned long long)mx);
    if (pmn != ~0ULL) atomicMin((unsigned long long*)&stats[3], (unsigned long long)pmn);
    if (pmx != 0ULL) atomicMax((unsigned long long*)&stats[4], (unsigned long long)pmx);
    if (pbad) atomicAdd((unsigned long long*)&stats[5], (unsigned long long)pbad);
  }
}

// S.flat[::N+1] = preference;  S += (eps * S + tiny * 100) * noise  (three roundings, in that order)
__global__ __launch_bounds__(256) void ap_prepare_kernel(double* __restrict__ S, int N, const double* __restrict__ pref, int pref_n,
                                                         const double* __restrict__ noise) {
  const size_t total = (size_t)N * (size_t)N;
  const double tiny100 = DBL_MIN * 100.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t i = e / (size_t)N, j = e % (size_t)N;
    double s = S[e];
    if (i == j) s = pref[pref_n > 1 ? i : 0];
    const double t1 = DBL_EPSILON * s;
    const double t2 = t1 + tiny100;
    const double t3 = t2 * noise[e];
    S[e] = s + t3;
  }
}

// ---- exact median: radix select of two ranks over order-preserving 64-bit keys, 13-bit digits, state on the device
// sel: [0..1] key prefix of rank r, [2..3] rank left inside the prefix; ghist [2][SEL_BINS] (rank 1's table only when the prefixes differ)
__global__ __launch_bounds__(1024) void ap_select_init_kernel(uint64_t* __restrict__ ws, uint64_t r0, uint64_t r1) {
  for (int b = threadIdx.x; b < 2 * SEL_BINS + 4; b += 1024) ws[b] = b == 2 * SEL_BINS + 2 ? r0 : (b == 2 * SEL_BINS + 3 ? r1 : 0ULL);
}

__global__ __launch_bounds__(256) void ap_select_hist_kernel(const double* __restrict__ X, size_t n, int shift, int width,
                                                             const uint64_t* __restrict__ sel, unsigned long long* __restrict__ ghist) {
  __shared__ unsigned s_h[2][SEL_BINS];
  for (int b = threadIdx.x; b < 2 * SEL_BINS; b += 256) (&s_h[0][0])[b] = 0u;
  __syncthreads();
  const int top = shift + width;                         // bits above the digit
  const uint64_t p0 = sel[0], p1 = sel[1];
  const bool same = p0 == p1;
  const uint64_t dm = (1ULL << width) - 1ULL;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const uint64_t k = key_of(X[e]);
    const uint64_t hi = top >= 64 ? 0ULL : (k >> top);
    const unsigned dg = (unsigned)((k >> shift) & dm);
    if (hi == p0) atomicAdd(&s_h[0][dg], 1u);
    if (!same && hi == p1) atomicAdd(&s_h[1][dg], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 2 * SEL_BINS; b += 256) {
    const unsigned c = (&s_h[0][0])[b];
    if (c) atomicAdd(&ghist[b], (unsigned long long)c);
  }
}

__global__ __launch_bounds__(1024) void ap_select_scan_kernel(int width, int last, uint64_t* __restrict__ sel, unsigned long long* __restrict__ ghist,
                                                              double* __restrict__ out) {
  __shared__ unsigned long long s_sum[1024];
  __shared__ uint64_t s_new[4];
  const int tid = threadIdx.x, nb = 1 << width;
  const int per = SEL_BINS / 1024;
  const bool same = sel[0] == sel[1];
  for (int r = 0; r < 2; ++r) {
    const unsigned long long* h = ghist + ((r == 1 && !same) ? SEL_BINS : 0);
    unsigned long long loc[SEL_BINS / 1024], tot = 0;
#pragma unroll
    for (int q = 0; q < per; ++q) { const int b = tid * per + q; loc[q] = b < nb ? h[b] : 0ULL; tot += loc[q]; }
    s_sum[tid] = tot;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const unsigned long long add = tid >= o ? s_sum[tid - o] : 0ULL;
      __syncthreads();
      s_sum[tid] += add;
      __syncthreads();
    }
    const unsigned long long incl = s_sum[tid], excl = incl - tot, want = sel[2 + r];
    if (want >= excl && want < incl) {
      unsigned long long cum = excl;
#pragma unroll
      for (int q = 0; q < per; ++q) {
        if (want >= cum && want < cum + loc[q]) { s_new[r] = (sel[r] << width) | (uint64_t)(tid * per + q); s_new[2 + r] = want - cum; }
        cum += loc[q];
      }
    }
    __syncthreads();
  }
  for (int b = tid; b < 2 * SEL_BINS; b += 1024) ghist[b] = 0ULL;
  if (tid == 0) {
    const bool one = same && sel[2] == sel[3];           // N*N odd: both ranks are the same element
    sel[0] = s_new[0]; sel[1] = s_new[1]; sel[2] = s_new[2]; sel[3] = s_new[3];
    if (last) {
      const double a = unkey(s_new[0]), b = unkey(s_new[1]);
      out[0] = (one || s_new[0] == s_new[1]) ? a : (a + b) / 2.0;
    }
  }
}

// ---- finish
// I = flatnonzero(E) (ascending), ctrl[2] = K.  One workgroup.
__global__ __launch_bounds__(1024) void ap_compact_kernel(const uint8_t* __restrict__ E, int N, int32_t* __restrict__ I, int64_t* __restrict__ ctrl) {
  __shared__ int s_sum[1024];
  const int tid = threadIdx.x;
  const int per = (N + 1023) / 1024;
  const int lo = min(N, tid * per), hi = min(N, lo + per);
  int cnt = 0;
  for (int k = lo; k < hi; ++k) cnt += E[k] != 0;
  s_sum[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int add = tid >= o ? s_sum[tid - o] : 0;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  int pos = s_sum[tid] - cnt;
  for (int k = lo; k < hi; ++k) if (E[k]) I[pos++] = k;
  if (tid == 1023) ctrl[2] = s_sum[1023];
}

// c[i] = argmax_k S[i, I[k]], first maximum.  One wave per row.
__global__ __launch_bounds__(64) void ap_assign_kernel(const double* __restrict__ S, int N, const int32_t* __restrict__ I, const int64_t* __restrict__ ctrl,
                                                       int32_t* __restrict__ c) {
  const int K = (int)ctrl[2];
  if (K <= 0) return;
  const int i = blockIdx.x;
  const size_t base = (size_t)i * (size_t)N;
  double best = -INFINITY;
  int bk = 0x7fffffff;
  for (int k = threadIdx.x; k < K; k += 64) {
    const double v = S[base + (size_t)I[k]];
    if (v > best || bk == 0x7fffffff) { best = v; bk = k; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int ok = __shfl_xor(bk, o);
    if (ok != 0x7fffffff && (bk == 0x7fffffff || ob > best || (ob == best && ok < bk))) { best = ob; bk = ok; }
  }
  if (threadIdx.x == 0) c[i] = bk;
}

// c[I] = arange(K)
__global__ __launch_bounds__(256) void ap_fix_kernel(const int32_t* __restrict__ I, const int64_t* __restrict__ ctrl, int N, int32_t* __restrict__ c) {
  const int K = (int)ctrl[2];
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < K && k < N) c[I[k]] = k;
}

// I[k] = the member of cluster k with the largest within-cluster similarity sum, lowest member index on ties.  One workgroup per cluster.
__global__ __launch_bounds__(256) void ap_refine_kernel(const double* __restrict__ sums, const int32_t* __restrict__ c, int N,
                                                        const int64_t* __restrict__ ctrl, int32_t* __restrict__ I) {
  const int K = (int)ctrl[2];
  const int k = blockIdx.x;
  if (k >= K) return;
  double best = -INFINITY;
  int bj = 0x7fffffff;
  for (int j = threadIdx.x; j < N; j += 256) {
    if (c[j] != k) continue;
    const double v = sums[j];
    if (bj == 0x7fffffff || v > best) { best = v; bj = j; }
  }
  __shared__ double s_b[4];
  __shared__ int s_j[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int oj = __shfl_xor(bj, o);
    if (oj != 0x7fffffff && (bj == 0x7fffffff || ob > best || (ob == best && oj < bj))) { best = ob; bj = oj; }
  }
  if ((threadIdx.x & 63) == 0) { s_b[threadIdx.x >> 6] = best; s_j[threadIdx.x >> 6] = bj; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      const double ob = s_b[w];
      const int oj = s_j[w];
      if (oj != 0x7fffffff && (bj == 0x7fffffff || ob > best || (ob == best && oj < bj))) { best = ob; bj = oj; }
    }
    if (bj != 0x7fffffff) I[k] = bj;
  }
}

template <int MODE, int C, int L, int U>
static void colwalk_launch(const double* M, int N, const int32_t* cl, double* out, const int64_t* ctrl, hipStream_t st) {
  hipLaunchKernelGGL((ap_colwalk_kernel<MODE, C, L, U>), dim3((N + C - 1) / C), dim3(64 + C * L), 0, st, M, N, cl, out, ctrl);
}

constexpr int CW_CONFIGS = 4;

template <int MODE>
static int colwalk(const double* M, int N, const int32_t* cl, double* out, const int64_t* ctrl, int cfg, hipStream_t st) {
  if (cfg < 0) cfg = (N + 15) / 16 <= CW_BIG_MAX_WGS ? 0 : CW_SMALL_CFG;
  switch (cfg) {
    case 0: colwalk_launch<MODE, 16, 32, 4>(M, N, cl, out, ctrl, st); break;
    case 1: colwalk_launch<MODE, 16, 16, 8>(M, N, cl, out, ctrl, st); break;
    case 2: colwalk_launch<MODE, 16, 32, 8>(M, N, cl, out, ctrl, st); break;
    case 3: colwalk_launch<MODE, 32, 16, 4>(M, N, cl, out, ctrl, st); break;
    default: ssg_set_error("column walk: tile index %d outside [0, %d)", cfg, CW_CONFIGS); return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

static int check_n(const char* what, int N) {
  if (N < 1) { ssg_set_error("%s: N must be >= 1, got %d", what, N); return SSG_ERR_INVALID; }
  return SSG_OK;
}

static unsigned stream_grid(size_t total) {
  const size_t want = (total + 256 * 8 - 1) / (256 * 8);
  return (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
}

}  // namespace ap
}  // namespace ssg

extern "C" {

size_t ssg_ap_median_workspace_bytes(void) { return (2 * (size_t)ssg::ap::SEL_BINS + 4) * sizeof(uint64_t); }

int ssg_ap_median_f64(const double* X, int64_t n, void* ws, size_t ws_bytes, double* out, hipStream_t stream) {
  using namespace ssg::ap;
  if (!X || !ws || !out || n < 1) { ssg_set_error("ssg_ap_median_f64: NULL pointer or n < 1"); return SSG_ERR_INVALID; }
  if (ws_bytes < ssg_ap_median_workspace_bytes()) { ssg_set_error("ssg_ap_median_f64: workspace too small"); return SSG_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* ghist = (unsigned long long*)ws;
  uint64_t* sel = (uint64_t*)ws + 2 * SEL_BINS;
  // the two middle order statistics (equal when n is odd)
  hipLaunchKernelGGL(ap_select_init_kernel, dim3(1), dim3(1024), 0, st, (uint64_t*)ws, (uint64_t)((n - 1) / 2), (uint64_t)(n / 2));
  static const int levels[5][2] = {{51, 13}, {38, 13}, {25, 13}, {12, 13}, {0, 12}};
  for (int l = 0; l < 5; ++l) {
    hipLaunchKernelGGL(ap_select_hist_kernel, dim3(stream_grid((size_t)n)), dim3(256), 0, st, X, (size_t)n, levels[l][0], levels[l][1], sel, ghist);
    hipLaunchKernelGGL(ap_select_scan_kernel, dim3(1), dim3(1024), 0, st, levels[l][1], l == 4 ? 1 : 0, sel, ghist, out);
  }
  SSG_LAUNCH_CHECK("ssg_ap_median_f64");
  return SSG_OK;
}

int ssg_ap_stats_f64(const double* S, int N, const double* pref, int pref_n, int64_t* stats, hipStream_t stream) {
  using namespace ssg::ap;
  if (int rc = check_n("ssg_ap_stats_f64", N)) return rc;
  if (!S || !pref || !stats || (pref_n != 1 && pref_n != N)) { ssg_set_error("ssg_ap_stats_f64: NULL pointer or preference of the wrong length"); return SSG_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ap_stats_init_kernel, dim3(1), dim3(64), 0, st, (uint64_t*)stats);
  hipLaunchKernelGGL(ap_stats_kernel, dim3(stream_grid((size_t)N * N)), dim3(256), 0, st, S, N, pref, pref_n, (uint64_t*)stats);
  SSG_LAUNCH_CHECK("ssg_ap_stats_f64");
  return SSG_OK;
}

int ssg_ap_prepare_f64(double* S, int N, const double* pref, int pref_n, const double* noise, hipStream_t stream) {
  using namespace ssg::ap;
  if (int rc = check_n("ssg_ap_prepare_f64", N)) return rc;
  if (!S || !pref || !noise || (pref_n != 1 && pref_n != N)) { ssg_set_error("ssg_ap_prepare_f64: NULL pointer or preference of the wrong length"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(ap_prepare_kernel, dim3(stream_grid((size_t)N * N)), dim3(256), 0, (hipStream_t)stream, S, N, pref, pref_n, noise);
  SSG_LAUNCH_CHECK("ssg_ap_prepare_f64");
  return SSG_OK;
}

int ssg_ap_row_f64(const double* S, double* A, double* R, const double* cs, int N, double damping, int it, int do_r, const int64_t* ctrl,
                   hipStream_t stream) {
  using namespace ssg::ap;
  if (int rc = check_n("ssg_ap_row_f64", N)) return rc;
  if (!S || !A || !R || !cs || !ctrl || it < 0) { ssg_set_error("ssg_ap_row_f64: NULL pointer or negative iteration"); return SSG_ERR_INVALID; }
  const double omd = 1.0 - damping;
  if (N % 2 == 0 && (((uintptr_t)S | (uintptr_t)A | (uintptr_t)R | (uintptr_t)cs) & 15) == 0)
    hipLaunchKernelGGL(ap_row_kernel<2>, dim3(N), dim3(ROW_THREADS), 0, (hipStream_t)stream, S, A, R, cs, N, damping, omd, it, do_r, ctrl);
  else
    hipLaunchKernelGGL(ap_row_kernel<1>, dim3(N), dim3(ROW_THREADS), 0, (hipStream_t)stream, S, A, R, cs, N, damping, omd, it, do_r, ctrl);
  SSG_LAUNCH_CHECK("ssg_ap_row_f64");
  return SSG_OK;
}

int ssg_ap_colsum_cfg_f64(const double* R, int N, double* cs, const int64_t* ctrl, int cfg, hipStream_t stream) {
  using namespace ssg::ap;
  if (int rc = check_n("ssg_ap_colsum_f64", N)) return rc;
  if (!R || !cs || !ctrl) { ssg_set_error("ssg_ap_colsum_f64: NULL pointer"); return SSG_ERR_INVALID; }
  if (int rc = colwalk<0>(R, N, nullptr, cs, ctrl, cfg, stream)) return rc;
  SSG_LAUNCH_CHECK("ssg_ap_colsum_f64");
  return SSG_OK;
}

int ssg_ap_colsum_f64(const double* R, int N, double* cs, const int64_t* ctrl, hipStream_t stream) {
  return ssg_ap_colsum_cfg_f64(R, N, cs, ctrl, -1, stream);
}

int ssg_ap_colsum_configs(void) { return ssg::ap::CW_CONFIGS; }

int ssg_ap_iterate_f64(const double* S, double* A, double* R, double* cs, uint8_t* window, uint8_t* E, int64_t* ctrl, int N, double damping,
                       int convergence_iter, int it0, int count, hipStream_t stream) {
  using namespace ssg::ap;
  if (int rc = check_n("ssg_ap_iterate_f64", N)) return rc;
  if (!window || !E || !ctrl || convergence_iter < 1 || it0 < 0 || count < 0 || !(damping >= 0.5 && damping < 1.0)) {
    ssg_set_error("ssg_ap_iterate_f64: NULL pointer, convergence_iter < 1, a negative iteration range or damping outside [0.5, 1)");
    return SSG_ERR_INVALID;
  }
  const double omd = 1.0 - damping;
  for (int it = it0; it < it0 + count; ++it) {
    if (int rc = ssg_ap_row_f64(S, A, R, cs, N, damping, it, 1, ctrl, stream)) return rc;
    if (int rc = ssg_ap_colsum_f64(R, N, cs, ctrl, stream)) return rc;
    hipLaunchKernelGGL(ap_check_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, A, R, cs, N, damping, omd, it, convergence_iter, window, E, ctrl);
  }
  SSG_LAUNCH_CHECK("ssg_ap_iterate_f64");
  return SSG_OK;
}

int ssg_ap_finish_f64(const double* S, const uint8_t* E, int N, int32_t* I, int32_t* c, double* sums, int64_t* ctrl, hipStream_t stream) {
  using namespace ssg::ap;
  if (int rc = check_n("ssg_ap_finish_f64", N)) return rc;
  if (!S || !E || !I || !c || !sums || !ctrl) { ssg_set_error("ssg_ap_finish_f64: NULL pointer"); return SSG_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  const dim3 fixg((N + 255) / 256);
  hipLaunchKernelGGL(ap_compact_kernel, dim3(1), dim3(1024), 0, st, E, N, I, ctrl);
  hipLaunchKernelGGL(ap_assign_kernel, dim3(N), dim3(64), 0, st, S, N, I, ctrl, c);
  hipLaunchKernelGGL(ap_fix_kernel, fixg, dim3(256), 0, st, I, ctrl, N, c);
  if (int rc = colwalk<1>(S, N, c, sums, ctrl, -1, st)) return rc;
  hipLaunchKernelGGL(ap_refine_kernel, dim3(N), dim3(256), 0, st, sums, c, N, ctrl, I);
  hipLaunchKernelGGL(ap_assign_kernel, dim3(N), dim3(64), 0, st, S, N, I, ctrl, c);
  hipLaunchKernelGGL(ap_fix_kernel, fixg, dim3(256), 0, st, I, ctrl, N, c);
  SSG_LAUNCH_CHECK("ssg_ap_finish_f64");
  return SSG_OK;
}

}  // extern "C"
