// kissme.hip -- KISSME metric learning (reid/metric_learning/kissme.py:33-55): pair enumeration and the two pair-difference
// covariances  C = sum_p (x_a - x_b)(x_a - x_b)^T / divisor  on the FP64 matrix cores.
//
// The reference builds two n x n int64 meshgrids and masks them; here the same pair ORDER (b ascending, a ascending inside b, a < b)
// is addressed through a stable counting sort of the class ids and two int64 scans over b, so a pair is found from its position:
//   matching pairs of row b      : the rank[b] members of b's class that lie below b, positions m_scan[b] ..
//   non-matching pairs of row b  : the b - rank[b] other indices below b,             positions nm_scan[b] ..
// Nothing here depends on the order in which atomics land (the one atomicAdd counts class sizes: integer sums).
//
// Covariance: one workgroup per 128 x 128 output tile on or above the diagonal, walking ALL P pairs in slices of BK = 16 (no split
// of the pair axis, no workspace, no float atomics: the summation order follows from the shape alone).  Rows are gathered as
// float32, widened and subtracted in float64 while the slice is staged into LDS in [pair][column] order (16-double pad per pair:
// the fragment reads lane = column + 16 * pair are bank-conflict free); 8 waves (4 x 2), each 32 x 64 = 2 x 4 tiles of
// v_mfma_f64_16x16x4_f64.  Elements on or above the diagonal are stored and mirrored: C[i][j] and C[j][i] are the same bits.
#include "ssg_common.h"
#include <algorithm>

namespace ssg {
namespace kissme {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int KT = 128, KBK = 16, KLDR = 144;       // output tile edge, pairs per slice, padded columns per pair
constexpr int KMAXN = 1 << 24;

// rank[i] = number of j < i with den[j] == den[i]; counts[den[i]] += 1.  All-pairs compare over LDS tiles of 1024 ids: n = 131 072
// is 8.6e9 compares, a few milliseconds, and the result needs no sort and no per-chunk histogram.
__global__ __launch_bounds__(256) void rank_kernel(const int32_t* __restrict__ den, int n, int G, int32_t* __restrict__ rank,
                                                   int32_t* __restrict__ counts) {
  __shared__ int32_t tile[1024];
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  const int mine = i < n ? den[i] : -1;
  const int last = min((int)(blockIdx.x * 256 + 255), n - 1);       // the block needs ids 0 .. last - 1
  int r = 0;
  for (int j0 = 0; j0 < last; j0 += 1024) {
    __syncthreads();
    for (int t = (int)threadIdx.x; t < 1024; t += 256) tile[t] = j0 + t < n ? den[j0 + t] : -2;
    __syncthreads();
    const int lim = min(1024, i - j0);                               // j < i only
    if (lim >= 1024) {
#pragma unroll 8
      for (int t = 0; t < 1024; t += 4) {
        const int4 v = *reinterpret_cast<const int4*>(tile + t);
        r += (v.x == mine) + (v.y == mine) + (v.z == mine) + (v.w == mine);
      }
    } else {
      for (int t = 0; t < lim; t++) r += tile[t] == mine;
    }
  }
  if (i < n) {
    rank[i] = r;
    if (mine >= 0 && mine < G) atomicAdd(counts + mine, 1);
  }
}

__device__ __forceinline__ int64_t wave_incl_scan(int64_t v) {
  const int lane = lane_id();
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    const int64_t o = __shfl_up((long long)v, sh, 64);
    if (lane >= sh) v += o;
  }
  return v;
}

// block-wide inclusive scan of one value per thread (1024 threads); *total = the block's sum
__device__ __forceinline__ int64_t block_incl_scan(int64_t v, int64_t* wsum, int64_t* total) {
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  v = wave_incl_scan(v);
  __syncthreads();                                   // wsum of the previous trip has been read
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  int64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 16; w++) { const int64_t s = wsum[w]; all += s; if (w < wave) before += s; }
  *total = all;
  return v + before;
}

// one workgroup: counts[G] -> cls_ptr[G+1] (exclusive, in place: counts = cls_ptr + 1), rank[n] -> m_scan[n+1], nm_scan[n+1]
__global__ __launch_bounds__(1024) void scan_kernel(int32_t* __restrict__ cls_ptr, int G, const int32_t* __restrict__ rank, int n,
                                                    int64_t* __restrict__ m_scan, int64_t* __restrict__ nm_scan) {
  __shared__ int64_t wsum[16];
  const int tid = (int)threadIdx.x;
  int64_t carry = 0, total;
  if (tid == 0) cls_ptr[0] = 0;
  for (int g0 = 0; g0 < G; g0 += 1024) {
    const int g = g0 + tid;
    const int64_t v = g < G ? (int64_t)cls_ptr[g + 1] : 0;
    const int64_t s = block_incl_scan(v, wsum, &total);
    if (g < G) cls_ptr[g + 1] = (int32_t)(carry + s);
    carry += total;
  }
  int64_t cm = 0, cn = 0;
  if (tid == 0) { m_scan[0] = 0; nm_scan[0] = 0; }
  for (int b0 = 0; b0 < n; b0 += 1024) {
    const int b = b0 + tid;
    const int64_t r = b < n ? (int64_t)rank[b] : 0;
    const int64_t sm = block_incl_scan(r, wsum, &total);
    if (b < n) m_scan[b + 1] = cm + sm;
    cm += total;
    const int64_t sn = block_incl_scan(b < n ? (int64_t)b - r : 0, wsum, &total);
    if (b < n) nm_scan[b + 1] = cn + sn;
    cn += total;
  }
}

__global__ __launch_bounds__(256) void members_kernel(const int32_t* __restrict__ den, const int32_t* __restrict__ rank,
                                                      const int32_t* __restrict__ cls_ptr, int n, int G, int32_t* __restrict__ members) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  const int g = den[i];
  if (g < 0 || g >= G) return;
  const int64_t at = (int64_t)cls_ptr[g] + rank[i];
  if (at < n) members[at] = i;
}

// slot m_scan[b] + j = (members[cls_ptr[g] + j], b) for j < rank[b]
__global__ __launch_bounds__(256) void match_pairs_kernel(const int32_t* __restrict__ den, const int32_t* __restrict__ rank,
                                                          const int32_t* __restrict__ cls_ptr, const int32_t* __restrict__ members,
                                                          const int64_t* __restrict__ m_scan, int n, int G, int64_t P1,
                                                          int32_t* __restrict__ ia, int32_t* __restrict__ ib) {
  const int b = (int)(blockIdx.x * 256 + threadIdx.x);
  if (b >= n) return;
  const int g = den[b];
  if (g < 0 || g >= G) return;
  const int r = rank[b];
  const int64_t base = m_scan[b];
  const int32_t* L = members + cls_ptr[g];
  for (int j = 0; j < r; j++) {
    if (base + j >= P1) break;
    ia[base + j] = L[j];
    ib[base + j] = b;
  }
}

// position p in the order of the non-matching pairs -> (a, b); positions outside [0, nm_scan[n]) give (-1, -1)
__global__ __launch_bounds__(256) void unrank_kernel(const int64_t* __restrict__ pos, int64_t T, const int32_t* __restrict__ den,
                                                     const int32_t* __restrict__ rank, const int32_t* __restrict__ cls_ptr,
                                                     const int32_t* __restrict__ members, const int64_t* __restrict__ nm_scan, int n, int G,
                                                     int32_t* __restrict__ ia, int32_t* __restrict__ ib) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int64_t p = pos[t];
  int a = -1, b = -1;
  if (p >= 0 && p < nm_scan[n]) {
    int lo = 0, hi = n;                               // the b with nm_scan[b] <= p < nm_scan[b + 1]: first index whose scan exceeds p, minus one
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (nm_scan[mid + 1] > p) hi = mid; else lo = mid + 1; }
    b = lo;
    const int64_t q = p - nm_scan[b];
    const int g = den[b];
    if (g >= 0 && g < G) {
      const int32_t* L = members + cls_ptr[g];
      int jl = 0, jh = rank[b];                       // smallest j with L[j] - j > q (L[j] - j does not decrease); rank[b] when there is none
      while (jl < jh) { const int mid = (jl + jh) >> 1; if ((int64_t)L[mid] - mid > q) jh = mid; else jl = mid + 1; }
      a = (int)(q + jl);
    } else {
      b = -1;
    }
  }
  ia[t] = a;
  ib[t] = b;
}

// C [d, d] = sum_p s_p s_p^T / divisor, s_p = (double) X[ia[p]] - (double) X[ib[p]].  blockIdx.x walks the tiles (tm <= tn) row-major over the
// upper triangle.  Pairs with an index outside [0, n) contribute nothing.
__global__ __launch_bounds__(512) void pairdiff_cov_kernel(const float* __restrict__ X, int n, int64_t ldx, const int32_t* __restrict__ ia,
                                                           const int32_t* __restrict__ ib, int64_t P, int d, double divisor,
                                                           double* __restrict__ C, int T) {
  __shared__ double lds[2 * 2 * KBK * KLDR];          // [stage][row side | column side][pair][column (+ pad)]
  int tm = 0, t = (int)blockIdx.x;
  while (t >= T - tm) { t -= T - tm; tm++; }
  const int tn = tm + t;
  const bool diag = tm == tn;                         // the column side is the row side: staged once
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;            // 8 waves, 4 x 2: each 32 rows x 64 columns of the tile
  // staging map: 32 threads x float4 cover the 128 columns of one pair; the 16 pairs of a slice in one pass
  const int c4 = (tid & 31) * 4, pr = tid >> 5;
  const int ca = tm * KT + c4, cb = tn * KT + c4;
  const bool aok = ca < d, bok = !diag && cb < d;     // d % 4 == 0: a float4 is inside or outside as a whole
  const int cas = aok ? ca : 0, cbs = bok ? cb : 0;   // masked loads still point inside the row

  v4d acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (v4d){0., 0., 0., 0.};

  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra, rb, sa, sb;                              // r*: row side (x_a, x_b) of this thread's pair; s*: column side
#define SSG_KGL(KS)                                                                                  \
  {                                                                                                  \
    const int64_t p_ = (int64_t)(KS) * KBK + pr;                                                     \
    int xa = -1, xb = -1;                                                                            \
    if (p_ < P) { xa = ia[p_]; xb = ib[p_]; }                                                        \
    const bool ok_ = xa >= 0 && xa < n && xb >= 0 && xb < n;                                         \
    const float* xa_ = X + (int64_t)(ok_ ? xa : 0) * ldx; const float* xb_ = X + (int64_t)(ok_ ? xb : 0) * ldx; \
    ra = (ok_ && aok) ? *reinterpret_cast<const float4*>(xa_ + cas) : z4;                            \
    rb = (ok_ && aok) ? *reinterpret_cast<const float4*>(xb_ + cas) : z4;                            \
    sa = (ok_ && bok) ? *reinterpret_cast<const float4*>(xa_ + cbs) : z4;                            \
    sb = (ok_ && bok) ? *reinterpret_cast<const float4*>(xb_ + cbs) : z4;                            \
  }
#define SSG_KDIFF(DST, XA, XB)                                                                       \
  {                                                                                                  \
    (DST)[0] = (double)(XA).x - (double)(XB).x; (DST)[1] = (double)(XA).y - (double)(XB).y;          \
    (DST)[2] = (double)(XA).z - (double)(XB).z; (DST)[3] = (double)(XA).w - (double)(XB).w;          \
  }
#define SSG_KLS(BUF)                                                                                 \
  {                                                                                                  \
    double* As_ = lds + (BUF) * (2 * KBK * KLDR);                                                    \
    double* Bs_ = As_ + KBK * KLDR;                                                                  \
    SSG_KDIFF(As_ + pr * KLDR + c4, ra, rb)                                                          \
    if (!diag) SSG_KDIFF(Bs_ + pr * KLDR + c4, sa, sb)                                               \
  }
  const int64_t nk = (P + KBK - 1) / KBK;
  const int l16 = lane & 15, lk = lane >> 4;
  SSG_KGL(0)
  SSG_KLS(0)
  __syncthreads();
  for (int64_t kt = 0; kt < nk; kt++) {
    if (kt + 1 < nk) SSG_KGL(kt + 1)                  // the next slice's gather latency hides under this slice's MFMAs
    const double* As = lds + (int)(kt & 1) * (2 * KBK * KLDR);
    const double* Bs = diag ? As : As + KBK * KLDR;
    double a[2][2], b[2][4];
#pragma unroll
    for (int i = 0; i < 2; i++) a[0][i] = As[lk * KLDR + wm * 32 + i * 16 + l16];
#pragma unroll
    for (int j = 0; j < 4; j++) b[0][j] = Bs[lk * KLDR + wn * 64 + j * 16 + l16];
#pragma unroll
    for (int kk = 0; kk < KBK / 4; kk++) {
      const int cur = kk & 1, nxt = cur ^ 1;
      if (kk + 1 < KBK / 4) {
        const int k = (kk + 1) * 4 + lk;
#pragma unroll
        for (int i = 0; i < 2; i++) a[nxt][i] = As[k * KLDR + wm * 32 + i * 16 + l16];
#pragma unroll
        for (int j = 0; j < 4; j++) b[nxt][j] = Bs[k * KLDR + wn * 64 + j * 16 + l16];
      }
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) SSG_KLS((int)((kt + 1) & 1))     // the other stage: its readers finished before the previous barrier
    __syncthreads();
  }
#undef SSG_KGL
#undef SSG_KDIFF
#undef SSG_KLS

  // f64 MFMA C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int gi = tm * KT + wm * 32 + i * 16 + lk + 4 * r;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int gj = tn * KT + wn * 64 + j * 16 + l16;
        if (gi < d && gj < d && gj >= gi) {
          const double v = acc[i][j][r] / divisor;
          C[(int64_t)gi * d + gj] = v;
          if (gj != gi) C[(int64_t)gj * d + gi] = v;
        }
      }
    }
}

int check_index(const char* fn, int n, int G) {
  if (n < 1 || n > KMAXN || G < 1 || G > n) {
    ssg_set_error("%s: needs 1 <= n <= %d rows and 1 <= G <= n classes (n=%d G=%d)", fn, KMAXN, n, G);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

}  // namespace kissme
}  // namespace ssg

extern "C" int ssg_kissme_index(const int32_t* den, int n, int G, int32_t* cls_ptr, int32_t* members, int32_t* rank, int64_t* m_scan,
                                int64_t* nm_scan, hipStream_t stream) {
  using namespace ssg::kissme;
  const char* fn = "ssg_kissme_index";
  if (int rc = check_index(fn, n, G)) return rc;
  if (!den || !cls_ptr || !members || !rank || !m_scan || !nm_scan) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  SSG_HIP(hipMemsetAsync(cls_ptr, 0, (size_t)(G + 1) * sizeof(int32_t), stream));
  SSG_HIP(hipMemsetAsync(members, 0xff, (size_t)n * sizeof(int32_t), stream));      // -1 where an id outside [0, G) left a hole
  const int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(rank_kernel, dim3(blocks), dim3(256), 0, stream, den, n, G, rank, cls_ptr + 1);
  SSG_LAUNCH_CHECK("kissme rank_kernel");
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, stream, cls_ptr, G, rank, n, m_scan, nm_scan);
  SSG_LAUNCH_CHECK("kissme scan_kernel");
  hipLaunchKernelGGL(members_kernel, dim3(blocks), dim3(256), 0, stream, den, rank, cls_ptr, n, G, members);
  SSG_LAUNCH_CHECK("kissme members_kernel");
  return SSG_OK;
}

extern "C" int ssg_kissme_match_pairs(const int32_t* den, const int32_t* rank, const int32_t* cls_ptr, const int32_t* members,
                                      const int64_t* m_scan, int n, int G, int64_t P1, int32_t* ia, int32_t* ib, hipStream_t stream) {
  using namespace ssg::kissme;
  const char* fn = "ssg_kissme_match_pairs";
  if (int rc = check_index(fn, n, G)) return rc;
  if (P1 < 1 || P1 > (int64_t)n * (n - 1) / 2) { ssg_set_error("%s: P1=%lld is not a pair count of n=%d rows", fn, (long long)P1, n); return SSG_ERR_INVALID; }
  if (!den || !rank || !cls_ptr || !members || !m_scan || !ia || !ib) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(match_pairs_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, den, rank, cls_ptr, members, m_scan, n, G, P1, ia, ib);
  SSG_LAUNCH_CHECK("kissme match_pairs_kernel");
  return SSG_OK;
}

extern "C" int ssg_kissme_unrank(const int64_t* pos, int64_t T, const int32_t* den, const int32_t* rank, const int32_t* cls_ptr,
                                 const int32_t* members, const int64_t* nm_scan, int n, int G, int32_t* ia, int32_t* ib, hipStream_t stream) {
  using namespace ssg::kissme;
  const char* fn = "ssg_kissme_unrank";
  if (int rc = check_index(fn, n, G)) return rc;
  if (T < 1 || T > ((int64_t)1 << 38)) { ssg_set_error("%s: T=%lld positions", fn, (long long)T); return SSG_ERR_INVALID; }
  if (!pos || !den || !rank || !cls_ptr || !members || !nm_scan || !ia || !ib) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(unrank_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, pos, T, den, rank, cls_ptr, members, nm_scan, n, G, ia, ib);
  SSG_LAUNCH_CHECK("kissme unrank_kernel");
  return SSG_OK;
}

extern "C" int ssg_pairdiff_cov_f64(const float* X, int n, int64_t ldx, const int32_t* ia, const int32_t* ib, int64_t P, int d, double divisor,
                                    double* C, hipStream_t stream) {
  using namespace ssg::kissme;
  const char* fn = "ssg_pairdiff_cov_f64";
  if (n < 1 || n > KMAXN || P < 1 || d < 16 || (d % 16) || d > 16384 || ldx < d || (ldx % 4) || !(divisor > 0.0)) {
    ssg_set_error("%s: needs 1 <= n <= %d rows, P >= 1 pairs, 16 <= d <= 16384 with d %% 16 == 0, a row pitch ldx >= d with ldx %% 4 == 0 and a "
                  "divisor > 0 (n=%d P=%lld d=%d ldx=%lld divisor=%g)", fn, KMAXN, n, (long long)P, d, (long long)ldx, divisor);
    return SSG_ERR_INVALID;
  }
  if (!X || !ia || !ib || !C) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  if ((reinterpret_cast<uintptr_t>(X) & 15) != 0) { ssg_set_error("%s: X must be 16-byte aligned", fn); return SSG_ERR_INVALID; }
  const int T = (d + KT - 1) / KT;
  hipLaunchKernelGGL(pairdiff_cov_kernel, dim3(T * (T + 1) / 2), dim3(512), 0, stream, X, n, ldx, ia, ib, P, d, divisor, C, T);
  SSG_LAUNCH_CHECK("kissme pairdiff_cov_kernel");
  return SSG_OK;
}
