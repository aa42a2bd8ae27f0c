// triplet_loss.hip -- the mining and hinge of the fine-tune phase's TripletLoss (reid/loss/triplet.py:32-77) on the GPU.
//
// The reference mines with Python loops of boolean indexing (one blocking nonzero per anchor) and small torch ops.  Here:
//   forward:  one workgroup per anchor reads its row of the distance matrix (sq at the Gram kernel's pitch, clamped and square-rooted
//             on the fly with the expression of clamp_sqrt_kernel, or a finished dist), finds the hardest negative (and in
//             hardest-pair mode the hardest positive) with its tie count, and writes the pairs in the reference's append order;
//             [w branch: one thread per pair counts the hinge terms it takes part in;] one workgroup reduces the hinge terms in a fixed
//             order into loss and prec.  No float atomics, no host reads.
//   backward: d loss / d dist[a,c] is rebuilt per element from that record: the coefficients of the pairs that hit (a, c), ties of a
//             min / max sharing evenly like torch's min() / max() backward, a hinge term passing the gradient where its input is >= 0
//             (clamp_min).  Either written densely (from-dist entry points) or folded into S = W + W^T, W = G / dist where the clamp
//             passes the gradient, for the S x GEMM of the feature gradient.
//
// Record layout (floats / ints of one call; A = n anchor slots, M pairs):
//   rec_f: an[A] | ap[A] | dist_ap[M] | dist_an[M] | xh[M] (hinge input -(an - ap) + margin) | wrow[M] (w branch: sum_m hinge(i, m))
//   rec_i: an_cnt[A] | ap_cnt[A] | cnt_ap[M] | cnt_an[M]   (cnt_*: number of hinge terms >= 0 the pair's ap / an takes part in)
#include "ssg_common.h"

namespace ssg {

constexpr int TL_MAX_N = 4096;
constexpr int TL_W_MAX_M = 65536;   // the w branch is M x M hinge terms

struct TlRec {
  float *an, *ap, *dap, *dan, *xh, *wrow;
  int *an_cnt, *ap_cnt, *cnt_ap, *cnt_an;
};

__host__ __device__ __forceinline__ TlRec tl_rec(float* f, int* i, int n, int M) {
  TlRec r;
  r.an = f; r.ap = f + n; r.dap = f + 2 * n; r.dan = r.dap + M; r.xh = r.dan + M; r.wrow = r.xh + M;
  r.an_cnt = i; r.ap_cnt = i + n; r.cnt_ap = i + 2 * n; r.cnt_an = r.cnt_ap + M;
  return r;
}

// dist[a, c] as pairwise_dist(x) holds it: sqrt(clamp(sq, min = lo)) (clamp_sqrt_kernel's expression), or the given matrix
__device__ __forceinline__ float tl_dist(const float* __restrict__ in, int ld, int is_sq, float lo, int a, int c) {
  const float v = in[(int64_t)a * ld + c];
  return is_sq ? sqrtf(v < lo ? lo : v) : v;
}

// first pair index of anchor a = i*K + j in the semi branch's append order (triplet.py:50-57)
__device__ __forceinline__ int tl_pair_base(int a, int K) {
  const int i = a / K, j = a - i * K;
  return i * (K * (K - 1) / 2) + j * (K - 1) - j * (j - 1) / 2;
}

// hinge input of MarginRankingLoss with y = 1: -(an - ap) + margin, rounded like torch
__device__ __forceinline__ float tl_hinge_in(float an, float ap, float margin) {
  const float t = an - ap;
  return -t + margin;
}

// (value, tie count) of a min (SIGN = 1) or max (SIGN = -1); NaN never wins, an empty set has count 0
template <int SIGN>
__device__ __forceinline__ void tl_merge(float& v, int& c, float ov, int oc) {
  if (oc == 0) return;
  if (c == 0 || (SIGN > 0 ? ov < v : ov > v)) { v = ov; c = oc; }
  else if (ov == v) c += oc;
}

// one workgroup (256 threads) per anchor row a
__global__ __launch_bounds__(256) void triplet_mine_kernel(const float* __restrict__ in, int ld, int is_sq, float lo, const int64_t* __restrict__ tg,
                                                           int n, int K, int semi, float margin, int weighted, float* __restrict__ rf,
                                                           int* __restrict__ ri, int M) {
  __shared__ float s_v[2][4];
  __shared__ int s_c[2][4];
  const TlRec r = tl_rec(rf, ri, n, M);
  const int a = (int)blockIdx.x, tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const int64_t la = tg[a];
  float nv = 0.f, pv = 0.f;
  int nc = 0, pc = 0;
  for (int c = tid; c < n; c += 256) {
    const float v = tl_dist(in, ld, is_sq, lo, a, c);
    if (v != v) continue;
    if (tg[c] != la) tl_merge<1>(nv, nc, v, 1);
    else if (!semi) tl_merge<-1>(pv, pc, v, 1);
  }
  for (int sh = 1; sh < 64; sh <<= 1) {
    const float onv = __shfl_xor(nv, sh, 64), opv = __shfl_xor(pv, sh, 64);
    const int onc = __shfl_xor(nc, sh, 64), opc = __shfl_xor(pc, sh, 64);
    tl_merge<1>(nv, nc, onv, onc);
    tl_merge<-1>(pv, pc, opv, opc);
  }
  if (lane == 0) { s_v[0][wave] = nv; s_c[0][wave] = nc; s_v[1][wave] = pv; s_c[1][wave] = pc; }
  __syncthreads();
  nv = s_v[0][0]; nc = s_c[0][0]; pv = s_v[1][0]; pc = s_c[1][0];
  for (int w = 1; w < 4; w++) { tl_merge<1>(nv, nc, s_v[0][w], s_c[0][w]); tl_merge<-1>(pv, pc, s_v[1][w], s_c[1][w]); }
  const float an = nc ? nv : __int_as_float(0x7fc00000);      // no negative: the reference raises here; NaN, detected without a host read
  if (tid == 0) { r.an[a] = an; r.an_cnt[a] = nc; r.ap[a] = pv; r.ap_cnt[a] = pc; }
  if (semi) {
    const int i = a / K, j = a - i * K, base = tl_pair_base(a, K);
    for (int q = tid; q < K - 1 - j; q += 256) {
      const int m = base + q;
      const float ap = tl_dist(in, ld, is_sq, lo, a, i * K + j + 1 + q);
      const float x = tl_hinge_in(an, ap, margin);
      r.dap[m] = ap; r.dan[m] = an; r.xh[m] = x;
      if (!weighted) { const int g = x >= 0.f ? 1 : 0; r.cnt_ap[m] = g; r.cnt_an[m] = g; }
    }
  } else if (tid == 0) {
    const float x = tl_hinge_in(an, pv, margin);
    r.dap[a] = pv; r.dan[a] = an; r.xh[a] = x;
    if (!weighted) { const int g = x >= 0.f ? 1 : 0; r.cnt_ap[a] = g; r.cnt_an[a] = g; }
  }
}

// w branch (triplet.py:69-73): loss = (1/M) sum_i mean_m clamp_min(-(an_i - ap_m) + margin, 0).  Thread m: the row sum of anchor
// term m and the number of terms >= 0 its an and its ap take part in (sequential, fixed order)
__global__ __launch_bounds__(256) void triplet_weighted_kernel(float* __restrict__ rf, int* __restrict__ ri, int n, int M, float margin) {
  const TlRec r = tl_rec(rf, ri, n, M);
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= M) return;
  const float anm = r.dan[m], apm = r.dap[m];
  double s = 0.0;                                            // float64 sum: M float32 terms, the result rounded once
  int ca = 0, cn = 0;
  for (int k = 0; k < M; k++) {
    const float xr = tl_hinge_in(anm, r.dap[k], margin);     // term (m, k): this an against every ap
    s += xr < 0.f ? 0.0 : (double)xr;
    cn += xr >= 0.f ? 1 : 0;
    const float xc = tl_hinge_in(r.dan[k], apm, margin);     // term (k, m): every an against this ap
    ca += xc >= 0.f ? 1 : 0;
  }
  r.wrow[m] = (float)s; r.cnt_an[m] = cn; r.cnt_ap[m] = ca;
}

// loss and prec, one workgroup of 1024 threads: strided sequential partial sums, then a fixed tree (float64 sums of the float32
// hinge terms, the loss rounded once)
__global__ __launch_bounds__(1024) void triplet_finish_kernel(float* __restrict__ rf, int* __restrict__ ri, int n, int M, int nanchors, int weighted,
                                                              float* __restrict__ loss, float* __restrict__ prec) {
  __shared__ double s_sum[1024];
  __shared__ int s_cnt[1024], s_empty[1024];
  const TlRec r = tl_rec(rf, ri, n, M);
  const int tid = (int)threadIdx.x;
  const float fM = (float)M;
  double s = 0.0;
  int cnt = 0, empty = 0;
  for (int m = tid; m < M; m += 1024) {
    if (weighted) s += (double)r.wrow[m] / (double)M;
    else { const float x = r.xh[m]; s += x < 0.f ? 0.0 : (double)x; }
    cnt += r.dan[m] > r.dap[m] ? 1 : 0;
  }
  for (int a = tid; a < nanchors; a += 1024) empty |= r.an_cnt[a] == 0;
  s_sum[tid] = s; s_cnt[tid] = cnt; s_empty[tid] = empty;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if (tid < h) { s_sum[tid] += s_sum[tid + h]; s_cnt[tid] += s_cnt[tid + h]; s_empty[tid] |= s_empty[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    const float qnan = __int_as_float(0x7fc00000);
    loss[0] = s_empty[0] ? qnan : (float)(s_sum[0] / (double)M);
    prec[0] = s_empty[0] ? qnan : (float)s_cnt[0] / fM;
  }
}

// d (objective) / d dist[a, c] from the record.  Coefficients of a pair's ap / an: count mode (gloss != NULL) s * cnt with
// s = gloss / M (w branch: / M / M) -- the an side negated; otherwise the upstream gradients gap[m] / gan[m] (either may be NULL)
struct TlGrad {
  const float* in; int ld, is_sq; float lo; const int64_t* tg; int n, K, semi, M, weighted;
  const float* rf; const int* ri; const float* gloss; const float* gap; const float* gan;
};

__device__ __forceinline__ float tl_coef(const TlGrad& p, const TlRec& r, float s, int m, bool ap_side) {
  if (p.gloss) return ap_side ? s * (float)r.cnt_ap[m] : -(s * (float)r.cnt_an[m]);
  const float* g = ap_side ? p.gap : p.gan;
  return g ? g[m] : 0.f;
}

__device__ __forceinline__ float tl_grad_elem(const TlGrad& p, const TlRec& r, float s, int a, int c, float dac) {
  const int P = p.n / p.K;
  float acc = 0.f;
  const bool same = p.tg[c] == p.tg[a];
  if (p.semi) {
    if (a >= P * p.K) return 0.f;                  // trailing n % K rows are never anchors
    const int i = a / p.K, j = a - i * p.K, base = tl_pair_base(a, p.K);
    if (c / p.K == i && c - i * p.K > j) acc += tl_coef(p, r, s, base + (c - i * p.K - j - 1), true);       // positional pair
    if (!same && r.an_cnt[a] > 0 && dac == r.an[a]) {
      float g = 0.f;
      for (int q = 0; q < p.K - 1 - j; q++) g += tl_coef(p, r, s, base + q, false);
      acc += g / (float)r.an_cnt[a];
    }
  } else {
    if (same && r.ap_cnt[a] > 0 && dac == r.ap[a]) acc += tl_coef(p, r, s, a, true) / (float)r.ap_cnt[a];
    if (!same && r.an_cnt[a] > 0 && dac == r.an[a]) acc += tl_coef(p, r, s, a, false) / (float)r.an_cnt[a];
  }
  return acc;
}

__device__ __forceinline__ float tl_scale(const TlGrad& p) {
  if (!p.gloss) return 0.f;
  const float fM = (float)p.M, g = p.gloss[0];
  return p.weighted ? (g / fM) / fM : g / fM;
}

// dense d / d dist, one thread per element
__global__ __launch_bounds__(256) void triplet_grad_dist_kernel(TlGrad p, float* __restrict__ gdist) {
  const TlRec r = tl_rec(const_cast<float*>(p.rf), const_cast<int*>(p.ri), p.n, p.M);
  const float s = tl_scale(p);
  const int64_t nn = (int64_t)p.n * p.n;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nn; t += (int64_t)gridDim.x * blockDim.x) {
    const int a = (int)(t / p.n), c = (int)(t - (int64_t)a * p.n);
    gdist[t] = tl_grad_elem(p, r, s, a, c, tl_dist(p.in, p.ld, p.is_sq, p.lo, a, c));
  }
}

// S = W + W^T with row pitch ldS and its row sums (one wave per row i; the lane that owns (i, j) evaluates both directions), like
// triplet_grad_weights_kernel: W[a,c] = sq[a,c] >= lo ? G[a,c] / dist[a,c] : 0, diagonal left out.  Blocks past the S rows write
// xt = x^T [dp][ldS] zero padded (the GEMM's weights) and zeros [dp] (its bias)
__global__ __launch_bounds__(256) void triplet_grad_weights_rec_kernel(TlGrad p, int ldS, float* __restrict__ S, float* __restrict__ rowsum,
                                                                       const float* __restrict__ x, int d, int dp, float* __restrict__ xt,
                                                                       float* __restrict__ zeros, int srow_blocks) {
  if ((int)blockIdx.x >= srow_blocks) {
    const int64_t t = (int64_t)(blockIdx.x - srow_blocks) * blockDim.x + threadIdx.x;
    if (t < dp) zeros[t] = 0.f;
    if (t < (int64_t)dp * ldS) {
      const int c = (int)(t / ldS), row = (int)(t - (int64_t)c * ldS);
      xt[t] = (c < d && row < p.n) ? x[(int64_t)row * d + c] : 0.f;
    }
    return;
  }
  const TlRec r = tl_rec(const_cast<float*>(p.rf), const_cast<int*>(p.ri), p.n, p.M);
  const float s = tl_scale(p);
  const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (i >= p.n) return;
  const int lane = lane_id();
  float acc = 0.f;
  for (int j = lane; j < ldS; j += 64) {
    float v = 0.f;
    if (j < p.n && j != i) {
      const float sij = p.in[(int64_t)i * p.ld + j], sji = p.in[(int64_t)j * p.ld + i];
      const float dij = sqrtf(sij < p.lo ? p.lo : sij), dji = sqrtf(sji < p.lo ? p.lo : sji);
      const float wij = sij >= p.lo ? tl_grad_elem(p, r, s, i, j, dij) / dij : 0.f;
      const float wji = sji >= p.lo ? tl_grad_elem(p, r, s, j, i, dji) / dji : 0.f;
      v = wij + wji;
    }
    S[(int64_t)i * ldS + j] = v;
    acc += v;
  }
  for (int sh = 1; sh < 64; sh <<= 1) acc += __shfl_xor(acc, sh, 64);
  if (lane == 0) rowsum[i] = acc;
}

}  // namespace ssg

using namespace ssg;

static int tl_check(const char* fn, int n, int ld, int is_sq, int K, int semi, int M, int weighted) {
  if (n < 1 || n > TL_MAX_N) { ssg_set_error("%s: n=%d outside [1, %d]", fn, n, TL_MAX_N); return SSG_ERR_INVALID; }
  if (ld < n) { ssg_set_error("%s: row pitch ld=%d < n=%d", fn, ld, n); return SSG_ERR_INVALID; }
  if (is_sq != 0 && is_sq != 1) { ssg_set_error("%s: is_sq=%d must be 0 or 1", fn, is_sq); return SSG_ERR_INVALID; }
  if (semi != 0 && semi != 1) { ssg_set_error("%s: mode semi=%d must be 0 or 1", fn, semi); return SSG_ERR_INVALID; }
  if (weighted != 0 && weighted != 1) { ssg_set_error("%s: weighted=%d must be 0 or 1", fn, weighted); return SSG_ERR_INVALID; }
  if (K < 1) { ssg_set_error("%s: K=%d must be >= 1", fn, K); return SSG_ERR_INVALID; }
  const int P = n / K;
  const int64_t want = semi ? (int64_t)P * K * (K - 1) / 2 : (int64_t)n;
  if (M < 1 || M != want) { ssg_set_error("%s: M=%d, the mining gives %lld pairs (need >= 1)", fn, M, (long long)want); return SSG_ERR_INVALID; }
  if (weighted && M > TL_W_MAX_M) { ssg_set_error("%s: the w branch supports M <= %d (M=%d)", fn, TL_W_MAX_M, M); return SSG_ERR_INVALID; }
  return SSG_OK;
}

extern "C" int ssg_triplet_mine_f32(const float* in, int ld, int is_sq, float lo, const int64_t* targets, int n, int K, int semi, int M,
                                    float margin, int weighted, float* rec_f, int32_t* rec_i, float* loss, float* prec, hipStream_t stream) {
  if (int rc = tl_check("ssg_triplet_mine_f32", n, ld, is_sq, K, semi, M, weighted)) return rc;
  if (!in || !targets || !rec_f || !rec_i || !loss || !prec) { ssg_set_error("ssg_triplet_mine_f32: NULL pointer"); return SSG_ERR_INVALID; }
  const int nanchors = semi ? (n / K) * K : n;
  hipLaunchKernelGGL(triplet_mine_kernel, dim3(nanchors), dim3(256), 0, stream, in, ld, is_sq, lo, targets, n, K, semi, margin, weighted, rec_f,
                     rec_i, M);
  SSG_LAUNCH_CHECK("triplet_mine_kernel");
  if (weighted) {
    hipLaunchKernelGGL(triplet_weighted_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, rec_f, rec_i, n, M, margin);
    SSG_LAUNCH_CHECK("triplet_weighted_kernel");
  }
  hipLaunchKernelGGL(triplet_finish_kernel, dim3(1), dim3(1024), 0, stream, rec_f, rec_i, n, M, nanchors, weighted, loss, prec);
  SSG_LAUNCH_CHECK("triplet_finish_kernel");
  return SSG_OK;
}

extern "C" int ssg_triplet_grad_dist_f32(const float* in, int ld, int is_sq, float lo, const int64_t* targets, int n, int K, int semi, int M,
                                         int weighted, const float* rec_f, const int32_t* rec_i, const float* gloss, const float* gap,
                                         const float* gan, float* gdist, hipStream_t stream) {
  if (int rc = tl_check("ssg_triplet_grad_dist_f32", n, ld, is_sq, K, semi, M, weighted)) return rc;
  if (!in || !targets || !rec_f || !rec_i || !gdist) { ssg_set_error("ssg_triplet_grad_dist_f32: NULL pointer"); return SSG_ERR_INVALID; }
  const TlGrad p = {in, ld, is_sq, lo, targets, n, K, semi, M, weighted, rec_f, rec_i, gloss, gap, gan};
  const int64_t nn = (int64_t)n * n;
  hipLaunchKernelGGL(triplet_grad_dist_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, stream, p, gdist);
  SSG_LAUNCH_CHECK("triplet_grad_dist_kernel");
  return SSG_OK;
}

extern "C" int ssg_triplet_grad_weights_rec(const float* sq, int ldq, float lo, const int64_t* targets, int n, int K, int semi, int M, int weighted,
                                            const float* rec_f, const int32_t* rec_i, const float* gloss, const float* x, int d, int ldS, int dp,
                                            float* S, float* rowsum, float* xt, float* zeros, hipStream_t stream) {
  if (int rc = tl_check("ssg_triplet_grad_weights_rec", n, ldq, 1, K, semi, M, weighted)) return rc;
  if (d < 1 || dp < d || (dp % 64) || ldS < n || (ldS % 32)) {
    ssg_set_error("ssg_triplet_grad_weights_rec: bad shape d=%d dp=%d ldS=%d (dp >= d, dp %% 64 == 0, ldS >= n, ldS %% 32 == 0)", d, dp, ldS);
    return SSG_ERR_INVALID;
  }
  if (!sq || !targets || !rec_f || !rec_i || !gloss || !x || !S || !rowsum || !xt || !zeros) {
    ssg_set_error("ssg_triplet_grad_weights_rec: NULL pointer"); return SSG_ERR_INVALID;
  }
  const TlGrad p = {sq, ldq, 1, lo, targets, n, K, semi, M, weighted, rec_f, rec_i, gloss, nullptr, nullptr};
  const int srow_blocks = (n + 3) / 4;
  const int tblocks = (int)(((int64_t)dp * ldS + 255) / 256);
  hipLaunchKernelGGL(triplet_grad_weights_rec_kernel, dim3(srow_blocks + tblocks), dim3(256), 0, stream, p, ldS, S, rowsum, x, d, dp, xt, zeros,
                     srow_blocks);
  SSG_LAUNCH_CHECK("triplet_grad_weights_rec_kernel");
  return SSG_OK;
}
