// softmax_ce.hip -- the classification losses of the fine-tune phase (reid/loss/triplet.py:79-106 FocalLoss, weight_cross_entropy.py,
// oim.py, nn.CrossEntropyLoss of eug.py:132) and reid/evaluation_metrics/classification.py's accuracy (gfx950 only).
//
// All four criteria are one family: row-wise log-softmax cross-entropy over logits x [B, C] with a per-row factor.
//
//   forward, one workgroup per row    the row is read from memory once (float4s where the row is 16-byte aligned) and staged in LDS up
//                                     to CE_ROW_CAP floats, the maximum taken on the way in; the float64 sum of exp(x - max) is then
//                                     taken from LDS.  A longer row takes the second route: the same kernel reads the row a second
//                                     time from memory instead of LDS.  lse = max + log(sum), logpt = x[t] - lse,
//                                     s = row_w * class_w[t] * (1 - exp(logpt))^gamma, row loss = -s * logpt
//   forward, one workgroup in all     the batch loss: the float64 row losses (-s * (x[t] - lse), formed again from the kept lse and s)
//                                     and the weights are added in ascending row order by one thread, 256 rows per LDS stage, divided
//                                     as the reduction asks and rounded once; r (1, 1 / B or 1 / sum w) stays on the device
//   backward, 1024 columns per group  dx[i][j] = (g_i * r * s_i) * (exp(x[i][j] - lse_i) - [j == t_i]) in float64, rounded once
//   accuracy                          rank_i = #{j : x[i][j] > x[i][t] or (x[i][j] == x[i][t] and j < t)} per row, then one workgroup
//                                     counts the rows with rank < k for every k (integer counts)
//   OIM table update                  one workgroup per batch row; the workgroup of the first row with a target walks the later rows
//                                     with that target in batch order: v = m lut[y] + (1 - m) x in float64, lut[y] = float32(v / |v|)
//
// Order: a thread owns the quads (4 consecutive columns) q = tid, tid + 256, ... of its row and adds their terms in ascending column
// order; the 256 partial sums are added by a shuffle tree inside each wave and the four waves in ascending order.  Ownership and tree
// depend on C alone -- not on the alignment of the row, not on the route -- so the same logits give the same bits wherever they lie.
// No float atomics, no workspace, no host read.
//
// A target outside [0, C) that is not ignore_index never indexes memory: its row has s = NaN, so its loss, the batch loss and its row of
// dx are NaN; in the weighted mean's denominator it counts with class weight 1, so that the other rows keep finite gradients.
#include "train_common.h"
#include <math.h>

#ifndef SSG_CE_ROW_CAP
#define SSG_CE_ROW_CAP 8192
#endif

namespace ssg {

constexpr int CE_ROW_CAP = SSG_CE_ROW_CAP;        // floats of a row staged in LDS (32 KB)
constexpr int CE_BWD_CHUNK = 1024;                // columns per workgroup of the backward: one float4 per thread
constexpr int TOPK_MAX_K = 8;                     // values of k per ssg_topk_correct_f32 call
static_assert(CE_ROW_CAP % 4 == 0 && CE_ROW_CAP >= 4 && CE_ROW_CAP * 4 <= 48 * 1024, "the staged row is a whole number of float4s in static LDS");

enum { CE_NONE = 0, CE_SUM = 1, CE_MEAN = 2, CE_WMEAN = 3 };

struct TopkKs {
  int k[TOPK_MAX_K];
  int n;
};

// Sum of v over the 256 threads in a fixed order, returned to every thread: lanes by a shuffle tree inside each wave (the lanes whose
// partner is past the wave add their own value, which lane 0 never takes), then the four waves ascending.  sh: 4 doubles of LDS.
__device__ __forceinline__ double ce_block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();                                // sh may still be read from the call before
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Maximum over the 256 threads (fmaxf: a NaN loses here and comes back through exp(NaN - max)).  Its barriers also publish the staged row.
__device__ __forceinline__ float ce_block_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__device__ __forceinline__ int ce_block_count(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// row_w * class_w[t] in float64, an absent weight 1; t < 0 says that the class weight cannot be read (a target out of range)
__device__ __forceinline__ double ce_weight(const float* row_w, const float* class_w, int64_t i, int64_t t) {
  double w = row_w ? (double)row_w[i] : 1.0;
  if (class_w && t >= 0) w = w * (double)class_w[t];
  return w;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void ce_fwd_rows_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ target, int64_t ignore_index,
                                                          const float* __restrict__ row_w, const float* __restrict__ class_w, double gamma, int C, int write_one,
                                                          double* __restrict__ lse_out, double* __restrict__ s_out, double* __restrict__ r_out,
                                                          float* __restrict__ row_loss) {
  __shared__ float4 row4[STAGED ? CE_ROW_CAP / 4 : 1];
  __shared__ double shd[4];
  __shared__ float shf[4];
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  const float* __restrict__ xr = x + i * ldx;
  float* row = reinterpret_cast<float*>(row4);
  const bool vec = ((uintptr_t)xr & 15) == 0;
  const int nq = C >> 2;                          // whole quads; quad nq holds the C & 3 last columns

  // pass 1: the row comes in once, the maximum is taken on the way (a maximum does not depend on the order)
  float mx = -INFINITY;
  if (vec) {
    for (int q = tid; q < nq; q += 256) {
      const float4 v = reinterpret_cast<const float4*>(xr)[q];
      if (STAGED) row4[q] = v;
      mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    for (int e = (nq << 2) + tid; e < C; e += 256) {
      const float v = xr[e];
      if (STAGED) row[e] = v;
      mx = fmaxf(mx, v);
    }
  } else {
    for (int e = tid; e < C; e += 256) {
      const float v = xr[e];
      if (STAGED) row[e] = v;
      mx = fmaxf(mx, v);
    }
  }
  mx = ce_block_max(mx, shf);

  // pass 2: float64 sum of exp(x - max); a thread takes its quads in ascending order, whatever the source
  const double dm = (double)mx;
  double acc = 0.0;
  for (int q = tid; q <= nq; q += 256) {
    const int e0 = q << 2;
    const int cnt = C - e0 < 4 ? C - e0 : 4;      // 4, or the 0..3 columns of the last quad
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (cnt == 4 && (STAGED || vec)) {
      const float4 f = STAGED ? row4[q] : reinterpret_cast<const float4*>(xr)[q];
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
      for (int k = 0; k < cnt; k++) v[k] = STAGED ? row[e0 + k] : xr[e0 + k];
    }
    for (int k = 0; k < cnt; k++) acc += exp((double)v[k] - dm);
  }
  const double sum = ce_block_sum(acc, shd);

  if (tid == 0) {
    const int64_t t = target[i];
    const double lse = dm + log(sum);
    double s, loss;
    if (t == ignore_index) {
      s = 0.0;
      loss = 0.0;
    } else if (t < 0 || t >= (int64_t)C) {        // never used as an index
      s = NAN;
      loss = NAN;
    } else {
      const double logpt = (double)xr[t] - lse;
      const double f = gamma == 0.0 ? 1.0 : pow(1.0 - exp(logpt), gamma);
      s = ce_weight(row_w, class_w, i, t) * f;
      loss = -s * logpt;
    }
    lse_out[i] = lse;
    s_out[i] = s;
    if (row_loss) row_loss[i] = (float)loss;
    if (write_one && i == 0) *r_out = 1.0;        // no batch reduction follows
  }
}

// the batch loss: one workgroup; thread 0 adds in ascending row order what all threads stage 256 rows at a time
__global__ __launch_bounds__(256) void ce_fwd_reduce_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ target, int64_t ignore_index,
                                                            const float* __restrict__ row_w, const float* __restrict__ class_w, const double* __restrict__ lse,
                                                            const double* __restrict__ s, int B, int C, int reduction, float* __restrict__ loss,
                                                            double* __restrict__ r_out) {
  __shared__ double shl[256], shw[256];
  const int tid = threadIdx.x;
  double tot = 0.0, wtot = 0.0;
  for (int base = 0; base < B; base += 256) {
    const int n = B - base < 256 ? B - base : 256;
    double li = 0.0, wi = 0.0;                    // an ignored row adds nothing
    if (tid < n) {
      const int64_t i = (int64_t)base + tid;
      const int64_t t = target[i];
      if (t == ignore_index) {
      } else if (t < 0 || t >= (int64_t)C) {
        li = NAN;
        wi = ce_weight(row_w, class_w, i, -1);
      } else {
        li = -s[i] * ((double)x[i * ldx + t] - lse[i]);
        wi = ce_weight(row_w, class_w, i, t);
      }
    }
    shl[tid] = li;
    shw[tid] = wi;
    __syncthreads();
    if (tid == 0)
      for (int k = 0; k < n; k++) {
        tot += shl[k];
        wtot += shw[k];
      }
    __syncthreads();
  }
  if (tid == 0) {
    const double den = reduction == CE_SUM ? 1.0 : reduction == CE_MEAN ? (double)B : wtot;
    *loss = (float)(reduction == CE_SUM ? tot : tot / den);
    *r_out = 1.0 / den;
  }
}

__device__ __forceinline__ float ce_bwd_element(float v, bool hit, bool ignored, double coef, double lse) {
  return ignored ? 0.f : (float)(coef * (exp((double)v - lse) - (hit ? 1.0 : 0.0)));
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ target, int64_t ignore_index,
                                                     const double* __restrict__ lse, const double* __restrict__ s, const double* __restrict__ r,
                                                     const float* __restrict__ g, int g_stride, float* __restrict__ dx, int64_t lddx, int C, int chunks) {
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x / chunks;
  const int c0 = (int)((int64_t)blockIdx.x % chunks) * CE_BWD_CHUNK;
  const int cnt = C - c0 < CE_BWD_CHUNK ? C - c0 : CE_BWD_CHUNK;
  const int64_t t = target[i];
  const bool ignored = t == ignore_index;
  const double coef = ignored ? 0.0 : ((double)g[i * g_stride] * r[0]) * s[i];
  const double l = lse[i];
  const int64_t tt = t - c0;                      // the target's column inside this chunk, if it is there
  const float* __restrict__ xr = x + i * ldx + c0;
  float* __restrict__ dr = dx + i * lddx + c0;
  int done = 0;
  if ((((uintptr_t)xr | (uintptr_t)dr) & 15) == 0) {
    const int nv = cnt >> 2;                      // at most 256: one float4 per thread
    if (tid < nv) {
      const float4 v = reinterpret_cast<const float4*>(xr)[tid];
      const int e = tid << 2;
      float4 o;
      o.x = ce_bwd_element(v.x, e == tt, ignored, coef, l);
      o.y = ce_bwd_element(v.y, e + 1 == tt, ignored, coef, l);
      o.z = ce_bwd_element(v.z, e + 2 == tt, ignored, coef, l);
      o.w = ce_bwd_element(v.w, e + 3 == tt, ignored, coef, l);
      reinterpret_cast<float4*>(dr)[tid] = o;
    }
    done = nv << 2;
  }
  for (int e = done + tid; e < cnt; e += 256) dr[e] = ce_bwd_element(xr[e], e == tt, ignored, coef, l);
}

// rank of the target's logit in its row, ties to the lower index; C for a target out of range (never correct, never an index)
__global__ __launch_bounds__(256) void topk_rank_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ target, int C,
                                                        int* __restrict__ rank) {
  __shared__ int shi[4];
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int64_t t = target[i];
  if (t < 0 || t >= (int64_t)C) {                 // the whole workgroup takes this branch
    if (tid == 0) rank[i] = C;
    return;
  }
  const float* __restrict__ xr = x + i * ldx;
  const float xt = xr[t];
  const int ti = (int)t;
  int cnt = 0, done = 0;
  if (((uintptr_t)xr & 15) == 0) {
    const int nq = C >> 2;
    for (int q = tid; q < nq; q += 256) {
      const float4 v = reinterpret_cast<const float4*>(xr)[q];
      const int e = q << 2;
      cnt += (v.x > xt || (v.x == xt && e < ti)) + (v.y > xt || (v.y == xt && e + 1 < ti)) + (v.z > xt || (v.z == xt && e + 2 < ti)) +
             (v.w > xt || (v.w == xt && e + 3 < ti));
    }
    done = nq << 2;
  }
  for (int e = done + tid; e < C; e += 256) {
    const float v = xr[e];
    cnt += (v > xt || (v == xt && e < ti));
  }
  cnt = ce_block_count(cnt, shi);
  if (tid == 0) rank[i] = cnt;
}

__global__ __launch_bounds__(256) void topk_count_kernel(const int* __restrict__ rank, int B, const TopkKs ks, float* __restrict__ out) {
  __shared__ int shi[4];
  const int tid = threadIdx.x;
  int c[TOPK_MAX_K];
#pragma unroll
  for (int a = 0; a < TOPK_MAX_K; a++) c[a] = 0;
  for (int i = tid; i < B; i += 256) {
    const int r = rank[i];
#pragma unroll
    for (int a = 0; a < TOPK_MAX_K; a++) c[a] += (a < ks.n && r < ks.k[a]);
  }
  const float inv = (float)(1.0 / (double)B);     // torch's correct_k.mul_(1. / batch_size): a float32 product
#pragma unroll
  for (int a = 0; a < TOPK_MAX_K; a++) {
    const int n = ce_block_count(c[a], shi);
    if (tid == 0 && a < ks.n) out[a] = (float)n * inv;
  }
}

// reid/loss/oim.py:24-26.  The workgroup of batch row b works only when b is the first row with its target; it then applies, in batch
// order, every row with that target.  A thread owns the columns j = tid, tid + 256, ... of the table row in every step, so a step reads
// what the step before wrote without a barrier of its own.
__global__ __launch_bounds__(256) void oim_update_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ target, float* __restrict__ lut,
                                                         int64_t ldl, int B, int C, int F, double m) {
  __shared__ double shd[4];
  __shared__ int shi[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int64_t y = target[b];
  if (y < 0 || y >= (int64_t)C) return;           // the whole workgroup: a target out of range updates nothing
  int seen = 0;
  for (int k = tid; k < b; k += 256) seen += target[k] == y;
  if (ce_block_count(seen, shi) > 0) return;      // the whole workgroup: an earlier row owns this target
  const double om = 1.0 - m;
  float* __restrict__ row = lut + y * ldl;
  for (int k = b; k < B; k++) {
    if (target[k] != y) continue;                 // the whole workgroup
    const float* __restrict__ xr = x + (int64_t)k * ldx;
    double acc = 0.0;
    for (int j = tid; j < F; j += 256) {
      const double v = m * (double)row[j] + om * (double)xr[j];
      acc += v * v;
    }
    const double nrm = sqrt(ce_block_sum(acc, shd));
    for (int j = tid; j < F; j += 256) {
      const double v = m * (double)row[j] + om * (double)xr[j];
      row[j] = (float)(v / nrm);
    }
  }
}

}  // namespace ssg

namespace {

using namespace ssg;

int ce_check_shape(const char* fn, int B, int C, int64_t ldx, const char* ld_name) {
  if (B < 1 || C < 1 || ldx < (int64_t)C) {
    ssg_set_error("%s: need B >= 1, C >= 1 and a row stride %s >= C (B=%d C=%d %s=%lld)", fn, ld_name, B, C, ld_name, (long long)ldx);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_softmax_ce_row_capacity(void) { return CE_ROW_CAP; }
extern "C" int ssg_topk_correct_max_k(void) { return TOPK_MAX_K; }

extern "C" int ssg_softmax_ce_fwd_f32(const float* x, int64_t ldx, const int64_t* target, int64_t ignore_index, const float* row_w, const float* class_w,
                                      double gamma, int reduction, int B, int C, double* lse, double* s, double* r, float* row_loss, float* loss,
                                      hipStream_t stream) {
  const char* fn = "ssg_softmax_ce_fwd_f32";
  if (int rc = ce_check_shape(fn, B, C, ldx, "ldx")) return rc;
  if (reduction < CE_NONE || reduction > CE_WMEAN) {
    ssg_set_error("%s: the reduction code must be 0 (none), 1 (sum), 2 (mean over B) or 3 (weighted mean) (reduction=%d)", fn, reduction);
    return SSG_ERR_INVALID;
  }
  if (!(gamma >= 0.0) || !isfinite(gamma)) { ssg_set_error("%s: gamma must be finite and not negative (gamma=%g)", fn, gamma); return SSG_ERR_INVALID; }
  if (!x || !target || !lse || !s || !r || (reduction != CE_NONE && !loss)) {
    ssg_set_error("%s: NULL pointer (x, target, lse, s and r are needed, and loss unless the reduction is none)", fn);
    return SSG_ERR_INVALID;
  }
  const int one = reduction == CE_NONE;
  if (C <= CE_ROW_CAP)
    hipLaunchKernelGGL(ce_fwd_rows_kernel<true>, dim3(B), dim3(256), 0, stream, x, ldx, target, ignore_index, row_w, class_w, gamma, C, one, lse, s, r, row_loss);
  else
    hipLaunchKernelGGL(ce_fwd_rows_kernel<false>, dim3(B), dim3(256), 0, stream, x, ldx, target, ignore_index, row_w, class_w, gamma, C, one, lse, s, r, row_loss);
  SSG_LAUNCH_CHECK("ce_fwd_rows_kernel");
  if (reduction != CE_NONE) {
    hipLaunchKernelGGL(ce_fwd_reduce_kernel, dim3(1), dim3(256), 0, stream, x, ldx, target, ignore_index, row_w, class_w, lse, s, B, C, reduction, loss, r);
    SSG_LAUNCH_CHECK("ce_fwd_reduce_kernel");
  }
  return SSG_OK;
}

extern "C" int ssg_softmax_ce_bwd_f32(const float* x, int64_t ldx, const int64_t* target, int64_t ignore_index, const double* lse, const double* s,
                                      const double* r, const float* g, int g_stride, float* dx, int64_t lddx, int B, int C, hipStream_t stream) {
  const char* fn = "ssg_softmax_ce_bwd_f32";
  if (int rc = ce_check_shape(fn, B, C, ldx, "ldx")) return rc;
  if (int rc = ce_check_shape(fn, B, C, lddx, "lddx")) return rc;
  if (g_stride != 0 && g_stride != 1) { ssg_set_error("%s: the stride of g must be 0 (a scalar) or 1 (one per row) (g_stride=%d)", fn, g_stride); return SSG_ERR_INVALID; }
  const int chunks = (C + CE_BWD_CHUNK - 1) / CE_BWD_CHUNK;
  if ((int64_t)B * chunks > 0x7fffffffLL) { ssg_set_error("%s: B * ceil(C / %d) exceeds the grid limit (B=%d C=%d)", fn, CE_BWD_CHUNK, B, C); return SSG_ERR_INVALID; }
  if (int rc = ssg_need_pointers(fn, x && target && lse && s && r && g && dx)) return rc;
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)((int64_t)B * chunks)), dim3(256), 0, stream, x, ldx, target, ignore_index, lse, s, r, g, g_stride, dx, lddx, C,
                     chunks);
  SSG_LAUNCH_CHECK("ce_bwd_kernel");
  return SSG_OK;
}

extern "C" int ssg_topk_correct_f32(const float* x, int64_t ldx, const int64_t* target, int B, int C, const int* ks, int num_k, int* rank, float* out,
                                    hipStream_t stream) {
  const char* fn = "ssg_topk_correct_f32";
  if (int rc = ce_check_shape(fn, B, C, ldx, "ldx")) return rc;
  if (num_k < 1 || num_k > TOPK_MAX_K) { ssg_set_error("%s: between 1 and %d values of k per call (num_k=%d)", fn, TOPK_MAX_K, num_k); return SSG_ERR_INVALID; }
  if (int rc = ssg_need_pointers(fn, x && target && ks && rank && out)) return rc;
  TopkKs K = {};
  K.n = num_k;
  for (int a = 0; a < num_k; a++) {
    if (ks[a] < 1) { ssg_set_error("%s: k must be at least 1 (k[%d]=%d)", fn, a, ks[a]); return SSG_ERR_INVALID; }
    K.k[a] = ks[a];
  }
  hipLaunchKernelGGL(topk_rank_kernel, dim3(B), dim3(256), 0, stream, x, ldx, target, C, rank);
  SSG_LAUNCH_CHECK("topk_rank_kernel");
  hipLaunchKernelGGL(topk_count_kernel, dim3(1), dim3(256), 0, stream, rank, B, K, out);
  SSG_LAUNCH_CHECK("topk_count_kernel");
  return SSG_OK;
}

extern "C" int ssg_oim_update_f32(const float* x, int64_t ldx, const int64_t* target, float* lut, int64_t ldl, int B, int C, int F, double momentum,
                                  hipStream_t stream) {
  const char* fn = "ssg_oim_update_f32";
  if (B < 1 || C < 1 || F < 1 || ldx < (int64_t)F || ldl < (int64_t)F) {
    ssg_set_error("%s: need B >= 1, C >= 1, F >= 1 and row strides ldx >= F, ldl >= F (B=%d C=%d F=%d ldx=%lld ldl=%lld)", fn, B, C, F, (long long)ldx, (long long)ldl);
    return SSG_ERR_INVALID;
  }
  if (!(momentum >= 0.0) || !isfinite(momentum)) { ssg_set_error("%s: momentum must be finite and not negative (momentum=%g)", fn, momentum); return SSG_ERR_INVALID; }
  if (int rc = ssg_need_pointers(fn, x && target && lut)) return rc;
  hipLaunchKernelGGL(oim_update_kernel, dim3(B), dim3(256), 0, stream, x, ldx, target, lut, ldl, B, C, F, momentum);
  SSG_LAUNCH_CHECK("oim_update_kernel");
  return SSG_OK;
}
