// dec.hip -- the DEC cluster head of the fine-tune phase (--dce-loss) on the GPU: reid/models/dce.py:39-51 (soft assignment),
// reid/trainers.py:284-292 (target distribution) and the KLDivLoss term of FinedTrainer2 / JointTrainer2._forward (:268-279).
//
//   ns[i,j] = sum_d (x[i,d] - c[j,d])^2          direct differences, no Gram expansion
//   n[i,j]  = (1 / (1 + ns/alpha)) ^ -(alpha+1)/2,   q[i,j] = n[i,j] / sum_j n[i,j]
//   f[j] = sum_i q[i,j],  w = q^2 / f,  p[i,j] = w[i,j] / sum_j w[i,j]
//   loss = sum_ij p (log p - log q) / B          p is NOT detached: the gradient reaches q through log q and through p
//
// The torch chain materialises [B, K, D] and rounds every step to float32; the loss is a sum of terms ~ (q - 1/K)^2 and loses
// 2-3 digits that way.  Here every D-long sum, the column sums, the row sums and the loss are float64 (differences taken in
// float64 too: float32 inputs, exact), rounded to float32 once on the way out.  No float atomics: every reduction has a fixed order
// (lane-strided partial sums, xor butterflies, then partials combined in index order), so two runs give the same bits.
//
//   assignment forward : one workgroup (8 waves) per batch row; a wave takes 4 centres at a time and shares the x loads between them
//   loss / grad wrt q  : one workgroup of 16 waves for the whole [B, K] matrix (B*K <= 262144 elements), a wave per row
//   assignment backward: g = d loss / d ns [B, K] in float64 (workspace), then
//                          gx[i,:] = 2 (rowsum_i(g) x[i,:] - sum_j g[i,j] c[j,:])     one workgroup per row
//                          gc[j,:] = 2 (colsum_j(g) c[j,:] - sum_i g[i,j] x[i,:])     64 columns x 8 centres per workgroup, rows split over 4 waves
//                        -- no [B, K, D] temporary; the 256 KB of centres are read from L2.
#include "ssg_common.h"

namespace ssg {

constexpr int DEC_MAX_B = 4096;
constexpr int DEC_MAX_K = 64;

__device__ __forceinline__ double dec_wave_sum(double v) {
  for (int sh = 1; sh < 64; sh <<= 1) v += __shfl_xor(v, sh, 64);      // butterfly: every lane ends with the same bits
  return v;
}

// numerator of the soft assignment from the squared distance (dce.py:48-50), float64
__device__ __forceinline__ double dec_num(double ns, double alpha) {
  const double r = 1.0 / (1.0 + ns / alpha);
  return pow(r, -(alpha + 1.0) / 2.0);
}

// ---------------------------------------------------------------- soft assignment, forward
__global__ __launch_bounds__(512) void dec_assign_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ c, int K, int D,
                                                         double alpha, float* __restrict__ q, float* __restrict__ ns_out) {
  __shared__ double s_ns[DEC_MAX_K];
  const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const float* xr = x + (int64_t)i * ldx;
  for (int j0 = wave * 4; j0 < K; j0 += 32) {
    // centres j0 .. j0+3 (indices clamped: the surplus sums are dropped)
    const float* c0 = c + (int64_t)min(j0, K - 1) * D;
    const float* c1 = c + (int64_t)min(j0 + 1, K - 1) * D;
    const float* c2 = c + (int64_t)min(j0 + 2, K - 1) * D;
    const float* c3 = c + (int64_t)min(j0 + 3, K - 1) * D;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int d = lane; d < D; d += 64) {
      const double xv = (double)xr[d];
      const double d0 = xv - (double)c0[d], d1 = xv - (double)c1[d], d2 = xv - (double)c2[d], d3 = xv - (double)c3[d];
      a0 += d0 * d0; a1 += d1 * d1; a2 += d2 * d2; a3 += d3 * d3;
    }
    a0 = dec_wave_sum(a0); a1 = dec_wave_sum(a1); a2 = dec_wave_sum(a2); a3 = dec_wave_sum(a3);
    if (lane == 0) {
      s_ns[j0] = a0;
      if (j0 + 1 < K) s_ns[j0 + 1] = a1;
      if (j0 + 2 < K) s_ns[j0 + 2] = a2;
      if (j0 + 3 < K) s_ns[j0 + 3] = a3;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const bool on = lane < K;
    const double nsv = on ? s_ns[lane] : 0.0;
    const double num = on ? dec_num(nsv, alpha) : 0.0;
    const double tot = dec_wave_sum(num);
    if (on) {
      q[(int64_t)i * K + lane] = (float)(num / tot);
      if (ns_out) ns_out[(int64_t)i * K + lane] = (float)nsv;
    }
  }
}

// ---------------------------------------------------------------- target distribution, loss, gradient wrt q
// One workgroup of 1024 threads.  Column sums f[j]: thread (r, j) = (tid / 64, tid % 64) sums rows r, r+16, ... of column j, the 16
// partials are added in order.
__device__ __forceinline__ void dec_colsum_q(const float* __restrict__ q, int B, int K, double (*s_part)[DEC_MAX_K], double* s_f) {
  const int tid = (int)threadIdx.x, j = tid & 63, r = tid >> 6;
  double acc = 0.0;
  if (j < K)
    for (int i = r; i < B; i += 16) acc += (double)q[(int64_t)i * K + j];
  s_part[r][j] = acc;
  __syncthreads();
  if (tid < 64) {
    double f = 0.0;
    for (int k = 0; k < 16; k++) f += s_part[k][tid];
    s_f[tid] = f;
  }
  __syncthreads();
}

// one row of the target distribution in a wave (lane = column): w, p, a = log p - log q (0 where p == 0, like KLDivLoss), the row's
// sum of w and its KL term sum_j p a
struct DecRow { double qv, w, s, p, a, kl; };

__device__ __forceinline__ DecRow dec_row(const float* __restrict__ q, int i, int K, const double* s_f) {
  const int lane = lane_id();
  DecRow r;
  const bool on = lane < K;
  r.qv = on ? (double)q[(int64_t)i * K + lane] : 0.0;
  r.w = on ? r.qv * r.qv / s_f[lane] : 0.0;
  r.s = dec_wave_sum(r.w);
  r.p = r.w / r.s;
  r.a = (on && r.p > 0.0) ? log(r.p / r.qv) : 0.0;
  r.kl = dec_wave_sum(r.p * r.a);
  return r;
}

__global__ __launch_bounds__(1024) void dec_loss_kernel(const float* __restrict__ q, int B, int K, float* __restrict__ p_out, float* __restrict__ loss) {
  __shared__ double s_part[16][DEC_MAX_K];
  __shared__ double s_f[DEC_MAX_K];
  __shared__ double s_kl[16];
  dec_colsum_q(q, B, K, s_part, s_f);
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
  double kl = 0.0;
  for (int i = wave; i < B; i += 16) {
    const DecRow r = dec_row(q, i, K, s_f);
    kl += r.kl;
    if (p_out && lane < K) p_out[(int64_t)i * K + lane] = (float)r.p;
  }
  if (lane == 0) s_kl[wave] = kl;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int k = 0; k < 16; k++) tot += s_kl[k];
    loss[0] = (float)(tot / (double)B);
  }
}

// d loss / d q, both paths (h = d loss / d w = (a - KL_i) / (s_i B), t[j] = sum_i h w):
//   gq[m,j] = gloss * ((2 q[m,j] h[m,j] - t[j]) / f[j] - p[m,j] / (q[m,j] B))
__global__ __launch_bounds__(1024) void dec_loss_grad_kernel(const float* __restrict__ q, int B, int K, const float* __restrict__ gloss,
                                                             float* __restrict__ gq) {
  __shared__ double s_part[16][DEC_MAX_K];
  __shared__ double s_f[DEC_MAX_K];
  __shared__ double s_t[DEC_MAX_K];
  dec_colsum_q(q, B, K, s_part, s_f);
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const double fB = (double)B;
  double t = 0.0;
  for (int i = wave; i < B; i += 16) {
    const DecRow r = dec_row(q, i, K, s_f);
    t += (r.a - r.kl) / (r.s * fB) * r.w;
  }
  s_part[wave][lane] = t;                                  // (dec_colsum_q ended with a barrier after its last read of s_part)
  __syncthreads();
  if (tid < 64) {
    double tot = 0.0;
    for (int k = 0; k < 16; k++) tot += s_part[k][tid];
    s_t[tid] = tot;
  }
  __syncthreads();
  const double g = (double)gloss[0];
  for (int i = wave; i < B; i += 16) {
    const DecRow r = dec_row(q, i, K, s_f);
    if (lane < K) {
      const double h = (r.a - r.kl) / (r.s * fB);
      const double direct = r.p > 0.0 ? r.p / (r.qv * fB) : 0.0;
      gq[(int64_t)i * K + lane] = (float)(g * ((2.0 * r.qv * h - s_t[lane]) / s_f[lane] - direct));
    }
  }
}

// ---------------------------------------------------------------- soft assignment, backward
// g[i,j] = d loss / d ns[i,j] from gq and the forward's ns: with n = (1 + ns/alpha)^e, e = (alpha+1)/2, S = sum_j n, q = n / S:
//   d loss / d n = (gq - sum_k gq q) / S,   d n / d ns = (e / alpha) n / (1 + ns/alpha).     A wave per row.
__global__ __launch_bounds__(256) void dec_assign_gns_kernel(const float* __restrict__ ns, const float* __restrict__ gq, int B, int K, double alpha,
                                                             double* __restrict__ g) {
  const int lane = lane_id();
  const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (i >= B) return;                                      // whole waves leave together
  const bool on = lane < K;
  const double nsv = on ? (double)ns[(int64_t)i * K + lane] : 0.0;
  const double num = on ? dec_num(nsv, alpha) : 0.0;
  const double S = dec_wave_sum(num);
  const double gqv = on ? (double)gq[(int64_t)i * K + lane] : 0.0;
  const double dot = dec_wave_sum(gqv * (num / S));
  if (on) g[(int64_t)i * K + lane] = (gqv - dot) / S * ((alpha + 1.0) / 2.0 / alpha) * num / (1.0 + nsv / alpha);
}

__global__ __launch_bounds__(256) void dec_assign_gx_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ c, int K, int D,
                                                            const double* __restrict__ g, float* __restrict__ gx) {
  __shared__ double s_g[DEC_MAX_K];
  __shared__ double s_rs;
  const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (tid < K) s_g[tid] = g[(int64_t)i * K + tid];
  __syncthreads();
  if (tid == 0) {
    double rs = 0.0;
    for (int j = 0; j < K; j++) rs += s_g[j];
    s_rs = rs;
  }
  __syncthreads();
  const double rs = s_rs;
  for (int d = tid; d < D; d += 256) {
    double acc = 0.0;
    for (int j = 0; j < K; j++) acc += s_g[j] * (double)c[(int64_t)j * D + d];
    gx[(int64_t)i * D + d] = (float)(2.0 * (rs * (double)x[(int64_t)i * ldx + d] - acc));
  }
}

// grid (ceil(D / 64), ceil(K / 8)); lane = column d, wave w sums rows i = w, w+4, ... for the 8 centres of the tile
__global__ __launch_bounds__(256) void dec_assign_gc_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ c, int B, int K, int D,
                                                            const double* __restrict__ g, float* __restrict__ gc) {
  __shared__ double s_acc[4][8][64];
  __shared__ double s_cs[4][8];
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = (int)blockIdx.x * 64 + lane, dl = min(d, D - 1);
  const int j0 = (int)blockIdx.y * 8;
  int jj[8];
#pragma unroll
  for (int t = 0; t < 8; t++) jj[t] = min(j0 + t, K - 1);
  double acc[8], cs[8];
#pragma unroll
  for (int t = 0; t < 8; t++) { acc[t] = 0.0; cs[t] = 0.0; }
  for (int i = wave; i < B; i += 4) {
    const double xv = (double)x[(int64_t)i * ldx + dl];
    const double* gr = g + (int64_t)i * K;
#pragma unroll
    for (int t = 0; t < 8; t++) {
      const double gv = gr[jj[t]];
      acc[t] += gv * xv;
      cs[t] += gv;
    }
  }
#pragma unroll
  for (int t = 0; t < 8; t++) {
    s_acc[wave][t][lane] = acc[t];
    if (lane == 0) s_cs[wave][t] = cs[t];
  }
  __syncthreads();
  if (d >= D) return;
  for (int t = wave; t < 8; t += 4) {                      // each wave finishes 2 of the 8 centres
    const int j = j0 + t;
    if (j >= K) break;
    const double a = ((s_acc[0][t][lane] + s_acc[1][t][lane]) + s_acc[2][t][lane]) + s_acc[3][t][lane];
    const double s = ((s_cs[0][t] + s_cs[1][t]) + s_cs[2][t]) + s_cs[3][t];
    gc[(int64_t)j * D + d] = (float)(2.0 * (s * (double)c[(int64_t)j * D + d] - a));
  }
}

}  // namespace ssg

using namespace ssg;

static int dec_check_bk(const char* fn, int B, int K) {
  if (B < 1 || B > DEC_MAX_B) { ssg_set_error("%s: B=%d outside [1, %d]", fn, B, DEC_MAX_B); return SSG_ERR_INVALID; }
  if (K < 1 || K > DEC_MAX_K) { ssg_set_error("%s: K=%d outside [1, %d]", fn, K, DEC_MAX_K); return SSG_ERR_INVALID; }
  return SSG_OK;
}

static int dec_check_xd(const char* fn, int D, int64_t ldx, double alpha) {
  if (D < 1) { ssg_set_error("%s: D=%d must be >= 1", fn, D); return SSG_ERR_INVALID; }
  if (ldx < D) { ssg_set_error("%s: row pitch ldx=%lld < D=%d", fn, (long long)ldx, D); return SSG_ERR_INVALID; }
  if (!(alpha > 0.0) || alpha > 1.79e308) { ssg_set_error("%s: alpha=%g must be a positive finite number", fn, alpha); return SSG_ERR_INVALID; }
  return SSG_OK;
}

extern "C" int ssg_dec_assign_f32(const float* x, int64_t ldx, const float* c, int B, int K, int D, double alpha, float* q, float* ns,
                                  hipStream_t stream) {
  const char* fn = "ssg_dec_assign_f32";
  if (int rc = dec_check_bk(fn, B, K)) return rc;
  if (int rc = dec_check_xd(fn, D, ldx, alpha)) return rc;
  if (!x || !c || !q) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(dec_assign_kernel, dim3(B), dim3(512), 0, stream, x, ldx, c, K, D, alpha, q, ns);
  SSG_LAUNCH_CHECK("dec_assign_kernel");
  return SSG_OK;
}

extern "C" int ssg_dec_kl_loss_f32(const float* q, int B, int K, float* p, float* loss, hipStream_t stream) {
  const char* fn = "ssg_dec_kl_loss_f32";
  if (int rc = dec_check_bk(fn, B, K)) return rc;
  if (!q || !loss) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(dec_loss_kernel, dim3(1), dim3(1024), 0, stream, q, B, K, p, loss);
  SSG_LAUNCH_CHECK("dec_loss_kernel");
  return SSG_OK;
}

extern "C" int ssg_dec_kl_loss_grad_f32(const float* q, int B, int K, const float* gloss, float* gq, hipStream_t stream) {
  const char* fn = "ssg_dec_kl_loss_grad_f32";
  if (int rc = dec_check_bk(fn, B, K)) return rc;
  if (!q || !gloss || !gq) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(dec_loss_grad_kernel, dim3(1), dim3(1024), 0, stream, q, B, K, gloss, gq);
  SSG_LAUNCH_CHECK("dec_loss_grad_kernel");
  return SSG_OK;
}

extern "C" int ssg_dec_assign_grad_f32(const float* x, int64_t ldx, const float* c, const float* ns, const float* gq, int B, int K, int D,
                                       double alpha, double* gns, float* gx, float* gc, hipStream_t stream) {
  const char* fn = "ssg_dec_assign_grad_f32";
  if (int rc = dec_check_bk(fn, B, K)) return rc;
  if (int rc = dec_check_xd(fn, D, ldx, alpha)) return rc;
  if (!x || !c || !ns || !gq || !gns || !gx || !gc) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(dec_assign_gns_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, ns, gq, B, K, alpha, gns);
  SSG_LAUNCH_CHECK("dec_assign_gns_kernel");
  hipLaunchKernelGGL(dec_assign_gx_kernel, dim3(B), dim3(256), 0, stream, x, ldx, c, K, D, gns, gx);
  SSG_LAUNCH_CHECK("dec_assign_gx_kernel");
  hipLaunchKernelGGL(dec_assign_gc_kernel, dim3((D + 63) / 64, (K + 7) / 8), dim3(256), 0, stream, x, ldx, c, B, K, D, gns, gc);
  SSG_LAUNCH_CHECK("dec_assign_gc_kernel");
  return SSG_OK;
}
