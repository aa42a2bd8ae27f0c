// batchnorm.hip -- train-mode batch normalisation of the fine-tune phase (the reference's trainers call model.train(),
// reid/trainers.py:21,128,212: the 53 BatchNorm2d layers of ResNet-50 and feat_bn, reid/models/resnet.py:65, run on batch statistics),
// forward and backward, with the ReLU and the residual add that follow it fused into the same passes.
//
//   forward : mean[c], var[c] (biased) over the n = N*H*W values of a channel, invstd = 1 / sqrt(var + eps)
//             y = (x - mean) * invstd * weight + bias  [+ residual]  [max(., 0)]
//             running_mean = (1 - f) running_mean + f mean,  running_var = (1 - f) running_var + f var n / (n - 1)
//   backward: g = dy  (with ReLU: g = dy where the saved y > 0, else 0 -- no mask tensor),  xh = (x - mean) * invstd
//             dbias = sum g,  dweight = sum g xh,  dx = (g - dbias / n - xh dweight / n) * invstd * weight,  d_residual = g
//
// float32 tensors in and out; every channel sum is float64 and so is the per-element arithmetic (float32 inputs widened, one rounding
// on the way out: the passes stay memory-bound, a CU has 64 float64 lanes per clock for ~10 bytes of HBM traffic).  The statistics
// are sums of (x - s) and (x - s)^2 with s = the channel's first value (exact differences in float64): a constant channel gives
// var = 0 exactly and a large mean does not cancel.
//
// Reductions are two-stage with a fixed order and no float atomics (the same call gives the same bits): P workgroups per channel
// each leave one pair of partial sums (thread-sequential sums, xor butterflies, the waves' sums added in index order), a finalise
// kernel adds the P pairs in index order.  P is chosen from the shape alone (ssg_bn_num_partials) so that a small C still fills the
// 256 CUs: layer1's 64 channels are split over 32 workgroups each.
//
// Two layouts, one kernel family each:
//   planar : NCHW contiguous, HW > 1.  A channel is N planes of HW contiguous values; a workgroup's channel is uniform (blockIdx.y),
//            its threads stride over the channel's N * HW / VEC units.  VEC = 4 (float4) when HW % 4 == 0 and the base pointers are
//            16-byte aligned -- every plane then starts aligned -- else scalar.
//   rows   : [M, C] with the channel contiguous: channels_last (M = N*H*W), BatchNorm1d's [B, C], and NCHW with HW == 1.  A lane owns
//            VEC consecutive channels (VEC = 4 when C % 4 == 0, C >= 256 and the pointers are aligned, else 1: 64 lanes then read one
//            256-byte segment of a row), the 4 waves of a workgroup and the workgroups of a column tile stride over the rows.
#include "ssg_common.h"

namespace ssg {

constexpr int BN_THREADS = 256;
constexpr int BN_TARGET_WGS = 2048;        // workgroups a reduction aims at: 8 per CU
constexpr int BN_MIN_PER_WG = 4096;        // planar: values of a channel a workgroup takes at least (4 float4 per thread)
constexpr int BN_MIN_ROWS_PER_WG = 64;     // rows: rows a workgroup takes at least (16 per wave)
constexpr int BN_MAX_PARTIALS = 256;

__device__ __forceinline__ double bn_wave_sum(double v) {
  for (int sh = 1; sh < 64; sh <<= 1) v += __shfl_xor(v, sh, 64);       // butterfly: every lane ends with the same bits
  return v;
}

// sums of a and b over the 256 threads of the workgroup (valid in every thread); s: 4 x 2 doubles of LDS
__device__ __forceinline__ void bn_block_sum2(double& a, double& b, double (*s)[2]) {
  a = bn_wave_sum(a);
  b = bn_wave_sum(b);
  const int wave = (int)threadIdx.x >> 6;
  if (lane_id() == 0) { s[wave][0] = a; s[wave][1] = b; }
  __syncthreads();
  a = ((s[0][0] + s[1][0]) + s[2][0]) + s[3][0];
  b = ((s[0][1] + s[1][1]) + s[2][1]) + s[3][1];
}

template <int VEC> __device__ __forceinline__ void bn_load(const float* __restrict__ p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}

template <int VEC> __device__ __forceinline__ void bn_store(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

// NaN stays NaN, like torch's relu
__device__ __forceinline__ double bn_relu(double z) { return z < 0.0 ? 0.0 : z; }

// planar geometry: unit i of a channel (VEC values) lies in plane n = i / q at offset (i % q) * VEC
struct BnPlanar {
  int C, HW;
  uint32_t q;        // units per plane = HW / VEC
  int qshift;        // log2(q) when q is a power of two, else -1
  uint32_t units;    // N * q  (< 2^31)
};

template <int VEC> __device__ __forceinline__ int64_t bn_planar_offset(const BnPlanar& g, int c, uint32_t i) {
  const uint32_t n = g.qshift >= 0 ? i >> g.qshift : i / g.q;
  const uint32_t off = i - n * g.q;
  return ((int64_t)n * g.C + c) * g.HW + (int64_t)off * VEC;
}

// ---------------------------------------------------------------- planar: partial sums
// stats: a = sum (x - s), b = sum (x - s)^2 with s = x[0, c, 0]
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_planar_kernel(const float* __restrict__ x, BnPlanar g, int P, double* __restrict__ part) {
  __shared__ double s_red[4][2];
  const int c = (int)blockIdx.y, p = (int)blockIdx.x;
  const double shift = (double)x[(int64_t)c * g.HW];
  double a = 0.0, b = 0.0;
  const uint32_t step = (uint32_t)P * BN_THREADS;
#pragma unroll 2
  for (uint32_t i = (uint32_t)p * BN_THREADS + threadIdx.x; i < g.units; i += step) {
    float v[VEC];
    bn_load<VEC>(x + bn_planar_offset<VEC>(g, c, i), v);
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const double d = (double)v[k] - shift;
      a += d;
      b += d * d;
    }
  }
  bn_block_sum2(a, b, s_red);
  if (threadIdx.x == 0) {
    part[((int64_t)c * P + p) * 2] = a;
    part[((int64_t)c * P + p) * 2 + 1] = b;
  }
}

// backward: a = sum g, b = sum g (x - mean); y == NULL: g = dy, else g = dy where y > 0
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce_planar_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                          const float* __restrict__ y, const double* __restrict__ stat, BnPlanar g,
                                                                          int P, double* __restrict__ part) {
  __shared__ double s_red[4][2];
  const int c = (int)blockIdx.y, p = (int)blockIdx.x;
  const double mean = stat[c];
  double a = 0.0, b = 0.0;
  const uint32_t step = (uint32_t)P * BN_THREADS;
#pragma unroll 2
  for (uint32_t i = (uint32_t)p * BN_THREADS + threadIdx.x; i < g.units; i += step) {
    const int64_t o = bn_planar_offset<VEC>(g, c, i);
    float gv[VEC], xv[VEC];
    bn_load<VEC>(dy + o, gv);
    bn_load<VEC>(x + o, xv);
    if (y) {
      float yv[VEC];
      bn_load<VEC>(y + o, yv);
#pragma unroll
      for (int k = 0; k < VEC; k++) gv[k] = yv[k] > 0.0f ? gv[k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const double gd = (double)gv[k];
      a += gd;
      b += gd * ((double)xv[k] - mean);
    }
  }
  bn_block_sum2(a, b, s_red);
  if (threadIdx.x == 0) {
    part[((int64_t)c * P + p) * 2] = a;
    part[((int64_t)c * P + p) * 2 + 1] = b;
  }
}

// ---------------------------------------------------------------- planar: element-wise passes
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_planar_kernel(const float* __restrict__ x, const double* __restrict__ stat,
                                                                     const float* __restrict__ weight, const float* __restrict__ bias,
                                                                     const float* __restrict__ res, int relu, BnPlanar g, float* __restrict__ y) {
  const int c = (int)blockIdx.y;
  const double mean = stat[c], scale = stat[2 * g.C + c] * (double)weight[c], shift = (double)bias[c];
  const uint32_t step = gridDim.x * BN_THREADS;
  for (uint32_t i = blockIdx.x * BN_THREADS + threadIdx.x; i < g.units; i += step) {
    const int64_t o = bn_planar_offset<VEC>(g, c, i);
    float xv[VEC], rv[VEC], out[VEC];
    bn_load<VEC>(x + o, xv);
    if (res) bn_load<VEC>(res + o, rv);
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      double z = ((double)xv[k] - mean) * scale + shift;
      if (res) z += (double)rv[k];
      if (relu) z = bn_relu(z);
      out[k] = (float)z;
    }
    bn_store<VEC>(y + o, out);
  }
}

// coef[c] = mean of g, coef[C + c] = mean of g xh
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_planar_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                         const float* __restrict__ y, const double* __restrict__ stat,
                                                                         const float* __restrict__ weight, const double* __restrict__ coef, BnPlanar g,
                                                                         float* __restrict__ dx, float* __restrict__ dres) {
  const int c = (int)blockIdx.y;
  const double mean = stat[c], invstd = stat[2 * g.C + c], scale = invstd * (double)weight[c];
  const double mg = coef[c], mgx = coef[g.C + c];
  const uint32_t step = gridDim.x * BN_THREADS;
  for (uint32_t i = blockIdx.x * BN_THREADS + threadIdx.x; i < g.units; i += step) {
    const int64_t o = bn_planar_offset<VEC>(g, c, i);
    float gv[VEC], xv[VEC], out[VEC];
    bn_load<VEC>(dy + o, gv);
    bn_load<VEC>(x + o, xv);
    if (y) {
      float yv[VEC];
      bn_load<VEC>(y + o, yv);
#pragma unroll
      for (int k = 0; k < VEC; k++) gv[k] = yv[k] > 0.0f ? gv[k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const double xh = ((double)xv[k] - mean) * invstd;
      out[k] = (float)((((double)gv[k] - mg) - xh * mgx) * scale);
    }
    bn_store<VEC>(dx + o, out);
    if (dres) bn_store<VEC>(dres + o, gv);
  }
}

// ---------------------------------------------------------------- rows: partial sums
// grid (column tiles of 64 * VEC channels, P); thread (lane, wave): channels c0 .. c0 + VEC - 1, rows blockIdx.y * 4 + wave, step 4 P
template <int VEC, bool BWD>
__global__ __launch_bounds__(BN_THREADS) void bn_reduce_rows_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                                    const double* __restrict__ stat, int M, int C, int P, double* __restrict__ part) {
  __shared__ double s_acc[4][64][2 * VEC];
  const int lane = lane_id(), wave = (int)threadIdx.x >> 6, p = (int)blockIdx.y;
  const int c0 = ((int)blockIdx.x * 64 + lane) * VEC;
  const bool on = c0 < C;                                  // C % VEC == 0: a unit is inside or outside as a whole
  double a[VEC], b[VEC], ref[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    a[k] = 0.0; b[k] = 0.0;
    ref[k] = on ? (BWD ? stat[c0 + k] : (double)x[c0 + k]) : 0.0;      // backward: the mean; forward: the shift, row 0's value
  }
  if (on) {
#pragma unroll 2
    for (int r = p * 4 + wave; r < M; r += P * 4) {
      const int64_t o = (int64_t)r * C + c0;
      float xv[VEC];
      bn_load<VEC>(x + o, xv);
      if constexpr (BWD) {
        float gv[VEC];
        bn_load<VEC>(dy + o, gv);
        if (y) {
          float yv[VEC];
          bn_load<VEC>(y + o, yv);
#pragma unroll
          for (int k = 0; k < VEC; k++) gv[k] = yv[k] > 0.0f ? gv[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < VEC; k++) {
          const double gd = (double)gv[k];
          a[k] += gd;
          b[k] += gd * ((double)xv[k] - ref[k]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < VEC; k++) {
          const double d = (double)xv[k] - ref[k];
          a[k] += d;
          b[k] += d * d;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    s_acc[wave][lane][2 * k] = a[k];
    s_acc[wave][lane][2 * k + 1] = b[k];
  }
  __syncthreads();
  if (wave == 0 && on) {
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const double sa = ((s_acc[0][lane][2 * k] + s_acc[1][lane][2 * k]) + s_acc[2][lane][2 * k]) + s_acc[3][lane][2 * k];
      const double sb = ((s_acc[0][lane][2 * k + 1] + s_acc[1][lane][2 * k + 1]) + s_acc[2][lane][2 * k + 1]) + s_acc[3][lane][2 * k + 1];
      part[((int64_t)(c0 + k) * P + p) * 2] = sa;
      part[((int64_t)(c0 + k) * P + p) * 2 + 1] = sb;
    }
  }
}

// ---------------------------------------------------------------- rows: element-wise passes
// grid (column tiles, row groups); the thread's channels are fixed, their constants live in registers
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_rows_kernel(const float* __restrict__ x, const double* __restrict__ stat,
                                                                   const float* __restrict__ weight, const float* __restrict__ bias,
                                                                   const float* __restrict__ res, int relu, int M, int C, float* __restrict__ y) {
  const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
  const int c0 = ((int)blockIdx.x * 64 + lane) * VEC;
  if (c0 >= C) return;
  double mean[VEC], scale[VEC], shift[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    mean[k] = stat[c0 + k];
    scale[k] = stat[2 * C + c0 + k] * (double)weight[c0 + k];
    shift[k] = (double)bias[c0 + k];
  }
  for (int r = (int)blockIdx.y * 4 + wave; r < M; r += (int)gridDim.y * 4) {
    const int64_t o = (int64_t)r * C + c0;
    float xv[VEC], rv[VEC], out[VEC];
    bn_load<VEC>(x + o, xv);
    if (res) bn_load<VEC>(res + o, rv);
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      double z = ((double)xv[k] - mean[k]) * scale[k] + shift[k];
      if (res) z += (double)rv[k];
      if (relu) z = bn_relu(z);
      out[k] = (float)z;
    }
    bn_store<VEC>(y + o, out);
  }
}

template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_rows_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                                       const double* __restrict__ stat, const float* __restrict__ weight,
                                                                       const double* __restrict__ coef, int M, int C, float* __restrict__ dx,
                                                                       float* __restrict__ dres) {
  const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
  const int c0 = ((int)blockIdx.x * 64 + lane) * VEC;
  if (c0 >= C) return;
  double mean[VEC], invstd[VEC], scale[VEC], mg[VEC], mgx[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    mean[k] = stat[c0 + k];
    invstd[k] = stat[2 * C + c0 + k];
    scale[k] = invstd[k] * (double)weight[c0 + k];
    mg[k] = coef[c0 + k];
    mgx[k] = coef[C + c0 + k];
  }
  for (int r = (int)blockIdx.y * 4 + wave; r < M; r += (int)gridDim.y * 4) {
    const int64_t o = (int64_t)r * C + c0;
    float gv[VEC], xv[VEC], out[VEC];
    bn_load<VEC>(dy + o, gv);
    bn_load<VEC>(x + o, xv);
    if (y) {
      float yv[VEC];
      bn_load<VEC>(y + o, yv);
#pragma unroll
      for (int k = 0; k < VEC; k++) gv[k] = yv[k] > 0.0f ? gv[k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const double xh = ((double)xv[k] - mean[k]) * invstd[k];
      out[k] = (float)((((double)gv[k] - mg[k]) - xh * mgx[k]) * scale[k]);
    }
    bn_store<VEC>(dx + o, out);
    if (dres) bn_store<VEC>(dres + o, gv);
  }
}

// ---------------------------------------------------------------- finalise: the P partials of a channel, added in index order
// shift_stride: distance between the first values of consecutive channels (HW planar, 1 rows).  momentum < 0: the cumulative average,
// f = 1 / nbt[0] (the caller has already counted this batch).
__global__ __launch_bounds__(BN_THREADS) void bn_stats_finalize_kernel(const float* __restrict__ x, int64_t shift_stride, const double* __restrict__ part,
                                                                       int C, int P, double n, double eps, double momentum,
                                                                       const int64_t* __restrict__ nbt, float* __restrict__ running_mean,
                                                                       float* __restrict__ running_var, double* __restrict__ stat) {
  const int c = (int)(blockIdx.x * BN_THREADS + threadIdx.x);
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int p = 0; p < P; p++) {
    a += part[((int64_t)c * P + p) * 2];
    b += part[((int64_t)c * P + p) * 2 + 1];
  }
  const double dm = a / n;
  const double mean = (double)x[(int64_t)c * shift_stride] + dm;
  double var = b / n - dm * dm;
  if (var < 0.0) var = 0.0;
  stat[c] = mean;
  stat[C + c] = var;
  stat[2 * C + c] = 1.0 / sqrt(var + eps);
  const double f = momentum >= 0.0 ? momentum : 1.0 / (double)nbt[0];
  if (running_mean) running_mean[c] = (float)((1.0 - f) * (double)running_mean[c] + f * mean);
  if (running_var) running_var[c] = (float)((1.0 - f) * (double)running_var[c] + f * (var * (n / (n - 1.0))));
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_finalize_kernel(const double* __restrict__ part, const double* __restrict__ stat, int C, int P, double n,
                                                                     double* __restrict__ coef, float* __restrict__ dweight, float* __restrict__ dbias) {
  const int c = (int)(blockIdx.x * BN_THREADS + threadIdx.x);
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int p = 0; p < P; p++) {
    a += part[((int64_t)c * P + p) * 2];
    b += part[((int64_t)c * P + p) * 2 + 1];
  }
  const double gx = b * stat[2 * C + c];               // sum g xh
  coef[c] = a / n;
  coef[C + c] = gx / n;
  if (dweight) dweight[c] = (float)gx;
  if (dbias) dbias[c] = (float)a;
}

}  // namespace ssg

using namespace ssg;

namespace {

struct BnShape {
  bool rows;             // the rows family (channels_last, [B, C], HW == 1)
  int M;                 // rows: N * HW
  int tile_vec;          // rows: VEC the shape allows (pointer alignment may still force 1)
  int tiles;             // rows: column tiles at tile_vec
  int P;
  int64_t per_channel;
};

int bn_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

BnShape bn_shape(int N, int C, int HW, int channels_last) {
  BnShape s;
  s.per_channel = (int64_t)N * HW;
  s.rows = channels_last || HW == 1;
  s.M = (int)s.per_channel;
  s.tile_vec = (C % 4 == 0 && C >= 256) ? 4 : 1;
  s.tiles = bn_ceil_div(C, 64 * s.tile_vec);
  int by_fill, by_size;
  if (s.rows) {
    by_fill = bn_ceil_div(BN_TARGET_WGS, s.tiles);
    by_size = bn_ceil_div(s.M, BN_MIN_ROWS_PER_WG);
  } else {
    by_fill = bn_ceil_div(BN_TARGET_WGS, C);
    by_size = bn_ceil_div(s.per_channel, BN_MIN_PER_WG);
  }
  int P = by_fill < by_size ? by_fill : by_size;
  if (P > BN_MAX_PARTIALS) P = BN_MAX_PARTIALS;
  if (P < 1) P = 1;
  s.P = P;
  return s;
}

int bn_check_shape(const char* fn, int N, int C, int HW, int channels_last) {
  if (C <= 0) { ssg_set_error("%s: C=%d must be >= 1", fn, C); return SSG_ERR_INVALID; }
  if (N <= 0 || HW <= 0) { ssg_set_error("%s: N=%d HW=%d must be >= 1", fn, N, HW); return SSG_ERR_INVALID; }
  if ((int64_t)N * HW < 2) { ssg_set_error("%s: N=%d HW=%d: fewer than 2 values per channel", fn, N, HW); return SSG_ERR_INVALID; }
  if ((int64_t)N * C * HW >= ((int64_t)1 << 31)) {
    ssg_set_error("%s: N=%d C=%d HW=%d: 2^31 or more elements", fn, N, C, HW);
    return SSG_ERR_INVALID;
  }
  if (!channels_last && HW > 1 && C > 65535) { ssg_set_error("%s: C=%d > 65535 in the NCHW layout", fn, C); return SSG_ERR_INVALID; }
  return SSG_OK;
}

bool bn_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

BnPlanar bn_planar(int N, int C, int HW, int vec) {
  BnPlanar g;
  g.C = C; g.HW = HW;
  g.q = (uint32_t)(HW / vec);
  g.qshift = -1;
  for (int s = 0; s < 31; s++)
    if (g.q == (1u << s)) g.qshift = s;
  g.units = (uint32_t)N * g.q;
  return g;
}

// workgroups along x (planar) / y (rows) of an element-wise pass: about 4096 in all, none without work
int bn_apply_groups(int other, int64_t work_items) {
  int g = bn_ceil_div(2 * BN_TARGET_WGS, other);
  const int64_t cap = work_items < 1 ? 1 : work_items;
  if (g > cap) g = (int)cap;
  if (g > 65535) g = 65535;
  return g < 1 ? 1 : g;
}

int bn_check_ws(const char* fn, const BnShape& s, int C, const void* ws, size_t ws_bytes) {
  const size_t need = (size_t)C * s.P * 2 * sizeof(double);
  if (!ws || ws_bytes < need || ((uintptr_t)ws & 7)) {
    ssg_set_error("%s: workspace of %zu bytes (8-byte aligned) needed, got %zu", fn, need, ws ? ws_bytes : (size_t)0);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_bn_num_partials(int N, int C, int HW, int channels_last) {
  if (bn_check_shape("ssg_bn_num_partials", N, C, HW, channels_last)) return SSG_ERR_INVALID;
  return bn_shape(N, C, HW, channels_last).P;
}

extern "C" size_t ssg_bn_workspace_bytes(int N, int C, int HW, int channels_last) {
  if (bn_check_shape("ssg_bn_workspace_bytes", N, C, HW, channels_last)) return 0;
  return (size_t)C * bn_shape(N, C, HW, channels_last).P * 2 * sizeof(double);
}

extern "C" int ssg_bn_stats_f32(const float* x, int N, int C, int HW, int channels_last, double eps, double momentum, const int64_t* num_batches_tracked,
                                float* running_mean, float* running_var, double* stat, void* ws, size_t ws_bytes, hipStream_t stream) {
  const char* fn = "ssg_bn_stats_f32";
  if (int rc = bn_check_shape(fn, N, C, HW, channels_last)) return rc;
  if (!x || !stat) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  if (!(eps >= 0.0) || eps > 1.79e308) { ssg_set_error("%s: eps=%g must be a finite number >= 0", fn, eps); return SSG_ERR_INVALID; }
  if (momentum != momentum || momentum > 1.0) { ssg_set_error("%s: momentum=%g must be in [0, 1], or negative for the cumulative average", fn, momentum); return SSG_ERR_INVALID; }
  if (momentum < 0.0 && !num_batches_tracked) { ssg_set_error("%s: the cumulative average needs num_batches_tracked", fn); return SSG_ERR_INVALID; }
  const BnShape s = bn_shape(N, C, HW, channels_last);
  if (int rc = bn_check_ws(fn, s, C, ws, ws_bytes)) return rc;
  double* part = (double*)ws;
  if (s.rows) {
    if (s.tile_vec == 4 && bn_aligned16(x)) {
      hipLaunchKernelGGL((bn_reduce_rows_kernel<4, false>), dim3(s.tiles, s.P), dim3(BN_THREADS), 0, stream, nullptr, x, nullptr, nullptr, s.M, C, s.P, part);
    } else {
      hipLaunchKernelGGL((bn_reduce_rows_kernel<1, false>), dim3(bn_ceil_div(C, 64), s.P), dim3(BN_THREADS), 0, stream, nullptr, x, nullptr, nullptr, s.M, C,
                         s.P, part);
    }
  } else if (HW % 4 == 0 && bn_aligned16(x)) {
    hipLaunchKernelGGL(bn_stats_planar_kernel<4>, dim3(s.P, C), dim3(BN_THREADS), 0, stream, x, bn_planar(N, C, HW, 4), s.P, part);
  } else {
    hipLaunchKernelGGL(bn_stats_planar_kernel<1>, dim3(s.P, C), dim3(BN_THREADS), 0, stream, x, bn_planar(N, C, HW, 1), s.P, part);
  }
  SSG_LAUNCH_CHECK("bn_stats kernel");
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(bn_ceil_div(C, BN_THREADS)), dim3(BN_THREADS), 0, stream, x, (int64_t)(s.rows ? 1 : HW), part, C, s.P,
                     (double)s.per_channel, eps, momentum, num_batches_tracked, running_mean, running_var, stat);
  SSG_LAUNCH_CHECK("bn_stats_finalize_kernel");
  return SSG_OK;
}

extern "C" int ssg_bn_apply_f32(const float* x, const double* stat, const float* weight, const float* bias, const float* residual, int relu, int N, int C,
                                int HW, int channels_last, float* y, hipStream_t stream) {
  const char* fn = "ssg_bn_apply_f32";
  if (int rc = bn_check_shape(fn, N, C, HW, channels_last)) return rc;
  if (!x || !stat || !weight || !bias || !y) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  const BnShape s = bn_shape(N, C, HW, channels_last);
  const bool al = bn_aligned16(x) && bn_aligned16(y) && (!residual || bn_aligned16(residual));
  if (s.rows) {
    if (s.tile_vec == 4 && al) {
      hipLaunchKernelGGL(bn_apply_rows_kernel<4>, dim3(s.tiles, bn_apply_groups(s.tiles, bn_ceil_div(s.M, 4))), dim3(BN_THREADS), 0, stream, x, stat, weight, bias,
                         residual, relu, s.M, C, y);
    } else {
      const int tiles = bn_ceil_div(C, 64);
      hipLaunchKernelGGL(bn_apply_rows_kernel<1>, dim3(tiles, bn_apply_groups(tiles, bn_ceil_div(s.M, 4))), dim3(BN_THREADS), 0, stream, x, stat, weight, bias,
                         residual, relu, s.M, C, y);
    }
  } else if (HW % 4 == 0 && al) {
    const BnPlanar g = bn_planar(N, C, HW, 4);
    hipLaunchKernelGGL(bn_apply_planar_kernel<4>, dim3(bn_apply_groups(C, bn_ceil_div(g.units, BN_THREADS)), C), dim3(BN_THREADS), 0, stream, x, stat, weight,
                       bias, residual, relu, g, y);
  } else {
    const BnPlanar g = bn_planar(N, C, HW, 1);
    hipLaunchKernelGGL(bn_apply_planar_kernel<1>, dim3(bn_apply_groups(C, bn_ceil_div(g.units, BN_THREADS)), C), dim3(BN_THREADS), 0, stream, x, stat, weight,
                       bias, residual, relu, g, y);
  }
  SSG_LAUNCH_CHECK("bn_apply kernel");
  return SSG_OK;
}

extern "C" int ssg_bn_backward_reduce_f32(const float* dy, const float* x, const float* y, const double* stat, int N, int C, int HW, int channels_last,
                                          double* coef, float* dweight, float* dbias, void* ws, size_t ws_bytes, hipStream_t stream) {
  const char* fn = "ssg_bn_backward_reduce_f32";
  if (int rc = bn_check_shape(fn, N, C, HW, channels_last)) return rc;
  if (!dy || !x || !stat || !coef) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  const BnShape s = bn_shape(N, C, HW, channels_last);
  if (int rc = bn_check_ws(fn, s, C, ws, ws_bytes)) return rc;
  double* part = (double*)ws;
  const bool al = bn_aligned16(dy) && bn_aligned16(x) && (!y || bn_aligned16(y));
  if (s.rows) {
    if (s.tile_vec == 4 && al) {
      hipLaunchKernelGGL((bn_reduce_rows_kernel<4, true>), dim3(s.tiles, s.P), dim3(BN_THREADS), 0, stream, dy, x, y, stat, s.M, C, s.P, part);
    } else {
      hipLaunchKernelGGL((bn_reduce_rows_kernel<1, true>), dim3(bn_ceil_div(C, 64), s.P), dim3(BN_THREADS), 0, stream, dy, x, y, stat, s.M, C, s.P, part);
    }
  } else if (HW % 4 == 0 && al) {
    hipLaunchKernelGGL(bn_bwd_reduce_planar_kernel<4>, dim3(s.P, C), dim3(BN_THREADS), 0, stream, dy, x, y, stat, bn_planar(N, C, HW, 4), s.P, part);
  } else {
    hipLaunchKernelGGL(bn_bwd_reduce_planar_kernel<1>, dim3(s.P, C), dim3(BN_THREADS), 0, stream, dy, x, y, stat, bn_planar(N, C, HW, 1), s.P, part);
  }
  SSG_LAUNCH_CHECK("bn_bwd_reduce kernel");
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(bn_ceil_div(C, BN_THREADS)), dim3(BN_THREADS), 0, stream, part, stat, C, s.P, (double)s.per_channel, coef,
                     dweight, dbias);
  SSG_LAUNCH_CHECK("bn_bwd_finalize_kernel");
  return SSG_OK;
}

extern "C" int ssg_bn_backward_apply_f32(const float* dy, const float* x, const float* y, const double* stat, const float* weight, const double* coef, int N,
                                         int C, int HW, int channels_last, float* dx, float* dresidual, hipStream_t stream) {
  const char* fn = "ssg_bn_backward_apply_f32";
  if (int rc = bn_check_shape(fn, N, C, HW, channels_last)) return rc;
  if (!dy || !x || !stat || !weight || !coef || !dx) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  const BnShape s = bn_shape(N, C, HW, channels_last);
  const bool al = bn_aligned16(dy) && bn_aligned16(x) && bn_aligned16(dx) && (!y || bn_aligned16(y)) && (!dresidual || bn_aligned16(dresidual));
  if (s.rows) {
    if (s.tile_vec == 4 && al) {
      hipLaunchKernelGGL(bn_bwd_apply_rows_kernel<4>, dim3(s.tiles, bn_apply_groups(s.tiles, bn_ceil_div(s.M, 4))), dim3(BN_THREADS), 0, stream, dy, x, y, stat,
                         weight, coef, s.M, C, dx, dresidual);
    } else {
      const int tiles = bn_ceil_div(C, 64);
      hipLaunchKernelGGL(bn_bwd_apply_rows_kernel<1>, dim3(tiles, bn_apply_groups(tiles, bn_ceil_div(s.M, 4))), dim3(BN_THREADS), 0, stream, dy, x, y, stat,
                         weight, coef, s.M, C, dx, dresidual);
    }
  } else if (HW % 4 == 0 && al) {
    const BnPlanar g = bn_planar(N, C, HW, 4);
    hipLaunchKernelGGL(bn_bwd_apply_planar_kernel<4>, dim3(bn_apply_groups(C, bn_ceil_div(g.units, BN_THREADS)), C), dim3(BN_THREADS), 0, stream, dy, x, y, stat,
                       weight, coef, g, dx, dresidual);
  } else {
    const BnPlanar g = bn_planar(N, C, HW, 1);
    hipLaunchKernelGGL(bn_bwd_apply_planar_kernel<1>, dim3(bn_apply_groups(C, bn_ceil_div(g.units, BN_THREADS)), C), dim3(BN_THREADS), 0, stream, dy, x, y, stat,
                       weight, coef, g, dx, dresidual);
  }
  SSG_LAUNCH_CHECK("bn_bwd_apply kernel");
  return SSG_OK;
}
