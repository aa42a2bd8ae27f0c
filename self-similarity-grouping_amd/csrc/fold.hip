// fold.hip -- the embedder's weights from the training model's, on the device: Conv2d + eval-mode BatchNorm folded, packed in the
// convolution kernels' reduction order and, for precision='split', scaled per row and cut into half pairs (gfx950 only).
//
// One launch folds one convolution (or the [conv3 | downsample] pair of a downsample block, or feat + feat_bn) into exactly the bits
// `_fold` of ssg_amd/resnet.py produces on the host; the arithmetic is element-wise and deterministic, so there is no tolerance:
//
//   fold      float64, no contraction: scale = gamma / sqrt(var + eps), w' = float32(w * scale), bias = float32(beta - mean * scale);
//             the float64 square root and division are the correctly rounded ones
//   pack      Cin % 32 == 0: k = ((c / 32) * KH*KW + r*KW + s) * 32 + c % 32 (pack_weight_khwc);  Cin == 3 (stem): RGB0 taps,
//             k = (r*KW + s) * 4 + c, row zero-padded to Kpad = 32 * ceil(KH*KW / 8)
//   row scale split mode only: 2^e, e = clamp(floor(log2(16384 / max|w'_row|)), -40, 40), 0 for an all-zero row.  No log2 here: the
//             exponent comes from the bits of the maximum -- for mx = m * 2^q, m in [1, 2): e = 14 - q when m == 1, else 13 - q
//             (float32 subnormals normalised first)
//   split     v = w' * 2^e (float32), hi = half(v), lo = half(v - float(hi)); 8 values -> 32 bytes [8 hi][8 lo] (h8l8), the stem
//             4 values -> 16 bytes [4 hi][4 lo] (h4l4); ch_scale = 2^-e.  f32 mode stores the packed float32 row, no ch_scale
//   dual      two 1x1 sources with their own BatchNorm, each folded and packed on its own, concatenated along K; one row scale over
//             the concatenated row; bias = float32(b1) + float32(b2), added in float32
//
// Launch shape: one workgroup of 256 threads per output row.  The row is read in the order it lies in memory (contiguous or
// channels_last weight, given by element strides) and written to LDS at its packed index, so the global reads are coalesced for both
// layouts; the scattered side is the LDS write (a 3x3 row from a contiguous weight lands 9-way on a bank: 25 M elements per
// ResNet-50, a few microseconds in all).  The row maximum is the unsigned maximum of the |w'| bit patterns, reduced over the wave by
// shuffles and over the four waves through LDS.  The second pass gives every thread 8 consecutive packed values: it scales, splits
// and stores one whole 32-byte group.  No atomics, no workspace, no host read.
#include "train_common.h"
#include <math.h>

namespace ssg {

constexpr int FOLD_MAX_K = 8192;                  // floats of one packed row (32 KB of LDS); the longest ResNet row is 512 * 3 * 3 = 4608

// ---- the scalar rules (tests/test_fold_host.py compiles this text for the host and holds it to resnet.py)
__device__ __forceinline__ double fold_scale(float gamma, float var, double eps) { return (double)gamma / sqrt((double)var + eps); }
__device__ __forceinline__ float fold_weight(float w, double scale) { return (float)((double)w * scale); }
__device__ __forceinline__ float fold_bias(float beta, float mean, double scale) { return (float)((double)beta - (double)mean * scale); }
// e of the row scale 2^e from the bit pattern of the row maximum (sign bit clear)
__device__ __forceinline__ int fold_row_exponent(uint32_t mx_bits) {
  if (mx_bits == 0) return 0;
  const int ef = (int)(mx_bits >> 23);
  const uint32_t mant = mx_bits & 0x7fffffu;
  int q;
  bool one;                                       // the significand m is exactly 1
  if (ef == 0) {                                  // subnormal: mant * 2^-149
    const int top = 31 - __builtin_clz(mant);
    q = top - 149;
    one = mant == (1u << top);
  } else {
    q = ef - 127;
    one = mant == 0;
  }
  const int e = (one ? 14 : 13) - q;
  return e < -40 ? -40 : e > 40 ? 40 : e;
}
__device__ __forceinline__ float fold_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }   // |e| <= 126
__device__ __forceinline__ void fold_split(float w, float sc, hbits& hi, hbits& lo) {
  const float v = w * sc;
  hi = f2h(v);
  lo = f2h(v - h2f(hi));
}
__device__ __forceinline__ int fold_packed_index(int c, int tap, int taps) { return ((c >> 5) * taps + tap) * 32 + (c & 31); }
__device__ __forceinline__ int fold_stem_index(int c, int tap) { return tap * 4 + c; }
// ---- end of the scalar rules

struct FoldSrc {
  const float* w;                                 // [Cout, Cin, KH, KW] at element strides
  int64_t s_co, s_ci, s_r, s_s;
  const float *gamma, *beta, *mean, *var;         // [Cout]
  int Cin, KH, KW;
  int K;                                          // packed floats of this source's part of a row
};

// one source's part of row `co`: folded, at its packed index in `row`; returns this thread's maximum of the |w'| bit patterns
__device__ __forceinline__ uint32_t fold_gather(const FoldSrc& s, int co, double eps, bool stem, float* row, int tid) {
  const double scale = fold_scale(s.gamma[co], s.var[co], eps);
  const float* __restrict__ w = s.w + (int64_t)co * s.s_co;
  const int taps = s.KH * s.KW, n = s.Cin * taps;
  const bool c_fastest = s.s_ci == 1;             // channels_last (and every 1x1): the channel is the fastest index in memory
  uint32_t mx = 0;
  for (int i = tid; i < n; i += 256) {
    int c, tap;
    if (c_fastest) { tap = i / s.Cin; c = i - tap * s.Cin; } else { c = i / taps; tap = i - c * taps; }
    const int r = tap / s.KW, q = tap - r * s.KW;
    const float v = fold_weight(w[c * s.s_ci + r * s.s_r + q * s.s_s], scale);
    row[stem ? fold_stem_index(c, tap) : fold_packed_index(c, tap, taps)] = v;
    const uint32_t mag = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
    mx = mag > mx ? mag : mx;
  }
  return mx;
}

__device__ __forceinline__ uint32_t fold_pack_h2(hbits a, hbits b) { return (uint32_t)a | ((uint32_t)b << 16); }

__global__ __launch_bounds__(256) void fold_conv_bn_kernel(const FoldSrc a, const FoldSrc b, const int nsrc, const double eps, const int split, const int stem,
                                                           float* __restrict__ w_out, float* __restrict__ bias, float* __restrict__ ch_scale) {
  __shared__ __attribute__((aligned(16))) float row[FOLD_MAX_K];
  __shared__ uint32_t wave_mx[4];
  const int tid = threadIdx.x, co = (int)blockIdx.x;
  const int Kp = a.K + (nsrc == 2 ? b.K : 0);
  if (stem) {                                     // the padding channel and the tail past the last tap: no weight lands there
    const int used = a.KH * a.KW * 4;
    for (int k = tid; k < Kp; k += 256)
      if (k >= used || (k & 3) == 3) row[k] = 0.f;
  }
  uint32_t mx = fold_gather(a, co, eps, stem != 0, row, tid);
  if (nsrc == 2) {
    const uint32_t m2 = fold_gather(b, co, eps, false, row + a.K, tid);
    mx = m2 > mx ? m2 : mx;
  }
  if (tid == 0) {
    float bv = fold_bias(a.beta[co], a.mean[co], fold_scale(a.gamma[co], a.var[co], eps));
    if (nsrc == 2) bv = bv + fold_bias(b.beta[co], b.mean[co], fold_scale(b.gamma[co], b.var[co], eps));
    bias[co] = bv;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if ((tid & 63) == 0) wave_mx[tid >> 6] = mx;
  __syncthreads();                                // the row and the four wave maxima are in LDS
  mx = wave_mx[0];
#pragma unroll
  for (int w = 1; w < 4; w++) mx = wave_mx[w] > mx ? wave_mx[w] : mx;
  const int e = split ? fold_row_exponent(mx) : 0;
  const float sc = fold_pow2(e);
  if (split && tid == 0) ch_scale[co] = fold_pow2(-e);

  float* __restrict__ out = w_out + (int64_t)co * Kp;
  for (int g = tid; g < (Kp >> 3); g += 256) {
    const float4 v0 = reinterpret_cast<const float4*>(row)[2 * g], v1 = reinterpret_cast<const float4*>(row)[2 * g + 1];
    if (!split) {
      reinterpret_cast<float4*>(out)[2 * g] = v0;
      reinterpret_cast<float4*>(out)[2 * g + 1] = v1;
      continue;
    }
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    hbits hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; j++) fold_split(v[j], sc, hi[j], lo[j]);
    uint4 q0, q1;
    if (stem) {                                   // h4l4: [4 hi][4 lo] per tap, two taps
      q0 = make_uint4(fold_pack_h2(hi[0], hi[1]), fold_pack_h2(hi[2], hi[3]), fold_pack_h2(lo[0], lo[1]), fold_pack_h2(lo[2], lo[3]));
      q1 = make_uint4(fold_pack_h2(hi[4], hi[5]), fold_pack_h2(hi[6], hi[7]), fold_pack_h2(lo[4], lo[5]), fold_pack_h2(lo[6], lo[7]));
    } else {                                      // h8l8: [8 hi][8 lo]
      q0 = make_uint4(fold_pack_h2(hi[0], hi[1]), fold_pack_h2(hi[2], hi[3]), fold_pack_h2(hi[4], hi[5]), fold_pack_h2(hi[6], hi[7]));
      q1 = make_uint4(fold_pack_h2(lo[0], lo[1]), fold_pack_h2(lo[2], lo[3]), fold_pack_h2(lo[4], lo[5]), fold_pack_h2(lo[6], lo[7]));
    }
    reinterpret_cast<uint4*>(out)[2 * g] = q0;
    reinterpret_cast<uint4*>(out)[2 * g + 1] = q1;
  }
}

}  // namespace ssg

namespace {

using namespace ssg;

// shape rules of one source -> its packed length in *K; the error names the entry point
int fold_check_source(const char* fn, const char* which, int Cout, int Cin, int KH, int KW, bool allow_stem, int* K) {
  // (Cout == 32: the InceptionNet stem layers, csrc/inception.hip)
  if (Cout <= 0 || (Cout % 64 && Cout != 32) || Cin <= 0 || KH <= 0 || KW <= 0 || KH > 64 || KW > 64 || !(Cin % 32 == 0 || (allow_stem && Cin == 3))) {
    ssg_set_error("%s: unsupported shape (%s: Cout=%d Cin=%d KH=%d KW=%d): Cout %% 64 == 0 (or Cout == 32) and Cin %% 32 == 0%s are needed", fn, which, Cout, Cin, KH, KW,
                  allow_stem ? " (or Cin == 3, the stem)" : "");
    return SSG_ERR_INVALID;
  }
  const int64_t k = Cin == 3 ? 32 * (((int64_t)KH * KW + 7) / 8) : (int64_t)Cin * KH * KW;
  if (k > FOLD_MAX_K) {
    ssg_set_error("%s: unsupported shape (%s: Cin=%d KH=%d KW=%d): a packed row of %lld floats is beyond the %d that fit in LDS", fn, which, Cin, KH, KW,
                  (long long)k, FOLD_MAX_K);
    return SSG_ERR_INVALID;
  }
  *K = (int)k;
  return SSG_OK;
}

int fold_check_pointers(const char* fn, const FoldSrc& s) {
  if (int rc = ssg_need_pointers(fn, s.w && s.gamma && s.beta && s.mean && s.var)) return rc;
  return ssg_need_weight_strides(fn, s.s_co, s.s_ci, s.s_r, s.s_s);
}

int fold_launch(const char* fn, const FoldSrc& a, const FoldSrc& b, int nsrc, double eps, int Cout, int split, float* w_out, float* bias, float* ch_scale,
                hipStream_t stream) {
  if (int rc = fold_check_pointers(fn, a)) return rc;
  if (nsrc == 2)
    if (int rc = fold_check_pointers(fn, b)) return rc;
  if (int rc = ssg_need_pointers(fn, w_out && bias && (ch_scale || !split))) return rc;
  if (int rc = ssg_need_aligned16(fn, "w_out", {w_out})) return rc;
  hipLaunchKernelGGL(fold_conv_bn_kernel, dim3(Cout), dim3(256), 0, stream, a, b, nsrc, eps, split ? 1 : 0, a.Cin == 3 ? 1 : 0, w_out, bias, ch_scale);
  SSG_LAUNCH_CHECK("fold_conv_bn_kernel");
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_fold_max_k(void) { return FOLD_MAX_K; }

extern "C" int ssg_fold_conv_bn_f32(const float* w, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, int Cout, int Cin, int KH, int KW, const float* gamma,
                                    const float* beta, const float* mean, const float* var, double eps, int split, float* w_out, float* bias, float* ch_scale,
                                    hipStream_t stream) {
  const char* fn = "ssg_fold_conv_bn_f32";
  FoldSrc a = {w, s_co, s_ci, s_r, s_s, gamma, beta, mean, var, Cin, KH, KW, 0};
  if (int rc = fold_check_source(fn, "source", Cout, Cin, KH, KW, true, &a.K)) return rc;
  return fold_launch(fn, a, a, 1, eps, Cout, split, w_out, bias, ch_scale, stream);
}

extern "C" int ssg_fold_conv_bn_dual_f32(const float* w1, int64_t s1_co, int64_t s1_ci, int64_t s1_r, int64_t s1_s, int Cin1, int KH1, int KW1, const float* gamma1,
                                         const float* beta1, const float* mean1, const float* var1, const float* w2, int64_t s2_co, int64_t s2_ci, int64_t s2_r,
                                         int64_t s2_s, int Cin2, int KH2, int KW2, const float* gamma2, const float* beta2, const float* mean2, const float* var2,
                                         double eps, int Cout, int split, float* w_out, float* bias, float* ch_scale, hipStream_t stream) {
  const char* fn = "ssg_fold_conv_bn_dual_f32";
  FoldSrc a = {w1, s1_co, s1_ci, s1_r, s1_s, gamma1, beta1, mean1, var1, Cin1, KH1, KW1, 0};
  FoldSrc b = {w2, s2_co, s2_ci, s2_r, s2_s, gamma2, beta2, mean2, var2, Cin2, KH2, KW2, 0};
  if (KH1 != 1 || KW1 != 1 || KH2 != 1 || KW2 != 1) {
    ssg_set_error("%s: unsupported shape: both sources of the dual form are 1x1 convolutions (first %dx%d, second %dx%d)", fn, KH1, KW1, KH2, KW2);
    return SSG_ERR_INVALID;
  }
  if (int rc = fold_check_source(fn, "first source", Cout, Cin1, KH1, KW1, false, &a.K)) return rc;
  if (int rc = fold_check_source(fn, "second source", Cout, Cin2, KH2, KW2, false, &b.K)) return rc;
  if (a.K + b.K > FOLD_MAX_K) {
    ssg_set_error("%s: unsupported shape (Cin1=%d Cin2=%d): a packed row of %d floats is beyond the %d that fit in LDS", fn, Cin1, Cin2, a.K + b.K, FOLD_MAX_K);
    return SSG_ERR_INVALID;
  }
  return fold_launch(fn, a, b, 2, eps, Cout, split, w_out, bias, ch_scale, stream);
}
