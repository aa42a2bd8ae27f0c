// inception.hip -- the layers of the InceptionNet embedder (reid/models/inception.py:50-119) that the ResNet kernels of conv.hip
// do not cover: convolutions with 32 output channels (the stem conv1 / conv2 / conv3), convolutions and pools that write a CHANNEL SLICE
// of a wider [B,H,W,Ctot] tensor (the branches of a block land where torch.cat would put them: no concatenation pass), MaxPool2d(2,2,1),
// AvgPool2d(3,1,1) and the head's ReLU / L2 norm.  Both activation layouts of conv.hip: fp32 NHWC and "h8l8" split halves.
//
// Convolution: the implicit GEMM of conv.hip (m = output pixel, n = output channel, weights [Cout][Kpad] in the same reduction order,
// D = W_tile * A_tile^T on v_mfma_f32_32x32x2_f32 or, split, three v_mfma_f32_32x32x16_f16 products per k-step) WITHOUT an LDS
// stage: every wave owns 64 pixels x 32 or 64 channels and its lanes read their own operand rows -- a lane's MFMA operands of one
// k-group are 16 (fp32) or 32 (split) contiguous bytes of its pixel / its weight row -- straight from global memory.  These maps are small
// and ragged (73 x 29 ... 10 x 4) and the 32-channel layers are byte-bound (K = 27 and 288); the rows a workgroup re-reads for the
// nine taps come from L1/L2.  No barrier, no shared memory; a wave whose tile lies behind M leaves at once.
#include "ssg_common.h"
#include "train_common.h"

namespace ssg {

struct IncConvParams {
  const float* in; const float* w; const float* bias; const float* cscale; float* out; int* overflow;
  int B, H, W, Cin, OH, OW, Cout, K, stride, pad, relu;
  int M, Kpad;        // M = B*OH*OW, Kpad = weight row length in floats
  int out_ld;         // floats between two output pixels (the width of the tensor the slice lies in); out points at the slice
  int out_split;      // out is h8l8
};

__device__ __forceinline__ v16f inc_mma_f32(const float4 w, const float4 a, v16f acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, a.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, a.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, a.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, a.w, acc, 0, 0, 0);
  return acc;
}
// x*w = xh*wl + xl*wh + xh*wh (conv.hip split_mma_step)
__device__ __forceinline__ v16f inc_mma_split(const v8h wh, const v8h wl, const v8h ah, const v8h al, v16f acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, al, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, ah, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, ah, acc, 0, 0, 0);
  return acc;
}
// two h4l4 taps (16 bytes each: [4 hi][4 lo]) -> the 8 hi and the 8 lo halves of one k-group
__device__ __forceinline__ void inc_taps_h4l4(const float4 t0, const float4 t1, v8h& hi, v8h& lo) {
  const v4f h = {t0.x, t0.y, t1.x, t1.y}, l = {t0.z, t0.w, t1.z, t1.w};
  hi = __builtin_bit_cast(v8h, h); lo = __builtin_bit_cast(v8h, l);
}

// NT: 32-channel MFMA tiles per wave (1: Cout % 32, 2: Cout % 64).  CIN4: the input is the 4-channel image layout
// (ssg_nchw_to_nhwc4 / _h4l4), one 16-byte unit per filter tap, weights [Cout][32 * ceil(K*K / 8)] tap-major.
template <int NT, bool SPLIT, bool CIN4>
__global__ __launch_bounds__(256) void inc_conv_kernel(const IncConvParams p) {
  constexpr int MT = 2;
  const int lane = (int)threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
  const int tiles_n = p.Cout / (32 * NT);
  const int64_t gw = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  const int tm = (int)(gw / tiles_n), tn = (int)(gw - (int64_t)tm * tiles_n);
  if ((int64_t)tm * 64 >= p.M) return;                       // wave-uniform; the kernel has no barrier

  int pb[MT], ph[MT], pw[MT]; bool pv[MT];
#pragma unroll
  for (int i = 0; i < MT; i++) {
    const int m = tm * 64 + i * 32 + l32;
    pv[i] = m < p.M;
    const int mm = pv[i] ? m : 0;
    const int b = mm / (p.OH * p.OW), rem = mm - b * (p.OH * p.OW), oh = rem / p.OW;
    pb[i] = b; ph[i] = oh * p.stride - p.pad; pw[i] = (rem - oh * p.OW) * p.stride - p.pad;
  }
  const float* wrow[NT];
#pragma unroll
  for (int j = 0; j < NT; j++) wrow[j] = p.w + (int64_t)(tn * 32 * NT + j * 32 + l32) * p.Kpad;

  v16f acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; i++)
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

  const int KK = p.K * p.K;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (CIN4) {
    // a k-group is two taps (fp32: one tap per half-wave; split: two taps per half-wave, four per k-step); taps behind the last one
    // read zeros on both sides (the fold leaves the weight row's tail zero)
    const int per = SPLIT ? 4 : 2, steps = (KK + per - 1) / per;
    for (int st = 0; st < steps; st++) {
      const int t0 = SPLIT ? st * 4 + h * 2 : st * 2 + h;
      float4 a0[MT], a1[MT];
#pragma unroll
      for (int i = 0; i < MT; i++) {
        a0[i] = a1[i] = zero4;
#pragma unroll
        for (int u = 0; u < (SPLIT ? 2 : 1); u++) {
          const int t = t0 + u, r = t / p.K, s = t - r * p.K;
          const int ih = ph[i] + r, iw = pw[i] + s;
          if (pv[i] && t < KK && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
            const float4 v = *reinterpret_cast<const float4*>(p.in + ((int64_t)(pb[i] * p.H + ih) * p.W + iw) * 4);
            if (u == 0) a0[i] = v; else a1[i] = v;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const float4 w0 = *reinterpret_cast<const float4*>(wrow[j] + t0 * 4);
        if (SPLIT) {
          const float4 w1 = *reinterpret_cast<const float4*>(wrow[j] + t0 * 4 + 4);
          v8h wh, wl;
          inc_taps_h4l4(w0, w1, wh, wl);
#pragma unroll
          for (int i = 0; i < MT; i++) {
            v8h ah, al;
            inc_taps_h4l4(a0[i], a1[i], ah, al);
            acc[i][j] = inc_mma_split(wh, wl, ah, al, acc[i][j]);
          }
        } else {
#pragma unroll
          for (int i = 0; i < MT; i++) acc[i][j] = inc_mma_f32(w0, a0[i], acc[i][j]);
        }
      }
    }
  } else {
    const int chunks = p.Cin / 32;
    for (int cc = 0; cc < chunks; cc++) {
      for (int t = 0; t < KK; t++) {
        const int r = t / p.K, s = t - r * p.K;
        const float* arow[MT]; bool ok[MT];
#pragma unroll
        for (int i = 0; i < MT; i++) {
          const int ih = ph[i] + r, iw = pw[i] + s;
          ok[i] = pv[i] && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
          arow[i] = p.in + ((int64_t)(pb[i] * p.H + (ok[i] ? ih : 0)) * p.W + (ok[i] ? iw : 0)) * p.Cin + cc * 32;
        }
        const int kb = (cc * KK + t) * 32;
        if (SPLIT) {
#pragma unroll
          for (int st = 0; st < 2; st++) {                     // 16 channels per k-step; half-wave h takes the 8-channel group 2*st + h
            const int o = (2 * st + h) * 8;
            v8h ah[MT], al[MT];
#pragma unroll
            for (int i = 0; i < MT; i++) {
              float4 q0 = *reinterpret_cast<const float4*>(arow[i] + o), q1 = *reinterpret_cast<const float4*>(arow[i] + o + 4);
              if (!ok[i]) q0 = q1 = zero4;                       // (arow is a valid address either way)
              ah[i] = __builtin_bit_cast(v8h, q0); al[i] = __builtin_bit_cast(v8h, q1);
            }
#pragma unroll
            for (int j = 0; j < NT; j++) {
              const v8h wh = *reinterpret_cast<const v8h*>(wrow[j] + kb + o), wl = *reinterpret_cast<const v8h*>(wrow[j] + kb + o + 4);
#pragma unroll
              for (int i = 0; i < MT; i++) acc[i][j] = inc_mma_split(wh, wl, ah[i], al[i], acc[i][j]);
            }
          }
        } else {
#pragma unroll
          for (int g = 0; g < 4; g++) {                        // 8 channels per group; half-wave h takes channels 8g + 4h .. + 3
            const int o = g * 8 + h * 4;
            float4 a[MT];
#pragma unroll
            for (int i = 0; i < MT; i++) {
              a[i] = *reinterpret_cast<const float4*>(arow[i] + o);
              if (!ok[i]) a[i] = zero4;                          // (arow is a valid address either way)
            }
#pragma unroll
            for (int j = 0; j < NT; j++) {
              const float4 wv = *reinterpret_cast<const float4*>(wrow[j] + kb + o);
#pragma unroll
              for (int i = 0; i < MT; i++) acc[i][j] = inc_mma_f32(wv, a[i], acc[i][j]);
            }
          }
        }
      }
    }
  }

  // epilogue: lane (l32, h) holds, of pixel l32 of each pixel tile, the channels 8q + 4h .. + 3 of each channel tile (q = 0..3)
#pragma unroll
  for (int j = 0; j < NT; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ch = tn * 32 * NT + j * 32 + 8 * q + 4 * h;
      const float4 bias = *reinterpret_cast<const float4*>(p.bias + ch);
      const float4 cs = p.cscale ? *reinterpret_cast<const float4*>(p.cscale + ch) : make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
      for (int i = 0; i < MT; i++) {
        const int m = tm * 64 + i * 32 + l32;
        float4 v = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
        v.x = v.x * cs.x + bias.x; v.y = v.y * cs.y + bias.y; v.z = v.z * cs.z + bias.z; v.w = v.w * cs.w + bias.w;
        if (p.relu) { v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f; }
        if (!pv[i]) continue;
        float* o = p.out + (int64_t)m * p.out_ld;
        if (p.out_split) {                                     // the 8-channel group [8 hi][8 lo]: this lane's four channels are its half h
          uint2 hp, lp;
          split_encode4(v, hp, lp);
          if (p.overflow && split_hi_nonfinite(hp)) *p.overflow = 1;
          const int g0 = ch - 4 * h;
          *reinterpret_cast<uint2*>(o + g0 + 2 * h) = hp;
          *reinterpret_cast<uint2*>(o + g0 + 4 + 2 * h) = lp;
        } else *reinterpret_cast<float4*>(o + ch) = v;
      }
    }
}

// ---- pools.  One thread per (output pixel, 4 channels) or, h8l8, (output pixel, 8-channel group); out_ld as above.
// MaxPool2d(k, stride, pad): padding never wins (-inf start, taps outside the map are skipped); exact.
template <bool SPLIT>
__global__ void inc_maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int H, int W, int C, int OH, int OW, int k, int stride,
                                   int pad, int out_ld) {
  constexpr int V = SPLIT ? 8 : 4;
  const int CV = C / V;
  const int64_t total = (int64_t)B * OH * OW * CV;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int cv = (int)(x % CV); int64_t t = x / CV;
    const int ow = (int)(t % OW); t /= OW; const int oh = (int)(t % OH); const int b = (int)(t / OH);
    float4 m0 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), m1 = m0;
    for (int r = 0; r < k; r++) {
      const int ih = oh * stride - pad + r; if (ih < 0 || ih >= H) continue;
      for (int s = 0; s < k; s++) {
        const int iw = ow * stride - pad + s; if (iw < 0 || iw >= W) continue;
        const float* q = in + ((int64_t)(b * H + ih) * W + iw) * C + cv * V;
        float4 a, c = m1;
        if (SPLIT) h8l8_load8(q, a, c); else a = *reinterpret_cast<const float4*>(q);
        m0.x = fmaxf(m0.x, a.x); m0.y = fmaxf(m0.y, a.y); m0.z = fmaxf(m0.z, a.z); m0.w = fmaxf(m0.w, a.w);
        m1.x = fmaxf(m1.x, c.x); m1.y = fmaxf(m1.y, c.y); m1.z = fmaxf(m1.z, c.z); m1.w = fmaxf(m1.w, c.w);
      }
    }
    float* o = out + ((int64_t)(b * OH + oh) * OW + ow) * out_ld + cv * V;
    if (SPLIT) h8l8_store8(o, m0, m1); else *reinterpret_cast<float4*>(o) = m0;
  }
}

// AvgPool2d(3, 1, 1), count_include_pad: float32 sum of the nine taps in row-major order (r = 0..2 outer, s = 0..2 inner) starting from
// +0, a tap outside the map adds nothing; then one float32 division by 9.  h8l8: taps decoded (hi + lo), the quotient encoded again.
template <bool SPLIT>
__global__ void inc_avgpool3_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int H, int W, int C, int out_ld) {
  constexpr int V = SPLIT ? 8 : 4;
  const int CV = C / V;
  const int64_t total = (int64_t)B * H * W * CV;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int cv = (int)(x % CV); int64_t t = x / CV;
    const int ow = (int)(t % W); t /= W; const int oh = (int)(t % H); const int b = (int)(t / H);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    for (int r = 0; r < 3; r++) {
      const int ih = oh - 1 + r; if (ih < 0 || ih >= H) continue;
      for (int s = 0; s < 3; s++) {
        const int iw = ow - 1 + s; if (iw < 0 || iw >= W) continue;
        const float* q = in + ((int64_t)(b * H + ih) * W + iw) * C + cv * V;
        float4 a, c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (SPLIT) h8l8_load8(q, a, c); else a = *reinterpret_cast<const float4*>(q);
        s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
        s1.x += c.x; s1.y += c.y; s1.z += c.z; s1.w += c.w;
      }
    }
    s0.x /= 9.f; s0.y /= 9.f; s0.z /= 9.f; s0.w /= 9.f; s1.x /= 9.f; s1.y /= 9.f; s1.z /= 9.f; s1.w /= 9.f;
    float* o = out + ((int64_t)(b * H + oh) * W + ow) * out_ld + cv * V;
    if (SPLIT) h8l8_store8(o, s0, s1); else *reinterpret_cast<float4*>(o) = s0;
  }
}

// head (inception.py:111-114): mode 0 out = relu(x); mode 1 out = x / max(||x||_2, 1e-12) per row (F.normalize); one wave per row
__global__ __launch_bounds__(256) void inc_head_finish_kernel(const float* __restrict__ x, float* __restrict__ out, int rows, int C, int mode) {
  const int row = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= rows) return;
  const int lane = lane_id();
  const float* px = x + (int64_t)row * C;
  float* po = out + (int64_t)row * C;
  if (mode == 0) {
    for (int c = lane; c < C; c += 64) { const float v = px[c]; po[c] = v > 0.f ? v : 0.f; }
    return;
  }
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) ss += px[c] * px[c];
  for (int sh = 1; sh < 64; sh <<= 1) ss += __shfl_xor(ss, sh, 64);
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  for (int c = lane; c < C; c += 64) po[c] = px[c] / nrm;
}

}  // namespace ssg

namespace {

using namespace ssg;

// a slice of `width` channels at out (already offset) inside rows of out_ld floats, in units of the layout's channel group
int inc_check_slice(const char* fn, const void* in, const void* out, int width, int out_ld, int unit) {
  if (int rc = ssg_need_pointers(fn, in && out)) return rc;
  if (int rc = ssg_need_aligned16(fn, "in and out", {in, out})) return rc;
  if (out_ld < width || (out_ld % unit) || (((uintptr_t)out / 4) % unit)) {
    ssg_set_error("%s: the output slice needs out_ld >= %d and out_ld, the slice offset multiples of %d channels (out_ld=%d)", fn, width, unit, out_ld);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

int inc_check_bytes(const char* fn, int64_t in_bytes, int64_t out_bytes) {
  if (in_bytes > 0x7fffffffLL || out_bytes > 0x7fffffffLL) {
    ssg_set_error("%s: tensor of %lld bytes exceeds the 2 GiB buffer-resource range of this kernel; use a smaller batch", fn,
                  (long long)(in_bytes > out_bytes ? in_bytes : out_bytes));
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_inc_conv2d_nhwc_x(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout, int K,
                                     int stride, int pad, int relu, int flags, const float* ch_scale, int out_ld, int32_t* overflow, hipStream_t stream) {
  const char* fn = "ssg_inc_conv2d_nhwc_x";
  const bool in_split = (flags & 1) != 0, out_split = (flags & 2) != 0, cin4 = Cin == 4;
  if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || (Cout % 32) || !(cin4 || (Cin > 0 && Cin % 32 == 0)) || !(K == 1 || K == 3) || (cin4 && K != 3) ||
      stride < 1 || stride > 2 || pad < 0 || pad > 1 || H + 2 * pad < K || W + 2 * pad < K) {
    ssg_set_error("%s: unsupported shape B=%d H=%d W=%d Cin=%d Cout=%d k=%d s=%d p=%d (Cout %% 32 == 0, Cin %% 32 == 0 or 4, 1x1 or 3x3, stride 1 or 2)",
                  fn, B, H, W, Cin, Cout, K, stride, pad);
    return SSG_ERR_INVALID;
  }
  IncConvParams p;
  p.OH = (H + 2 * pad - K) / stride + 1; p.OW = (W + 2 * pad - K) / stride + 1;
  const int64_t M = (int64_t)B * p.OH * p.OW;
  if (int rc = inc_check_bytes(fn, (int64_t)B * H * W * Cin * 4, M * out_ld * 4)) return rc;
  if (int rc = ssg_need_pointers(fn, w && bias && (ch_scale || !in_split))) return rc;
  if (int rc = ssg_need_aligned16(fn, "w, bias and ch_scale", {w, bias, ch_scale})) return rc;
  if (int rc = inc_check_slice(fn, in, out, Cout, out_ld, 8)) return rc;
  p.in = (const float*)in; p.w = (const float*)w; p.bias = bias; p.cscale = ch_scale; p.out = (float*)out; p.overflow = out_split ? overflow : nullptr;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = K; p.stride = stride; p.pad = pad; p.relu = relu;
  p.M = (int)M; p.Kpad = cin4 ? 32 * ((K * K + 7) / 8) : K * K * Cin; p.out_ld = out_ld; p.out_split = out_split ? 1 : 0;
  const int nt = (Cout % 64 == 0) ? 2 : 1;
  const int64_t waves = ((M + 63) / 64) * (Cout / (32 * nt));
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
#define SSG_INC_LAUNCH(NT_, SP_, C4_) hipLaunchKernelGGL((inc_conv_kernel<NT_, SP_, C4_>), grid, block, 0, stream, p)
  if (nt == 2) {
    if (in_split) { if (cin4) SSG_INC_LAUNCH(2, true, true); else SSG_INC_LAUNCH(2, true, false); }
    else { if (cin4) SSG_INC_LAUNCH(2, false, true); else SSG_INC_LAUNCH(2, false, false); }
  } else {
    if (in_split) { if (cin4) SSG_INC_LAUNCH(1, true, true); else SSG_INC_LAUNCH(1, true, false); }
    else { if (cin4) SSG_INC_LAUNCH(1, false, true); else SSG_INC_LAUNCH(1, false, false); }
  }
#undef SSG_INC_LAUNCH
  SSG_LAUNCH_CHECK("inc_conv_kernel");
  return SSG_OK;
}

extern "C" int ssg_inc_maxpool_nhwc_x(const void* in, void* out, int B, int H, int W, int C, int k, int stride, int pad, int split, int out_ld,
                                      hipStream_t stream) {
  const char* fn = "ssg_inc_maxpool_nhwc_x";
  const int unit = split ? 8 : 4;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % unit) || k < 1 || k > 3 || stride < 1 || stride > 2 || pad < 0 || 2 * pad > k || H + 2 * pad < k ||
      W + 2 * pad < k) {
    ssg_set_error("%s: unsupported shape B=%d H=%d W=%d C=%d k=%d s=%d p=%d (C %% %d == 0, k <= 3, stride <= 2, 2 * pad <= k)", fn, B, H, W, C, k, stride, pad, unit);
    return SSG_ERR_INVALID;
  }
  const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
  if (int rc = inc_check_bytes(fn, (int64_t)B * H * W * C * 4, (int64_t)B * OH * OW * out_ld * 4)) return rc;
  if (int rc = inc_check_slice(fn, in, out, C, out_ld, unit)) return rc;
  const int64_t total = (int64_t)B * OH * OW * (C / unit);
  const dim3 grid((unsigned)ssg_blocks256(total, 1 << 20)), block(256);
  if (split) hipLaunchKernelGGL((inc_maxpool_kernel<true>), grid, block, 0, stream, (const float*)in, (float*)out, B, H, W, C, OH, OW, k, stride, pad, out_ld);
  else hipLaunchKernelGGL((inc_maxpool_kernel<false>), grid, block, 0, stream, (const float*)in, (float*)out, B, H, W, C, OH, OW, k, stride, pad, out_ld);
  SSG_LAUNCH_CHECK("inc_maxpool_kernel");
  return SSG_OK;
}

extern "C" int ssg_inc_avgpool3_nhwc_x(const void* in, void* out, int B, int H, int W, int C, int split, int out_ld, hipStream_t stream) {
  const char* fn = "ssg_inc_avgpool3_nhwc_x";
  const int unit = split ? 8 : 4;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % unit)) {
    ssg_set_error("%s: unsupported shape B=%d H=%d W=%d C=%d (C %% %d == 0)", fn, B, H, W, C, unit);
    return SSG_ERR_INVALID;
  }
  if (int rc = inc_check_bytes(fn, (int64_t)B * H * W * C * 4, (int64_t)B * H * W * out_ld * 4)) return rc;
  if (int rc = inc_check_slice(fn, in, out, C, out_ld, unit)) return rc;
  const int64_t total = (int64_t)B * H * W * (C / unit);
  const dim3 grid((unsigned)ssg_blocks256(total, 1 << 20)), block(256);
  if (split) hipLaunchKernelGGL((inc_avgpool3_kernel<true>), grid, block, 0, stream, (const float*)in, (float*)out, B, H, W, C, out_ld);
  else hipLaunchKernelGGL((inc_avgpool3_kernel<false>), grid, block, 0, stream, (const float*)in, (float*)out, B, H, W, C, out_ld);
  SSG_LAUNCH_CHECK("inc_avgpool3_kernel");
  return SSG_OK;
}

extern "C" int ssg_inc_head_finish(const float* x, float* out, int rows, int C, int mode, hipStream_t stream) {
  const char* fn = "ssg_inc_head_finish";
  if (rows <= 0 || C <= 0 || (mode != 0 && mode != 1)) { ssg_set_error("%s: rows=%d C=%d mode=%d", fn, rows, C, mode); return SSG_ERR_INVALID; }
  if (int rc = ssg_need_pointers(fn, x && out)) return rc;
  hipLaunchKernelGGL(inc_head_finish_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, out, rows, C, mode);
  SSG_LAUNCH_CHECK("inc_head_finish_kernel");
  return SSG_OK;
}
