// conv_train.hip -- train-mode Conv2d of the fine-tune phase: weight packing and the weight gradient (gfx950 only).
//
// The reference trains torch's ResNet (reid/trainers.py), whose convolutions are cuDNN / MIOpen forward, data gradient and weight
// gradient.  Here, for the class  groups 1, dilation 1, no bias, stride 1, 1x1 pad 0 or 3x3 pad 1, Cin % 64 == 0, Cout % 64 == 0,
// float32 NHWC:
//   forward  y  = ssg_conv2d_nhwc_f32(x,  w_fwd)                       (csrc/conv.hip, zero bias, no residual, no ReLU)
//   dgrad    dX = ssg_conv2d_nhwc_f32(dY, w_dgrad)                     the same kernel: the data gradient of a stride-1 convolution
//                                                                      is the stride-1 convolution of dY with the weight transposed
//                                                                      in (Cout, Cin) and rotated by 180 degrees in (r, s)
//   wgrad    dW[co][tap][ci] = sum_m dY[m][co] * x[m + tap shift][ci]  this file
// ssg_conv_pack_train_f32 writes w_fwd and w_dgrad from the [Cout,Cin,KH,KW] weight in one launch (the weight changes every step).
//
// Weight gradient, two stages, no float atomics:
//   1. the pixel range M = B*H*W is cut into num_slices contiguous slices of slice_len pixels (a function of the shape alone,
//      ssg_conv_wgrad_num_slices).  One workgroup owns a (Cout tile of 64 or 128) x (K tile = one tap x 64 input channels) x slice
//      triple: it stages 32 pixels of dY rows and of tap-shifted x rows (zeros outside the image) through LDS and accumulates on
//      v_mfma_f32_32x32x2_f32 with A[i = co][k = pixel], B[k = pixel][j = ci].  In NHWC both operands have their lane index (co, ci)
//      contiguous in memory and in LDS, so no tile is transposed and every LDS read is 32 consecutive dwords.  The fp32 partial tile
//      goes to ws [slice][Cout][KH*KW*Cin].
//   2. every element adds its slices in float64 in ascending slice order, rounds once and is stored with the caller's strides.
#include "train_common.h"

namespace ssg {

constexpr int WG_PIX = 32;          // pixels per LDS stage
constexpr int WG_MIN_SLICE = 256;   // pixels: below this a slice is not worth its workspace pass
constexpr int WG_TARGET = 1024;     // workgroups wanted in stage 1 (4 per CU)

__global__ __launch_bounds__(256) void conv_pack_train_kernel(const float* __restrict__ w, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int Cout,
                                                              int Cin, int KH, int KW, float* __restrict__ w_fwd, float* __restrict__ w_dgrad) {
  const int T = KH * KW;
  const int64_t Kf = (int64_t)T * Cin, Kd = (int64_t)T * Cout, total = (int64_t)Cout * Kf;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(idx / Kf), k = (int)(idx % Kf);
    const int chunk = k / (T * 32), rem = k % (T * 32), tap = rem >> 5, ci = chunk * 32 + (rem & 31);
    const int r = tap / KW, s = tap % KW;
    const float v = w[co * s0 + ci * s1 + r * s2 + s * s3];
    if (w_fwd) w_fwd[idx] = v;
    if (w_dgrad) w_dgrad[ci * Kd + ((int64_t)(co >> 5) * T + (KH - 1 - r) * KW + (KW - 1 - s)) * 32 + (co & 31)] = v;
  }
}

// stage 1.  grid (K tiles = KH*KW*Cin/64, Cout / (64*CT), slices); 256 threads = 2 x 2 waves, wave (wr, wc) owns CT 32x32 tiles:
// co rows (wr*CT + i)*32 .. +32, ci columns wc*32 .. +32 of the workgroup's tile.
// MODE picks the x row of output pixel m and tap (r, s) -- the only thing the strided convolutions (csrc/conv_strided.hip) change:
//   WG_UNIT   stride 1: the output pixel's own row shifted by the tap, H x W is both the input and the output size
//   WG_STRIDE (oh*stride + r - pad, ow*stride + s - pad) of an H x W input; M counts the B*OH*OW output pixels
//   WG_STEM   the same on RGB0 pixels (Cin = 4 in memory): the K tile is 16 taps x 4 channels, grid.x = ceil(KH*KW/16) tiles, the taps
//             from KH*KW up are zero; ws rows are gridDim.x*64 long, k = tap*4 + c
enum { WG_UNIT = 0, WG_STRIDE = 1, WG_STEM = 2 };
template <int CT, int MODE = WG_UNIT>
__global__ __launch_bounds__(256) void conv_wgrad_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ ws, int H,
                                                                 int W, int Cin, int Cout, int KH, int KW, int pad, int M, int slice_len, int OH = 0,
                                                                 int OW = 0, int stride = 1) {
  constexpr int CO_T = 64 * CT;                 // Cout tile
  constexpr int YV = CO_T / 4;                  // float4 per dY row of the tile
  __shared__ float4 ys[WG_PIX * YV];
  __shared__ float4 xs[WG_PIX * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int cchunks = MODE == WG_STEM ? 1 : Cin >> 6;
  const int tap = blockIdx.x / cchunks, ci0 = (blockIdx.x % cchunks) << 6, co0 = blockIdx.y * CO_T;      // WG_STEM: tap = the tile of 16 taps
  const int dr = tap / KW - pad, ds = tap % KW - pad;
  const int64_t m_begin = (int64_t)blockIdx.z * slice_len;
  const int64_t m_end = m_begin + slice_len < (int64_t)M ? m_begin + slice_len : (int64_t)M;

  float4 yr[2 * CT], xr[2];
  auto load = [&](int64_t m0) {
#pragma unroll
    for (int u = 0; u < 2 * CT; u++) {
      const int f = tid + 256 * u, row = f / YV, c4 = f % YV;
      const int64_t m = m0 + row;
      yr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < m_end) yr[u] = *reinterpret_cast<const float4*>(dy + m * Cout + co0 + c4 * 4);
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int f = tid + 256 * u, row = f >> 4, c4 = f & 15;
      const int64_t m = m0 + row;
      xr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (MODE == WG_UNIT) {
        if (m < m_end) {
          const int ow = (int)(m % W), oh = (int)((m / W) % H);
          const int ih = oh + dr, iw = ow + ds;
          if (ih >= 0 && ih < H && iw >= 0 && iw < W)      // the tap stays inside the pixel's own image: m + dr*W + ds is in [0, M)
            xr[u] = *reinterpret_cast<const float4*>(x + (m + (int64_t)dr * W + ds) * Cin + ci0 + c4 * 4);
        }
      } else if (m < m_end) {
        const int ow = (int)(m % OW), oh = (int)((m / OW) % OH);
        const int64_t b = m / ((int64_t)OW * OH);
        const int t = MODE == WG_STEM ? tap * 16 + c4 : tap;                 // WG_STEM: this float4 is one tap's RGB0 pixel
        const int ih = oh * stride + t / KW - pad, iw = ow * stride + t % KW - pad;
        if (t < KH * KW && ih >= 0 && ih < H && iw >= 0 && iw < W) {         // inside image b: the row index is in [0, B*H*W)
          const int64_t row = (b * H + ih) * W + iw;
          xr[u] = *reinterpret_cast<const float4*>(MODE == WG_STEM ? x + row * 4 : x + row * Cin + ci0 + c4 * 4);
        }
      }
    }
  };

  f32x16 acc[CT];
#pragma unroll
  for (int i = 0; i < CT; i++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[i][e] = 0.f;

  const float* ysf = reinterpret_cast<const float*>(ys);
  const float* xsf = reinterpret_cast<const float*>(xs);
  const int l31 = lane & 31, lk = lane >> 5;
  if (m_begin < m_end) load(m_begin);
  for (int64_t m0 = m_begin; m0 < m_end; m0 += WG_PIX) {
#pragma unroll
    for (int u = 0; u < 2 * CT; u++) ys[tid + 256 * u] = yr[u];
#pragma unroll
    for (int u = 0; u < 2; u++) xs[tid + 256 * u] = xr[u];
    __syncthreads();
    if (m0 + WG_PIX < m_end) load(m0 + WG_PIX);          // the next stage's global loads fly under this stage's MFMAs
#pragma unroll
    for (int kk = 0; kk < WG_PIX / 2; kk++) {
      const int px = 2 * kk + lk;
      const float b = xsf[px * 64 + wc * 32 + l31];
#pragma unroll
      for (int i = 0; i < CT; i++) {
        const float a = ysf[px * CO_T + (wr * CT + i) * 32 + l31];
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  const int64_t Ktot = MODE == WG_STEM ? (int64_t)gridDim.x * 64 : (int64_t)KH * KW * Cin;
  float* out = ws + (int64_t)blockIdx.z * Cout * Ktot + (MODE == WG_STEM ? (int64_t)tap * 64 : (int64_t)tap * Cin + ci0) + wc * 32 + l31;
#pragma unroll
  for (int i = 0; i < CT; i++)
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int co = co0 + (wr * CT + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lk;   // C/D map of the 32x32 MFMA: row = co, column = lane & 31 = ci
      out[co * Ktot] = acc[i][e];
    }
}

// stage 2: dW[co][ci][r][s] = float(sum over slices, float64, ascending)
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, int slices, int Cout, int Cin, int KH, int KW,
                                                                float* __restrict__ dw, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
  const int64_t Ktot = (int64_t)KH * KW * Cin, total = (int64_t)Cout * Ktot;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    double sum = 0.0;
    for (int sl = 0; sl < slices; sl++) sum += (double)ws[sl * total + idx];
    const int co = (int)(idx / Ktot), k = (int)(idx % Ktot), tap = k / Cin, ci = k % Cin;
    dw[co * s0 + ci * s1 + (tap / KW) * s2 + (tap % KW) * s3] = (float)sum;
  }
}

// stage 2 of the stem (csrc/conv_strided.hip, with the stem's other kernels)
__global__ __launch_bounds__(256) void conv_wgrad_reduce_stem_kernel(const float* __restrict__ ws, int slices, int Cout, int KH, int KW, int Kws,
                                                                     float* __restrict__ dw, int64_t s0, int64_t s1, int64_t s2, int64_t s3);

}  // namespace ssg

namespace {

using namespace ssg;

struct WgradPlan { int ct, slices, slice_len; };

int conv_train_check_shape(const char* fn, int64_t M, int Cout, int KH, int KW, int Cin) {
  const bool k1 = (KH == 1 && KW == 1), k3 = (KH == 3 && KW == 3);
  if (M <= 0 || M > 0x7fffffffLL || Cin <= 0 || Cout <= 0 || (Cin % 64) || (Cout % 64) || !(k1 || k3)) {
    ssg_set_error("%s: the train-mode convolution is 1x1 (pad 0) or 3x3 (pad 1), stride 1, Cin %% 64 == 0, Cout %% 64 == 0, 0 < B*H*W < 2^31 "
                  "(M=%lld Cin=%d Cout=%d k=%dx%d)", fn, (long long)M, Cin, Cout, KH, KW);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

constexpr int STEM_KTILES = 13;                         // ceil(49 / 16) K tiles of 16 taps x RGB0
constexpr int STEM_KWS = STEM_KTILES * 64;              // workspace row of the stem: 208 taps x 4 channels

// The functions below take the class of the convolution as the MODE of its stage 1 kernel (WG_UNIT, WG_STRIDE or WG_STEM), already
// validated by the caller, and M = the B*OH*OW output pixels.

// K tiles of 64 columns: one tap x 64 input channels; the stem: 16 taps x RGB0
int wgrad_ktiles(int mode, int KH, int KW, int Cin) { return mode == WG_STEM ? STEM_KTILES : KH * KW * Cin / 64; }

// floats of one workspace row
size_t wgrad_row(int mode, int KH, int KW, int Cin) { return mode == WG_STEM ? (size_t)STEM_KWS : (size_t)KH * KW * Cin; }

WgradPlan wgrad_plan(int mode, int M, int Cout, int KH, int KW, int Cin) {
  WgradPlan p;
  p.ct = (Cout % 128 == 0) ? 2 : 1;
  const int64_t tiles = (int64_t)(Cout / (64 * p.ct)) * wgrad_ktiles(mode, KH, KW, Cin);
  const int64_t want = (WG_TARGET + tiles - 1) / tiles;                    // >= 1
  int64_t len = ((int64_t)M + want - 1) / want;
  len = (len + WG_PIX - 1) / WG_PIX * WG_PIX;
  if (len < WG_MIN_SLICE) len = WG_MIN_SLICE;
  p.slice_len = (int)(len > 0x7fffffc0LL ? 0x7fffffc0LL : len);
  p.slices = (int)(((int64_t)M + p.slice_len - 1) / p.slice_len);
  return p;
}

size_t wgrad_workspace_bytes(int mode, int M, int Cout, int KH, int KW, int Cin) {
  return (size_t)wgrad_plan(mode, M, Cout, KH, KW, Cin).slices * Cout * wgrad_row(mode, KH, KW, Cin) * sizeof(float);
}

// what both weight gradient entry points refuse first
int wgrad_check_call(const char* fn, int stages, int B, int H, int W) {
  if (stages < 1 || stages > 3) { ssg_set_error("%s: stages=%d (1: partial tiles, 2: slice sum, 3: both)", fn, stages); return SSG_ERR_INVALID; }
  if (B <= 0 || H <= 0 || W <= 0) { ssg_set_error("%s: empty input B=%d H=%d W=%d", fn, B, H, W); return SSG_ERR_INVALID; }
  return SSG_OK;
}

// The weight gradient of every class behind ssg_conv_wgrad_f32 and ssg_conv_wgrad_strided_f32 (csrc/conv_strided.hip): the pointer,
// stride and workspace checks, the plan, stage 1 (CT x MODE) and the matching stage 2.  H x W is the input, OH x OW the output size.
int conv_wgrad_launch(const char* fn, int mode, const float* dy, const float* x, int H, int W, int Cin, int Cout, int KH, int KW, int OH, int OW, int stride,
                      int M, float* dw, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, void* ws, size_t ws_bytes, int stages, hipStream_t stream) {
  if (int rc = ssg_need_pointers(fn, dy && x && dw)) return rc;
  if (int rc = ssg_need_aligned16(fn, "dy and x", {dy, x})) return rc;
  if (int rc = ssg_need_weight_strides(fn, s_co, s_ci, s_r, s_s)) return rc;
  const WgradPlan p = wgrad_plan(mode, M, Cout, KH, KW, Cin);
  const size_t need = wgrad_workspace_bytes(mode, M, Cout, KH, KW, Cin);
  if (!ws || ws_bytes < need || ((uintptr_t)ws & 3)) {
    ssg_set_error("%s: workspace of %zu bytes (4-byte aligned) needed, got %zu", fn, need, ws ? ws_bytes : (size_t)0);
    return SSG_ERR_INVALID;
  }
  if (p.slices > 65535) { ssg_set_error("%s: %d slices", fn, p.slices); return SSG_ERR_INVALID; }
  const int pad = KH / 2, cin_mem = mode == WG_STEM ? 4 : Cin;             // the stem reads RGB0 pixels
  const dim3 grid(wgrad_ktiles(mode, KH, KW, Cin), Cout / (64 * p.ct), p.slices);
#define SSG_WG_PARTIAL(CT, MODE)                                                                                                                \
  hipLaunchKernelGGL((conv_wgrad_partial_kernel<CT, MODE>), grid, dim3(256), 0, stream, dy, x, (float*)ws, H, W, cin_mem, Cout, KH, KW, pad, M, \
                     p.slice_len, OH, OW, stride)
  if (!(stages & 1)) {
  } else if (mode == WG_UNIT) {
    if (p.ct == 2) SSG_WG_PARTIAL(2, WG_UNIT); else SSG_WG_PARTIAL(1, WG_UNIT);
  } else if (mode == WG_STEM) {
    SSG_WG_PARTIAL(1, WG_STEM);
  } else {
    if (p.ct == 2) SSG_WG_PARTIAL(2, WG_STRIDE); else SSG_WG_PARTIAL(1, WG_STRIDE);
  }
#undef SSG_WG_PARTIAL
  SSG_LAUNCH_CHECK(mode == WG_UNIT ? "conv_wgrad_partial_kernel" : "conv_wgrad_partial_kernel (strided)");
  if (!(stages & 2)) {
  } else if (mode == WG_STEM) {
    hipLaunchKernelGGL(conv_wgrad_reduce_stem_kernel, dim3((Cout * KH * KW * 3 + 255) / 256), dim3(256), 0, stream, (const float*)ws, p.slices, Cout, KH, KW,
                       STEM_KWS, dw, s_co, s_ci, s_r, s_s);
  } else {
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(ssg_blocks256((int64_t)Cout * KH * KW * Cin, 8192)), dim3(256), 0, stream, (const float*)ws, p.slices,
                       Cout, Cin, KH, KW, dw, s_co, s_ci, s_r, s_s);
  }
  SSG_LAUNCH_CHECK(mode == WG_UNIT ? "conv_wgrad_reduce_kernel" : "conv_wgrad_reduce_kernel (strided)");
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_conv_wgrad_num_slices(int M, int Cout, int KH, int KW, int Cin) {
  if (conv_train_check_shape("ssg_conv_wgrad_num_slices", M, Cout, KH, KW, Cin)) return SSG_ERR_INVALID;
  return wgrad_plan(WG_UNIT, M, Cout, KH, KW, Cin).slices;
}

extern "C" size_t ssg_conv_wgrad_workspace_bytes(int M, int Cout, int KH, int KW, int Cin) {
  if (conv_train_check_shape("ssg_conv_wgrad_workspace_bytes", M, Cout, KH, KW, Cin)) return 0;
  return wgrad_workspace_bytes(WG_UNIT, M, Cout, KH, KW, Cin);
}

extern "C" int ssg_conv_pack_train_f32(const float* w, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, int Cout, int Cin, int KH, int KW,
                                       float* w_fwd, float* w_dgrad, hipStream_t stream) {
  const char* fn = "ssg_conv_pack_train_f32";
  if (int rc = conv_train_check_shape(fn, 1, Cout, KH, KW, Cin)) return rc;
  if (int rc = ssg_need_pointers(fn, w && (w_fwd || w_dgrad))) return rc;
  if (int rc = ssg_need_weight_strides(fn, s_co, s_ci, s_r, s_s)) return rc;
  const int blocks = ssg_blocks256((int64_t)Cout * Cin * KH * KW, 4096);
  hipLaunchKernelGGL(conv_pack_train_kernel, dim3(blocks), dim3(256), 0, stream, w, s_co, s_ci, s_r, s_s, Cout, Cin, KH, KW, w_fwd, w_dgrad);
  SSG_LAUNCH_CHECK("conv_pack_train_kernel");
  return SSG_OK;
}

extern "C" int ssg_conv_wgrad_f32(const float* dy, const float* x, int B, int H, int W, int Cin, int Cout, int KH, int KW, float* dw, int64_t s_co,
                                  int64_t s_ci, int64_t s_r, int64_t s_s, void* ws, size_t ws_bytes, int stages, hipStream_t stream) {
  const char* fn = "ssg_conv_wgrad_f32";
  if (int rc = wgrad_check_call(fn, stages, B, H, W)) return rc;
  const int64_t M = (int64_t)B * H * W;                // stride 1 with pad KH / 2: the output has the input's size
  if (int rc = conv_train_check_shape(fn, M, Cout, KH, KW, Cin)) return rc;
  return conv_wgrad_launch(fn, WG_UNIT, dy, x, H, W, Cin, Cout, KH, KW, H, W, 1, (int)M, dw, s_co, s_ci, s_r, s_s, ws, ws_bytes, stages, stream);
}
