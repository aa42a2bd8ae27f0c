// conv_strided.hip -- train-mode strided convolutions, the 7x7 stem and the 3x3 max-pool of the fine-tune phase (gfx950 only).
//
// The rest of the backbone that csrc/conv_train.hip leaves to the vendor library, float32 NHWC, no float atomics, every cut of a
// reduction a function of the shape alone:
//   class S  groups 1, dilation 1, no bias, stride 2, 1x1 pad 0 or 3x3 pad 1, Cin % 64 == 0, Cout % 64 == 0
//   stem     7x7, stride 2, pad 3, 3 -> 64 on RGB0 pixels (ssg_nchw_to_nhwc4); no data gradient (the images do not require grad)
//   pool     MaxPool2d(3, stride 2, padding 1), C % 4 == 0
//
//   forward  y  = ssg_conv2d_nhwc_f32(x, w_fwd, stride 2)              csrc/conv.hip; class S: the w_fwd of ssg_conv_pack_train_f32's
//                                                                      layout, stem: [64][224], k = (r*7 + s)*4 + c
//   dgrad    the input pixels fall into four (h mod 2, w mod 2) classes.  Tap (r, s) reaches input row ih from output row oh when
//            ih = 2 oh + r - pad, so a class sees only the taps with r = (ih + pad) mod 2 (mod 2), likewise s: 1, 2, 2 or 4 taps of a
//            3x3, one tap of a 1x1 in the (even, even) class and none in the other three.  Each class is a dense implicit GEMM
//            dX[px][ci] = sum over (tap, co) dY[px shifted by the tap][co] * w[tap][co][ci] with a tap set that is uniform over the
//            grid's z index; no zero of a zero-stuffed dY is ever multiplied.  Every dX element is written once, the zeros of the
//            empty classes included.
//   wgrad    conv_wgrad_partial_kernel<CT, WG_STRIDE / WG_STEM> of csrc/conv_train.hip + the float64 slice sum
//   pool     the forward records the winner's tap (torch's CPU rule: `val > max || isnan(val)` in row-major window order), the
//            backward gathers: an input element adds, oh ascending then ow ascending, the dY of the at most 2 x 2 windows that
//            contain it and whose winner it is.
#include "train_common.h"

namespace ssg {

constexpr int DG_PX = 64;        // input pixels of one parity class per workgroup
constexpr int DG_CO = 32;        // output channels (K of the GEMM) per LDS stage
constexpr int DG_PITCH = 33;     // dY stage [pixel][co]: the MFMA reads it with the pixel in the lane index, so an odd pitch

// w [Cout,Cin,KH,KW] at element strides -> wp [KH*KW][Cout][Cin]
__global__ __launch_bounds__(256) void conv_pack_dgrad_s2_kernel(const float* __restrict__ w, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int Cout,
                                                                 int Cin, int KH, int KW, float* __restrict__ wp) {
  const int64_t per_tap = (int64_t)Cout * Cin, total = per_tap * KH * KW;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int tap = (int)(idx / per_tap), rem = (int)(idx % per_tap), co = rem / Cin, ci = rem % Cin;
    wp[idx] = w[co * s0 + ci * s1 + (tap / KW) * s2 + (tap % KW) * s3];
  }
}

// w [Cout,3,KH,KW] at element strides -> w_fwd [Cout][Kpad], k = (r*KW + s)*4 + c, zero where c == 3 or the tap is past KH*KW
__global__ __launch_bounds__(256) void conv_pack_stem_kernel(const float* __restrict__ w, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int Cout, int KH,
                                                             int KW, int Kpad, float* __restrict__ w_fwd) {
  const int total = Cout * Kpad;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int co = idx / Kpad, k = idx % Kpad, tap = k >> 2, c = k & 3;
    w_fwd[idx] = (tap < KH * KW && c < 3) ? w[co * s0 + c * s1 + (tap / KW) * s2 + (tap % KW) * s3] : 0.f;
  }
}

// Data gradient of a stride-2 convolution.  grid (pixel tiles of the largest class, Cin / 64, 4 classes); 256 threads = 2 x 2 waves,
// wave (wr, wc) owns the 32 ci x 32 pixel tile D[i = ci][j = pixel] = sum_k A[i][k = co] B[k][j]: A is the packed weight (ci contiguous),
// B the dY stage.  A lane's four consecutive accumulator rows are four consecutive ci of one pixel: one 16-byte store.
__global__ __launch_bounds__(256) void conv_dgrad_s2_kernel(const float* __restrict__ dy, const float* __restrict__ wp, float* __restrict__ dx, int B, int H,
                                                            int W, int OH, int OW, int Cin, int Cout, int KH, int KW, int pad) {
  __shared__ float ys[DG_PX * DG_PITCH];
  __shared__ float4 wsh[DG_CO * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int ph = blockIdx.z >> 1, pw = blockIdx.z & 1;
  const int Hc = (H - ph + 1) >> 1, Wc = (W - pw + 1) >> 1;                 // rows / columns of this parity
  const int64_t Mc = (int64_t)B * Hc * Wc, px0 = (int64_t)blockIdx.x * DG_PX;
  if (px0 >= Mc) return;                                                    // the whole workgroup leaves: a smaller (or empty) class
  const int ci0 = blockIdx.y * 64;
  const int r0 = (ph + pad) & 1, s0 = (pw + pad) & 1;                       // the taps of this class: r = r0, r0 + 2, ... < KH
  const int nr = (KH - r0 + 1) >> 1, ns = (KW - s0 + 1) >> 1;               // 1x1: one tap in the (even, even) class, else none
  const int cchunks = Cout / DG_CO, nstage = nr * ns * cchunks;

  // the two dY rows this thread stages: pixel -> (b, ih, iw)
  int pb[2], pih[2], piw[2];
  bool pok[2];
#pragma unroll
  for (int u = 0; u < 2; u++) {
    const int64_t q = px0 + ((tid + 256 * u) >> 3);
    pok[u] = q < Mc;
    const int64_t qq = pok[u] ? q : 0;
    piw[u] = 2 * (int)(qq % Wc) + pw;
    pih[u] = 2 * (int)((qq / Wc) % Hc) + ph;
    pb[u] = (int)(qq / ((int64_t)Wc * Hc));
  }

  float4 yr[2], wv[2];
  auto load = [&](int st) {
    const int t = st / cchunks, co0 = (st % cchunks) * DG_CO;
    const int r = r0 + 2 * (t / ns), s = s0 + 2 * (t % ns);
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int c4 = (tid + 256 * u) & 7;
      const int oh = (pih[u] + pad - r) >> 1, ow = (piw[u] + pad - s) >> 1; // exact and >= 0: r and s have the class's parity
      yr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pok[u] && oh < OH && ow < OW) yr[u] = *reinterpret_cast<const float4*>(dy + (((int64_t)pb[u] * OH + oh) * OW + ow) * Cout + co0 + c4 * 4);
      const int f = tid + 256 * u, row = f >> 4, w4 = f & 15;
      wv[u] = *reinterpret_cast<const float4*>(wp + ((int64_t)(r * KW + s) * Cout + co0 + row) * Cin + ci0 + w4 * 4);
    }
  };

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; e++) acc[e] = 0.f;
  const float* wsf = reinterpret_cast<const float*>(wsh);
  const int l31 = lane & 31, lk = lane >> 5;
  if (nstage > 0) load(0);
  for (int st = 0; st < nstage; st++) {
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int f = tid + 256 * u;
      float* d = ys + (f >> 3) * DG_PITCH + (f & 7) * 4;
      d[0] = yr[u].x; d[1] = yr[u].y; d[2] = yr[u].z; d[3] = yr[u].w;
      wsh[f] = wv[u];
    }
    __syncthreads();
    if (st + 1 < nstage) load(st + 1);                    // the next stage's global loads fly under this stage's MFMAs
#pragma unroll
    for (int kk = 0; kk < DG_CO / 2; kk++) {
      const int co = 2 * kk + lk;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wsf[co * 64 + wr * 32 + l31], ys[(wc * 32 + l31) * DG_PITCH + co], acc, 0, 0, 0);
    }
    __syncthreads();
  }

  const int64_t q = px0 + wc * 32 + l31;
  if (q < Mc) {
    const int iw = 2 * (int)(q % Wc) + pw, ih = 2 * (int)((q / Wc) % Hc) + ph;
    const int64_t b = q / ((int64_t)Wc * Hc);
    float* out = dx + ((b * H + ih) * W + iw) * Cin + ci0 + wr * 32 + 4 * lk;   // C/D map: row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) = ci
#pragma unroll
    for (int g = 0; g < 4; g++) *reinterpret_cast<float4*>(out + 8 * g) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
  }
}

// stage 2 of the stem's weight gradient: ws [slice][Cout][Kws], k = tap*4 + c -> dW[co][c][r][s], c < 3
__global__ __launch_bounds__(256) void conv_wgrad_reduce_stem_kernel(const float* __restrict__ ws, int slices, int Cout, int KH, int KW, int Kws,
                                                                     float* __restrict__ dw, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
  const int T = KH * KW, total = Cout * T * 3;
  const int64_t per_slice = (int64_t)Cout * Kws;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int co = idx / (T * 3), rem = idx % (T * 3), tap = rem / 3, c = rem % 3;
    double sum = 0.0;
    for (int sl = 0; sl < slices; sl++) sum += (double)ws[sl * per_slice + (int64_t)co * Kws + tap * 4 + c];
    dw[co * s0 + c * s1 + (tap / KW) * s2 + (tap % KW) * s3] = (float)sum;
  }
}

// MaxPool2d(3, 2, 1) forward that also records the winner's tap r*3 + s.  torch's CPU rule: the running maximum starts at -inf on
// the window's first element, and an element replaces it when `val > max || isnan(val)`.
__global__ __launch_bounds__(256) void maxpool3x3s2_idx_kernel(const float* __restrict__ in, float* __restrict__ out, uint8_t* __restrict__ idx, int B, int H,
                                                               int W, int C, int OH, int OW) {
  const int C4 = C / 4;
  const int64_t total = (int64_t)B * OH * OW * C4;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(x % C4); int64_t t = x / C4;
    const int ow = (int)(t % OW); t /= OW; const int oh = (int)(t % OH); const int b = (int)(t / OH);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const int first = (oh == 0 ? 3 : 0) + (ow == 0 ? 1 : 0);               // the window's first element inside the image
    int wi[4] = {first, first, first, first};
    for (int r = 0; r < 3; r++) {
      const int ih = oh * 2 - 1 + r; if (ih < 0 || ih >= H) continue;
      for (int s = 0; s < 3; s++) {
        const int iw = ow * 2 - 1 + s; if (iw < 0 || iw >= W) continue;
        const float4 v4 = reinterpret_cast<const float4*>(in + ((int64_t)(b * H + ih) * W + iw) * C)[c4];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (v[j] > m[j] || v[j] != v[j]) { m[j] = v[j]; wi[j] = r * 3 + s; }
      }
    }
    reinterpret_cast<float4*>(out)[x] = make_float4(m[0], m[1], m[2], m[3]);
    reinterpret_cast<uchar4*>(idx)[x] = make_uchar4((uint8_t)wi[0], (uint8_t)wi[1], (uint8_t)wi[2], (uint8_t)wi[3]);
  }
}

// MaxPool2d(3, 2, 1) backward as a gather: no atomics, a fixed order (oh ascending, then ow ascending), every dX element written once
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx, float* __restrict__ dx, int B,
                                                               int H, int W, int C, int OH, int OW) {
  const int C4 = C / 4;
  const int64_t total = (int64_t)B * H * W * C4;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(x % C4); int64_t t = x / C4;
    const int iw = (int)(t % W); t /= W; const int ih = (int)(t % H); const int b = (int)(t / H);
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    const int oh_hi = (ih + 1) >> 1, ow_hi = (iw + 1) >> 1;                  // window oh covers rows 2 oh - 1 .. 2 oh + 1
    for (int oh = ih >> 1; oh <= oh_hi; oh++) {
      if (oh >= OH) continue;
      for (int ow = iw >> 1; ow <= ow_hi; ow++) {
        if (ow >= OW) continue;
        const int tap = (ih - 2 * oh + 1) * 3 + (iw - 2 * ow + 1);
        const int64_t o = ((int64_t)(b * OH + oh) * OW + ow) * C4 + c4;
        const uchar4 w4 = reinterpret_cast<const uchar4*>(idx)[o];
        const float4 d4 = reinterpret_cast<const float4*>(dy)[o];
        if (w4.x == tap) g[0] += d4.x;
        if (w4.y == tap) g[1] += d4.y;
        if (w4.z == tap) g[2] += d4.z;
        if (w4.w == tap) g[3] += d4.w;
      }
    }
    reinterpret_cast<float4*>(dx)[x] = make_float4(g[0], g[1], g[2], g[3]);
  }
}

}  // namespace ssg

namespace {

// 0: bad shape, WG_STRIDE: class S (1x1 pad 0 / 3x3 pad 1), WG_STEM: the stem
int conv_strided_class(const char* fn, int64_t M, int Cout, int KH, int KW, int Cin, int stride) {
  const bool k1 = (KH == 1 && KW == 1), k3 = (KH == 3 && KW == 3), k7 = (KH == 7 && KW == 7);
  if (M > 0 && M <= 0x7fffffffLL && stride == 2) {
    if ((k1 || k3) && Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % 64 == 0) return WG_STRIDE;
    if (k7 && Cin == 3 && Cout == 64) return WG_STEM;
  }
  ssg_set_error("%s: the strided train-mode convolution is stride 2 and either 1x1 (pad 0) or 3x3 (pad 1) with Cin %% 64 == 0, Cout %% 64 == 0, or the "
                "7x7 (pad 3) stem 3 -> 64; 0 < pixels < 2^31 (M=%lld Cin=%d Cout=%d k=%dx%d stride=%d)", fn, (long long)M, Cin, Cout, KH, KW, stride);
  return 0;
}

int pool_check(const char* fn, int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 4) || (int64_t)B * H * W > 0x7fffffffLL) {
    ssg_set_error("%s: MaxPool2d(3, 2, 1) on NHWC takes B, H, W > 0, C %% 4 == 0 and B*H*W < 2^31 (B=%d H=%d W=%d C=%d)", fn, B, H, W, C);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_conv_pack_strided_f32(const float* w, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, int Cout, int Cin, int KH, int KW,
                                         float* w_fwd, float* w_dgrad, hipStream_t stream) {
  const char* fn = "ssg_conv_pack_strided_f32";
  const int cls = conv_strided_class(fn, 1, Cout, KH, KW, Cin, 2);
  if (!cls) return SSG_ERR_INVALID;
  if (int rc = ssg_need_pointers(fn, w && (w_fwd || w_dgrad))) return rc;
  if (int rc = ssg_need_weight_strides(fn, s_co, s_ci, s_r, s_s)) return rc;
  if (cls == WG_STEM && w_dgrad) { ssg_set_error("%s: the stem has no data gradient (w_dgrad must be NULL)", fn); return SSG_ERR_INVALID; }
  if (cls == WG_STEM) {
    if (!w_fwd) { ssg_set_error("%s: the stem has only a forward packing (w_fwd is NULL)", fn); return SSG_ERR_INVALID; }
    const int Kpad = 32 * ((KH * KW + 7) / 8);
    hipLaunchKernelGGL(conv_pack_stem_kernel, dim3((Cout * Kpad + 255) / 256), dim3(256), 0, stream, w, s_co, s_ci, s_r, s_s, Cout, KH, KW, Kpad, w_fwd);
    SSG_LAUNCH_CHECK("conv_pack_stem_kernel");
    return SSG_OK;
  }
  const int blocks = ssg_blocks256((int64_t)Cout * Cin * KH * KW, 4096);
  if (w_fwd) {
    hipLaunchKernelGGL(conv_pack_train_kernel, dim3(blocks), dim3(256), 0, stream, w, s_co, s_ci, s_r, s_s, Cout, Cin, KH, KW, w_fwd, (float*)nullptr);
    SSG_LAUNCH_CHECK("conv_pack_train_kernel");
  }
  if (w_dgrad) {
    hipLaunchKernelGGL(conv_pack_dgrad_s2_kernel, dim3(blocks), dim3(256), 0, stream, w, s_co, s_ci, s_r, s_s, Cout, Cin, KH, KW, w_dgrad);
    SSG_LAUNCH_CHECK("conv_pack_dgrad_s2_kernel");
  }
  return SSG_OK;
}

extern "C" int ssg_conv_dgrad_strided_f32(const float* dy, const float* w_dgrad, float* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                                          int stride, hipStream_t stream) {
  const char* fn = "ssg_conv_dgrad_strided_f32";
  if (B <= 0 || H <= 0 || W <= 0) { ssg_set_error("%s: empty input B=%d H=%d W=%d", fn, B, H, W); return SSG_ERR_INVALID; }
  const int cls = conv_strided_class(fn, (int64_t)B * H * W, Cout, KH, KW, Cin, stride);
  if (!cls) return SSG_ERR_INVALID;
  if (cls == WG_STEM) { ssg_set_error("%s: the stem has no data gradient (the images do not require grad)", fn); return SSG_ERR_INVALID; }
  if (int rc = ssg_need_pointers(fn, dy && w_dgrad && dx)) return rc;
  if (int rc = ssg_need_aligned16(fn, "dy, w_dgrad and dx", {dy, w_dgrad, dx})) return rc;
  const int pad = KH / 2, OH = (H + 2 * pad - KH) / 2 + 1, OW = (W + 2 * pad - KW) / 2 + 1;
  const int64_t m0 = (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2);             // the (even, even) class is the largest
  const dim3 grid((unsigned)((m0 + DG_PX - 1) / DG_PX), Cin / 64, 4);
  hipLaunchKernelGGL(conv_dgrad_s2_kernel, grid, dim3(256), 0, stream, dy, w_dgrad, dx, B, H, W, OH, OW, Cin, Cout, KH, KW, pad);
  SSG_LAUNCH_CHECK("conv_dgrad_s2_kernel");
  return SSG_OK;
}

extern "C" int ssg_conv_wgrad_strided_num_slices(int M, int Cout, int KH, int KW, int Cin, int stride) {
  const int cls = conv_strided_class("ssg_conv_wgrad_strided_num_slices", M, Cout, KH, KW, Cin, stride);
  return cls ? wgrad_plan(cls, M, Cout, KH, KW, Cin).slices : SSG_ERR_INVALID;
}

extern "C" size_t ssg_conv_wgrad_strided_workspace_bytes(int M, int Cout, int KH, int KW, int Cin, int stride) {
  const int cls = conv_strided_class("ssg_conv_wgrad_strided_workspace_bytes", M, Cout, KH, KW, Cin, stride);
  return cls ? wgrad_workspace_bytes(cls, M, Cout, KH, KW, Cin) : 0;
}

extern "C" int ssg_conv_wgrad_strided_f32(const float* dy, const float* x, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, float* dw,
                                          int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, void* ws, size_t ws_bytes, int stages, hipStream_t stream) {
  const char* fn = "ssg_conv_wgrad_strided_f32";
  if (int rc = wgrad_check_call(fn, stages, B, H, W)) return rc;
  if ((int64_t)B * H * W > 0x7fffffffLL) { ssg_set_error("%s: B*H*W = %lld is 2^31 or more", fn, (long long)B * H * W); return SSG_ERR_INVALID; }
  const int pad = KH / 2, OH = (H + 2 * pad - KH) / 2 + 1, OW = (W + 2 * pad - KW) / 2 + 1;     // stride 2 (checked next); OH, OW >= 1
  const int cls = conv_strided_class(fn, (int64_t)B * OH * OW, Cout, KH, KW, Cin, stride);
  if (!cls) return SSG_ERR_INVALID;
  return conv_wgrad_launch(fn, cls, dy, x, H, W, Cin, Cout, KH, KW, OH, OW, 2, B * OH * OW, dw, s_co, s_ci, s_r, s_s, ws, ws_bytes, stages, stream);
}

extern "C" int ssg_maxpool3x3s2_idx_nhwc(const float* in, float* out, uint8_t* idx, int B, int H, int W, int C, hipStream_t stream) {
  const char* fn = "ssg_maxpool3x3s2_idx_nhwc";
  if (int rc = pool_check(fn, B, H, W, C)) return rc;
  if (int rc = ssg_need_pointers(fn, in && out && idx)) return rc;
  if (((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)idx & 3)) { ssg_set_error("%s: in / out must be 16-byte, idx 4-byte aligned", fn); return SSG_ERR_INVALID; }
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int blocks = ssg_blocks256((int64_t)B * OH * OW * (C / 4), 16384);
  hipLaunchKernelGGL(maxpool3x3s2_idx_kernel, dim3(blocks), dim3(256), 0, stream, in, out, idx, B, H, W, C, OH, OW);
  SSG_LAUNCH_CHECK("maxpool3x3s2_idx_kernel");
  return SSG_OK;
}

extern "C" int ssg_maxpool3x3s2_bwd_nhwc(const float* dy, const uint8_t* idx, float* dx, int B, int H, int W, int C, hipStream_t stream) {
  const char* fn = "ssg_maxpool3x3s2_bwd_nhwc";
  if (int rc = pool_check(fn, B, H, W, C)) return rc;
  if (int rc = ssg_need_pointers(fn, dy && idx && dx)) return rc;
  if (((uintptr_t)dy & 15) || ((uintptr_t)dx & 15) || ((uintptr_t)idx & 3)) { ssg_set_error("%s: dy / dx must be 16-byte, idx 4-byte aligned", fn); return SSG_ERR_INVALID; }
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int blocks = ssg_blocks256((int64_t)B * H * W * (C / 4), 16384);
  hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3(blocks), dim3(256), 0, stream, dy, idx, dx, B, H, W, C, OH, OW);
  SSG_LAUNCH_CHECK("maxpool3x3s2_bwd_kernel");
  return SSG_OK;
}
