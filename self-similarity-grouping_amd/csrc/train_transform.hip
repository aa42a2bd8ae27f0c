// train_transform.hip -- the per-image transform of the fine-tune loader (ssg_amd/trainloader.py) on the GPU, one launch per batch.
//
// Replaces, for a batch of decoded RGB images of any mix of sizes, the per-item CPU transform of the reference's training loaders
// (selftraining.py:177-183, reid/eug.py:64-71, applied by reid/utils/data/preprocessor.py:22-30 inside DataLoader workers):
//   crop            PIL.Image.crop((x0, y0, x0 + cw, y0 + ch)) -- the whole image for Resize, RandomSizedRectCrop's window otherwise
//   resize          PIL.Image.resize((W, H), BILINEAR): Pillow's separable resampling on 8-bit channels (libImaging/Resample.c:
//                   22-bit fixed-point triangle-filter windows, accumulator started at 1 << 21, >> 22, clamped to 0..255, horizontal
//                   pass first, 8-bit intermediate), exactly as csrc/preprocess.hip states it
//   flip            RandomHorizontalFlip: out column x reads resized column W - 1 - x
//   ToTensor        uint8 HWC -> float32 CHW / 255
//   Normalize(m, s) (x - m[c]) / s[c] in IEEE float32 (no contraction: ssg_common.h)
//   RandomErasing   the reid one (reid/utils/data/transforms.py:52-94): rows [er, er + eh) x columns [ec, ec + ew) of the finished tensor
//                   set to float32(fill[c]); the rectangle is in output (flipped) coordinates, eh = 0: none
// The host draws every random choice (ssg_amd.trainloader.TrainSchedule); this kernel only applies them.
//
// One workgroup per (image, band of `band` output rows): the source rows the band's vertical windows touch are resampled horizontally
// into LDS (uint8, one plane per channel), then each thread produces one output pixel of the band in all three channel planes
// (coalesced along X).  The band height is chosen by the host from the batch's largest vertical scale so that the LDS rows fit.
#include "ssg_common.h"

namespace ssg {

// int32 words of one image's descriptor (include/ssg_hip.h: SSG_TT_WORDS per image)
enum {
  TT_SRC_LO = 0, TT_SRC_HI, TT_H, TT_W, TT_X0, TT_Y0, TT_CW, TT_CH, TT_XOFF, TT_XKS, TT_YOFF, TT_YKS, TT_FLIP, TT_EROW, TT_ECOL, TT_EH, TT_EW,
  TT_WORDS = 20
};

__device__ __forceinline__ int clip8(int a) { return min(max(a >> 22, 0), 255); }

// desc [B, TT_WORDS]; coef: packed int32 windows, per axis block at offset o: first[n], count[n], k[n, ks] (n = W for x, H for y; first is
// relative to the crop); lds = 3 planes of cap_rows x W bytes
__global__ __launch_bounds__(256) void train_transform_kernel(const int32_t* __restrict__ desc, const int32_t* __restrict__ coef, int H, int W,
                                                              int band, int cap_rows, float m0, float m1, float m2, float s0, float s1, float s2,
                                                              float f0, float f1, float f2, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tt_lds[];
  const int b = blockIdx.y;
  const int Y0 = blockIdx.x * band;
  const int Y1 = min(Y0 + band, H);
  const int32_t* d = desc + (int64_t)b * TT_WORDS;
  const uint8_t* src = (const uint8_t*)(((uint64_t)(uint32_t)d[TT_SRC_HI] << 32) | (uint64_t)(uint32_t)d[TT_SRC_LO]);
  const int w = d[TT_W], x0 = d[TT_X0], y0 = d[TT_Y0];
  const int32_t* xf = coef + d[TT_XOFF];
  const int32_t* xc = xf + W;
  const int32_t* xk = xc + W;
  const int xks = d[TT_XKS];
  const int32_t* yf = coef + d[TT_YOFF];
  const int32_t* yc = yf + H;
  const int32_t* yk = yc + H;
  const int yks = d[TT_YKS];

  // horizontal pass of the crop rows [r0, r0 + rows) the band's windows read (the windows are monotone in Y)
  const int r0 = yf[Y0];
  const int rows = min(yf[Y1 - 1] + yc[Y1 - 1] - r0, cap_rows);
  const int plane = cap_rows * W;
  for (int i = threadIdx.x; i < rows * W; i += blockDim.x) {
    const int r = i / W, X = i - r * W;
    const uint8_t* p = src + ((int64_t)(y0 + r0 + r) * w + x0 + xf[X]) * 3;
    const int32_t* k = xk + (int64_t)X * xks;
    const int n = xc[X];
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int t = 0; t < n; t++, p += 3) {
      const int c = k[t];
      a0 += (int)p[0] * c; a1 += (int)p[1] * c; a2 += (int)p[2] * c;
    }
    const int o = r * W + X;
    tt_lds[o] = (uint8_t)clip8(a0); tt_lds[plane + o] = (uint8_t)clip8(a1); tt_lds[2 * plane + o] = (uint8_t)clip8(a2);
  }
  __syncthreads();

  // vertical pass + flip + ToTensor + Normalize + erase, stored along X in each channel plane
  const int flip = d[TT_FLIP], er = d[TT_EROW], ec = d[TT_ECOL], eh = d[TT_EH], ew = d[TT_EW];
  const int64_t oplane = (int64_t)H * W;
  float* o = out + (int64_t)b * 3 * oplane;
  for (int i = threadIdx.x; i < (Y1 - Y0) * W; i += blockDim.x) {
    const int Y = Y0 + i / W, x = i % W;
    const int X = flip ? W - 1 - x : x;
    const int lo = yf[Y] - r0;
    const int n = min(yc[Y], rows - lo);
    const int32_t* k = yk + (int64_t)Y * yks;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int t = 0; t < n; t++) {
      const int c = k[t], q = (lo + t) * W + X;
      a0 += (int)tt_lds[q] * c; a1 += (int)tt_lds[plane + q] * c; a2 += (int)tt_lds[2 * plane + q] * c;
    }
    const bool erased = Y >= er && Y < er + eh && x >= ec && x < ec + ew;
    const int64_t q = (int64_t)Y * W + x;
    o[q] = erased ? f0 : ((float)clip8(a0) / 255.0f - m0) / s0;
    o[oplane + q] = erased ? f1 : ((float)clip8(a1) / 255.0f - m1) / s1;
    o[2 * oplane + q] = erased ? f2 : ((float)clip8(a2) / 255.0f - m2) / s2;
  }
}

}  // namespace ssg

extern "C" int ssg_train_transform_u8(const int32_t* desc, int B, const int32_t* coef, int H, int W, int band_rows, int lds_rows,
                                      const float* mean3_host, const float* std3_host, const float* fill3_host, float* out, hipStream_t stream) {
  if (!desc || !coef || !out || !mean3_host || !std3_host || !fill3_host || B <= 0 || B > 65535 || H <= 0 || W <= 0 || band_rows <= 0 ||
      band_rows > H || lds_rows <= 0) {
    ssg_set_error("ssg_train_transform_u8: bad arguments (B=%d H=%d W=%d band_rows=%d lds_rows=%d, null pointer?)", B, H, W, band_rows, lds_rows);
    return SSG_ERR_INVALID;
  }
  const int64_t lds = (int64_t)lds_rows * W * 3;
  if (lds > 65536) {
    ssg_set_error("ssg_train_transform_u8: %d source rows of width %d need %lld bytes of LDS (at most 65536)", lds_rows, W, (long long)lds);
    return SSG_ERR_INVALID;
  }
  const dim3 grid((unsigned)((H + band_rows - 1) / band_rows), (unsigned)B);
  hipLaunchKernelGGL(ssg::train_transform_kernel, grid, dim3(256), (size_t)lds, stream, desc, coef, H, W, band_rows, lds_rows, mean3_host[0],
                     mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2], fill3_host[0], fill3_host[1], fill3_host[2], out);
  SSG_LAUNCH_CHECK("train_transform_kernel");
  return SSG_OK;
}
