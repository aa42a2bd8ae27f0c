// basicblock.hip -- one identity BasicBlock of the ResNet-18 / ResNet-34 backbones in ONE kernel (split-half path): the blocks of
// layer1 (64 -> 64 channels on the H/4 x 32 map).
//
// reid/models/base.py:25-54 (torchvision BasicBlock without a downsample branch, stride 1), eval mode, BatchNorm folded:
//   out = relu( conv2_3x3( relu( conv1_3x3(x) + b1 ) ) + b2 + x )
// Run as two launches (conv.hip) the 64-channel intermediate is written to HBM and read back, x is read twice (conv1 and the
// residual) and both GEMMs have short reductions (K = 576).  Here a workgroup owns TH = 4 full-width image rows:
//   stage   x rows ty0-2 .. ty0+TH+1 (TH + 4 rows, 64 KB) global -> LDS once; rows outside the image are conv1's zero padding
//           (out-of-range buffer offsets return zeros), the columns left / right of the image one shared all-zero pixel row
//   phase 1 y1[(TH+2)*32, 64] = relu(conv1(x) + b1) on the TH + 2 halo rows: implicit GEMM, the pixel operand read from the x
//           rows in LDS (9 taps = 9 shifted fragment addresses); wave = 3 image rows x 32 channels.  y1 goes to LDS encoded
//           exactly as the unfused launch stores it (h8l8); its rows outside the IMAGE are conv2's zero padding, not relu(b1)
//   phase 2 acc[TH*32, 64] = conv2(y1): the same loop on the y1 rows (phase 2 of bottleneck.hip); wave = 1 image row x 64 channels
//   tail    + b2 + x (decoded from the x rows still in LDS: no second read from HBM), ReLU, re-encode, through the wave's own
//           (dead) y1 rows, then whole 256-byte pixel rows to global memory
// The weight k-tiles (chunk, tap) of 32 channels are staged global -> registers -> LDS six tiles ahead, one barrier per tile.
// LDS: 8 x rows 69 632 + 6 y1 rows 52 224 + zero row + 2 weight stages 18 432 = 140 800 bytes: one 4-wave workgroup per CU.
//
// Numerics: the same three-product split-half multiply, the same reduction order (k-tile = (32-channel chunk, tap), two k-steps
// of 16 channels) and the same epilogue arithmetic as conv.hip, so the block output is bit-identical to the two launches.
#include "ssg_common.h"

namespace ssg {
namespace bblock {

using bneck::v16f;
using bneck::v4u;
using bneck::v8h;
using bneck::v4f;
using bneck::relu4;

struct Params {
  const float* x; float* out;
  const float* w1; const float* b1; const float* cs1;   // [C][9*C] h8l8, k = ((c/32)*9 + tap)*32 + c%32, rows pre-scaled by 1/cs1
  const float* w2; const float* b2; const float* cs2;
  int B, H;
  int* overflow;
};

constexpr int C = 64, IW = 32, TH = 4, NW = 4, NTHR = NW * 64;
constexpr int XPIX = (TH + 4) * IW, YPIX = (TH + 2) * IW;
constexpr int PY = C * 4 + 16;                       // LDS pitch of a pixel row (all 64 channels, h8l8); pitch/16 odd: conflict-free b128
constexpr int P2 = 128 + 16;                         // ... of a weight stage row (128 bytes of a weight row)
constexpr int X_OFF = 0, Y_OFF = XPIX * PY, ZERO_OFF = Y_OFF + YPIX * PY;
constexpr int W_OFF = (ZERO_OFF + PY + 255) / 256 * 256, BUFW = C * P2;
constexpr int LDS = W_OFF + 2 * BUFW;
constexpr int KROW = 9 * C;                          // floats per weight row
constexpr int NK = (C / 32) * 9, PD = 6;             // k-tiles per convolution, weight tiles in flight
constexpr int XU = XPIX * 16 / NTHR, WU = C * 8 / NTHR;   // 16-byte pieces per thread: x halo, one weight stage
static_assert(LDS <= 160 * 1024 && NK % 6 == 0 && IW == 32 && (TH + 2) % 3 == 0 && C == 64, "one workgroup per CU; a pixel tile is one image row");

__global__ __launch_bounds__(NTHR, 1) void basicblock_kernel(Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
  const int tiles_img = p.H / TH, ntiles = p.B * tiles_img;
  int T;
  {   // workgroups are dealt round-robin to the 8 XCDs: give every XCD a contiguous run of tiles (halo rows hit its L2)
    const int b = (int)blockIdx.x, q = ntiles / 8, r = ntiles % 8, x = b % 8, s = b / 8;
    T = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + s;
  }
  const int img = T / tiles_img, ty0 = (T - img * tiles_img) * TH;
  if (tid < PY / 16) *reinterpret_cast<uint4*>(smem + ZERO_OFF + tid * 16) = make_uint4(0u, 0u, 0u, 0u);

  // ---- weight stages: 64 rows x 128 bytes per k-tile, ring of PD register sets
  const int ck8 = tid & 7, r8 = tid >> 3;
  const float* w1p = p.w1 + (int64_t)r8 * KROW + ck8 * 4;
  const float* w2p = p.w2 + (int64_t)r8 * KROW + ck8 * 4;
  v4f sw[PD][WU];
#define SSG_BB_LOADW(WP_, T_, S_)                                                                                     \
  { _Pragma("unroll") for (int u = 0; u < WU; u++) sw[S_][u] = *reinterpret_cast<const v4f*>((WP_) + (int64_t)(32 * u) * KROW + (T_) * 32); }
#define SSG_BB_STOREW(BUF_, S_)                                                                                       \
  { unsigned char* sb_ = smem + W_OFF + (BUF_) * BUFW;                                                                \
    _Pragma("unroll") for (int u = 0; u < WU; u++) *reinterpret_cast<v4f*>(sb_ + (r8 + 32 * u) * P2 + ck8 * 16) = sw[S_][u]; }
  SSG_BB_LOADW(w1p, 0, 0) SSG_BB_LOADW(w1p, 1, 1) SSG_BB_LOADW(w1p, 2, 2) SSG_BB_LOADW(w1p, 3, 3) SSG_BB_LOADW(w1p, 4, 4) SSG_BB_LOADW(w1p, 5, 5)

  // ---- x halo rows -> LDS (rows above / below the image: out-of-range offset -> the load returns zeros)
  {
    const float* ximg = p.x + (int64_t)img * p.H * IW * C;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg), 0, (unsigned)(p.H * IW * C * 4), 0x00020000);
    v4f sx[XU];
#pragma unroll
    for (int u = 0; u < XU; u++) {
      const int idx = tid + NTHR * u, hp = idx >> 4, piece = idx & 15, pix = (ty0 - 2) * IW + hp;
      const unsigned off = (pix >= 0 && pix < p.H * IW) ? (unsigned)((pix * C + piece * 4) * 4) : 0x80000000u;
      const v4u raw = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0);
      sx[u] = __builtin_bit_cast(v4f, raw);
    }
#pragma unroll
    for (int u = 0; u < XU; u++) {
      const int idx = tid + NTHR * u, hp = idx >> 4, piece = idx & 15;
      *reinterpret_cast<v4f*>(smem + X_OFF + hp * PY + piece * 16) = sx[u];
    }
  }
  SSG_BB_STOREW(0, 0)
  __syncthreads();

  // =========================== phase 1: y1 = relu(conv1(x) + b1) on the TH+2 halo rows ===========================
  // waves: 2 row groups of 3 y1 rows x 2 channel tiles of 32; y1 row yr = image row ty0 - 1 + yr reads x rows yr + r (LDS row 0 = image row ty0 - 2)
  constexpr int MT1 = (TH + 2) / 2;
  const int i1b = (wave >> 1) * MT1, j1 = wave & 1;
  v16f acc1[MT1];
#pragma unroll
  for (int i = 0; i < MT1; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc1[i][r] = 0.f;
  float4 cs1r[4], b1r[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    cs1r[q] = *reinterpret_cast<const float4*>(p.cs1 + j1 * 32 + 8 * q + 4 * h); b1r[q] = *reinterpret_cast<const float4*>(p.b1 + j1 * 32 + 8 * q + 4 * h);
  }
  // x*w = xh*wl + xl*wh + xh*wh (the order of conv.hip's split_mma_step), weights as the first MFMA operand
#define SSG_BB_STEP1(KT_, S_, B_)                                                                                     \
  {                                                                                                                  \
    if ((KT_) + PD < NK) SSG_BB_LOADW(w1p, (KT_) + PD, S_)                                                            \
    const int chunk = (KT_) / 9, tap = (KT_) - chunk * 9, r = tap / 3, s = tap - r * 3;                              \
    const int xin = l32 + s - 1;                                                                                     \
    const bool colok = xin >= 0 && xin < IW;                                                                         \
    const unsigned char* wb = smem + W_OFF + (B_) * BUFW + (j1 * 32 + l32) * P2 + h * 32;                             \
    v8h xh_[2][MT1], xl_[2][MT1], wh_[2], wl_[2];                                                                    \
    _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                               \
      _Pragma("unroll") for (int i = 0; i < MT1; i++) {                                                              \
        const int abase = colok ? X_OFF + ((i1b + i + r) * IW + xin) * PY : ZERO_OFF;                                \
        const unsigned char* q_ = smem + abase + (chunk * 4 + ks * 2 + h) * 32;                                      \
        xh_[ks][i] = *reinterpret_cast<const v8h*>(q_); xl_[ks][i] = *reinterpret_cast<const v8h*>(q_ + 16); }       \
      wh_[ks] = *reinterpret_cast<const v8h*>(wb + ks * 64); wl_[ks] = *reinterpret_cast<const v8h*>(wb + ks * 64 + 16); \
    }                                                                                                                \
    _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                               \
      _Pragma("unroll") for (int i = 0; i < MT1; i++) acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[ks], xl_[ks][i], acc1[i], 0, 0, 0); \
      _Pragma("unroll") for (int i = 0; i < MT1; i++) acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[ks], xh_[ks][i], acc1[i], 0, 0, 0); \
      _Pragma("unroll") for (int i = 0; i < MT1; i++) acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[ks], xh_[ks][i], acc1[i], 0, 0, 0); \
    }                                                                                                                \
    if ((KT_) + 1 < NK) SSG_BB_STOREW((B_) ^ 1, ((S_) + 1) % PD)                                                      \
    __syncthreads();                                                                                                 \
  }
  // six steps per trip: the register set of step i is a LITERAL index (i % PD), its LDS buffer i & 1
#pragma unroll
  for (int kt0 = 0; kt0 < NK; kt0 += 6) {
    SSG_BB_STEP1(kt0, 0, 0) SSG_BB_STEP1(kt0 + 1, 1, 1) SSG_BB_STEP1(kt0 + 2, 2, 0)
    SSG_BB_STEP1(kt0 + 3, 3, 1) SSG_BB_STEP1(kt0 + 4, 4, 0) SSG_BB_STEP1(kt0 + 5, 5, 1)
  }
#undef SSG_BB_STEP1

  // ---- conv2 weights: first k-tiles on their way while y1 is written (every wave is past its last weight-stage read)
  SSG_BB_LOADW(w2p, 0, 0) SSG_BB_LOADW(w2p, 1, 1) SSG_BB_LOADW(w2p, 2, 2) SSG_BB_LOADW(w2p, 3, 3) SSG_BB_LOADW(w2p, 4, 4) SSG_BB_LOADW(w2p, 5, 5)

  // ---- y1 -> LDS (h8l8 pixel rows).  Rows outside the image are conv2's zero padding, not relu(b1).
  unsigned ovf = 0u;
#pragma unroll
  for (int i = 0; i < MT1; i++) {
    const int yr = i1b + i, irow = ty0 - 1 + yr;
    const bool inside = irow >= 0 && irow < p.H;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ch = j1 * 32 + 8 * q + 4 * h;
      const float4 cs = cs1r[q], bi = b1r[q];
      float4 v = make_float4(acc1[i][4 * q] * cs.x + bi.x, acc1[i][4 * q + 1] * cs.y + bi.y, acc1[i][4 * q + 2] * cs.z + bi.z, acc1[i][4 * q + 3] * cs.w + bi.w);
      v = relu4(v);
      if (!inside) v = make_float4(0.f, 0.f, 0.f, 0.f);
      uint2 hi, lo;
      split_encode4(v, hi, lo);
      ovf |= split_hi_nonfinite_bits(hi);
      unsigned char* d = smem + Y_OFF + (yr * IW + l32) * PY + (ch >> 3) * 32 + h * 8;
      *reinterpret_cast<uint2*>(d) = hi; *reinterpret_cast<uint2*>(d + 16) = lo;
    }
  }
  SSG_BB_STOREW(0, 0)
  __syncthreads();

  // =========================== phase 2: conv2(y1), pixel operand from the y1 rows ===========================
  // wave = output row `wave` of the tile (32 pixels) x both channel tiles
  v16f acc2[2];
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc2[j][r] = 0.f;
  float4 cs2r[2][4], b2r[2][4];
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      cs2r[j][q] = *reinterpret_cast<const float4*>(p.cs2 + j * 32 + 8 * q + 4 * h); b2r[j][q] = *reinterpret_cast<const float4*>(p.b2 + j * 32 + 8 * q + 4 * h);
    }
#define SSG_BB_STEP2(KT_, S_, B_)                                                                                     \
  {                                                                                                                  \
    if ((KT_) + PD < NK) SSG_BB_LOADW(w2p, (KT_) + PD, S_)                                                            \
    const int chunk = (KT_) / 9, tap = (KT_) - chunk * 9, r = tap / 3, s = tap - r * 3;                              \
    const int xin = l32 + s - 1;                                                                                     \
    const int abase = (xin >= 0 && xin < IW) ? Y_OFF + ((wave + r) * IW + xin) * PY : ZERO_OFF;                      \
    const unsigned char* wb = smem + W_OFF + (B_) * BUFW + l32 * P2 + h * 32;                                         \
    v8h xh_[2], xl_[2], wh_[2][2], wl_[2][2];                                                                        \
    _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                               \
      const unsigned char* q_ = smem + abase + (chunk * 4 + ks * 2 + h) * 32;                                        \
      xh_[ks] = *reinterpret_cast<const v8h*>(q_); xl_[ks] = *reinterpret_cast<const v8h*>(q_ + 16);                 \
      _Pragma("unroll") for (int j = 0; j < 2; j++) {                                                                \
        wh_[ks][j] = *reinterpret_cast<const v8h*>(wb + j * 32 * P2 + ks * 64);                                      \
        wl_[ks][j] = *reinterpret_cast<const v8h*>(wb + j * 32 * P2 + ks * 64 + 16); }                               \
    }                                                                                                                \
    _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                               \
      _Pragma("unroll") for (int j = 0; j < 2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[ks][j], xl_[ks], acc2[j], 0, 0, 0); \
      _Pragma("unroll") for (int j = 0; j < 2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[ks][j], xh_[ks], acc2[j], 0, 0, 0); \
      _Pragma("unroll") for (int j = 0; j < 2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[ks][j], xh_[ks], acc2[j], 0, 0, 0); \
    }                                                                                                                \
    if ((KT_) + 1 < NK) SSG_BB_STOREW((B_) ^ 1, ((S_) + 1) % PD)                                                      \
    __syncthreads();                                                                                                 \
  }
#pragma unroll
  for (int kt0 = 0; kt0 < NK; kt0 += 6) {
    SSG_BB_STEP2(kt0, 0, 0) SSG_BB_STEP2(kt0 + 1, 1, 1) SSG_BB_STEP2(kt0 + 2, 2, 0)
    SSG_BB_STEP2(kt0 + 3, 3, 1) SSG_BB_STEP2(kt0 + 4, 4, 0) SSG_BB_STEP2(kt0 + 5, 5, 1)
  }
#undef SSG_BB_STEP2
#undef SSG_BB_LOADW
#undef SSG_BB_STOREW

  // ---- tail: + b2 + x (this lane's pixel, from the x rows in LDS), ReLU, re-encode into the wave's own y1 rows (dead after the
  // last barrier: the wave's output row `wave` is written where y1 row `wave` was), then whole pixel rows to global memory
  const unsigned char* xrow = smem + X_OFF + ((wave + 2) * IW + l32) * PY;
  unsigned char* orow = smem + Y_OFF + (wave * IW) * PY;
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ch = j * 32 + 8 * q + 4 * h;
      const float4 cs = cs2r[j][q], bi = b2r[j][q];
      float4 v = make_float4(acc2[j][4 * q] * cs.x + bi.x, acc2[j][4 * q + 1] * cs.y + bi.y, acc2[j][4 * q + 2] * cs.z + bi.z, acc2[j][4 * q + 3] * cs.w + bi.w);
      const unsigned char* rs = xrow + (ch >> 3) * 32 + h * 8;
      const float4 r4 = split_decode4(*reinterpret_cast<const uint2*>(rs), *reinterpret_cast<const uint2*>(rs + 16));
      v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
      v = relu4(v);
      uint2 hi, lo;
      split_encode4(v, hi, lo);
      ovf |= split_hi_nonfinite_bits(hi);
      unsigned char* d = orow + l32 * PY + (ch >> 3) * 32 + h * 8;
      *reinterpret_cast<uint2*>(d) = hi; *reinterpret_cast<uint2*>(d + 16) = lo;
    }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // same wave wrote it: LDS operations of one wave complete in order
  float* __restrict__ outp = p.out + (((int64_t)img * p.H + ty0 + wave) * IW) * C;
#pragma unroll
  for (int it = 0; it < 8; it++) {
    const int idx = it * 64 + lane, px = idx >> 4, piece = idx & 15;
    *reinterpret_cast<uint4*>(outp + px * C + piece * 4) = *reinterpret_cast<const uint4*>(orow + px * PY + piece * 16);
  }
  if ((ovf & 0x80008000u) && p.overflow) *p.overflow = 1;
}

}  // namespace bblock
}  // namespace ssg

// 1 when ssg_basicblock_nhwc_x has a kernel for this block shape: layer1 of ResNet-18 / ResNet-34 at 128-wide input
// (H x 32 x 64, 4-row tiles)
extern "C" int ssg_basicblock_supported(int H, int W, int C) {
  return (C == 64 && W == 32 && H > 0 && H % 4 == 0) ? 1 : 0;
}

// Identity BasicBlock (no downsample branch, stride 1), split-half tensors:
//   out = relu(conv2(relu(conv1(x) + b1)) + b2 + x),  x / out [B,H,W,C] h8l8, w1 / w2 [C][9*C] as ssg_conv2d_nhwc_x takes them
//   (k = (32-channel chunk, tap, channel), each row pre-multiplied by a power of two that cs* undoes), biases fp32.
//   out must not alias x (halo rows are read by other workgroups).
extern "C" int ssg_basicblock_nhwc_x(const void* x, const void* w1, const float* b1, const float* cs1, const void* w2, const float* b2, const float* cs2,
                                     void* out, int B, int H, int W, int C, int32_t* overflow, hipStream_t stream) {
  using namespace ssg::bblock;
  if (B <= 0 || !ssg_basicblock_supported(H, W, C) || (int64_t)H * W * C * 4 > 0x7fffffffLL || !cs1 || !cs2 || x == out) {
    ssg_set_error("ssg_basicblock_nhwc_x: unsupported block B=%d H=%d W=%d C=%d (see ssg_basicblock_supported)", B, H, W, C);
    return SSG_ERR_INVALID;
  }
  Params p;
  p.x = (const float*)x; p.out = (float*)out;
  p.w1 = (const float*)w1; p.b1 = b1; p.cs1 = cs1; p.w2 = (const float*)w2; p.b2 = b2; p.cs2 = cs2;
  p.B = B; p.H = H; p.overflow = overflow;
  static bool attr_set = false;
  if (!attr_set) {
    SSG_HIP(hipFuncSetAttribute((const void*)basicblock_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    attr_set = true;
  }
  hipLaunchKernelGGL(basicblock_kernel, dim3(B * (H / TH)), dim3(NTHR), LDS, stream, p);
  SSG_LAUNCH_CHECK("basicblock_kernel");
  return SSG_OK;
}
