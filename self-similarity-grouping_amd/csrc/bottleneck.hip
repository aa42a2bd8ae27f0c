// bottleneck.hip -- one bottleneck block of the ResNet-50 backbone in ONE kernel (split-half path): the three blocks of layer1
// and the three identity blocks of layer2.
//
// reid/models/base.py:57-90 (torchvision Bottleneck without a downsample branch), eval mode, BatchNorm folded:
//   out = relu( conv3_1x1( relu( conv2_3x3( relu( conv1_1x1(x) ) ) ) ) + x )
// Run as three launches (conv.hip) a layer1 block moves 16 "units" of 64-channel activations through HBM (x is read by
// conv1 and again as the residual, the two 64-channel intermediates are written and re-read) and its three GEMMs have short
// reductions (K = 256 / 576 / 64): the launches sit at 4.4-4.9 TB/s or stall on their pipeline fill.  Here a workgroup owns
// TH full-width image rows: it computes conv1 on TH+2 rows (one halo row above and below; the left/right halo is the zero
// padding of conv2, never computed), keeps that intermediate in LDS in the split-half format, runs conv2 as an implicit GEMM
// whose pixel operand is read from LDS (the 9 taps are 9 shifted fragment addresses), turns conv2's accumulators through LDS
// again into the pixel operand of conv3 and finishes with bias + residual + ReLU + re-encoding.  Measured (TCC_EA0_RDREQ): the
// L2 fetches 2.07 x |x| per launch -- x once, the halo rows mostly L2 hits of the neighbouring workgroup, and the residual
// re-read (14 us after phase 1, 64 workgroups streaming through each 4 MB L2) once more from HBM -- and writes |out| once:
// 3.1 units against the 16 of the three launches.  (Keeping the residual lines recent with touch loads during phase 2 does not
// work: the touches already miss.)
//
// Numerics: the same three-product split-half multiply, the same reduction order and the same epilogues as the separate
// launches (conv.hip), so the block output is bit-identical to the three-launch path.
//
// DS variant (the first block of layer1, base.py:75-90 with a stride-1 downsample branch): x has CIN = 64 channels, the
// downsample 1x1 convolution rides in conv3's reduction (K = MID + CIN, weights concatenated, as ssg_conv1x1_dual_nhwc_x does)
// and replaces the residual; its pixel operand (this wave's 32 pixels x CIN channels) is loaded straight into MFMA fragments.
//
// Both kernels here are 4-wave workgroups of 128 output pixels in <= 80 KB of LDS, two per CU: one's loads, stores and epilogue
// arithmetic run under the other's multiplies.  bottleneck_kernel is layer1 (C = 256, MID = 64, 32-pixel rows, TH = 4: the identity
// block, the DS variant and the next-conv instance); bottleneck_halves_kernel below is layer2 (C = 512, MID = 128,
// 16-pixel rows, TH = 8), whose 128-channel halo intermediate (85 KB) only fits in channel halves.
// All operand tiles are staged global -> registers -> LDS with the loads several k-tiles ahead (register rings), one barrier per
// stage:
//   phase 1  y1[(TH+2)*IW, MID] = relu(x W1^T)   k-tiles of 32 channels: x rows (whole 128-byte lines) + W1 rows; wave = 3 x 1 MFMA tiles
//   phase 2  y2[TH*IW, MID]     = relu(conv3x3(y1))   k-tiles = (32-channel chunk, tap): W2 rows (128 B); wave = 32 pixels x MID
//   phase 3  out[TH*IW, C]      = relu(y2 W3^T + x)   k-tiles of 16 channels: W3 rows; wave = its own 32 pixels x all C channels
#include "ssg_common.h"
#include <cstdlib>

namespace ssg {
namespace bneck {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));   // staging registers: arrays of HIP's float4 struct stay in scratch memory

struct Params {
  const float* x; float* out;
  const float* w1; const float* b1; const float* cs1;   // [MID][C]      h8l8, rows pre-scaled by 1/cs1
  const float* w2; const float* b2; const float* cs2;   // [MID][9*MID]  k = ((c/32)*9 + tap)*32 + c%32
  const float* w3; const float* b3; const float* cs3;   // [C][MID]
  int B, H;
  int* overflow;
  unsigned long long* prof = nullptr;   // SSG_BN_PROF builds: 8 phase timestamps (s_memtime) per workgroup
  // next-conv instance (NXT): conv1 of the following block on the tile this block has just produced
  const float* w1n = nullptr; const float* b1n = nullptr; const float* cs1n = nullptr;   // [MIDN][C] h8l8 row-major, rows pre-scaled by 1/cs1n
  float* y1n = nullptr;                 // [B,H,IW,MIDN]
  float* out_s2 = nullptr;              // [B,H/2,IW/2,C]: the pixels of `out` with even y and even x
};
#ifdef SSG_BN_PROF
#define SSG_BN_STAMP(I_) { if (p.prof && threadIdx.x == 0) p.prof[(size_t)blockIdx.x * 8 + (I_)] = __builtin_readcyclecounter(); }
#else
#define SSG_BN_STAMP(I_)
#endif

constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int C, int MID, int IW, int TH, int CIN = C>
struct Cfg {
  static constexpr int NW = 4, NTHR = NW * 64, HROWS = TH + 2, NPIX1 = HROWS * IW, NPIX = TH * IW;
  static constexpr int RPP = NTHR / 4;                 // 64-byte k-tile rows staged per pass of the workgroup (phase 3)
  // phase-1 k-tiles: 32 channels, whole 128-byte lines per pixel row (16-channel tiles, 64-byte pieces, cost two texture-addresser line
  // accesses per useful line and twice the load -> LDS -> barrier -> fragment round trips: identity blocks 1.59 -> 1.53 ms)
  static constexpr int K1T = 32, KS1 = K1T / 16, CPR1 = 4 * KS1, RPP1 = NTHR / CPR1;
  static constexpr int XROWS = (NPIX1 + RPP1 - 1) / RPP1 * RPP1;   // x rows of a phase-1 stage, padded to whole passes (the padding loads return zeros)
  static constexpr int P1 = 80;                        // LDS pitch of a 64-byte k-tile row (pitch/16 odd: conflict-free b128)
  static constexpr int P1T = K1T * 4 + 16;             // ... of a phase-1 row (144 bytes)
  static constexpr int P2 = 128 + 16;                  // ... of a phase-2 stage row (one (chunk, tap) k-tile: 128 bytes of a W2 row)
  static constexpr int PY = MID * 4 + 16;              // ... of a y1 / y2 pixel row (all MID channels, h8l8)
  static constexpr int BUF1 = (XROWS + MID) * P1T;     // phase-1 stage: x rows, then W1 rows
  static constexpr int ZERO_OFF = NPIX1 * PY;          // one all-zero pixel row (conv2's left / right padding)
  static constexpr int W2_OFF = (ZERO_OFF + PY + 255) / 256 * 256, BUF2 = MID * P2;
  static constexpr int W3_OFF = (NPIX * PY + 255) / 256 * 256, BUF3 = C * P1;
  static constexpr int LDS = cmax(cmax(2 * BUF1, W2_OFF + 2 * BUF2), W3_OFF + 2 * BUF3);
  static constexpr int DS = CIN != C;                  // downsample variant: conv3's reduction is [y2 | x]
  static constexpr int NK1 = CIN / K1T, NK2 = (MID / 32) * 9, NK3 = (MID + (DS ? CIN : 0)) / 16;
  // stages of global loads in flight ahead of the multiply (phase 1 is bound by HBM bandwidth, not latency: four are enough)
  static constexpr int PD1 = NK1 < 4 ? NK1 : 4, PD2 = 6;
  static_assert(NK2 % PD2 == 0, "phase-2 ring");
  static_assert(NPIX == 128 && NPIX1 % 32 == 0 && MID % RPP == 0 && MID % RPP1 == 0 && C % RPP == 0 && MID % (NW * 8) == 0, "128 output pixels, whole staging passes");
  static constexpr bool ZERO_EARLY = 2 * BUF1 <= ZERO_OFF;   // the zero row is written while phase 1 runs -- unless the stages cover it
  static_assert(LDS <= 80 * 1024, "two workgroups per CU");
};

// (the split-half codec -- split_encode4, split_pair_decode4, split_pair_pack, split_hi_nonfinite_bits -- is ssg_common.h's)
__device__ __forceinline__ float4 relu4(float4 v) {
  return make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f, v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
}
// x*w = xh*wl + xl*wh + xh*wh (the order of conv.hip's split_mma_step), weights as the first MFMA operand:
// C/D layout col = lane&31 -> pixel, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) -> channel

// Cache policy of the block's two streams that nobody re-reads from the L2 -- the residual re-read of x (its last use) and the stores of
// `out` (1-2 GB per launch at B = 1000).  With the default policy both allocate lines in the 4 MB L2s that the x rows, the halo rows of
// the neighbouring workgroup and the weights go through; with `nt` the layer1 identity blocks run 1.48 -> 1.30-1.35 ms and the layer2
// ones 1.22 -> 1.12 ms at nearly the same fabric traffic (FETCH_SIZE - 3 %: profiles/r06_ab_nt_policy.txt).  Same values, same order.
template <int C>
__device__ __forceinline__ float4 load_res_nt(const float* res, int row, int col) {   // channels col .. col + 3 of pixel row `row` of res [.][C]
  const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(res + (int64_t)row * C + col));
  return make_float4(t[0], t[1], t[2], t[3]);
}
__device__ __forceinline__ void store_out_nt(float* dst, const uint4 v) {
  const v4u sv = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(sv, reinterpret_cast<v4u*>(dst));
}
constexpr int AUX_NT = 2;   // the same policy as the cache-policy operand of a buffer instruction (the next-conv instance's streams)

template <int C, int MID, int IW, int TH, int CIN, bool NXT = false>
__global__ __launch_bounds__(256, 2) void bottleneck_kernel(Params p) {
  using K = Cfg<C, MID, IW, TH, CIN>;
  constexpr int NW = K::NW;
  constexpr bool DS = K::DS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
  const int tiles_img = p.H / TH, ntiles = p.B * tiles_img;
  int T;
  {   // workgroups are dealt round-robin to the 8 XCDs: give every XCD a contiguous run of tiles (halo rows hit its L2)
    const int b = (int)blockIdx.x, q = ntiles / 8, r = ntiles % 8, x = b % 8, s = b / 8;
    T = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + s;
  }
  const int img = T / tiles_img, ty0 = (T - img * tiles_img) * TH;
  SSG_BN_STAMP(0)
  if (K::ZERO_EARLY && tid < K::PY / 16) *reinterpret_cast<uint4*>(smem + K::ZERO_OFF + tid * 16) = make_uint4(0u, 0u, 0u, 0u);

  // =========================== phase 1: y1 = relu(conv1(x)) on the TH+2 halo rows ===========================
  constexpr int RPP = K::RPP, RPP1 = K::RPP1, AU = K::XROWS / RPP1, WU = MID / RPP1;   // 16-byte pieces per thread and k-tile: x rows, W1 rows
  const int ck = tid & 3, r0 = tid >> 2;               // phase 3 staging (64-byte rows)
  const int ck1 = tid % K::CPR1, r1 = tid / K::CPR1;   // phase 1 staging (128-byte rows)
  const float* ximg = p.x + (int64_t)img * p.H * IW * CIN;
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg), 0, (unsigned)(p.H * IW * CIN * 4), 0x00020000);
  // MFMA tiles of phase 1: (NPIX1/32) pixel tiles x (MID/32) channel tiles over the waves
  constexpr int MT1 = K::NPIX1 / 32, NT1 = MID / 32;
  // waves are split as WR x WC with WC = min(NT1, NW/2): each wave owns ceil(MT1/WR) pixel tiles x NT1/WC channel tiles (a pixel tile
  // beyond MT1 multiplies the zero padding rows of the stage and is not written)
  constexpr int WC1 = NT1 < NW / 2 ? NT1 : NW / 2, WR1 = NW / WC1, MTW1 = (MT1 + WR1 - 1) / WR1, NTW1 = NT1 / WC1;
  static_assert(NT1 % WC1 == 0 && (WR1 * MTW1) * 32 <= K::XROWS, "phase-1 tiles divide over the waves");
  const int i1b = (wave / WC1) * MTW1, j1b = (wave % WC1) * NTW1;
  v16f acc1[MTW1][NTW1];
#pragma unroll
  for (int i = 0; i < MTW1; i++)
#pragma unroll
    for (int j = 0; j < NTW1; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc1[i][j][r] = 0.f;
  // folded BatchNorm scale / bias of this wave's conv1 channels (needed after the loop: no L2 round trip there)
  float4 cs1r[NTW1][4], b1r[NTW1][4];
#pragma unroll
  for (int j = 0; j < NTW1; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      cs1r[j][q] = *reinterpret_cast<const float4*>(p.cs1 + (j1b + j) * 32 + 8 * q + 4 * h); b1r[j][q] = *reinterpret_cast<const float4*>(p.b1 + (j1b + j) * 32 + 8 * q + 4 * h);
    }
  unsigned aoff[AU];
#pragma unroll
  for (int u = 0; u < AU; u++) {
    const int hp = r1 + RPP1 * u, pix = (ty0 - 1) * IW + hp;  // rows above / below the image (and the padding rows of the stage): out-of-range offset -> the load returns zeros
    aoff[u] = (hp < K::NPIX1 && pix >= 0 && pix < p.H * IW) ? (unsigned)((pix * CIN + ck1 * 4) * 4) : 0x80000000u;
  }
  const float* w1p = p.w1 + (int64_t)r1 * CIN + ck1 * 4;
  v4f sa[K::PD1][AU], sw[K::PD1][WU];
#define SSG_BN_LOAD1(T_, S_)                                                                                         \
  {                                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < AU; u++) {                                                                  \
      const v4u raw = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, aoff[u], (T_) * (K::K1T * 4), 0);                  \
      sa[S_][u] = __builtin_bit_cast(v4f, raw);                                                                     \
    }                                                                                                                 \
    _Pragma("unroll") for (int u = 0; u < WU; u++) sw[S_][u] = *reinterpret_cast<const v4f*>(w1p + (int64_t)(RPP1 * u) * CIN + (T_) * K::K1T); \
  }
#define SSG_BN_STORE1(BUF_, S_)                                                                                      \
  {                                                                                                                  \
    unsigned char* sb_ = smem + (BUF_) * K::BUF1;                                                                    \
    _Pragma("unroll") for (int u = 0; u < AU; u++) *reinterpret_cast<v4f*>(sb_ + (r1 + RPP1 * u) * K::P1T + ck1 * 16) = sa[S_][u]; \
    _Pragma("unroll") for (int u = 0; u < WU; u++) *reinterpret_cast<v4f*>(sb_ + (K::XROWS + r1 + RPP1 * u) * K::P1T + ck1 * 16) = sw[S_][u]; \
  }
#define SSG_BN_MMA1(BUF_)                                                                                            \
  {                                                                                                                  \
    const unsigned char* sb_ = smem + (BUF_) * K::BUF1;                                                              \
    _Pragma("unroll") for (int ks = 0; ks < K::KS1; ks++) {                                                          \
    v8h xh_[MTW1], xl_[MTW1], wh_[NTW1], wl_[NTW1];                                                                  \
    _Pragma("unroll") for (int i = 0; i < MTW1; i++) {                                                               \
      const unsigned char* q_ = sb_ + ((i1b + i) * 32 + l32) * K::P1T + ks * 64 + h * 32;                            \
      xh_[i] = *reinterpret_cast<const v8h*>(q_); xl_[i] = *reinterpret_cast<const v8h*>(q_ + 16); }                 \
    _Pragma("unroll") for (int j = 0; j < NTW1; j++) {                                                               \
      const unsigned char* q_ = sb_ + (K::XROWS + (j1b + j) * 32 + l32) * K::P1T + ks * 64 + h * 32;                 \
      wh_[j] = *reinterpret_cast<const v8h*>(q_); wl_[j] = *reinterpret_cast<const v8h*>(q_ + 16); }                 \
    _Pragma("unroll") for (int i = 0; i < MTW1; i++) _Pragma("unroll") for (int j = 0; j < NTW1; j++)                \
      acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xl_[i], acc1[i][j], 0, 0, 0);                      \
    _Pragma("unroll") for (int i = 0; i < MTW1; i++) _Pragma("unroll") for (int j = 0; j < NTW1; j++)                \
      acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[j], xh_[i], acc1[i][j], 0, 0, 0);                      \
    _Pragma("unroll") for (int i = 0; i < MTW1; i++) _Pragma("unroll") for (int j = 0; j < NTW1; j++)                \
      acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xh_[i], acc1[i][j], 0, 0, 0);                      \
    }                                                                                                                \
  }
  // the register set of a tile is a LITERAL index (kt % PD1 of an unrolled loop variable leaves the rings in scratch memory)
#define SSG_BN_STEP1(KT_, S_)                                                                                        \
  {                                                                                                                  \
    if ((KT_) + K::PD1 < K::NK1) SSG_BN_LOAD1((KT_) + K::PD1, S_)   /* the set of tile KT_ went to LDS one step ago */ \
    SSG_BN_MMA1((S_) & 1)                                                                                            \
    if ((KT_) + 1 < K::NK1) SSG_BN_STORE1(((S_) + 1) & 1, ((S_) + 1) % K::PD1)                                        \
    __syncthreads();                                                                                                 \
  }
  static_assert(K::NK1 % K::PD1 == 0 && K::PD1 <= 4, "phase-1 ring of PD1 register sets");
#define SSG_BN_LOAD1_IF(S_) if constexpr ((S_) < K::PD1) SSG_BN_LOAD1(S_, S_)
  SSG_BN_LOAD1_IF(0) SSG_BN_LOAD1_IF(1) SSG_BN_LOAD1_IF(2) SSG_BN_LOAD1_IF(3)
#undef SSG_BN_LOAD1_IF
  SSG_BN_STORE1(0, 0)
  __syncthreads();
#define SSG_BN_STEP1_IF(KT_, S_) if constexpr ((S_) < K::PD1) SSG_BN_STEP1(KT_, S_)
#pragma unroll
  for (int kt0 = 0; kt0 < K::NK1; kt0 += K::PD1) {
    SSG_BN_STEP1_IF(kt0, 0) SSG_BN_STEP1_IF(kt0 + 1, 1) SSG_BN_STEP1_IF(kt0 + 2, 2) SSG_BN_STEP1_IF(kt0 + 3, 3)
  }
#undef SSG_BN_STEP1_IF
#undef SSG_BN_STEP1
  SSG_BN_STAMP(1)
#undef SSG_BN_LOAD1
#undef SSG_BN_STORE1
#undef SSG_BN_MMA1

  // ---- conv2 weights: first k-tiles on their way while y1 is written
  constexpr int RP8 = K::NTHR / 8, BU = MID / RP8;   // 16-byte pieces per thread and W2 stage (MID rows x 128 B)
  const int ck8 = tid % 8, r8 = tid / 8;
  const float* w2p = p.w2 + (int64_t)r8 * (9 * MID) + ck8 * 4;
  v4f sb2[K::PD2][BU];
#define SSG_BN_LOAD2(T_, S_)                                                                                         \
  { _Pragma("unroll") for (int u = 0; u < BU; u++) sb2[S_][u] = *reinterpret_cast<const v4f*>(w2p + (int64_t)(RP8 * u) * (9 * MID) + (T_) * 32); }
#define SSG_BN_STORE2(BUF_, S_)                                                                                      \
  { unsigned char* sb_ = smem + K::W2_OFF + (BUF_) * K::BUF2;                                                        \
    _Pragma("unroll") for (int u = 0; u < BU; u++) *reinterpret_cast<v4f*>(sb_ + (r8 + RP8 * u) * K::P2 + ck8 * 16) = sb2[S_][u]; }
  SSG_BN_LOAD2(0, 0) SSG_BN_LOAD2(1, 1) SSG_BN_LOAD2(2, 2) SSG_BN_LOAD2(3, 3) SSG_BN_LOAD2(4, 4) SSG_BN_LOAD2(5, 5)

  // ---- y1 -> LDS (h8l8 pixel rows).  Rows outside the image are conv2's zero padding, not relu(bias).
  unsigned ovf = 0u;
#pragma unroll
  for (int i = 0; i < MTW1; i++) {
    if (i1b + i >= MT1) continue;                           // (a padding tile of the last wave row)
    const int hp0 = (i1b + i) * 32;                         // first halo pixel of this MFMA tile
    const int irow = ty0 - 1 + (hp0 + l32) / IW;
    const bool inside = irow >= 0 && irow < p.H;
#pragma unroll
    for (int j = 0; j < NTW1; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int ch = (j1b + j) * 32 + 8 * q + 4 * h;
        const float4 cs = cs1r[j][q], bi = b1r[j][q];
        float4 v = make_float4(acc1[i][j][4 * q] * cs.x + bi.x, acc1[i][j][4 * q + 1] * cs.y + bi.y, acc1[i][j][4 * q + 2] * cs.z + bi.z,
                               acc1[i][j][4 * q + 3] * cs.w + bi.w);
        v = relu4(v);
        if (!inside) v = make_float4(0.f, 0.f, 0.f, 0.f);
        uint2 hi, lo;
        split_encode4(v, hi, lo);
        ovf |= split_hi_nonfinite_bits(hi);
        unsigned char* d = smem + (hp0 + l32) * K::PY + (ch >> 3) * 32 + h * 8;
        *reinterpret_cast<uint2*>(d) = hi; *reinterpret_cast<uint2*>(d + 16) = lo;
      }
  }
  if (!K::ZERO_EARLY && tid < K::PY / 16) *reinterpret_cast<uint4*>(smem + K::ZERO_OFF + tid * 16) = make_uint4(0u, 0u, 0u, 0u);   // (phase 1 is over: its stages covered this row)
  SSG_BN_STORE2(0, 0)
  __syncthreads();
  SSG_BN_STAMP(2)

  // =========================== phase 2: y2 = relu(conv2_3x3(y1)), pixel operand from LDS ===========================
  // wave = its own 32-pixel tile x all NT2 channel tiles
  constexpr int NT2 = MID / 32;
  v16f acc2[NT2];
#pragma unroll
  for (int j = 0; j < NT2; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc2[j][r] = 0.f;
  const int m2 = wave * 32 + l32, ty2 = m2 / IW, tx2 = m2 - ty2 * IW;       // this lane's output pixel (tile-local)
  float4 cs2r[NT2][4], b2r[NT2][4];                        // needed right after the loop (NXT: fetched there, its registers do not reach)
  if constexpr (!NXT)
#pragma unroll
  for (int j = 0; j < NT2; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      cs2r[j][q] = *reinterpret_cast<const float4*>(p.cs2 + j * 32 + 8 * q + 4 * h); b2r[j][q] = *reinterpret_cast<const float4*>(p.b2 + j * 32 + 8 * q + 4 * h);
    }
#define SSG_BN_STEP2(KT_, S_, B_)                                                                                     \
  {                                                                                                                  \
    if ((KT_) + K::PD2 < K::NK2) SSG_BN_LOAD2((KT_) + K::PD2, S_)                                                     \
    {                                                                                                                \
      const int chunk = (KT_) / 9, tap = (KT_) - chunk * 9, r = tap / 3, s = tap - r * 3;                            \
      const int xin = tx2 + s - 1;                                                                                   \
      const bool inrow = xin >= 0 && xin < IW;                                                                       \
      const int arow = ((ty2 + r) * IW + xin) * K::PY;     /* (taken unconditionally: a select, not a branch) */     \
      const int abase = inrow ? arow : K::ZERO_OFF;                                                                  \
      const unsigned char* wb = smem + K::W2_OFF + (B_) * K::BUF2 + l32 * K::P2 + h * 32;                             \
      v8h xh_[2], xl_[2], wh_[2][NT2], wl_[2][NT2];                                                                  \
      _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                             \
        const unsigned char* q_ = smem + abase + (chunk * 4 + ks * 2 + h) * 32;                                      \
        xh_[ks] = *reinterpret_cast<const v8h*>(q_); xl_[ks] = *reinterpret_cast<const v8h*>(q_ + 16);               \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) {                                                            \
          wh_[ks][j] = *reinterpret_cast<const v8h*>(wb + j * 32 * K::P2 + ks * 64);                                 \
          wl_[ks][j] = *reinterpret_cast<const v8h*>(wb + j * 32 * K::P2 + ks * 64 + 16); }                          \
      }                                                                                                              \
      _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                             \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[ks][j], xl_[ks], acc2[j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[ks][j], xh_[ks], acc2[j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[ks][j], xh_[ks], acc2[j], 0, 0, 0); \
      }                                                                                                              \
    }                                                                                                                \
    if ((KT_) + 1 < K::NK2) SSG_BN_STORE2((B_) ^ 1, ((S_) + 1) % K::PD2)                                              \
    __syncthreads();                                                                                                 \
  }
  // six steps per trip: the register set of step i is i (PD2 = 6), its LDS buffer i & 1
  static_assert(K::PD2 == 6, "phase-2 ring");
#pragma unroll
  for (int kt0 = 0; kt0 < K::NK2; kt0 += 6) {
    SSG_BN_STEP2(kt0, 0, 0) SSG_BN_STEP2(kt0 + 1, 1, 1) SSG_BN_STEP2(kt0 + 2, 2, 0)
    SSG_BN_STEP2(kt0 + 3, 3, 1) SSG_BN_STEP2(kt0 + 4, 4, 0) SSG_BN_STEP2(kt0 + 5, 5, 1)
  }
#undef SSG_BN_STEP2
  SSG_BN_STAMP(3)
#undef SSG_BN_LOAD2
#undef SSG_BN_STORE2

  if constexpr (NXT) {
  // =========================== next-conv instance: phase 3 in passes, then y1n = relu(conv1_next(out)) ===========================
  // The last layer1 block also multiplies the tile it has just produced by conv1 of the next block (W1n [MIDN][C]), so that launch --
  // a read of all of `out` from HBM -- goes away.  The wave keeps its y2 fragments in registers (K = 64: 32 of them); conv3 + epilogue
  // run in passes of 64 output channels; the epilogue writes each encoded pair back in place of the 32 bytes it read from the
  // wave's fp32 patch: at the 144-byte patch pitch that is the fragment format, and each 32-channel tile of `out` feeds two k-steps of
  // acc4[4] += W1n . out (32 pixels x 128 channels per wave).  W3 stages (64 rows x 64 channels) and W1n stages (128 rows x 32
  // channels) take turns in one two-buffer ring behind the wave rows: per pass W3, W1n, W1n; one barrier per stage.
  // k-steps ascend, the three products keep their order: y1n is bit-identical to ssg_conv2d_nhwc_x(out, W1n).
  static_assert(!DS && MID == 64 && C == 256 && IW == 32 && NT2 == 2, "the layer1 identity block");
  constexpr int MIDN = 128, NCP = 64, NPASS = C / NCP, NSTEP = 3 * NPASS;
  constexpr int P3N = MID * 4 + 16, PN = 144, NXSTG = cmax(NCP * P3N, MIDN * PN);   // stage rows: W3 256 B, W1n 128 B (pitch / 16 odd)
  constexpr int EP = 36, CPR = 8, RPI = 8, ITS = 4;
  static_assert(K::W3_OFF + 2 * NXSTG <= K::LDS && 32 * EP * 4 <= 32 * K::PY && EP * 4 == PN && NPASS % 2 == 0, "ring behind the wave rows, patch in them");
  const int ck16 = tid & 15, r16 = tid >> 4, ckn = tid & 7, rn = tid >> 3;
  // every global stream of this phase goes through a buffer resource: one 32-bit offset per lane and stream, the rest uniform (64-bit
  // lane addresses per row of the epilogue do not fit next to acc4)
  const __amdgpu_buffer_rsrc_t w3rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w3), 0, (unsigned)(C * MID * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t wnrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w1n), 0, (unsigned)(MIDN * C * 4), 0x00020000);
  const unsigned w3o = (unsigned)((r16 * MID + ck16 * 4) * 4), wno = (unsigned)((rn * C + ckn * 4) * 4);
  v4f sn[2][4];
#define SSG_BN_NLOAD(I_)      /* stage 6 pp + I_ -> register set I_ & 1 */                                           \
  { if (6 * pp + (I_) < NSTEP) { const int ps_ = 2 * pp + (I_) / 3;                                                  \
      if constexpr ((I_) % 3 == 0) { _Pragma("unroll") for (int u = 0; u < 4; u++) sn[(I_) & 1][u] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(w3rsrc, w3o, ((ps_ * NCP + 16 * u) * MID) * 4, 0)); } \
      else { _Pragma("unroll") for (int u = 0; u < 4; u++) sn[(I_) & 1][u] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(wnrsrc, wno, ((32 * u) * C + (2 * ps_ + (I_) % 3 - 1) * 32) * 4, 0)); } } }
#define SSG_BN_NSTORE(I_)     /* register set I_ & 1 -> LDS buffer I_ & 1 */                                         \
  { if (6 * pp + (I_) < NSTEP) { unsigned char* sb_ = smem + K::W3_OFF + ((I_) & 1) * NXSTG;                         \
      if constexpr ((I_) % 3 == 0) { _Pragma("unroll") for (int u = 0; u < 4; u++) *reinterpret_cast<v4f*>(sb_ + (r16 + 16 * u) * P3N + ck16 * 16) = sn[(I_) & 1][u]; } \
      else { _Pragma("unroll") for (int u = 0; u < 4; u++) *reinterpret_cast<v4f*>(sb_ + (rn + 32 * u) * PN + ckn * 16) = sn[(I_) & 1][u]; } } }
  { constexpr int pp = 0; SSG_BN_NLOAD(0) SSG_BN_NLOAD(1) }
  // ---- y2 -> this wave's rows (as below), then its MFMA fragments for all of conv3: the rows are dead from here on
  unsigned char* myrows = smem + (wave * 32) * K::PY;
#pragma unroll
  for (int j = 0; j < NT2; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ch = j * 32 + 8 * q + 4 * h;
      const float4 cs = *reinterpret_cast<const float4*>(p.cs2 + ch), bi = *reinterpret_cast<const float4*>(p.b2 + ch);
      float4 v = make_float4(acc2[j][4 * q] * cs.x + bi.x, acc2[j][4 * q + 1] * cs.y + bi.y, acc2[j][4 * q + 2] * cs.z + bi.z, acc2[j][4 * q + 3] * cs.w + bi.w);
      v = relu4(v);
      uint2 hi, lo;
      split_encode4(v, hi, lo);
      ovf |= split_hi_nonfinite_bits(hi);
      unsigned char* d = myrows + l32 * K::PY + (ch >> 3) * 32 + h * 8;
      *reinterpret_cast<uint2*>(d) = hi; *reinterpret_cast<uint2*>(d + 16) = lo;
    }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  v8h y2h[MID / 16], y2l[MID / 16];
#pragma unroll
  for (int ks = 0; ks < MID / 16; ks++) {
    const unsigned char* q_ = myrows + l32 * K::PY + (ks * 2 + h) * 32;
    y2h[ks] = *reinterpret_cast<const v8h*>(q_); y2l[ks] = *reinterpret_cast<const v8h*>(q_ + 16);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  { constexpr int pp = 0; SSG_BN_NSTORE(0) }
  __syncthreads();

  const int chunk = lane % CPR, prow = lane / CPR, odd = lane & 1;
  const int64_t gpix0 = ((int64_t)img * p.H + ty0) * IW + wave * 32;       // first output pixel of this wave: one image row
  // x / out: the tile's 128 pixels are contiguous; this lane's rows are pixels wave * 32 + it * RPI + prow
  const unsigned tpo = (unsigned)(((wave * 32 + prow) * C + chunk * 4) * 4);
  const unsigned xro = (unsigned)(ty0 * IW * C * 4) + tpo;
  const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(p.out ? p.out + ((int64_t)img * p.H + ty0) * IW * C : nullptr, 0,
                                                                         p.out ? (unsigned)(K::NPIX * C * 4) : 0u, 0x00020000);
  // out_s2: even image rows (ty0 is a multiple of 4: the even waves), even pixels of the row (pr even <=> prow even), whole 128-byte
  // segments; the other lanes carry an out-of-range offset: their stores are dropped
  const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(p.out_s2 ? p.out_s2 + (((int64_t)img * (p.H / 2) + ty0 / 2) * (IW / 2)) * C : nullptr, 0,
                                                                         p.out_s2 ? (unsigned)((TH / 2) * (IW / 2) * C * 4) : 0u, 0x00020000);
  const unsigned s2o = ((wave | prow) & 1) ? 0x80000000u : (unsigned)((((wave >> 1) * (IW / 2) + (prow >> 1)) * C + chunk * 4) * 4);
  float* const patch = reinterpret_cast<float*>(myrows);
  const unsigned char* const patchb = myrows;
  v16f acc3[NCP / 32], acc4[MIDN / 32];
#pragma unroll
  for (int j = 0; j < MIDN / 32; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc4[j][r] = 0.f;
  float4 rr[ITS], b3r, cs3r;
  // the epilogue operands of channel tile T_ (residual rows, bias, scale): fetched as soon as the tile before has used its own (one
  // register set: two leave no room for acc4), a multiply or more ahead of their use
#define SSG_BN_NEPIOPS(T_)                                                                                           \
  { _Pragma("unroll") for (int it = 0; it < ITS; it++) { const v4u t4_ = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, xro, (it * RPI * C + (T_) * 32) * 4, AUX_NT);  \
      rr[it] = make_float4(__uint_as_float(t4_[0]), __uint_as_float(t4_[1]), __uint_as_float(t4_[2]), __uint_as_float(t4_[3])); } \
    b3r = *reinterpret_cast<const float4*>(p.b3 + (T_) * 32 + chunk * 4); cs3r = *reinterpret_cast<const float4*>(p.cs3 + (T_) * 32 + chunk * 4); }
  SSG_BN_NEPIOPS(0)
  // stage I_ = W3 of pass 2 pp + I_ / 3: conv3 over the whole K = 64 for the pass's 64 output channels
#define SSG_BN_NSTEP3(I_)                                                                                            \
  { SSG_BN_NLOAD((I_) + 2)                                                                                         \
    _Pragma("unroll") for (int j = 0; j < NCP / 32; j++) _Pragma("unroll") for (int r = 0; r < 16; r++) acc3[j][r] = 0.f; \
    const unsigned char* wb_ = smem + K::W3_OFF + ((I_) & 1) * NXSTG + l32 * P3N + h * 32;                            \
    _Pragma("unroll") for (int ks = 0; ks < MID / 16; ks++) {                                                        \
      const v8h xh_ = y2h[ks], xl_ = y2l[ks];                                                                        \
      v8h wh_[NCP / 32], wl_[NCP / 32];                                                                              \
      _Pragma("unroll") for (int j = 0; j < NCP / 32; j++) {                                                         \
        wh_[j] = *reinterpret_cast<const v8h*>(wb_ + j * 32 * P3N + ks * 64); wl_[j] = *reinterpret_cast<const v8h*>(wb_ + j * 32 * P3N + ks * 64 + 16); } \
      _Pragma("unroll") for (int j = 0; j < NCP / 32; j++) acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xl_, acc3[j], 0, 0, 0); \
      _Pragma("unroll") for (int j = 0; j < NCP / 32; j++) acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[j], xh_, acc3[j], 0, 0, 0); \
      _Pragma("unroll") for (int j = 0; j < NCP / 32; j++) acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xh_, acc3[j], 0, 0, 0); \
    }                                                                                                                \
    SSG_BN_NSTORE((I_) + 1)                                                                                          \
    __syncthreads();                                                                                                 \
  }
  // stage I_ = W1n columns of out's channel tile ct_ = 2 ps_ + J_: the tile's epilogue (the code path of the plain instance; the encoded
  // pair goes back in place of the fp32 values), then two k-steps of conv1_next from the patch
#define SSG_BN_NSTEPN(I_, J_)                                                                                        \
  { const int ct_ = 2 * (2 * pp + (I_) / 3) + (J_);                                                                 \
    SSG_BN_NLOAD((I_) + 2)                                                                                           \
    const float4 bias = b3r, cs = cs3r;                                                                              \
    _Pragma("unroll") for (int q = 0; q < 4; q++)                                                                    \
      *reinterpret_cast<float4*>(patch + l32 * EP + 8 * q + 4 * h) = make_float4(acc3[J_][4 * q], acc3[J_][4 * q + 1], acc3[J_][4 * q + 2], acc3[J_][4 * q + 3]); \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                           \
    _Pragma("unroll") for (int it = 0; it < ITS; it++) {                                                             \
      const int pr = it * RPI + prow;                                                                                \
      float4 v = *reinterpret_cast<const float4*>(patch + pr * EP + chunk * 4);                                      \
      v.x = v.x * cs.x + bias.x; v.y = v.y * cs.y + bias.y; v.z = v.z * cs.z + bias.z; v.w = v.w * cs.w + bias.w;    \
      const float4 rw = rr[it];                                                                                      \
      float4 r4;                                                                                                     \
      {   /* even lane holds hi0..7 of the 8-channel group, odd lane lo0..7; each needs hi and lo of ITS four channels */ \
        const unsigned a0 = __float_as_uint(rw.x), a1 = __float_as_uint(rw.y), a2 = __float_as_uint(rw.z), a3 = __float_as_uint(rw.w); \
        const unsigned h0 = lane_pair_merge(a0, a2, odd), h1 = lane_pair_merge(a1, a3, odd);                         \
        const unsigned l0 = lane_pair_merge(a2, a0, !odd), l1 = lane_pair_merge(a3, a1, !odd);                       \
        r4 = split_decode4(make_uint2(h0, h1), make_uint2(l0, l1));                                                  \
      }                                                                                                              \
      v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;                                                            \
      v = relu4(v);                                                                                                  \
      uint2 hp, lp;                                                                                                  \
      split_encode4(v, hp, lp);                                                                                      \
      ovf |= split_hi_nonfinite_bits(hp);                                                                            \
      const uint4 pk = split_pair_pack(hp, lp, odd);                                                                 \
      const v4u sv_ = {pk.x, pk.y, pk.z, pk.w};                                                                      \
      *reinterpret_cast<v4u*>(patch + pr * EP + chunk * 4) = sv_;   /* lanes 2g, 2g + 1: hi x 8 | lo x 8 of channel group g */ \
      if (p.out) __builtin_amdgcn_raw_buffer_store_b128(sv_, orsrc, tpo, (it * RPI * C + ct_ * 32) * 4, AUX_NT);       \
      if (p.out_s2) __builtin_amdgcn_raw_buffer_store_b128(sv_, srsrc, s2o, (it * (RPI / 2) * C + ct_ * 32) * 4, AUX_NT); \
    }                                                                                                                \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                           \
    if (ct_ + 1 < C / 32) SSG_BN_NEPIOPS(ct_ + 1)                                                                    \
    const unsigned char* wb_ = smem + K::W3_OFF + ((I_) & 1) * NXSTG + l32 * PN + h * 32;                             \
    _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                               \
      const unsigned char* q_ = patchb + l32 * PN + (ks * 2 + h) * 32;                                               \
      const v8h xh_ = *reinterpret_cast<const v8h*>(q_), xl_ = *reinterpret_cast<const v8h*>(q_ + 16);               \
      _Pragma("unroll") for (int jj = 0; jj < MIDN / 32; jj += 2) {   /* (pairs of channel tiles: registers) */     \
        v8h wh_[2], wl_[2];                                                                                          \
        _Pragma("unroll") for (int j = 0; j < 2; j++) {                                                              \
          wh_[j] = *reinterpret_cast<const v8h*>(wb_ + (jj + j) * 32 * PN + ks * 64); wl_[j] = *reinterpret_cast<const v8h*>(wb_ + (jj + j) * 32 * PN + ks * 64 + 16); } \
        _Pragma("unroll") for (int j = 0; j < 2; j++) acc4[jj + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xl_, acc4[jj + j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < 2; j++) acc4[jj + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[j], xh_, acc4[jj + j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < 2; j++) acc4[jj + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xh_, acc4[jj + j], 0, 0, 0); \
      }                                                                                                              \
    }                                                                                                                \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                           \
    SSG_BN_NSTORE((I_) + 1)                                                                                          \
    __syncthreads();                                                                                                 \
  }
  // two passes per trip: the register set and the LDS buffer of step i are i & 1
#pragma unroll 1
  for (int pp = 0; pp < NPASS / 2; pp++) {
    SSG_BN_NSTEP3(0) SSG_BN_NSTEPN(1, 0) SSG_BN_NSTEPN(2, 1)
    SSG_BN_NSTEP3(3) SSG_BN_NSTEPN(4, 0) SSG_BN_NSTEPN(5, 1)
  }
  SSG_BN_STAMP(4)
#undef SSG_BN_NSTEPN
#undef SSG_BN_NSTEP3
#undef SSG_BN_NEPIOPS
#undef SSG_BN_NSTORE
#undef SSG_BN_NLOAD
  // ---- y1n: conv_dma_kernel's epilogue (scale, bias, ReLU, encode) per 32-channel tile through the patch; default cache policy: the
  // next launch's operand
  if (p.y1n) {
    float* __restrict__ ynp = p.y1n + gpix0 * MIDN;
#pragma unroll
    for (int j = 0; j < MIDN / 32; j++) {
      const int col = j * 32 + chunk * 4;
      const float4 bias = *reinterpret_cast<const float4*>(p.b1n + col), cs = *reinterpret_cast<const float4*>(p.cs1n + col);
#pragma unroll
      for (int q = 0; q < 4; q++)
        *reinterpret_cast<float4*>(patch + l32 * EP + 8 * q + 4 * h) = make_float4(acc4[j][4 * q], acc4[j][4 * q + 1], acc4[j][4 * q + 2], acc4[j][4 * q + 3]);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int it = 0; it < ITS; it++) {
        const int pr = it * RPI + prow;
        float4 v = *reinterpret_cast<const float4*>(patch + pr * EP + chunk * 4);
        v.x = v.x * cs.x + bias.x; v.y = v.y * cs.y + bias.y; v.z = v.z * cs.z + bias.z; v.w = v.w * cs.w + bias.w;
        v = relu4(v);
        uint2 hp, lp;
        split_encode4(v, hp, lp);
        ovf |= split_hi_nonfinite_bits(hp);
        const uint4 pk = split_pair_pack(hp, lp, odd);
        *reinterpret_cast<uint4*>(ynp + (int64_t)pr * MIDN + col) = pk;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
  } else {
  // ---- conv3 weights: k-tiles 0 and 1 on their way while y2 is written (every wave is past its last y1 / W2 read)
  constexpr int CU3 = C / RPP;                             // 16-byte pieces per thread and W3 k-tile (C rows x 64 B)
  constexpr int K3 = MID + (DS ? CIN : 0);                 // conv3's reduction length (the weight row)
  const float* w3p = p.w3 + (int64_t)r0 * K3 + ck * 4;
  v4f sc3[2][CU3];
#define SSG_BN_LOAD3(T_, S_)                                                                                         \
  { _Pragma("unroll") for (int u = 0; u < CU3; u++) sc3[S_][u] = *reinterpret_cast<const v4f*>(w3p + (int64_t)(RPP * u) * K3 + (T_) * 16); }
#define SSG_BN_STORE3(BUF_, S_)                                                                                      \
  { unsigned char* sb_ = smem + K::W3_OFF + (BUF_) * K::BUF3;                                                        \
    _Pragma("unroll") for (int u = 0; u < CU3; u++) *reinterpret_cast<v4f*>(sb_ + (r0 + RPP * u) * K::P1 + ck * 16) = sc3[S_][u]; }
  SSG_BN_LOAD3(0, 0)
  SSG_BN_LOAD3(1, 1)
  constexpr int NT3 = C / 32;                              // phase-3 wave = its own 32-pixel tile x all NT3 channel tiles
  const int64_t gpix0 = ((int64_t)img * p.H + ty0) * IW + wave * 32;       // first output pixel of this wave (pixels are contiguous)
  // DS: the downsample operand, this lane's pixel, k-tiles MID/16 .. NK3-1 = channels of x: [8 hi][8 lo] of group h per k-tile
  constexpr int NXK = DS ? CIN / 16 : 1;
  v8h xrh[NXK], xrl[NXK];
  if constexpr (DS) {
    const float* xq = p.x + (gpix0 + l32) * CIN + h * 8;
#pragma unroll
    for (int t = 0; t < NXK; t++) { xrh[t] = *reinterpret_cast<const v8h*>(xq + t * 16); xrl[t] = *reinterpret_cast<const v8h*>(xq + t * 16 + 4); }
  }
  // y2 rows: phase 2 writes the rows of this wave's pixel tile, phase 3 reads the same rows
  unsigned char* myrows = smem + (wave * 32) * K::PY;
#pragma unroll
  for (int j = 0; j < NT2; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ch = j * 32 + 8 * q + 4 * h;
      const float4 cs = cs2r[j][q], bi = b2r[j][q];
      float4 v = make_float4(acc2[j][4 * q] * cs.x + bi.x, acc2[j][4 * q + 1] * cs.y + bi.y, acc2[j][4 * q + 2] * cs.z + bi.z, acc2[j][4 * q + 3] * cs.w + bi.w);
      v = relu4(v);
      uint2 hi, lo;
      split_encode4(v, hi, lo);
      ovf |= split_hi_nonfinite_bits(hi);
      unsigned char* d = smem + (wave * 32 + l32) * K::PY + (ch >> 3) * 32 + h * 8;
      *reinterpret_cast<uint2*>(d) = hi; *reinterpret_cast<uint2*>(d + 16) = lo;
    }

  // =========================== phase 3: out = relu(conv3(y2) + x) ===========================
  static_assert(K::NK3 % 2 == 0, "phase 3 takes its k-tiles in rounds of two buffers");
  v16f acc3[NT3];
#pragma unroll
  for (int j = 0; j < NT3; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc3[j][r] = 0.f;
#define SSG_BN_MMA3K(BUF_, KT_)                                                                                      \
  {                                                                                                                  \
    v8h xh_, xl_;                                                                                                    \
    if constexpr (DS && (KT_) >= MID / 16) { xh_ = xrh[((KT_) - MID / 16) % NXK]; xl_ = xrl[((KT_) - MID / 16) % NXK]; } \
    else {                                                                                                           \
      const unsigned char* q_ = myrows + l32 * K::PY + (((KT_) % (MID / 16)) * 2 + h) * 32;                          \
      xh_ = *reinterpret_cast<const v8h*>(q_); xl_ = *reinterpret_cast<const v8h*>(q_ + 16);                         \
    }                                                                                                                \
    const unsigned char* wb_ = smem + K::W3_OFF + (BUF_) * K::BUF3 + l32 * K::P1 + h * 32;                           \
    _Pragma("unroll") for (int jj = 0; jj < NT3; jj += 4) {                                                          \
      v8h wh_[4], wl_[4];                                                                                            \
      _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                \
        wh_[j] = *reinterpret_cast<const v8h*>(wb_ + (jj + j) * 32 * K::P1); wl_[j] = *reinterpret_cast<const v8h*>(wb_ + (jj + j) * 32 * K::P1 + 16); } \
      _Pragma("unroll") for (int j = 0; j < 4; j++) acc3[jj + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xl_, acc3[jj + j], 0, 0, 0); \
      _Pragma("unroll") for (int j = 0; j < 4; j++) acc3[jj + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[j], xh_, acc3[jj + j], 0, 0, 0); \
      _Pragma("unroll") for (int j = 0; j < 4; j++) acc3[jj + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xh_, acc3[jj + j], 0, 0, 0); \
    }                                                                                                                \
  }
  // epilogue addressing / operands (the first channel tile's are fetched during the last round of the multiply)
  constexpr int EP = 36, CPR = 8, RPI = 8, ITS = 4;
  const int chunk = lane % CPR, prow = lane / CPR, odd = lane & 1;
  const float* __restrict__ resp = p.x + gpix0 * C;        // residual (identity blocks only)
  float* __restrict__ outp = p.out + gpix0 * C;
  float4 rr[2][ITS], b3r[2], cs3r[2];
  SSG_BN_STORE3(0, 0)
  SSG_BN_STORE3(1, 1)
  if constexpr (K::NK3 > 2) { SSG_BN_LOAD3(2, 0) SSG_BN_LOAD3(3, 1) }
  __syncthreads();
  static_assert(K::NK3 / 2 <= 4, "at most four rounds");
#define SSG_BN_ROUND3(R_)                                                                                            \
  if constexpr ((R_) < K::NK3 / 2) {                                                                                 \
    SSG_BN_MMA3K(0, 2 * (R_))                                                                                        \
    SSG_BN_MMA3K(1, 2 * (R_) + 1)                                                                                    \
    if constexpr ((R_) + 1 < K::NK3 / 2) {                                                                           \
      __syncthreads();                       /* everybody is done reading the two buffers */                         \
      SSG_BN_STORE3(0, 0)                                                                                            \
      SSG_BN_STORE3(1, 1)                                                                                            \
      if constexpr ((R_) + 2 < K::NK3 / 2) { SSG_BN_LOAD3(2 * (R_) + 4, 0) SSG_BN_LOAD3(2 * (R_) + 5, 1) }           \
      else {                                 /* last round ahead: the W3 staging registers are free for the epilogue's first operands */ \
        if constexpr (!DS) {                                                                                         \
          _Pragma("unroll") for (int it = 0; it < ITS; it++) rr[0][it] = load_res_nt<C>(resp, it * RPI + prow, chunk * 4); \
        }                                                                                                            \
        b3r[0] = *reinterpret_cast<const float4*>(p.b3 + chunk * 4); cs3r[0] = *reinterpret_cast<const float4*>(p.cs3 + chunk * 4); \
      }                                                                                                              \
      __syncthreads();                                                                                               \
    }                                                                                                                \
  }
  SSG_BN_ROUND3(0) SSG_BN_ROUND3(1) SSG_BN_ROUND3(2) SSG_BN_ROUND3(3)
#undef SSG_BN_ROUND3
  SSG_BN_STAMP(4)
#undef SSG_BN_LOAD3
#undef SSG_BN_STORE3
#undef SSG_BN_MMA3K

  // ---- epilogue: per channel tile a 32-pixel x 32-channel patch through LDS (this wave's own, now dead, y2 rows), then
  // whole 128-byte row segments: bias, residual (x, h8l8), ReLU, re-encode, store.  Same code path as conv.hip.
  static_assert(32 * EP * 4 <= 32 * K::PY, "patch fits in the wave's y2 rows");
  float* const patch = reinterpret_cast<float*>(myrows);                  // its y2 rows are this wave's alone and dead now
#pragma unroll
  for (int j = 0; j < NT3; j++) {
    const int col = j * 32 + chunk * 4;
    if (j + 1 < NT3) {
      if constexpr (!DS) {
#pragma unroll
        for (int it = 0; it < ITS; it++) rr[(j + 1) & 1][it] = load_res_nt<C>(resp, it * RPI + prow, col + 32);
      }
      b3r[(j + 1) & 1] = *reinterpret_cast<const float4*>(p.b3 + col + 32); cs3r[(j + 1) & 1] = *reinterpret_cast<const float4*>(p.cs3 + col + 32);
    }
    const float4 bias = b3r[j & 1], cs = cs3r[j & 1];
#pragma unroll
    for (int q = 0; q < 4; q++)
      *reinterpret_cast<float4*>(patch + l32 * EP + 8 * q + 4 * h) = make_float4(acc3[j][4 * q], acc3[j][4 * q + 1], acc3[j][4 * q + 2], acc3[j][4 * q + 3]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int it = 0; it < ITS; it++) {
      const int pr = it * RPI + prow;
      float4 v = *reinterpret_cast<const float4*>(patch + pr * EP + chunk * 4);
      v.x = v.x * cs.x + bias.x; v.y = v.y * cs.y + bias.y; v.z = v.z * cs.z + bias.z; v.w = v.w * cs.w + bias.w;
      if constexpr (!DS) {
      const float4 rw = rr[j & 1][it];
      float4 r4;
      {   // even lane holds hi0..7 of the 8-channel group, odd lane lo0..7; each needs hi and lo of ITS four channels
        // (component-wise selects: a select between uint2 / float4 aggregates goes through scratch memory)
        const unsigned a0 = __float_as_uint(rw.x), a1 = __float_as_uint(rw.y), a2 = __float_as_uint(rw.z), a3 = __float_as_uint(rw.w);
        const unsigned h0 = lane_pair_merge(a0, a2, odd), h1 = lane_pair_merge(a1, a3, odd);
        const unsigned l0 = lane_pair_merge(a2, a0, !odd), l1 = lane_pair_merge(a3, a1, !odd);
        r4 = split_decode4(make_uint2(h0, h1), make_uint2(l0, l1));
      }
      v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
      }
      v = relu4(v);
      uint2 hp, lp;
      split_encode4(v, hp, lp);
      ovf |= split_hi_nonfinite_bits(hp);
      const uint4 stv = split_pair_pack(hp, lp, odd);
      store_out_nt(outp + (int64_t)pr * C + col, stv);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  }   // (!NXT)
  if ((ovf & 0x80008000u) && p.overflow) *p.overflow = 1;
  SSG_BN_STAMP(5)
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Layer2 in channel halves: the same block, the same 128-pixel tile.  With all 128 y1 channels of the halo rows in
// LDS (85 KB) only one workgroup fits on a CU and its phases run one after the other; in halves the workgroup stays within 80 KB, so that
// two share a CU as the layer1 instance's do (measured at B = 1000 against such a one-per-CU instance: 1.13 -> 1.01 ms per block).
//   * y1 in two channel halves: conv2 reduces chunk -> tap -> channel, chunks 0-1 read only y1 channels 0-63, chunks 2-3 only 64-127.
//     Phase 1 computes all 128 channels in ONE pass over x (every wave owns a channel tile of each half); half 0 goes to LDS (272-byte
//     pixel rows, 160 halo pixels = 43.5 KB) and feeds 18 (chunk, tap) k-tiles of conv2 while the accumulators of half 1 stay parked in
//     registers (48 per lane); then half 1 takes over the same LDS rows for the other 18 k-tiles, into the same conv2 accumulators.
//     (A second phase-1 pass for half 1 instead of the parked registers reads x twice: HBM-bound at 0.98 ms, no gain.)
//   * phase-1 stages: whole 128-byte lines, rows unpadded and XOR-swizzled (two padded stages of 288 rows are 1 KB too large).
//   * y2 never lives in LDS as rows: each 32 x 32 accumulator tile turns through a wave-private patch (scale, bias, ReLU, encode as
//     before) and comes back as the MFMA fragments of conv3's pixel operand: 8 k-steps x (hi + lo) = 64 registers.
//   * conv3 + epilogue in four passes of 128 output channels, each over the whole K = 128 in four 32-channel stages (the W2 stage
//     shape and buffers); the epilogue is the code path of the kernel above.
// Every accumulator sees the same products in the same order as in the three launches of conv.hip: bit-identical to them.
template <int C, int MID, int IW, int TH>
struct CfgH {
  static constexpr int NW = 4, NTHR = NW * 64, HROWS = TH + 2, NPIX1 = HROWS * IW, NPIX = TH * IW;
  static constexpr int MH = MID / 2;                                    // y1 channels per half
  // phase-1 k-tiles: whole 128-byte lines, rows unpadded (two padded stages do not fit), 16-byte chunks XOR-swizzled with (row >> 1) & 7
  static constexpr int K1T = 32, P1T = K1T * 4, CPR1 = 8, RPP1 = NTHR / CPR1;
  static constexpr int XROWS = NPIX1, BUF1 = (XROWS + MID) * P1T;       // phase-1 stage: x rows, then W1 rows
  static constexpr int NK1 = C / K1T, PD1 = 2;
  static constexpr int PYH = MH * 4 + 16;                               // LDS pitch of a y1 pixel row of one half
  static constexpr int ZERO_OFF = NPIX1 * PYH;                          // conv2's left / right padding
  static constexpr int P2 = 144, W2_OFF = (ZERO_OFF + PYH + 255) / 256 * 256, BUF2 = MID * P2;   // W2 stages, later the W3 stages
  static constexpr int NK2H = (MH / 32) * 9, PD2 = 3;                   // (chunk, tap) k-tiles of conv2 per half
  static constexpr int NCP = 128, NPASS = C / NCP, KT3 = MID / 32;      // conv3: output channels per pass, passes, 32-channel stages per pass
  static constexpr int EP = 36, PATCH = 32 * EP * 4;                    // per-wave patch: the y2 turn (32 rows x 144 B) and the epilogue
  static constexpr int LDS = cmax(2 * BUF1, W2_OFF + 2 * BUF2);
  static_assert(NPIX == 128 && NPIX1 % RPP1 == 0 && MID % RPP1 == 0 && MH == 64 && MID == NCP && NK1 % PD1 == 0 && NK2H % 6 == 0 && KT3 == 4, "layer2 shape");
  static_assert(((NPIX1 + 31) / 32 + 1) / 2 == 3 && 6 * 32 <= XROWS + MID, "phase 1: 2 x 3 pixel tiles, the sixth one reads W1 rows of the stage");
  static_assert(RPP1 % 16 == 0 && XROWS % 16 == 0, "the swizzle of a row is that of its thread (r1) / its lane (l32)");
  static_assert(NW * PATCH <= ZERO_OFF && 32 * P2 == PATCH, "patches live in the dead y1 rows");
  static_assert(LDS <= 80 * 1024, "two workgroups per CU");
};

template <int C, int MID, int IW, int TH>
__global__ __launch_bounds__(256, 2) void bottleneck_halves_kernel(Params p) {
  using K = CfgH<C, MID, IW, TH>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
  const int tiles_img = p.H / TH, ntiles = p.B * tiles_img;
  int T;
  {   // the tile assignment of bottleneck_kernel: every XCD a contiguous run of tiles
    const int b = (int)blockIdx.x, q = ntiles / 8, r = ntiles % 8, x = b % 8, s = b / 8;
    T = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + s;
  }
  const int img = T / tiles_img, ty0 = (T - img * tiles_img) * TH;
  SSG_BN_STAMP(0)

  // phase-1 staging: thread = 16-byte piece ck1 of the 128-byte k-tile rows r1 + 32 u; waves = 2 rows of 3 pixel tiles x 2 pairs of
  // channel tiles {j1b, j1b + 2}: every wave owns one channel tile of each y1 half
  constexpr int RPP1 = K::RPP1, AU = K::XROWS / RPP1, WU = MID / RPP1, MT1 = K::NPIX1 / 32, MTW1 = 3;
  const int ck1 = tid & 7, r1 = tid >> 3;
  const float* ximg = p.x + (int64_t)img * p.H * IW * C;
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg), 0, (unsigned)(p.H * IW * C * 4), 0x00020000);
  const int i1b = (wave >> 1) * MTW1, j1b = wave & 1;
  v16f acc1[MTW1][2];                                        // [pixel tile][y1 half]
#pragma unroll
  for (int i = 0; i < MTW1; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc1[i][j][r] = 0.f;
  {
    // =========================== phase 1: y1 = relu(conv1(x)) on the TH+2 halo rows, all MID channels ===========================
    unsigned aoff[AU];
#pragma unroll
    for (int u = 0; u < AU; u++) {
      const int pix = (ty0 - 1) * IW + r1 + RPP1 * u;        // rows above / below the image: out-of-range offset -> the load returns zeros
      aoff[u] = (pix >= 0 && pix < p.H * IW) ? (unsigned)((pix * C + ck1 * 4) * 4) : 0x80000000u;
    }
    const float* w1p = p.w1 + (int64_t)r1 * C + ck1 * 4;
    const int wsw = ((ck1 ^ ((r1 >> 1) & 7)) * 16), rsw = (l32 >> 1) & 7;   // swizzled chunk of this thread's stores / swizzle of this lane's rows
    v4f sa[K::PD1][AU], sw[K::PD1][WU];
#define SSG_BH_LOAD1(T_, S_)                                                                                         \
    {                                                                                                                \
      _Pragma("unroll") for (int u = 0; u < AU; u++) {                                                                \
        const v4u raw = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, aoff[u], (T_) * (K::K1T * 4), 0);                \
        sa[S_][u] = __builtin_bit_cast(v4f, raw);                                                                   \
      }                                                                                                               \
      _Pragma("unroll") for (int u = 0; u < WU; u++) sw[S_][u] = *reinterpret_cast<const v4f*>(w1p + (int64_t)(RPP1 * u) * C + (T_) * K::K1T); \
    }
#define SSG_BH_STORE1(BUF_, S_)                                                                                      \
    {                                                                                                                \
      unsigned char* sb_ = smem + (BUF_) * K::BUF1;                                                                  \
      _Pragma("unroll") for (int u = 0; u < AU; u++) *reinterpret_cast<v4f*>(sb_ + (r1 + RPP1 * u) * K::P1T + wsw) = sa[S_][u]; \
      _Pragma("unroll") for (int u = 0; u < WU; u++) *reinterpret_cast<v4f*>(sb_ + (K::XROWS + r1 + RPP1 * u) * K::P1T + wsw) = sw[S_][u]; \
    }
    // (the sixth pixel tile of the second wave row does not exist: its fragment reads land in the W1 rows of the stage, its products
    // are never written)
#define SSG_BH_MMA1(BUF_)                                                                                            \
    {                                                                                                                \
      const unsigned char* sb_ = smem + (BUF_) * K::BUF1;                                                            \
      _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                             \
        const int ch_ = ((4 * ks + 2 * h) ^ rsw) * 16, cl_ = ((4 * ks + 2 * h + 1) ^ rsw) * 16;                      \
        v8h xh_[MTW1], xl_[MTW1], wh_[2], wl_[2];                                                                    \
        _Pragma("unroll") for (int i = 0; i < MTW1; i++) {                                                           \
          const unsigned char* q_ = sb_ + ((i1b + i) * 32 + l32) * K::P1T;                                           \
          xh_[i] = *reinterpret_cast<const v8h*>(q_ + ch_); xl_[i] = *reinterpret_cast<const v8h*>(q_ + cl_); }      \
        _Pragma("unroll") for (int j = 0; j < 2; j++) {                                                              \
          const unsigned char* q_ = sb_ + (K::XROWS + (j1b + 2 * j) * 32 + l32) * K::P1T;                            \
          wh_[j] = *reinterpret_cast<const v8h*>(q_ + ch_); wl_[j] = *reinterpret_cast<const v8h*>(q_ + cl_); }      \
        _Pragma("unroll") for (int i = 0; i < MTW1; i++) _Pragma("unroll") for (int j = 0; j < 2; j++)               \
          acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xl_[i], acc1[i][j], 0, 0, 0);                  \
        _Pragma("unroll") for (int i = 0; i < MTW1; i++) _Pragma("unroll") for (int j = 0; j < 2; j++)               \
          acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[j], xh_[i], acc1[i][j], 0, 0, 0);                  \
        _Pragma("unroll") for (int i = 0; i < MTW1; i++) _Pragma("unroll") for (int j = 0; j < 2; j++)               \
          acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xh_[i], acc1[i][j], 0, 0, 0);                  \
      }                                                                                                              \
    }
    // k-tile KT_ sits in LDS buffer S_ and its register set S_ is free: fetch tile KT_ + 2 into it, multiply, pass tile KT_ + 1 on
#define SSG_BH_STEP1(KT_, S_)                                                                                        \
    {                                                                                                                \
      if ((KT_) + K::PD1 < K::NK1) SSG_BH_LOAD1((KT_) + K::PD1, S_)                                                   \
      SSG_BH_MMA1(S_)                                                                                                \
      if ((KT_) + 1 < K::NK1) SSG_BH_STORE1(1 - (S_), 1 - (S_))                                                       \
      __syncthreads();                                                                                               \
    }
    SSG_BH_LOAD1(0, 0) SSG_BH_LOAD1(1, 1)
    SSG_BH_STORE1(0, 0)
    __syncthreads();
#pragma unroll 1
    for (int kt0 = 0; kt0 < K::NK1; kt0 += 2) { SSG_BH_STEP1(kt0, 0) SSG_BH_STEP1(kt0 + 1, 1) }
#undef SSG_BH_STEP1
#undef SSG_BH_MMA1
#undef SSG_BH_STORE1
#undef SSG_BH_LOAD1
  }
  SSG_BN_STAMP(1)

  // phase 2 / 3 staging: thread = 16-byte piece ck8 of the 128-byte stage rows r8 + 32 u; wave = its own 32 pixels x all channels
  constexpr int RP8 = K::NTHR / 8, BU = MID / RP8;
  const int ck8 = tid & 7, r8 = tid >> 3;
  const float* w2p = p.w2 + (int64_t)r8 * (9 * MID) + ck8 * 4;
  const int m2 = wave * 32 + l32, ty2 = m2 / IW, tx2 = m2 - ty2 * IW;    // this lane's output pixel (tile-local)
  constexpr int NT2 = MID / 32;
  v16f acc2[NT2];
#pragma unroll
  for (int j = 0; j < NT2; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc2[j][r] = 0.f;
  unsigned ovf = 0u;
  v4f sb2[K::PD2][BU];
#define SSG_BH_LOAD2(T_, S_)                                                                                         \
  { _Pragma("unroll") for (int u = 0; u < BU; u++) sb2[S_][u] = *reinterpret_cast<const v4f*>(w2p + (int64_t)(RP8 * u) * (9 * MID) + (T_) * 32); }
#define SSG_BH_STORE2(BUF_, S_)                                                                                      \
  { unsigned char* sb_ = smem + K::W2_OFF + (BUF_) * K::BUF2;                                                        \
    _Pragma("unroll") for (int u = 0; u < BU; u++) *reinterpret_cast<v4f*>(sb_ + (r8 + RP8 * u) * K::P2 + ck8 * 16) = sb2[S_][u]; }
#define SSG_BH_STEP2(HF_, KT_, S_, B_)                                                                                \
  {                                                                                                                  \
    if ((KT_) + K::PD2 < K::NK2H) SSG_BH_LOAD2((HF_) * K::NK2H + (KT_) + K::PD2, S_)                                  \
    {                                                                                                                \
      const int cl = (KT_) / 9, tap = (KT_) - cl * 9, r = tap / 3, s = tap - r * 3;   /* cl: the chunk within the half */ \
      const int xin = tx2 + s - 1;                                                                                   \
      const int abase = (xin >= 0 && xin < IW) ? ((ty2 + r) * IW + xin) * K::PYH : K::ZERO_OFF;                      \
      const unsigned char* wb = smem + K::W2_OFF + (B_) * K::BUF2 + l32 * K::P2 + h * 32;                             \
      _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                             \
        const unsigned char* q_ = smem + abase + (cl * 4 + ks * 2 + h) * 32;                                         \
        const v8h xh_ = *reinterpret_cast<const v8h*>(q_), xl_ = *reinterpret_cast<const v8h*>(q_ + 16);             \
        v8h wh_[NT2], wl_[NT2];                                                                                      \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) {                                                            \
          wh_[j] = *reinterpret_cast<const v8h*>(wb + j * 32 * K::P2 + ks * 64);                                     \
          wl_[j] = *reinterpret_cast<const v8h*>(wb + j * 32 * K::P2 + ks * 64 + 16); }                              \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xl_, acc2[j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[j], xh_, acc2[j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < NT2; j++) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xh_, acc2[j], 0, 0, 0); \
      }                                                                                                              \
    }                                                                                                                \
    if ((KT_) + 1 < K::NK2H) SSG_BH_STORE2((B_) ^ 1, ((S_) + 1) % K::PD2)                                             \
    __syncthreads();                                                                                                 \
  }
  // One y1 half: its conv2 weights' first k-tiles on their way, the half's accumulators -> LDS (h8l8 pixel rows; rows outside the image
  // are conv2's zero padding, not relu(bias)), then chunks 2 HF_, 2 HF_ + 1 of conv2 with the pixel operand from LDS.  The accumulators
  // of half 1 stay parked in registers while half 0 multiplies; the barrier that ends half 0's last step frees the rows for them.
  // Six steps per trip: the register set of step i is i % 3, its LDS buffer i & 1.
#define SSG_BH_HALF(HF_)                                                                                             \
  {                                                                                                                  \
    SSG_BH_LOAD2((HF_) * K::NK2H, 0) SSG_BH_LOAD2((HF_) * K::NK2H + 1, 1) SSG_BH_LOAD2((HF_) * K::NK2H + 2, 2)        \
    float4 cs1r[4], b1r[4];                                                                                          \
    _Pragma("unroll") for (int q = 0; q < 4; q++) {                                                                  \
      cs1r[q] = *reinterpret_cast<const float4*>(p.cs1 + (HF_) * K::MH + j1b * 32 + 8 * q + 4 * h);                  \
      b1r[q] = *reinterpret_cast<const float4*>(p.b1 + (HF_) * K::MH + j1b * 32 + 8 * q + 4 * h); }                  \
    _Pragma("unroll") for (int i = 0; i < MTW1; i++) {                                                               \
      if (i1b + i >= MT1) continue;                           /* (the padding tile of the second wave row) */       \
      const int hp0 = (i1b + i) * 32;                         /* first halo pixel of this MFMA tile */               \
      const int irow = ty0 - 1 + (hp0 + l32) / IW;                                                                   \
      const bool inside = irow >= 0 && irow < p.H;                                                                   \
      _Pragma("unroll") for (int q = 0; q < 4; q++) {                                                                \
        const int ch = j1b * 32 + 8 * q + 4 * h;              /* channel within the half */                          \
        const float4 cs = cs1r[q], bi = b1r[q];                                                                      \
        float4 v = make_float4(acc1[i][HF_][4 * q] * cs.x + bi.x, acc1[i][HF_][4 * q + 1] * cs.y + bi.y, acc1[i][HF_][4 * q + 2] * cs.z + bi.z, \
                               acc1[i][HF_][4 * q + 3] * cs.w + bi.w);                                               \
        v = relu4(v);                                                                                                \
        if (!inside) v = make_float4(0.f, 0.f, 0.f, 0.f);                                                            \
        uint2 hi, lo;                                                                                                \
        split_encode4(v, hi, lo);                                                                                    \
        ovf |= split_hi_nonfinite_bits(hi);                                                                          \
        unsigned char* d = smem + (hp0 + l32) * K::PYH + (ch >> 3) * 32 + h * 8;                                     \
        *reinterpret_cast<uint2*>(d) = hi; *reinterpret_cast<uint2*>(d + 16) = lo;                                   \
      }                                                                                                              \
    }                                                                                                                \
    if ((HF_) == 0 && tid < K::PYH / 16) *reinterpret_cast<uint4*>(smem + K::ZERO_OFF + tid * 16) = make_uint4(0u, 0u, 0u, 0u);   /* (the phase-1 stages covered this row) */ \
    SSG_BH_STORE2(0, 0)                                                                                              \
    __syncthreads();                                                                                                 \
    _Pragma("unroll 1") for (int kt0 = 0; kt0 < K::NK2H; kt0 += 6) {                                                 \
      SSG_BH_STEP2(HF_, kt0, 0, 0) SSG_BH_STEP2(HF_, kt0 + 1, 1, 1) SSG_BH_STEP2(HF_, kt0 + 2, 2, 0)                  \
      SSG_BH_STEP2(HF_, kt0 + 3, 0, 1) SSG_BH_STEP2(HF_, kt0 + 4, 1, 0) SSG_BH_STEP2(HF_, kt0 + 5, 2, 1)              \
    }                                                                                                                \
    SSG_BN_STAMP(2 + (HF_))                                                                                          \
  }
  SSG_BH_HALF(0)
  SSG_BH_HALF(1)      // (its last barrier: every wave is past its last y1 / W2 read)
#undef SSG_BH_HALF
#undef SSG_BH_STEP2
#undef SSG_BH_STORE2
#undef SSG_BH_LOAD2

  // ---- conv3 weights: stage s = (pass s / 4, 32-channel k-tile s % 4): rows of the pass's 128 output channels, 128 bytes each
  constexpr int NS3 = K::NPASS * K::KT3;
  const float* w3p = p.w3 + (int64_t)r8 * MID + ck8 * 4;
  v4f sc3[2][BU];
#define SSG_BH_LOAD3(T_, S_)                                                                                         \
  { _Pragma("unroll") for (int u = 0; u < BU; u++)                                                                    \
      sc3[S_][u] = *reinterpret_cast<const v4f*>(w3p + (int64_t)(((T_) / K::KT3) * K::NCP + RP8 * u) * MID + ((T_) % K::KT3) * 32); }
#define SSG_BH_STORE3(BUF_, S_)                                                                                      \
  { unsigned char* sb_ = smem + K::W2_OFF + (BUF_) * K::BUF2;                                                        \
    _Pragma("unroll") for (int u = 0; u < BU; u++) *reinterpret_cast<v4f*>(sb_ + (r8 + RP8 * u) * K::P2 + ck8 * 16) = sc3[S_][u]; }
  SSG_BH_LOAD3(0, 0)
  SSG_BH_LOAD3(1, 1)

  // ---- y2 -> MFMA fragments of conv3's pixel operand: each 32 x 32 accumulator tile through this wave's patch (in the dead y1 rows)
  unsigned char* const patchb = smem + wave * K::PATCH;
  v8h y2h[MID / 16], y2l[MID / 16];
#pragma unroll
  for (int j = 0; j < NT2; j++) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 cs = *reinterpret_cast<const float4*>(p.cs2 + j * 32 + 8 * q + 4 * h), bi = *reinterpret_cast<const float4*>(p.b2 + j * 32 + 8 * q + 4 * h);
      float4 v = make_float4(acc2[j][4 * q] * cs.x + bi.x, acc2[j][4 * q + 1] * cs.y + bi.y, acc2[j][4 * q + 2] * cs.z + bi.z, acc2[j][4 * q + 3] * cs.w + bi.w);
      v = relu4(v);
      uint2 hi, lo;
      split_encode4(v, hi, lo);
      ovf |= split_hi_nonfinite_bits(hi);
      unsigned char* d = patchb + l32 * K::P2 + q * 32 + h * 8;
      *reinterpret_cast<uint2*>(d) = hi; *reinterpret_cast<uint2*>(d + 16) = lo;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      const unsigned char* q_ = patchb + l32 * K::P2 + (ks * 2 + h) * 32;
      y2h[j * 2 + ks] = *reinterpret_cast<const v8h*>(q_); y2l[j * 2 + ks] = *reinterpret_cast<const v8h*>(q_ + 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  SSG_BH_STORE3(0, 0)
  __syncthreads();
  SSG_BN_STAMP(4)

  // =========================== phase 3 + epilogue: out = relu(conv3(y2) + x), 128 output channels per pass ===========================
  constexpr int EP = K::EP, CPR = 8, RPI = 8, ITS = 4, NT3 = K::NCP / 32;
  const int chunk = lane % CPR, prow = lane / CPR, odd = lane & 1;
  const int64_t gpix0 = ((int64_t)img * p.H + ty0) * IW + wave * 32;       // first output pixel of this wave (pixels are contiguous)
  const float* __restrict__ resp = p.x + gpix0 * C;
  float* __restrict__ outp = p.out + gpix0 * C;
  float* const patch = reinterpret_cast<float*>(patchb);
#pragma unroll 1
  for (int ps = 0; ps < K::NPASS; ps++) {
    const int cb3 = ps * NT3;
    v16f acc3[NT3];
#pragma unroll
    for (int j = 0; j < NT3; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc3[j][r] = 0.f;
    float4 rr[2][ITS], b3r[2], cs3r[2];
    // stage I_ of the pass sits in LDS buffer I_ & 1 and its register set is free: fetch two stages ahead, multiply, pass the next one on
#define SSG_BH_STEP3(I_)                                                                                             \
    {                                                                                                                \
      const int s_ = ps * K::KT3 + (I_);                                                                             \
      if (s_ + 2 < NS3) SSG_BH_LOAD3(s_ + 2, (I_) & 1)                                                                \
      if constexpr ((I_) == K::KT3 - 1) {    /* the epilogue's first operands (two tiles ahead measures the same: the epilogue is VALU work) */ \
        _Pragma("unroll") for (int it = 0; it < ITS; it++) rr[0][it] = load_res_nt<C>(resp, it * RPI + prow, cb3 * 32 + chunk * 4); \
        b3r[0] = *reinterpret_cast<const float4*>(p.b3 + cb3 * 32 + chunk * 4); cs3r[0] = *reinterpret_cast<const float4*>(p.cs3 + cb3 * 32 + chunk * 4); \
      }                                                                                                              \
      const unsigned char* wb_ = smem + K::W2_OFF + ((I_) & 1) * K::BUF2 + l32 * K::P2 + h * 32;                      \
      _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                             \
        const v8h xh_ = y2h[(I_) * 2 + ks], xl_ = y2l[(I_) * 2 + ks];                                                \
        v8h wh_[NT3], wl_[NT3];                                                                                      \
        _Pragma("unroll") for (int j = 0; j < NT3; j++) {                                                            \
          wh_[j] = *reinterpret_cast<const v8h*>(wb_ + j * 32 * K::P2 + ks * 64);                                    \
          wl_[j] = *reinterpret_cast<const v8h*>(wb_ + j * 32 * K::P2 + ks * 64 + 16); }                             \
        _Pragma("unroll") for (int j = 0; j < NT3; j++) acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xl_, acc3[j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < NT3; j++) acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl_[j], xh_, acc3[j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < NT3; j++) acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[j], xh_, acc3[j], 0, 0, 0); \
      }                                                                                                              \
      if (s_ + 1 < NS3) SSG_BH_STORE3(((I_) + 1) & 1, ((I_) + 1) & 1)                                                 \
      __syncthreads();                                                                                               \
    }
    SSG_BH_STEP3(0) SSG_BH_STEP3(1) SSG_BH_STEP3(2) SSG_BH_STEP3(3)
#undef SSG_BH_STEP3

    // ---- epilogue of the pass: per channel tile a 32-pixel x 32-channel patch through LDS, then whole 128-byte row segments:
    // bias, residual (x, h8l8), ReLU, re-encode, store.  The code path of bottleneck_kernel and conv.hip.
#pragma unroll
    for (int j = 0; j < NT3; j++) {
      const int col = (cb3 + j) * 32 + chunk * 4;
      if (j + 1 < NT3) {
#pragma unroll
        for (int it = 0; it < ITS; it++) rr[(j + 1) & 1][it] = load_res_nt<C>(resp, it * RPI + prow, col + 32);
        b3r[(j + 1) & 1] = *reinterpret_cast<const float4*>(p.b3 + col + 32); cs3r[(j + 1) & 1] = *reinterpret_cast<const float4*>(p.cs3 + col + 32);
      }
      const float4 bias = b3r[j & 1], cs = cs3r[j & 1];
#pragma unroll
      for (int q = 0; q < 4; q++)
        *reinterpret_cast<float4*>(patch + l32 * EP + 8 * q + 4 * h) = make_float4(acc3[j][4 * q], acc3[j][4 * q + 1], acc3[j][4 * q + 2], acc3[j][4 * q + 3]);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int it = 0; it < ITS; it++) {
        const int pr = it * RPI + prow;
        float4 v = *reinterpret_cast<const float4*>(patch + pr * EP + chunk * 4);
        v.x = v.x * cs.x + bias.x; v.y = v.y * cs.y + bias.y; v.z = v.z * cs.z + bias.z; v.w = v.w * cs.w + bias.w;
        const float4 rw = rr[j & 1][it];
        float4 r4;
        {   // even lane holds hi0..7 of the 8-channel group, odd lane lo0..7; each needs hi and lo of ITS four channels
          const unsigned a0 = __float_as_uint(rw.x), a1 = __float_as_uint(rw.y), a2 = __float_as_uint(rw.z), a3 = __float_as_uint(rw.w);
          const unsigned h0 = lane_pair_merge(a0, a2, odd), h1 = lane_pair_merge(a1, a3, odd);
          const unsigned l0 = lane_pair_merge(a2, a0, !odd), l1 = lane_pair_merge(a3, a1, !odd);
          r4 = split_decode4(make_uint2(h0, h1), make_uint2(l0, l1));
        }
        v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
        v = relu4(v);
        uint2 hp, lp;
        split_encode4(v, hp, lp);
        ovf |= split_hi_nonfinite_bits(hp);
        const uint4 stv = split_pair_pack(hp, lp, odd);
        store_out_nt(outp + (int64_t)pr * C + col, stv);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
#undef SSG_BH_STORE3
#undef SSG_BH_LOAD3
  if ((ovf & 0x80008000u) && p.overflow) *p.overflow = 1;
  SSG_BN_STAMP(5)
}

}  // namespace bneck
}  // namespace ssg

// 1 when ssg_bottleneck_nhwc_x / ssg_bottleneck_ds_nhwc_x has a kernel for this block shape (CIN == C: identity block):
//   layer1 of ResNet-50 at 256x128 input: H x 32 x 256, MID 64 (identity blocks and the first block, CIN = 64), 4-row tiles;
//   layer2 identity blocks: H x 16 x 512, MID 128, 8-row tiles (bottleneck_halves_kernel)
extern "C" int ssg_bottleneck_supported(int H, int W, int CIN, int C, int MID) {
  if (C == 256 && MID == 64 && (CIN == 256 || CIN == 64) && W == 32 && H > 0 && H % 4 == 0) return 1;
  if (C == 512 && MID == 128 && CIN == 512 && W == 16 && H > 0 && H % 8 == 0) return 1;
  return 0;
}

template <int C, int MID, int IW, int TH, int CIN, bool NXT = false>
static int launch_bottleneck(const ssg::bneck::Params& p, hipStream_t stream) {
  using namespace ssg::bneck;
  using K = Cfg<C, MID, IW, TH, CIN>;
  static bool attr_set = false;
  if (!attr_set) {
    SSG_HIP(hipFuncSetAttribute((const void*)bottleneck_kernel<C, MID, IW, TH, CIN, NXT>, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS));
    attr_set = true;
  }
  hipLaunchKernelGGL((bottleneck_kernel<C, MID, IW, TH, CIN, NXT>), dim3(p.B * (p.H / TH)), dim3(K::NTHR), K::LDS, stream, p);
  SSG_LAUNCH_CHECK("bottleneck_kernel");
  return SSG_OK;
}

template <int C, int MID, int IW, int TH>
static int launch_bottleneck_halves(const ssg::bneck::Params& p, hipStream_t stream) {
  using namespace ssg::bneck;
  using K = CfgH<C, MID, IW, TH>;
  static bool attr_set = false;
  if (!attr_set) {
    SSG_HIP(hipFuncSetAttribute((const void*)bottleneck_halves_kernel<C, MID, IW, TH>, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS));
    attr_set = true;
  }
  hipLaunchKernelGGL((bottleneck_halves_kernel<C, MID, IW, TH>), dim3(p.B * (p.H / TH)), dim3(K::NTHR), K::LDS, stream, p);
  SSG_LAUNCH_CHECK("bottleneck_halves_kernel");
  return SSG_OK;
}

// Next-conv instance of the layer1 identity block: conv1 of the FOLLOWING block rides in this block's epilogue.
// whether the embedder routes through it when SSG_BN_L1_NEXT is not set
#ifndef SSG_BN_L1_NEXT_DEFAULT
#define SSG_BN_L1_NEXT_DEFAULT 1
#endif

namespace {
struct NextDesc { const float* w1n; const float* b1n; const float* cs1n; float* y1n; float* out_s2; int midn; bool set; };
thread_local NextDesc g_next = {};   // attached by ssg_bottleneck_attach_next, consumed by this thread's next ssg_bottleneck_nhwc_x
}

// 1 when the last layer1 block (H x 32 x 256, MID 64, H % 4 == 0) can also compute a 256 -> MIDN = 128 1x1 convolution of its output
extern "C" int ssg_bottleneck_next_supported(int H, int W, int C, int MID, int MIDN) {
  return (H > 0 && H % 4 == 0 && W == 32 && C == 256 && MID == 64 && MIDN == 128) ? 1 : 0;
}

// SSG_BN_L1_NEXT (0 | 1, read per call; unset or empty: SSG_BN_L1_NEXT_DEFAULT): 1 when the embedder should take the fused route
extern "C" int ssg_bottleneck_next_enabled(void) {
  const char* e = getenv("SSG_BN_L1_NEXT");
  if (!e || !*e) return SSG_BN_L1_NEXT_DEFAULT;
  if ((e[0] == '0' || e[0] == '1') && !e[1]) return e[0] - '0';
  ssg_set_error("SSG_BN_L1_NEXT=%s (0 or 1)", e);
  return SSG_ERR_INVALID;
}

// Attach conv1 of the following block to this thread's next ssg_bottleneck_nhwc_x call, which then also writes
//   y1n [B,H,W,MIDN] = relu(conv1_next(out)) (w1n [MIDN][C] h8l8 row-major, rows pre-scaled by 1/cs1n; bit-identical to ssg_conv2d_nhwc_x(out, ...))
//   out_s2 [B,H/2,W/2,C] = out[:, ::2, ::2]
// either may be null, and so may that call's `out`.  That call consumes the descriptor whether it succeeds or not; a shape without
// ssg_bottleneck_next_supported is then an error, never a plain launch.
extern "C" int ssg_bottleneck_attach_next(const void* w1n, const float* b1n, const float* cs1n, void* y1n, void* out_s2, int MIDN) {
  g_next = NextDesc{};
  if (!w1n || !b1n || !cs1n || MIDN != 128 || (y1n && y1n == out_s2)) {
    ssg_set_error("ssg_bottleneck_attach_next: needs w1n, b1n, cs1n, MIDN = 128 and distinct outputs (MIDN=%d)", MIDN);
    return SSG_ERR_INVALID;
  }
  g_next = NextDesc{(const float*)w1n, b1n, cs1n, (float*)y1n, (float*)out_s2, MIDN, true};
  return SSG_OK;
}

// Identity bottleneck block (no downsample branch, stride 1), split-half tensors:
//   out = relu(conv3(relu(conv2(relu(conv1(x))))) + x),  x / out [B,H,W,C] h8l8, weights as ssg_conv2d_nhwc_x takes them
//   (w1 [MID][C], w2 [MID][9*MID] in the k = (32-channel chunk, tap, channel) order, w3 [C][MID], each row pre-multiplied by a
//   power of two that ch_scale* undoes), biases fp32.  out must not alias x (halo rows are read by other workgroups).
extern "C" int ssg_bottleneck_nhwc_x(const void* x, const void* w1, const float* b1, const float* cs1, const void* w2, const float* b2, const float* cs2,
                                     const void* w3, const float* b3, const float* cs3, void* out, int B, int H, int W, int C, int MID,
                                     int32_t* overflow, hipStream_t stream) {
  using namespace ssg::bneck;
  const NextDesc nd = g_next;
  g_next = NextDesc{};
  if (B <= 0 || !ssg_bottleneck_supported(H, W, C, C, MID) || !cs1 || !cs2 || !cs3 || x == out) {
    ssg_set_error("ssg_bottleneck_nhwc_x: unsupported block B=%d H=%d W=%d C=%d MID=%d (see ssg_bottleneck_supported)", B, H, W, C, MID);
    return SSG_ERR_INVALID;
  }
  if (nd.set && (!ssg_bottleneck_next_supported(H, W, C, MID, nd.midn) || x == nd.y1n || x == nd.out_s2 || (out && (out == nd.y1n || out == nd.out_s2)))) {
    ssg_set_error("ssg_bottleneck_nhwc_x: no next-conv instance for B=%d H=%d W=%d C=%d MID=%d MIDN=%d with distinct tensors (see ssg_bottleneck_next_supported)",
                  B, H, W, C, MID, nd.midn);
    return SSG_ERR_INVALID;
  }
  Params p;
  p.x = (const float*)x; p.out = (float*)out;
  p.w1 = (const float*)w1; p.b1 = b1; p.cs1 = cs1; p.w2 = (const float*)w2; p.b2 = b2; p.cs2 = cs2; p.w3 = (const float*)w3; p.b3 = b3; p.cs3 = cs3;
  p.B = B; p.H = H; p.overflow = overflow;
  if (nd.set) {
    p.w1n = nd.w1n; p.b1n = nd.b1n; p.cs1n = nd.cs1n; p.y1n = nd.y1n; p.out_s2 = nd.out_s2;
    return launch_bottleneck<256, 64, 32, 4, 256, true>(p, stream);
  }
  if (C == 512) return launch_bottleneck_halves<512, 128, 16, 8>(p, stream);   // layer2
  return launch_bottleneck<256, 64, 32, 4, 256>(p, stream);
}

// Bottleneck block with a stride-1 downsample branch (the first block of layer1):
//   out = relu(conv3(relu(conv2(relu(conv1(x))))) + downsample(x)),  x [B,H,W,CIN], out [B,H,W,C] h8l8;
//   w3cat [C][MID + CIN] = conv3 | downsample weights concatenated along K (the layout of ssg_conv1x1_dual_nhwc_x), b3 = b3 + b_ds.
extern "C" int ssg_bottleneck_ds_nhwc_x(const void* x, const void* w1, const float* b1, const float* cs1, const void* w2, const float* b2, const float* cs2,
                                        const void* w3cat, const float* b3, const float* cs3, void* out, int B, int H, int W, int CIN, int C, int MID,
                                        int32_t* overflow, hipStream_t stream) {
  using namespace ssg::bneck;
  if (B <= 0 || CIN == C || !ssg_bottleneck_supported(H, W, CIN, C, MID) || !cs1 || !cs2 || !cs3) {
    ssg_set_error("ssg_bottleneck_ds_nhwc_x: unsupported block B=%d H=%d W=%d CIN=%d C=%d MID=%d (see ssg_bottleneck_supported)", B, H, W, CIN, C, MID);
    return SSG_ERR_INVALID;
  }
  Params p;
  p.x = (const float*)x; p.out = (float*)out;
  p.w1 = (const float*)w1; p.b1 = b1; p.cs1 = cs1; p.w2 = (const float*)w2; p.b2 = b2; p.cs2 = cs2; p.w3 = (const float*)w3cat; p.b3 = b3; p.cs3 = cs3;
  p.B = B; p.H = H; p.overflow = overflow;
  return launch_bottleneck<256, 64, 32, 4, 64>(p, stream);
}
