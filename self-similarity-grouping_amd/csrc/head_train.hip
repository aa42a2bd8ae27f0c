// head_train.hip -- train-mode head of the fine-tune phase: stripe-pool backward and Linear forward / data gradient / weight and
// bias gradient (gfx950 only).
//
// The reference's head (reid/models/resnet.py:93-120) average-pools the layer4 map S + 2 times and sends the global average through
// feat = Linear(out_planes, num_features, bias=False) and, under SSG++, classifier_x2 = Linear(num_features, num_classes).
//   pool forward   ssg_gap_stripes (csrc/conv.hip): one launch, every set a serial float32 sum of its window and one division
//   pool backward  ssg_gap_stripes_bwd, this file: dX[b,y,x,c] = g0 / (h w) + g_stripe(y) / ((h / S) w), every element written once
//   Linear         three fp32-MFMA GEMMs that read nn.Linear's [N, K] weight where it lies -- no pack launch, no transposed copy:
//     y  [B,N] = x W^T (+ bias)    reduction over K, both operands K-contiguous
//     dX [B,K] = dY W              reduction over N, dY N-contiguous, W read along its rows
//     dW [N,K] = dY^T x            reduction over B, both operands read along their rows;  db [N] = sum_b dY[b][n] in float64
//
// One kernel template serves the three GEMMs.  A workgroup of 4 waves owns one 32 x 32 output tile.  Per stage it brings LIN_RED = 128
// reduction steps of both operands into LDS as [reduction step][32 outputs] at a pitch of 33 dwords, whichever way the operand lies in
// memory (a reduction-contiguous operand is transposed by the LDS write; the odd pitch keeps both that write and the MFMA reads off
// bank conflicts), masked with zeros past the ragged edge of the tile and of the reduction.  Wave w multiplies steps w*32 .. w*32+31
// of every stage on v_mfma_f32_32x32x2_f32; the next stage's global loads fly under the MFMAs.  At the end the four waves' fp32 tiles
// are added per element in float64 in wave order (+ bias), rounded once and stored with a mask.  The cut into four is fixed, so the
// summation order is a function of the shape alone; there are no float atomics and no workspace.
#include "train_common.h"

namespace ssg {

constexpr int LIN_T = 32;            // output tile side
constexpr int LIN_RED = 128;         // reduction steps per LDS stage: 32 per wave
constexpr int LIN_PITCH = 33;        // dwords per reduction step in LDS
constexpr int LIN_LD = LIN_T * LIN_RED / 256;   // elements per thread, operand and stage


// element (out index o, reduction index r) of an operand lies at p[o * so + r * sr]; RC (reduction-contiguous) operands have sr == 1,
// the others so == 1.  The thread -> element map of the global load follows the contiguous index so that a wave reads whole lines.
template <bool RC>
__device__ __forceinline__ void lin_load(const float* __restrict__ p, int64_t so, int64_t sr, int o0, int OUT, int r0, int RED, int tid, float (&v)[LIN_LD]) {
  // element u of this thread: RC (o_t + 2u, r_t), else (o_t, r_t + 8u) -- see lin_stage
  const int o_t = RC ? tid / LIN_RED : tid % LIN_T, r_t = RC ? tid % LIN_RED : tid / LIN_T;
  const int olim = OUT - o0 - o_t, rlim = RED - r0 - r_t;
  const float* q = p + (int64_t)(o0 + o_t) * so + (int64_t)(r0 + r_t) * sr;
  const int64_t step = RC ? (256 / LIN_RED) * so : (256 / LIN_T) * sr;
#pragma unroll
  for (int u = 0; u < LIN_LD; u++) {
    const bool ok = RC ? ((256 / LIN_RED) * u < olim && rlim > 0) : (olim > 0 && (256 / LIN_T) * u < rlim);
    const float t = *(ok ? q + u * step : p);          // an element past the edge reads p[0] instead, and counts as zero
    v[u] = ok ? t : 0.f;
  }
}

template <bool RC>
__device__ __forceinline__ void lin_stage(float* s, int tid, const float (&v)[LIN_LD]) {
#pragma unroll
  for (int u = 0; u < LIN_LD; u++) {
    const int e = tid + 256 * u;
    const int o = RC ? e / LIN_RED : e % LIN_T, r = RC ? e % LIN_RED : e / LIN_T;
    s[r * LIN_PITCH + o] = v[u];
  }
}

// c[i][j] = sum_r a(i, r) * b(j, r) (+ bias[j]); i < ROWS, j < COLS, r < RED; c at row pitch COLS.  grid (ceil(COLS/32), ceil(ROWS/32)).
template <bool A_RC, bool B_RC>
__global__ __launch_bounds__(256) void linear_gemm_kernel(const float* __restrict__ a, int64_t a_so, int64_t a_sr, const float* __restrict__ b, int64_t b_so,
                                                          int64_t b_sr, const float* __restrict__ bias, float* __restrict__ c, int ROWS, int COLS, int RED) {
  __shared__ float as[LIN_RED * LIN_PITCH];
  __shared__ float bs[LIN_RED * LIN_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lk = lane >> 5;
  const int i0 = blockIdx.y * LIN_T, j0 = blockIdx.x * LIN_T;
  float av[LIN_LD], bv[LIN_LD];
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; e++) acc[e] = 0.f;

  lin_load<A_RC>(a, a_so, a_sr, i0, ROWS, 0, RED, tid, av);
  lin_load<B_RC>(b, b_so, b_sr, j0, COLS, 0, RED, tid, bv);
  for (int r0 = 0; r0 < RED; r0 += LIN_RED) {
    lin_stage<A_RC>(as, tid, av);
    lin_stage<B_RC>(bs, tid, bv);
    __syncthreads();
    if (r0 + LIN_RED < RED) {
      lin_load<A_RC>(a, a_so, a_sr, i0, ROWS, r0 + LIN_RED, RED, tid, av);
      lin_load<B_RC>(b, b_so, b_sr, j0, COLS, r0 + LIN_RED, RED, tid, bv);
    }
    if (r0 + wave * 32 < RED) {                        // a wave whose 32 steps lie past the end would add zeros only
#pragma unroll
      for (int kk = 0; kk < 16; kk++) {
        const int r = wave * 32 + 2 * kk + lk;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[r * LIN_PITCH + l31], bs[r * LIN_PITCH + l31], acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // the four waves' tiles -> LDS [wave][row][col] (the operand stages are dead after the last barrier), then one float64 sum per element
  float* part = as;                                     // 4 * 1024 floats <= LIN_RED * LIN_PITCH
  static_assert(4 * LIN_T * LIN_T <= LIN_RED * LIN_PITCH, "the partial tiles must fit the A stage");
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int row = (e & 3) + 8 * (e >> 2) + 4 * lk;    // C/D map of the 32x32 MFMA: column = lane & 31
    part[wave * 1024 + row * LIN_T + l31] = acc[e];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int e = tid + 256 * u, row = e >> 5, col = e & 31;
    if (i0 + row < ROWS && j0 + col < COLS) {
      double s = (double)part[e];
      s += (double)part[1024 + e];
      s += (double)part[2048 + e];
      s += (double)part[3072 + e];
      if (bias) s += (double)bias[j0 + col];
      c[(int64_t)(i0 + row) * COLS + j0 + col] = (float)s;
    }
  }
}

// db[n] = float(sum over b ascending of dY[b][n], in float64)
__global__ __launch_bounds__(256) void linear_bias_grad_kernel(const float* __restrict__ dy, float* __restrict__ db, int B, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double s = 0.0;
  for (int b = 0; b < B; b++) s += (double)dy[(int64_t)b * N + n];
  db[n] = (float)s;
}

// dX [B,H,W,C] from g [nsets,B,C]; one thread per float4 of dX.  hs = H / S rows per stripe; rows from S*hs on are in no stripe.
__global__ __launch_bounds__(256) void gap_stripes_bwd_kernel(const float* __restrict__ g, unsigned mask, float* __restrict__ dx, int B, int H, int W, int C,
                                                              int S) {
  const int C4 = C >> 2, hs = S > 1 ? H / S : H;
  const int64_t total = (int64_t)B * H * W * C4, set_stride = (int64_t)B * C;
  const float n0 = (float)(H * W), n1 = (float)(hs * W);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C4) << 2;
    const int64_t pix = idx / C4;
    const int y = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    const int s = (S > 1 && y < S * hs) ? y / hs + 1 : 0;          // 0: no stripe term
    float4 t0 = make_float4(0.f, 0.f, 0.f, 0.f), t1 = t0;
    if (mask & 1u) {
      const float4 v = *reinterpret_cast<const float4*>(g + (int64_t)b * C + c);
      t0 = make_float4(v.x / n0, v.y / n0, v.z / n0, v.w / n0);
    }
    if (s > 0 && ((mask >> s) & 1u)) {
      const float4 v = *reinterpret_cast<const float4*>(g + s * set_stride + (int64_t)b * C + c);
      t1 = make_float4(v.x / n1, v.y / n1, v.z / n1, v.w / n1);
    }
    *reinterpret_cast<float4*>(dx + pix * C + c) = make_float4(t0.x + t1.x, t0.y + t1.y, t0.z + t1.z, t0.w + t1.w);
  }
}

}  // namespace ssg

namespace {

using namespace ssg;

int linear_check(const char* fn, int B, int K, int N) {
  if (B <= 0 || K <= 0 || N <= 0 || (K % 32) || B > 65535 * 32 || N > 65535 * 32) {
    ssg_set_error("%s: the train-mode Linear takes x [B, K] and weight [N, K] with B >= 1, N >= 1, K %% 32 == 0, B and N at most 65535 * 32 "
                  "(B=%d K=%d N=%d)", fn, B, K, N);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

int lin_tiles(int n) { return (n + LIN_T - 1) / LIN_T; }

}  // namespace

extern "C" int ssg_linear_fwd_f32(const float* x, const float* w, const float* bias, float* y, int B, int K, int N, hipStream_t stream) {
  const char* fn = "ssg_linear_fwd_f32";
  if (int rc = linear_check(fn, B, K, N)) return rc;
  if (int rc = ssg_need_pointers(fn, x && w && y)) return rc;
  hipLaunchKernelGGL((linear_gemm_kernel<true, true>), dim3(lin_tiles(N), lin_tiles(B)), dim3(256), 0, stream, x, (int64_t)K, (int64_t)1, w, (int64_t)K, (int64_t)1,
                     bias, y, B, N, K);
  SSG_LAUNCH_CHECK("linear_gemm_kernel (forward)");
  return SSG_OK;
}

extern "C" int ssg_linear_dgrad_f32(const float* dy, const float* w, float* dx, int B, int K, int N, hipStream_t stream) {
  const char* fn = "ssg_linear_dgrad_f32";
  if (int rc = linear_check(fn, B, K, N)) return rc;
  if (int rc = ssg_need_pointers(fn, dy && w && dx)) return rc;
  hipLaunchKernelGGL((linear_gemm_kernel<true, false>), dim3(lin_tiles(K), lin_tiles(B)), dim3(256), 0, stream, dy, (int64_t)N, (int64_t)1, w, (int64_t)1, (int64_t)K,
                     (const float*)nullptr, dx, B, K, N);
  SSG_LAUNCH_CHECK("linear_gemm_kernel (data gradient)");
  return SSG_OK;
}

extern "C" int ssg_linear_wgrad_f32(const float* dy, const float* x, float* dw, float* db, int B, int K, int N, hipStream_t stream) {
  const char* fn = "ssg_linear_wgrad_f32";
  if (int rc = linear_check(fn, B, K, N)) return rc;
  if (!dy || (!dw && !db) || (dw && !x)) { ssg_set_error("%s: NULL pointer (dy, and dw with x or db, are needed)", fn); return SSG_ERR_INVALID; }
  if (dw)
    hipLaunchKernelGGL((linear_gemm_kernel<false, false>), dim3(lin_tiles(K), lin_tiles(N)), dim3(256), 0, stream, dy, (int64_t)1, (int64_t)N, x, (int64_t)1,
                       (int64_t)K, (const float*)nullptr, dw, N, K, B);
  SSG_LAUNCH_CHECK("linear_gemm_kernel (weight gradient)");
  if (db) hipLaunchKernelGGL(linear_bias_grad_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, dy, db, B, N);
  SSG_LAUNCH_CHECK("linear_bias_grad_kernel");
  return SSG_OK;
}

extern "C" int ssg_gap_stripes_bwd(const float* g, int set_mask, float* dx, int B, int H, int W, int C, int num_split, hipStream_t stream) {
  const char* fn = "ssg_gap_stripes_bwd";
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || num_split < 1 || num_split > H || num_split > 30 || (int64_t)H * W > 0x7fffffffLL) {
    ssg_set_error("%s: need B, H, W >= 1, C %% 4 == 0, 1 <= num_split <= min(H, 30) (B=%d H=%d W=%d C=%d num_split=%d)", fn, B, H, W, C, num_split);
    return SSG_ERR_INVALID;
  }
  const int nsets = num_split > 1 ? num_split + 1 : 1;
  if (set_mask < 0 || (set_mask >> nsets)) { ssg_set_error("%s: set_mask %d names a set past the %d of num_split=%d", fn, set_mask, nsets, num_split); return SSG_ERR_INVALID; }
  if (int rc = ssg_need_pointers(fn, dx && (g || !set_mask))) return rc;
  if (int rc = ssg_need_aligned16(fn, "g and dx", {g, dx})) return rc;
  const int blocks = ssg_blocks256((int64_t)B * H * W * (C >> 2), 8192);
  hipLaunchKernelGGL(gap_stripes_bwd_kernel, dim3(blocks), dim3(256), 0, stream, g, (unsigned)set_mask, dx, B, H, W, C, num_split);
  SSG_LAUNCH_CHECK("gap_stripes_bwd_kernel");
  return SSG_OK;
}
