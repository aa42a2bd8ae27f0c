// tta.hip -- test-time extraction of reid/extract_feature.py on the GPU: the ten-crop transform the script keeps commented out
// (:47-52), the mean over the crops' features (:94-96) and the multi-query pooling of Market-1501 (:146-153).
//
//   ssg_tencrop_u8      Resize((RH, RW)) [Pillow bilinear, the integer arithmetic and tables of ssg_preprocess_u8] + TenCrop((CH, CW))
//                       + ToTensor + Normalize for a batch of equally sized decoded images, bit for bit.
//   ssg_crop_mean_f32   outputs.view(bs, ncrops, -1).mean(1): torch's CPU order -- an ascending sequential float32 sum over the crops
//                       (its scalar loop's interleaved order in the trailing columns on request), then one division.
//   ssg_group_pool_f32  sklearn.preprocessing.normalize over the rows that share a key, then np.max / np.mean over them.
//
// The horizontal resize pass is preprocess.hip's resize_h_u8_kernel (this file is included behind it in the unity TU).
// All three are streaming kernels: a few bytes per output element, no reuse worth staging in LDS.  Stores are one float per lane,
// like preprocess.hip's: the ten crops of 64 Market images take 0.15 ms (1.6 TB/s written), about 1 % of the 640 forwards they feed
// (profiles/tta_times.txt), so the kernels were left at that.
#include "ssg_common.h"
#include <algorithm>

namespace ssg {

struct CropTable { int top[5], left[5]; };

// One thread per pixel (b, Y, X) of the RESIZED image: the vertical filter is evaluated once, normalised, and stored into every
// crop whose window holds the pixel.  Crop k < 5 is the window (top[k], left[k]) of the resized image R; crop 5 + k is the same
// window of the mirrored image F[Y, X] = R[Y, RW - 1 - X] (torchvision ten_crop: five_crop(img) + five_crop(hflip(img))), so pixel X
// lands in column (RW - 1 - X) - left[k] there.  Consecutive lanes hold consecutive X: the stores of a wave into one crop row are one
// contiguous run, ascending for the plain crops and descending for the mirrored ones.
__global__ __launch_bounds__(256) void tencrop_v_normalize_kernel(const uint8_t* __restrict__ tmp, float* __restrict__ out, int B, int h, int RH, int RW,
                                                                  int CH, int CW, int ncrops, CropTable ct, const int32_t* __restrict__ ymin,
                                                                  const int32_t* __restrict__ ycnt, const int32_t* __restrict__ kk, int ksize, float m0,
                                                                  float m1, float m2, float s0, float s1, float s2) {
  const int64_t total = (int64_t)B * RH * RW;
  const int64_t plane = (int64_t)CH * CW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % RW);
    const int Y = (int)((i / RW) % RH);
    const int64_t b = i / ((int64_t)RW * RH);
    const int lo = ymin[Y], n = ycnt[Y];
    const int32_t* k = kk + (int64_t)Y * ksize;
    const uint8_t* col = tmp + (b * h * (int64_t)RW + X) * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int t = 0; t < n; t++) {
      const int c = k[t];
      const uint8_t* p = col + (int64_t)(lo + t) * RW * 3;
      a0 += (int)p[0] * c; a1 += (int)p[1] * c; a2 += (int)p[2] * c;
    }
    const float v0 = (float)min(max(a0 >> 22, 0), 255), v1 = (float)min(max(a1 >> 22, 0), 255), v2 = (float)min(max(a2 >> 22, 0), 255);
    const float r0 = (v0 / 255.0f - m0) / s0, r1 = (v1 / 255.0f - m1) / s1, r2 = (v2 / 255.0f - m2) / s2;
    const int Xm = RW - 1 - X;
#pragma unroll
    for (int c = 0; c < 5; c++) {
      const int y = Y - ct.top[c];
      if (y < 0 || y >= CH) continue;
      const int x = X - ct.left[c];
      if (x >= 0 && x < CW) {
        float* o = out + ((b * ncrops + c) * 3) * plane + (int64_t)y * CW + x;
        o[0] = r0; o[plane] = r1; o[2 * plane] = r2;
      }
      const int xm = Xm - ct.left[c];
      if (ncrops == 10 && xm >= 0 && xm < CW) {
        float* o = out + ((b * ncrops + 5 + c) * 3) * plane + (int64_t)y * CW + xm;
        o[0] = r0; o[plane] = r1; o[2 * plane] = r2;
      }
    }
  }
}

struct MeanTable { int n; int block[16], crop[16]; };

// out[b, d] = ((((0 + v0) + v1) + ...) + v(n-1)) / (float)n with vt = src[block t][b, crop t, d]: what torch's CPU sum kernel does with
// the columns it takes a SIMD vector at a time (fewer than 16 rows: one accumulator per column, rows ascending).  The columns that
// do not fill torch's last block of vectors, the `tail` last ones, are summed by its scalar loop instead: four partial sums
// p[k] = v[k] + v[4 + k] + ..., the rows past the last whole four onto p[0], then ((p[0] + p[1]) + p[2]) + p[3].
__global__ __launch_bounds__(256) void crop_mean_kernel(const float* __restrict__ s0, int nc0, const float* __restrict__ s1, int nc1, int B, int D,
                                                        MeanTable mt, int tail, float* __restrict__ out) {
  const int64_t total = (int64_t)B * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / D;
    const int d = (int)(i - b * D);
    const bool interleaved = d >= D - tail;
    const int whole = interleaved ? (mt.n / 4) * 4 : 0;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    for (int t = 0; t < mt.n; t++) {
      const float* s = mt.block[t] ? s1 : s0;
      const int nc = mt.block[t] ? nc1 : nc0;
      const float v = s[(b * nc + mt.crop[t]) * D + d];
      const int k = t < whole ? (t & 3) : 0;
      if (k == 0) p0 = p0 + v; else if (k == 1) p1 = p1 + v; else if (k == 2) p2 = p2 + v; else p3 = p3 + v;
    }
    if (interleaved) p0 = ((p0 + p1) + p2) + p3;
    out[i] = p0 / (float)mt.n;
  }
}

constexpr int POOL_ROWS = 256;      // rows of a group whose norms one pass keeps in LDS

// One workgroup per group g of rows order[offs[g] .. offs[g+1]).  The group is walked in passes of POOL_ROWS rows:
//   1. wave w takes rows w, w + 4, ... of the pass: lane l sums x[d]^2 over d = l, l + 64, ... in float64, ascending, the 64 partial
//      sums meet in a fixed xor butterfly; norm = sqrt(sum), 0 counts as 1 (sklearn's _handle_zeros_in_scale)
//   2. thread t takes columns t, t + 256, ...: y = (float)((double)x / norm) row by row in group order, a running max that keeps a
//      NaN once it has met one, and a running sequential float32 sum
// The running values of a group longer than one pass are kept in the output rows themselves (each element is re-read by the thread
// that wrote it), so there is no workspace.  The group's result goes to the row of the FIRST query that names the group;
// group_pool_gather_kernel then copies it to the group's other queries.  A group no query names only has its rows normalised.
// Indices that point outside their array (order, offs, qgroup come from the host wrapper) are not followed: such a row counts as NaN.
__global__ __launch_bounds__(256) void group_pool_kernel(const float* __restrict__ x, int M, int D, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ offs, int G, const int32_t* __restrict__ qgroup, int Q,
                                                         float* __restrict__ out_max, float* __restrict__ out_avg, float* __restrict__ ynorm) {
  __shared__ double norms[POOL_ROWS];
  __shared__ int rep_s;
  const int g = blockIdx.x;
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  if (tid == 0) rep_s = Q;
  __syncthreads();
  int mine = Q;
  for (int q = tid; q < Q; q += 256)
    if (qgroup[q] == g) { mine = q; break; }
  if (mine < Q) atomicMin(&rep_s, mine);
  __syncthreads();
  const int rep = rep_s;
  const int lo = min(max(offs[g], 0), M), hi = min(max(offs[g + 1], lo), M);
  const int m = hi - lo;
  if (rep >= Q && !ynorm) return;
  const float nanf_ = __builtin_nanf("");
  for (int r0 = 0; r0 < m; r0 += POOL_ROWS) {
    const int nr = min(POOL_ROWS, m - r0);
    __syncthreads();                                       // the pass before has read its norms
    for (int r = wave; r < nr; r += 4) {
      const int row = order[lo + r0 + r];
      double s = 0.0;
      if (row >= 0 && row < M) {
        const float* xr = x + (int64_t)row * D;
        for (int d = lane; d < D; d += 64) { const double v = (double)xr[d]; s += v * v; }
      }
      for (int sh = 1; sh < 64; sh <<= 1) s += __shfl_xor(s, sh, 64);
      if (lane == 0) { const double nrm = sqrt(s); norms[r] = nrm == 0.0 ? 1.0 : nrm; }
    }
    __syncthreads();
    for (int d = tid; d < D; d += 256) {
      float mx = 0.f, sum = 0.f;
      if (r0 > 0 && rep < Q) { mx = out_max[(int64_t)rep * D + d]; sum = out_avg[(int64_t)rep * D + d]; }
      for (int r = 0; r < nr; r++) {
        const int row = order[lo + r0 + r];
        const bool ok = row >= 0 && row < M;
        const float y = ok ? (float)((double)x[(int64_t)row * D + d] / norms[r]) : nanf_;
        if (ynorm && ok) ynorm[(int64_t)row * D + d] = y;
        if (r0 + r == 0) { mx = y; sum = y; }
        else { mx = (y > mx || y != y) ? y : mx; sum = sum + y; }
      }
      if (rep < Q) {
        out_max[(int64_t)rep * D + d] = mx;
        out_avg[(int64_t)rep * D + d] = (r0 + nr == m) ? sum / (float)m : sum;
      }
    }
  }
  if (m == 0 && rep < Q)                                    // an empty group: np.max would raise; the wrapper never builds one
    for (int d = tid; d < D; d += 256) { out_max[(int64_t)rep * D + d] = nanf_; out_avg[(int64_t)rep * D + d] = nanf_; }
}

// query q takes the row of the first query of its group (rep <= q), unless it is that query itself
__global__ __launch_bounds__(256) void group_pool_gather_kernel(const int32_t* __restrict__ qgroup, int Q, int G, int D, float* __restrict__ out_max,
                                                                float* __restrict__ out_avg) {
  __shared__ int rep_s;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int g = qgroup[q];
  if (tid == 0) rep_s = q;
  __syncthreads();
  int mine = q;
  for (int p = tid; p < q; p += 256)
    if (qgroup[p] == g) { mine = p; break; }
  if (mine < q) atomicMin(&rep_s, mine);
  __syncthreads();
  const int rep = rep_s;
  const bool bad = g < 0 || g >= G;
  if (rep == q && !bad) return;
  const float nanf_ = __builtin_nanf("");
  for (int d = tid; d < D; d += 256) {
    out_max[(int64_t)q * D + d] = bad ? nanf_ : out_max[(int64_t)rep * D + d];
    out_avg[(int64_t)q * D + d] = bad ? nanf_ : out_avg[(int64_t)rep * D + d];
  }
}

}  // namespace ssg

// src [B,h,w,3] uint8 -> out [B, ncrops, 3, CH, CW] float32.  crops_host: HOST int32 [5][2] (top, left) of tl, tr, bl, br, centre in
// the resized image (the host rounds the centre half-to-even like Python's round()); tmp [B,h,RW,3] uint8 scratch; the tables are
// ssg_preprocess_u8's.
extern "C" int ssg_tencrop_u8(const uint8_t* src, int B, int h, int w, int RH, int RW, int CH, int CW, int ncrops, const int32_t* crops_host,
                              const int32_t* xmin, const int32_t* xcnt, const int32_t* xk, int xksize, const int32_t* ymin, const int32_t* ycnt,
                              const int32_t* yk, int yksize, const float* mean3_host, const float* std3_host, uint8_t* tmp, float* out,
                              hipStream_t stream) {
  if (B <= 0 || h <= 0 || w <= 0 || RH <= 0 || RW <= 0 || CH <= 0 || CW <= 0 || xksize <= 0 || yksize <= 0 || !mean3_host || !std3_host || !crops_host) {
    ssg_set_error("ssg_tencrop_u8: bad shape B=%d %dx%d -> %dx%d, crop %dx%d", B, h, w, RH, RW, CH, CW);
    return SSG_ERR_INVALID;
  }
  if (CH > RH || CW > RW) {
    ssg_set_error("ssg_tencrop_u8: the crop %dx%d is larger than the resized image %dx%d", CH, CW, RH, RW);
    return SSG_ERR_INVALID;
  }
  if (ncrops != 5 && ncrops != 10) {
    ssg_set_error("ssg_tencrop_u8: ncrops must be 5 or 10, got %d", ncrops);
    return SSG_ERR_INVALID;
  }
  ssg::CropTable ct;
  for (int c = 0; c < 5; c++) {
    ct.top[c] = crops_host[2 * c]; ct.left[c] = crops_host[2 * c + 1];
    if (ct.top[c] < 0 || ct.top[c] > RH - CH || ct.left[c] < 0 || ct.left[c] > RW - CW) {
      ssg_set_error("ssg_tencrop_u8: crop %d at (%d, %d) leaves the resized image %dx%d (crop %dx%d)", c, ct.top[c], ct.left[c], RH, RW, CH, CW);
      return SSG_ERR_INVALID;
    }
  }
  if (!src || !tmp || !out || !xmin || !xcnt || !xk || !ymin || !ycnt || !yk) { ssg_set_error("ssg_tencrop_u8: NULL pointer"); return SSG_ERR_INVALID; }
  const int64_t n1 = (int64_t)B * h * RW, n2 = (int64_t)B * RH * RW;
  const int g1 = (int)std::min<int64_t>((n1 + 255) / 256, 16384), g2 = (int)std::min<int64_t>((n2 + 255) / 256, 16384);
  hipLaunchKernelGGL(ssg::resize_h_u8_kernel, dim3(g1), dim3(256), 0, stream, src, tmp, B, h, w, RW, xmin, xcnt, xk, xksize);
  hipLaunchKernelGGL(ssg::tencrop_v_normalize_kernel, dim3(g2), dim3(256), 0, stream, tmp, out, B, h, RH, RW, CH, CW, ncrops, ct, ymin, ycnt, yk, yksize,
                     mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
  SSG_LAUNCH_CHECK("tencrop kernels");
  return SSG_OK;
}

// out [B, D] = mean over n feature rows per image.  src0 [B, nc0, D] and (optional) src1 [B, nc1, D], nc in {5, 10};
// table_host: HOST int32 [n][2] (block 0 | 1, crop) in summation order, 1 <= n <= 15; tail: the last `tail` columns take the
// interleaved order (0: every column sequential).
extern "C" int ssg_crop_mean_f32(const float* src0, int nc0, const float* src1, int nc1, int B, int D, const int32_t* table_host, int n, int tail,
                                 float* out, hipStream_t stream) {
  if (B <= 0 || D <= 0 || n <= 0 || n > 15 || tail < 0 || tail > D || !table_host || (nc0 != 5 && nc0 != 10) || (src1 && nc1 != 5 && nc1 != 10)) {
    ssg_set_error("ssg_crop_mean_f32: bad arguments (B=%d D=%d n=%d tail=%d nc0=%d nc1=%d): n in 1..15, 0 <= tail <= D, 5 or 10 crops per block", B, D,
                  n, tail, nc0, nc1);
    return SSG_ERR_INVALID;
  }
  ssg::MeanTable mt;
  mt.n = n;
  for (int t = 0; t < 16; t++) { mt.block[t] = 0; mt.crop[t] = 0; }
  for (int t = 0; t < n; t++) {
    const int blk = table_host[2 * t], c = table_host[2 * t + 1];
    if ((blk != 0 && blk != 1) || (blk == 1 && !src1) || c < 0 || c >= (blk ? nc1 : nc0)) {
      ssg_set_error("ssg_crop_mean_f32: table entry %d = (block %d, crop %d) names no source row", t, blk, c);
      return SSG_ERR_INVALID;
    }
    mt.block[t] = blk; mt.crop[t] = c;
  }
  if (!src0 || !out) { ssg_set_error("ssg_crop_mean_f32: NULL pointer"); return SSG_ERR_INVALID; }
  const int64_t total = (int64_t)B * D;
  hipLaunchKernelGGL(ssg::crop_mean_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, stream, src0, nc0, src1, nc1, B, D, mt,
                     tail, out);
  SSG_LAUNCH_CHECK("crop_mean_kernel");
  return SSG_OK;
}

// x [M, D]; order [M] row indices grouped by key; offs [G + 1]; qgroup [Q] -> out_max, out_avg [Q, D]; ynorm [M, D] or NULL.
extern "C" int ssg_group_pool_f32(const float* x, int M, int D, const int32_t* order, const int32_t* offs, int G, const int32_t* qgroup, int Q,
                                  float* out_max, float* out_avg, float* ynorm, hipStream_t stream) {
  if (M <= 0 || D <= 0 || G <= 0 || Q <= 0 || G > M) {
    ssg_set_error("ssg_group_pool_f32: bad shape M=%d D=%d G=%d Q=%d (all positive, G <= M)", M, D, G, Q);
    return SSG_ERR_INVALID;
  }
  if (!x || !order || !offs || !qgroup || !out_max || !out_avg) { ssg_set_error("ssg_group_pool_f32: NULL pointer"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(ssg::group_pool_kernel, dim3(G), dim3(256), 0, stream, x, M, D, order, offs, G, qgroup, Q, out_max, out_avg, ynorm);
  hipLaunchKernelGGL(ssg::group_pool_gather_kernel, dim3(Q), dim3(256), 0, stream, qgroup, Q, G, D, out_max, out_avg);
  SSG_LAUNCH_CHECK("group_pool kernels");
  return SSG_OK;
}
