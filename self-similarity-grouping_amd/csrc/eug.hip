// eug.hip -- SSG++ label estimation and selection (reference: reid/eug.py:193-290, caller semitraining.py:228-244).
//
// Three steps that follow the feature extraction of the labelled / unlabelled sets:
//   a. rerank=False (eug.py:201-214): for every unlabelled row u, dist_l = np.linalg.norm(l_feas - u, axis=1) in float32 and its
//      np.argmin.  Exact: diff and square are rounded separately (no FMA, the library is built with -ffp-contract=off), the squares
//      are summed in numpy's float32 pairwise order (8 accumulators, leaves of at most 128, split at n/2 & ~7) in sequential chunks
//      of 8192 (s = s + pairwise(chunk): the reduction's buffer size), then a correctly rounded sqrtf.  The exact order rules out the
//      Gram form, so this is a VALU kernel: a 32 u x 64 l tile per workgroup, each pairwise leaf of both row sets staged in LDS once.
//   b. rerank=True (eug.py:223-244) on the [Nu, Nl] float32 matrix re_ranking_init returned: the row argmin (first index on ties,
//      first NaN wins: np.argmin), scores = -min, labels = l_label[argmin], confidence = 1 - min / np.max(column argmin) in float32
//      (np.max propagates NaN); the column maxima are one pass over the matrix, not one column scan per row.
//   c. select_top_data / select_top_true_data (eug.py:277-290): mask of the k largest float64 scores (radix select on one
//      workgroup).  np.argsort's order among equal scores is a property of the host CPU's sort, so ties that straddle the cut go to
//      the lowest indices; without such a tie the set is the reference's.
#include "ssg_common.h"

namespace ssg {

constexpr int EUG_TU = 32, EUG_TL = 64;       // u rows x l rows per workgroup (256 threads: 2 u x 4 l pairs each)
constexpr int EUG_KW = 128, EUG_LD = EUG_KW + 4;   // one pairwise leaf (<= 128 columns) per LDS stage; padded row pitch
constexpr int EUG_MAXD = 8;                    // evaluation stack of the pairwise tree: depth <= 7 for chunks of <= 8192
constexpr int EUG_CHUNK = 8192;                // numpy's reduction buffer
constexpr int EUG_MAXLEAF = 512;               // d <= 32768: <= 128 leaves per chunk
constexpr int EUG_CM_CHUNKS = 64;              // row chunks of the column-max pass

// Post-order leaf program of numpy's pairwise sum over [0, d): x = start, y = length, z = stack pops (adds) after the leaf,
// w = 1 on the last leaf of a chunk.  Built by one thread into LDS (a few hundred steps).
__device__ int eug_build_program(int d, int4* prog) {
  int nl = 0;
  for (int c0 = 0; c0 < d; c0 += EUG_CHUNK) {
    const int n = min(EUG_CHUNK, d - c0);
    int ss[16], sn[16], so[16], sp = 0;
    ss[0] = c0; sn[0] = n; so[0] = 0; sp = 1;
    while (sp > 0) {
      sp--;
      const int s = ss[sp], m = sn[sp], owe = so[sp];
      if (m <= EUG_KW) { prog[nl++] = make_int4(s, m, owe, 0); continue; }
      int m2 = m / 2; m2 -= m2 % 8;
      ss[sp] = s + m2; sn[sp] = m - m2; so[sp] = owe + 1; sp++;     // right half: its last leaf owes this node's add
      ss[sp] = s; sn[sp] = m2; so[sp] = 0; sp++;                    // left half first
    }
    prog[nl - 1].w = 1;
  }
  return nl;
}

// np.argmin's order: the first NaN wins, else the smaller value, else the lower index
__device__ __forceinline__ bool eug_better(float v, int i, float m, int j) {
  if (m != m) return (v != v) && i < j;
  if (v != v) return true;
  return v < m || (v == m && i < j);
}

__device__ __forceinline__ void eug_argmin_xor(float& v, int& i, int width) {
  for (int sh = 1; sh < width; sh <<= 1) {
    const float ov = __shfl_xor(v, sh, 64);
    const int oi = __shfl_xor(i, sh, 64);
    if (eug_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// part_val/part_idx[split, u] = (min, argmin) of |l - u| over the l tiles of split blockIdx.y
__global__ __launch_bounds__(256) void eug_nn_kernel(const float* __restrict__ U, int nu, const float* __restrict__ Lf, int nl, int d,
                                                     int tiles_per_split, float* __restrict__ part_val, int32_t* __restrict__ part_idx) {
  __shared__ __attribute__((aligned(16))) float su[EUG_TU * EUG_LD];
  __shared__ __attribute__((aligned(16))) float sl[EUG_TL * EUG_LD];
  __shared__ int4 prog[EUG_MAXLEAF];
  __shared__ int s_np;
  const int tid = (int)threadIdx.x, tl = tid & 15, tu = tid >> 4;
  if (tid == 0) s_np = eug_build_program(d, prog);
  __syncthreads();
  const int np_ = s_np;
  const int u0 = (int)blockIdx.x * EUG_TU;
  const int ntiles = (nl + EUG_TL - 1) / EUG_TL;
  const int t0 = (int)blockIdx.y * tiles_per_split, t1 = min(ntiles, t0 + tiles_per_split);
  float bestv[2] = {INFINITY, INFINITY};
  int besti[2] = {0x7fffffff, 0x7fffffff};
  const int kc = tid & (EUG_KW - 1), r0 = tid >> 7;     // staging: column kc of rows r0, r0 + 2, ...
  for (int lt = t0; lt < t1; lt++) {
    const int l0 = lt * EUG_TL;
    float st[2][4][EUG_MAXD];
    float cs[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        cs[a][b] = 0.f;
#pragma unroll
        for (int q = 0; q < EUG_MAXD; q++) st[a][b][q] = 0.f;
      }
    for (int li = 0; li < np_; li++) {
      const int4 p = prog[li];
      const int start = p.x, len = p.y;
      __syncthreads();                                   // the previous leaf's reads are done
      if (kc < len) {
        for (int r = r0; r < EUG_TU + EUG_TL; r += 2) {
          float x = 0.f;
          if (r < EUG_TU) {
            const int gu = u0 + r;
            if (gu < nu) x = U[(int64_t)gu * d + start + kc];
            su[r * EUG_LD + kc] = x;
          } else {
            const int gl = l0 + r - EUG_TU;
            if (gl < nl) x = Lf[(int64_t)gl * d + start + kc];
            sl[(r - EUG_TU) * EUG_LD + kc] = x;
          }
        }
      }
      __syncthreads();
      float res[2][4];
      if (len >= 8) {
        float acc[2][4][8];
        const int body = len - (len & 7);
        for (int k = 0; k < body; k += 8) {
          float4 ua[2][2], lb[4][2];
#pragma unroll
          for (int a = 0; a < 2; a++) {
            ua[a][0] = *reinterpret_cast<const float4*>(&su[(tu + 16 * a) * EUG_LD + k]);
            ua[a][1] = *reinterpret_cast<const float4*>(&su[(tu + 16 * a) * EUG_LD + k + 4]);
          }
#pragma unroll
          for (int b = 0; b < 4; b++) {
            lb[b][0] = *reinterpret_cast<const float4*>(&sl[(tl + 16 * b) * EUG_LD + k]);
            lb[b][1] = *reinterpret_cast<const float4*>(&sl[(tl + 16 * b) * EUG_LD + k + 4]);
          }
#pragma unroll
          for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
              const float uv[8] = {ua[a][0].x, ua[a][0].y, ua[a][0].z, ua[a][0].w, ua[a][1].x, ua[a][1].y, ua[a][1].z, ua[a][1].w};
              const float lv[8] = {lb[b][0].x, lb[b][0].y, lb[b][0].z, lb[b][0].w, lb[b][1].x, lb[b][1].y, lb[b][1].z, lb[b][1].w};
#pragma unroll
              for (int j = 0; j < 8; j++) {
                const float df = lv[j] - uv[j];
                const float sq = df * df;
                acc[a][b][j] = (k == 0) ? sq : acc[a][b][j] + sq;
              }
            }
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) {
            const float* r = acc[a][b];
            res[a][b] = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
          }
        for (int k = body; k < len; k++)
#pragma unroll
          for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
              const float df = sl[(tl + 16 * b) * EUG_LD + k] - su[(tu + 16 * a) * EUG_LD + k];
              res[a][b] = res[a][b] + df * df;
            }
      } else {                                           // a chunk of fewer than 8 columns: res = 0; res += x
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) res[a][b] = 0.f;
        for (int k = 0; k < len; k++)
#pragma unroll
          for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
              const float df = sl[(tl + 16 * b) * EUG_LD + k] - su[(tu + 16 * a) * EUG_LD + k];
              res[a][b] = res[a][b] + df * df;
            }
      }
      // push the leaf, then the adds of the subtrees it completes: pairwise(left) + pairwise(right)
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
#pragma unroll
          for (int q = EUG_MAXD - 1; q > 0; q--) st[a][b][q] = st[a][b][q - 1];
          st[a][b][0] = res[a][b];
        }
      for (int pop = 0; pop < p.z; pop++)
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) {
            st[a][b][0] = st[a][b][1] + st[a][b][0];
#pragma unroll
            for (int q = 1; q < EUG_MAXD - 1; q++) st[a][b][q] = st[a][b][q + 1];
          }
      if (p.w)
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) cs[a][b] = cs[a][b] + st[a][b][0];
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int gl = l0 + tl + 16 * b;
        if (gl < nl) {
          const float v = sqrtf(cs[a][b]);
          if (eug_better(v, gl, bestv[a], besti[a])) { bestv[a] = v; besti[a] = gl; }
        }
      }
  }
#pragma unroll
  for (int a = 0; a < 2; a++) {
    float v = bestv[a]; int i = besti[a];
    eug_argmin_xor(v, i, 16);                            // the 16 lanes that share u row tu + 16a
    const int gu = u0 + tu + 16 * a;
    if (tl == 0 && gu < nu) { part_val[(int64_t)blockIdx.y * nu + gu] = v; part_idx[(int64_t)blockIdx.y * nu + gu] = i; }
  }
}

// shared epilogue of a and b: labels = l_label[argmin], scores = -min (float32, widened)
__global__ void eug_nn_finish_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx, int nsplit, int nu,
                                     const int64_t* __restrict__ l_label, int32_t* __restrict__ argmin, float* __restrict__ minval,
                                     int64_t* __restrict__ labels, double* __restrict__ scores) {
  const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (u >= nu) return;
  float v = part_val[u]; int i = part_idx[u];
  for (int s = 1; s < nsplit; s++) {
    const float ov = part_val[(int64_t)s * nu + u]; const int oi = part_idx[(int64_t)s * nu + u];
    if (eug_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
  if (argmin) argmin[u] = i;
  if (minval) minval[u] = v;
  if (labels) labels[u] = l_label[i];
  if (scores) scores[u] = (double)(-v);
}

// np.max semantics: NaN propagates
__device__ __forceinline__ float eug_nanmax(float m, float x) { return (x > m || x != x) ? x : m; }

// part[c, j] = max of column j over row chunk c
__global__ __launch_bounds__(256) void eug_colmax_part_kernel(const float* __restrict__ D, int nu, int nl, float* __restrict__ part) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= nl) return;
  const int c = (int)blockIdx.y, per = (nu + EUG_CM_CHUNKS - 1) / EUG_CM_CHUNKS;
  const int r1 = min(nu, (c + 1) * per);
  float m = -INFINITY;
  for (int r = c * per; r < r1; r++) m = eug_nanmax(m, D[(int64_t)r * nl + j]);
  part[(int64_t)c * nl + j] = m;
}

__global__ void eug_colmax_final_kernel(const float* __restrict__ part, int nl, float* __restrict__ colmax) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= nl) return;
  float m = -INFINITY;
  for (int c = 0; c < EUG_CM_CHUNKS; c++) m = eug_nanmax(m, part[(int64_t)c * nl + j]);
  colmax[j] = m;
}

// one wave per row: argmin, label, score, confidence
__global__ __launch_bounds__(256) void eug_rowmin_kernel(const float* __restrict__ D, int nu, int nl, const float* __restrict__ colmax,
                                                         const int64_t* __restrict__ l_label, int32_t* __restrict__ argmin,
                                                         int64_t* __restrict__ labels, double* __restrict__ scores, double* __restrict__ conf) {
  const int row = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= nu) return;
  const int lane = lane_id();
  float v = INFINITY; int i = 0x7fffffff;
  for (int j = lane; j < nl; j += 64) {
    const float x = D[(int64_t)row * nl + j];
    if (eug_better(x, j, v, i)) { v = x; i = j; }
  }
  eug_argmin_xor(v, i, 64);
  if (lane == 0) {
    if (argmin) argmin[row] = i;
    labels[row] = l_label[i];
    scores[row] = (double)(-v);
    conf[row] = (double)(1.f - v / colmax[i]);
  }
}

// key order of -score under np.argsort: larger score first, -0 == +0, NaN last
__device__ __forceinline__ uint64_t eug_score_key(double x) {
  if (x != x) return 0ULL;
  if (x == 0.0) x = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

// mask[i] = score i is among the k largest (ties at the cut: lowest indices) [&& labels[i] != -1]
__global__ __launch_bounds__(1024) void eug_select_top_kernel(const double* __restrict__ scores, int n, int k, const double* __restrict__ labels,
                                                              uint8_t* __restrict__ mask) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t s_prefix;
  __shared__ int s_rem, s_wcnt[16];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = lane_id();
  if (k <= 0) {
    for (int i = tid; i < n; i += 1024) mask[i] = 0;
    return;
  }
  uint64_t prefix = 0, pmask = 0;
  int rem = k;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
      const uint64_t key = eug_score_key(scores[i]);
      if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      int acc = 0, b = 255;
      for (; b > 0; b--) {
        if (acc + (int)hist[b] >= rem) break;
        acc += (int)hist[b];
      }
      s_prefix = prefix | ((uint64_t)b << shift);
      s_rem = rem - acc;
    }
    __syncthreads();
    prefix = s_prefix; rem = s_rem; pmask |= 0xFFULL << shift;
  }
  // prefix = the k-th largest key; rem = how many of the keys equal to it are taken, in index order
  int taken = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    uint64_t key = 0;
    if (i < n) key = eug_score_key(scores[i]);
    const bool eq = i < n && key == prefix;
    const uint64_t bal = __ballot(eq);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, tot = 0;
    for (int w = 0; w < 16; w++) { const int c = s_wcnt[w]; before += (w < wave) ? c : 0; tot += c; }
    if (i < n) {
      const bool sel = key > prefix || (eq && taken + before + __popcll(bal & lanemask_lt()) < rem);
      mask[i] = (uint8_t)(sel && (labels == nullptr || labels[i] != -1.0));
    }
    taken += tot;
    __syncthreads();
  }
}

}  // namespace ssg

using namespace ssg;

extern "C" int ssg_eug_nn_splits(int nu, int nl) {
  if (nu <= 0 || nl <= 0) return 1;
  const int ublocks = (nu + EUG_TU - 1) / EUG_TU, ntiles = (nl + EUG_TL - 1) / EUG_TL;
  int s = (2048 + ublocks - 1) / ublocks;               // >= ~8 workgroups per CU
  if (s > ntiles) s = ntiles;
  const int per = (ntiles + s - 1) / s;
  return (ntiles + per - 1) / per;                      // no empty split
}

extern "C" int ssg_eug_nn_f32(const float* u, int nu, const float* l, int nl, int d, const int64_t* l_label, int nsplit, float* part_val,
                              int32_t* part_idx, int32_t* argmin, float* minval, int64_t* labels, double* scores, hipStream_t stream) {
  if (nu <= 0 || nl <= 0 || d <= 0 || d > EUG_MAXLEAF * 64) { ssg_set_error("ssg_eug_nn_f32: need nu, nl > 0 and 0 < d <= %d", EUG_MAXLEAF * 64); return SSG_ERR_INVALID; }
  if (nsplit != ssg_eug_nn_splits(nu, nl)) { ssg_set_error("ssg_eug_nn_f32: nsplit must be ssg_eug_nn_splits(nu, nl) = %d", ssg_eug_nn_splits(nu, nl)); return SSG_ERR_INVALID; }
  if ((labels && !l_label) || !part_val || !part_idx) { ssg_set_error("ssg_eug_nn_f32: missing buffer"); return SSG_ERR_INVALID; }
  const int ntiles = (nl + EUG_TL - 1) / EUG_TL, per = (ntiles + nsplit - 1) / nsplit;
  hipLaunchKernelGGL(eug_nn_kernel, dim3((nu + EUG_TU - 1) / EUG_TU, nsplit), dim3(256), 0, stream, u, nu, l, nl, d, per, part_val, part_idx);
  hipLaunchKernelGGL(eug_nn_finish_kernel, dim3((nu + 255) / 256), dim3(256), 0, stream, part_val, part_idx, nsplit, nu, l_label, argmin, minval,
                     labels, scores);
  SSG_LAUNCH_CHECK("eug_nn_kernel");
  return SSG_OK;
}

extern "C" int ssg_eug_dist_label_f32(const float* D, int nu, int nl, const int64_t* l_label, float* ws, int32_t* argmin, int64_t* labels,
                                      double* scores, double* confidence, hipStream_t stream) {
  if (nu <= 0 || nl <= 0) { ssg_set_error("ssg_eug_dist_label_f32: need nu, nl > 0"); return SSG_ERR_INVALID; }
  if (!D || !l_label || !ws || !labels || !scores || !confidence) { ssg_set_error("ssg_eug_dist_label_f32: missing buffer"); return SSG_ERR_INVALID; }
  float* colmax = ws + (size_t)EUG_CM_CHUNKS * nl;
  hipLaunchKernelGGL(eug_colmax_part_kernel, dim3((nl + 255) / 256, EUG_CM_CHUNKS), dim3(256), 0, stream, D, nu, nl, ws);
  hipLaunchKernelGGL(eug_colmax_final_kernel, dim3((nl + 255) / 256), dim3(256), 0, stream, ws, nl, colmax);
  hipLaunchKernelGGL(eug_rowmin_kernel, dim3((nu + 3) / 4), dim3(256), 0, stream, D, nu, nl, colmax, l_label, argmin, labels, scores, confidence);
  SSG_LAUNCH_CHECK("eug_dist_label");
  return SSG_OK;
}

extern "C" int ssg_eug_select_top(const double* scores, int n, int k, const double* labels, uint8_t* mask, hipStream_t stream) {
  if (n <= 0 || k < 0 || k > n) { ssg_set_error("ssg_eug_select_top: need n > 0 and 0 <= k <= n (n = %d, k = %d)", n, k); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(eug_select_top_kernel, dim3(1), dim3(1024), 0, stream, scores, n, k, labels, mask);
  SSG_LAUNCH_CHECK("eug_select_top_kernel");
  return SSG_OK;
}
