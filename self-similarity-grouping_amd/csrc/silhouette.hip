// silhouette.hip -- the silhouette coefficient of one or several labelings of a precomputed distance matrix: the per-row cluster sums
// and the nearest other cluster's mean, and the diagonal check.
//
// Replaces the N x N part of sklearn 1.7.2's `silhouette_samples(X, labels, metric='precomputed')` -- `_silhouette_reduce` -- bit for bit
// (ssg_amd/silhouette.py holds the look-alikes and everything that works on N-long arrays: the label encoding, the member lists, the
// four numpy lines after the reduction, the mean):
//   the sums = for row i and every cluster c, s[i,c] = np.bincount(labels, weights=X[i])[c]: a float64 sum that starts at +0.0, walks
//              the members of c in ASCENDING COLUMN ORDER and rounds once per add.  That order is the contract: no tree, no atomic and
//              no reordering gives numpy's bits.  intra_sum[i] = s[i, own]; inter_min[i] = min over c != own of s[i,c] / double(freq[c]),
//              an IEEE division.  The cluster means are never -0.0 (a sum that starts at +0.0 cannot become -0.0) and the caller refuses
//              NaN and infinity beforehand (ssg_agglo_check), so the minimum does not depend on the order of its fold;
//              negatives[0] = how many staged entries are below zero (sklearn's pairwise_distances refuses a negative precomputed
//              distance; the count covers exactly the sub-matrix sklearn would look at);
//   the diag = how many selected samples have |X[i,i]| > atol (sklearn refuses such a matrix).
//
// A workgroup owns one selected row at a time.  It decodes the row's m selected entries ONCE into a float64 stage, in selection order --
// LDS while 8 m bytes fit, else the workgroup's slice of a workspace -- and then, for each of the K labelings, thread t of T walks the
// clusters t, t + T, ...: it adds the cluster's members one after the other from the stage through the labeling's member list, divides,
// and the workgroup folds the minimum.  T is 256 while a CU's LDS holds four stages or more, else 512 or 1024, so that a CU keeps at
// least sixteen waves summing clusters side by side when the stages are large.  The row is read and decoded once for all K labelings: the matrix is the expensive thing, the labelings
// are m-long.  No float atomic, no synchronisation between workgroups, no spin loop; every loop is bounded by m or by the number of
// clusters; the only atomic is the integer count of negative entries, once per wave.  One chain of dependent adds per cluster sets the
// time of a row: a labeling with one very large cluster leaves most threads idle.  That is the floor of the summation order and is
// not traded away.
//
// Every index read from the caller's arrays is clamped before it is used as an address.
#include "matview.h"

namespace ssg {

constexpr int SIL_MAX_WAVES = 16;           // a workgroup has 4, 8 or 16 waves: the fewer stages a CU's LDS holds, the more waves share one
constexpr int SIL_RED = 2 * SIL_MAX_WAVES;  // doubles at the head of the dynamic LDS: the wave minima, double-buffered

// one entry of the view, widened like load_vals widens it
template <int MODE>
__device__ __forceinline__ double sil_entry(const MatView& mv, int i, int j) {
  const int64_t off = (int64_t)i * mv.N + j;
  if (MODE == 2) return reinterpret_cast<const double*>(mv.M)[off];
  const hbits raw = reinterpret_cast<const hbits*>(mv.M)[off];
  if (MODE == 0) return final_dist_value(raw, mv.v[i], mv.v[j], mv.lambda_value);
  return (double)h2f(raw);
}

// sel == NULL: the identity, streamed as the other matrix passes stream a row (the waves take the 512-entry chunks in turn); else a gather.
// labels / members [K, m], start [K, cstride], ncl [K].  Positions whose label is negative take no part in that labeling: they are in no
// member list and their two outputs are left alone.
template <int MODE, bool LDS>
__global__ __launch_bounds__(64 * SIL_MAX_WAVES) void silhouette_sums_kernel(MatView mv, const int* __restrict__ sel, int m, int K, int cstride,
                                                                      const int* __restrict__ labels, const int* __restrict__ members,
                                                                      const int* __restrict__ start, const int* __restrict__ ncl, int diag,
                                                                      double* __restrict__ gstage, size_t slice, double* __restrict__ intra_sum,
                                                                      double* __restrict__ inter_min, unsigned long long* __restrict__ negatives) {
  extern __shared__ __align__(16) double sil_lds[];
  double* red = sil_lds;
  double* stage = LDS ? sil_lds + SIL_RED : gstage + (size_t)blockIdx.x * slice;
  const int N = mv.N, tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = lane_id(), wave = tid >> 6, nwaves = nthr >> 6;
  const double inf = __builtin_inf();
  int par = 0;
  unsigned neg = 0;                                           // staged entries below zero (sklearn refuses a negative precomputed distance)
  for (int a = (int)blockIdx.x; a < m; a += (int)gridDim.x) {
    const int i = sel ? sel[a] : a;
    const bool row_ok = (unsigned)i < (unsigned)N;
    if (!sel) {
      RowStream rs(i, N, N);
      for (int ch = wave; ch < rs.nchunks; ch += nwaves) {
        double d[8];
        load_vals<MODE>(mv, rs, ch, lane, i, d);
        const int j0 = rs.col0(ch, lane);
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int j = j0 + e;
          if (j >= 0 && j < m) { const double x = (diag && j == a) ? 0.0 : d[e]; neg += x < 0.0; stage[j] = x; }
        }
      }
    } else {
      for (int b = tid; b < m; b += nthr) {
        const int j = sel[b];
        double x = __builtin_nan("");
        if (row_ok && (unsigned)j < (unsigned)N) x = sil_entry<MODE>(mv, i, j);
        if (diag && b == a) x = 0.0;
        neg += x < 0.0;
        stage[b] = x;
      }
    }
    __syncthreads();
    for (int k = 0; k < K; k++) {
      const int own = labels[(size_t)k * m + a];
      if (own < 0) continue;                                  // (the same in every thread: the barriers below stay matched)
      int C = ncl[k];
      C = C < 0 ? 0 : (C >= cstride ? cstride - 1 : C);
      const int* mem = members + (size_t)k * m;
      const int* st = start + (size_t)k * cstride;
      double best = inf;
      for (int c = tid; c < C; c += nthr) {
        int s0 = st[c], s1 = st[c + 1];
        s0 = s0 < 0 ? 0 : (s0 > m ? m : s0);
        s1 = s1 < s0 ? s0 : (s1 > m ? m : s1);
        double sum = 0.0;
        int p = s0;
        for (; p + 4 <= s1; p += 4) {                         // four loads in flight, four adds in order
          const unsigned i0 = (unsigned)mem[p], i1 = (unsigned)mem[p + 1], i2 = (unsigned)mem[p + 2], i3 = (unsigned)mem[p + 3];
          const unsigned top = (unsigned)(m - 1);
          const double x0 = stage[i0 < top ? i0 : top], x1 = stage[i1 < top ? i1 : top], x2 = stage[i2 < top ? i2 : top], x3 = stage[i3 < top ? i3 : top];
          sum = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(sum, x0), x1), x2), x3);
        }
        for (; p < s1; p++) {
          const unsigned i0 = (unsigned)mem[p], top = (unsigned)(m - 1);
          sum = __dadd_rn(sum, stage[i0 < top ? i0 : top]);
        }
        if (c == own) intra_sum[(size_t)k * m + a] = sum;
        else {
          const double q = __ddiv_rn(sum, (double)(s1 - s0));
          if (q < best) best = q;
        }
      }
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) { const double o = __shfl_xor(best, x, 64); if (o < best) best = o; }
      if (lane == 0) red[par * SIL_MAX_WAVES + wave] = best;
      __syncthreads();
      if (tid == 0) {
        double b = red[par * SIL_MAX_WAVES];
        for (int w = 1; w < nwaves; w++) if (red[par * SIL_MAX_WAVES + w] < b) b = red[par * SIL_MAX_WAVES + w];
        inter_min[(size_t)k * m + a] = b;
      }
      par ^= 1;
    }
    __syncthreads();                                          // every thread is done with the stage before the next row overwrites it
  }
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) neg += __shfl_xor(neg, x, 64);
  if (lane == 0 && neg) atomicAdd(negatives, (unsigned long long)neg);      // (an integer count: one atomic per wave)
}

template <int MODE>
__global__ __launch_bounds__(256) void silhouette_diag_kernel(MatView mv, const int* __restrict__ sel, int m, double atol, unsigned long long* __restrict__ count) {
  const int a = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  bool bad = false;
  if (a < m) {
    const int i = sel ? sel[a] : a;
    if ((unsigned)i < (unsigned)mv.N) bad = __builtin_fabs(sil_entry<MODE>(mv, i, i)) > atol;
  }
  const unsigned long long b = __ballot(bad);
  if (lane_id() == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

}  // namespace ssg

using namespace ssg;

// the stage (8 bytes per selected sample, rounded up to two) and the wave minima inside the 160 KB a workgroup may hold
constexpr size_t SIL_LDS_LIMIT = 160 * 1024;
extern "C" int ssg_silhouette_lds_max_m(void) { return (int)(((SIL_LDS_LIMIT - SIL_RED * 8) / 8) & ~(size_t)1); }

static int silhouette_check_matrix(const char* fn, const void* M, const uint16_t* v, int N, int mode, const int32_t* sel, const int32_t* sel_host, int m) {
  if (!M || N < 1 || mode < 0 || mode > 2 || (mode == 0 && !v) || ((uintptr_t)M & (mode == 2 ? 7 : 1)) || (v && ((uintptr_t)v & 1))) {
    ssg_set_error("%s: bad matrix (M=%p N=%d mode=%d%s); mode 0..2, mode 0 needs v, pointers aligned to their element", fn, M, N, mode,
                  (mode == 0 && !v) ? " v=NULL" : "");
    return SSG_ERR_INVALID;
  }
  if (m > N || (!sel && m != N) || (sel && ((uintptr_t)sel & 3)) || (sel_host && !sel)) {
    ssg_set_error("%s: m=%d selected samples of N=%d: m <= N, m == N without sel, sel 4-byte aligned, sel_host only beside sel", fn, m, N);
    return SSG_ERR_INVALID;
  }
  if (sel_host) {
    for (int b = 0; b < m; b++) if (sel_host[b] < 0 || sel_host[b] >= N) {
      ssg_set_error("%s: sel[%d] = %d is outside [0, %d)", fn, b, sel_host[b], N);
      return SSG_ERR_INVALID;
    }
  }
  return SSG_OK;
}

extern "C" int ssg_silhouette_diag(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const int32_t* sel, const int32_t* sel_host, int m,
                                   double atol, int64_t* count, hipStream_t stream) {
  if (m < 1) { ssg_set_error("ssg_silhouette_diag: m=%d must be at least 1", m); return SSG_ERR_INVALID; }
  int rc = silhouette_check_matrix("ssg_silhouette_diag", M, v, N, mode, sel, sel_host, m); if (rc) return rc;
  if (!count || ((uintptr_t)count & 7)) { ssg_set_error("ssg_silhouette_diag: count must be an 8-byte aligned int64 word, got %p", (void*)count); return SSG_ERR_INVALID; }
  if (!(atol >= 0.0)) { ssg_set_error("ssg_silhouette_diag: atol=%g must be >= 0", atol); return SSG_ERR_INVALID; }
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
  SSG_HIP(hipMemsetAsync(count, 0, 8, stream));
#define SSG_SD(MD) hipLaunchKernelGGL(silhouette_diag_kernel<MD>, dim3((m + 255) / 256), dim3(256), 0, stream, mv, sel, m, atol, (unsigned long long*)count)
  if (mode == 0) SSG_SD(0); else if (mode == 1) SSG_SD(1); else SSG_SD(2);
#undef SSG_SD
  SSG_LAUNCH_CHECK("silhouette_diag_kernel");
  return SSG_OK;
}

extern "C" int ssg_silhouette_sums(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const int32_t* sel, const int32_t* sel_host, int m,
                                   int K, int Cmax, const int32_t* labels, const int32_t* members, const int32_t* start, const int32_t* ncl, int diag, int state,
                                   void* ws, size_t ws_bytes, double* intra_sum, double* inter_min, int64_t* negatives, hipStream_t stream) {
  if (m < 3 || K < 1 || Cmax < 1 || Cmax > m) {
    ssg_set_error("ssg_silhouette_sums: m=%d K=%d Cmax=%d: m >= 3, K >= 1, 1 <= Cmax <= m", m, K, Cmax);
    return SSG_ERR_INVALID;
  }
  int rc = silhouette_check_matrix("ssg_silhouette_sums", M, v, N, mode, sel, sel_host, m); if (rc) return rc;
  if (!labels || !members || !start || !ncl || !intra_sum || !inter_min || !negatives) {
    ssg_set_error("ssg_silhouette_sums: null labels / members / start / ncl / intra_sum / inter_min / negatives"); return SSG_ERR_INVALID;
  }
  if (((uintptr_t)labels & 3) || ((uintptr_t)members & 3) || ((uintptr_t)start & 3) || ((uintptr_t)ncl & 3) || ((uintptr_t)intra_sum & 7) || ((uintptr_t)inter_min & 7) ||
      ((uintptr_t)negatives & 7)) {
    ssg_set_error("ssg_silhouette_sums: labels / members / start / ncl must be 4-byte aligned, intra_sum / inter_min / negatives 8-byte aligned"); return SSG_ERR_INVALID;
  }
  if (diag != 0 && diag != 1) { ssg_set_error("ssg_silhouette_sums: diag=%d must be 0 (as stored) or 1 (the own entry enters as +0.0)", diag); return SSG_ERR_INVALID; }
  if (state < 0 || state > 2) { ssg_set_error("ssg_silhouette_sums: state=%d must be 0 (auto), 1 (LDS) or 2 (global)", state); return SSG_ERR_INVALID; }
  const bool fits = m <= ssg_silhouette_lds_max_m();
  if (state == 1 && !fits) { ssg_set_error("ssg_silhouette_sums: state=1 (LDS) holds at most m=%d samples, got m=%d", ssg_silhouette_lds_max_m(), m); return SSG_ERR_INVALID; }
  const bool lds = state == 1 || (state == 0 && fits);
  const size_t slice = ((size_t)m + 1) & ~(size_t)1, need = slice * 8;
  if (!lds && (!ws || ws_bytes < need || ((uintptr_t)ws & 15))) {
    ssg_set_error("ssg_silhouette_sums: the global stage needs a 16-byte aligned workspace of at least %zu bytes (one slice per workgroup), got %zu", need,
                  ws ? ws_bytes : (size_t)0);
    return SSG_ERR_INVALID;
  }
  const MatView mv = make_view(M, v, N, 0, N, mode, lambda_value);
  const size_t dyn = SIL_RED * 8 + (lds ? need : 0);
  // a persistent grid: as many workgroups as a CU's LDS holds stages (at most 8 per CU), or as the workspace holds slices (at most 1024)
  // and the fewer workgroups a CU holds, the more waves each gets (16 waves per CU at least): more clusters are summed side by side
  size_t blocks;
  int threads = 256;
  if (lds) { size_t per_cu = SIL_LDS_LIMIT / dyn; blocks = 256 * (per_cu > 8 ? 8 : per_cu); threads = per_cu >= 4 ? 256 : per_cu >= 2 ? 512 : 1024; }
  else { blocks = ws_bytes / need; if (blocks > 1024) blocks = 1024; }
  if (blocks > (size_t)m) blocks = (size_t)m;
  SSG_HIP(hipMemsetAsync(negatives, 0, 8, stream));
#define SSG_SS(KERNEL) do { \
    if (dyn > 48 * 1024) SSG_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn)); \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(threads), dyn, stream, mv, sel, m, K, Cmax + 1, labels, members, start, ncl, diag, (double*)ws, slice, \
                       intra_sum, inter_min, (unsigned long long*)negatives); \
  } while (0)
  if (lds) { if (mode == 0) SSG_SS((silhouette_sums_kernel<0, true>)); else if (mode == 1) SSG_SS((silhouette_sums_kernel<1, true>)); else SSG_SS((silhouette_sums_kernel<2, true>)); }
  else { if (mode == 0) SSG_SS((silhouette_sums_kernel<0, false>)); else if (mode == 1) SSG_SS((silhouette_sums_kernel<1, false>)); else SSG_SS((silhouette_sums_kernel<2, false>)); }
#undef SSG_SS
  SSG_LAUNCH_CHECK("silhouette_sums_kernel");
  return SSG_OK;
}
