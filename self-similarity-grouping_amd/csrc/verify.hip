// verify.hip -- the verification protocol of reid/evaluation_metrics/eval_far_gar.py (findMetricThreshold_MPI :103-202,
// CalClassificationError_MPI :61-100) on the query x gallery block that ssg_pairwise_sqdist_f32 left in HBM.
//
//   element (i, j) is INTRA when rlab[j] == qlab[i], else INTER (no camera filter, :127,136);  s = sqrtf(d <= 0 ? 0 : d)  (:110-111)
//   pass A  per class: count (int64), sum s and sum s^2 (float64, s widened before squaring), min, max (float32); one status word
//           for "a query row has no intra or no inter element", one for "NaN seen"
//   pass B  exact order statistics of the inter class: the value at each of up to 64 zero-based ranks (np.sort(inter_v)[num], :186,199)
//   pass C  per threshold t (up to 64, float64): #intra s >= t, #inter s < t (:80-81), #intra s < t (:193,200), compared in double
//
// All three are streaming reads of the block (4 B per element, nothing written back).  A workgroup of 256 threads owns 16 rows x 1024
// columns: a thread keeps the gallery labels of its 4 columns in registers and reads its 4 floats of every row with one 16-byte load.
// Columns are counted from the 16-byte boundary at or below D (k = misalignment of D in elements), so that with ld % 4 == 0 every slot
// of every row is aligned; the slots that hang over column 0 or column n (a row's head and tail) and every slot of a block with
// ld % 4 != 0 are read element by element.
//
// No float atomics.  Pass A writes one partial per workgroup and a single workgroup adds them in index order (butterflies, then waves
// in order): the same call gives the same bits.  Passes B and C only count: LDS histograms with integer adds, one global 64-bit add per
// non-empty bin per workgroup.
//
// Pass B is a four-level radix select on the 31 value bits of s (a non-negative float orders as its bit pattern): 11 + 7 + 7 + 6 bits.
// Every level is one pass over the block that serves all ranks at once: after level L every rank has a prefix (the high bits of its
// value) and a rank inside that prefix's elements; the distinct prefixes (at most 64) are kept sorted, an element finds its prefix by a
// range test and a binary search, and the level's histogram is [prefix][bin].  A one-workgroup kernel between two levels walks the
// histograms.  Equal values land in the same bin at every level, so a rank inside a run of ties returns the tied value.
#include <algorithm>
#include <math.h>

#include "ssg_common.h"

namespace ssg {

constexpr int VF_ROWS = 16;           // rows per workgroup
constexpr int VF_THREADS = 256;       // 4 columns per thread: 1024 columns per workgroup
constexpr int VF_MAXQ = 64;           // ranks / thresholds per call
constexpr int VF_L0_BINS = 2048;      // level 0: 11 bits
constexpr int VF_LX_BINS = 128;       // levels 1..3: at most 7 bits

struct VfGeom {
  const float* D;
  size_t ld;
  int m, n;
  int k;                // (address of D / 4) % 4 when vec, else 0
  unsigned nct;         // column tiles
  int vec;
};

struct VfPart {         // one workgroup's share of pass A, 64 bytes; index 0 = intra, 1 = inter
  long long cnt[2];
  double sum[2], sum2[2];
  float mn[2], mx[2];
};

struct VfSel {          // pass B state between two levels
  unsigned nslot;
  int bad;                          // a rank >= the number of inter elements
  unsigned prefix[VF_MAXQ];         // sorted, distinct
  unsigned slot[VF_MAXQ];           // per rank: index into prefix
  long long krem[VF_MAXQ];          // per rank: rank among the elements that carry its prefix
};

struct VfRanks { long long r[VF_MAXQ]; int nr; };
struct VfThr { double t[VF_MAXQ]; int pos[VF_MAXQ]; int nt; };      // t ascending; pos[q] = place of the caller's q-th threshold in t

__device__ __forceinline__ float vf_s(float d) { return sqrtf(d <= 0.f ? 0.f : d); }      // NaN stays NaN
__device__ __forceinline__ unsigned vf_key(float s) { return __float_as_uint(s) & 0x7fffffffu; }
__device__ __host__ __forceinline__ int vf_shift(int level) { return level == 0 ? 20 : level == 1 ? 13 : level == 2 ? 6 : 0; }
__device__ __host__ __forceinline__ int vf_bits(int level) { return level == 0 ? 11 : level == 3 ? 6 : 7; }

// rows i0 .. i1 - 1 of one thread's slot, four rows' loads in flight before the first is used.  WIDE: the slot lies inside the row and is
// 16-byte aligned (one load); else element loads of the columns that exist
template <bool WIDE, class F>
__device__ __forceinline__ void vf_rows(const VfGeom& g, const int32_t* __restrict__ qlab, long long j0, const bool (&ok)[4], const int32_t (&rl)[4],
                                        int i0, int i1, F& f) {
  for (int ib = i0; ib < i1; ib += 4) {
    float v[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = min(ib + r, i1 - 1);                        // surplus rows of the last batch read the last row again and are dropped
      const float* row = g.D + (size_t)i * g.ld;
      if (WIDE) {
        const float4 t = *reinterpret_cast<const float4*>(row + j0);
        v[r][0] = t.x; v[r][1] = t.y; v[r][2] = t.z; v[r][3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[r][e] = ok[e] ? row[j0 + e] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ib + r;
      if (i < i1) {
        const int32_t ql = qlab[i];
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (WIDE || ok[e]) f(i - i0, v[r][e], rl[e] == ql);
      }
    }
  }
}

// f(r, d, intra): r = row inside the workgroup's 16, d = the block's element as stored
template <bool VEC, class F>
__device__ __forceinline__ void vf_walk(const VfGeom& g, const int32_t* __restrict__ qlab, const int32_t* __restrict__ rlab, F&& f) {
  const unsigned ct = blockIdx.x % g.nct, rc = blockIdx.x / g.nct;
  const long long j0 = ((long long)ct * VF_THREADS + (long long)threadIdx.x) * 4 - g.k;
  bool ok[4];
  int32_t rl[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const long long j = j0 + e;
    ok[e] = j >= 0 && j < (long long)g.n;
    rl[e] = ok[e] ? rlab[j] : 0;
  }
  const int i0 = (int)rc * VF_ROWS, i1 = min(i0 + VF_ROWS, g.m);
  if (VEC && ok[0] && ok[3]) vf_rows<true>(g, qlab, j0, ok, rl, i0, i1, f);
  else vf_rows<false>(g, qlab, j0, ok, rl, i0, i1, f);
}

template <class T>
__device__ __forceinline__ T vf_wave_sum(T v) {
  for (int sh = 1; sh < 64; sh <<= 1) v += __shfl_xor(v, sh, 64);      // butterfly: every lane ends with the same bits
  return v;
}
__device__ __forceinline__ float vf_wave_min(float v) {
  for (int sh = 1; sh < 64; sh <<= 1) v = fminf(v, __shfl_xor(v, sh, 64));
  return v;
}
__device__ __forceinline__ float vf_wave_max(float v) {
  for (int sh = 1; sh < 64; sh <<= 1) v = fmaxf(v, __shfl_xor(v, sh, 64));
  return v;
}
__device__ __forceinline__ unsigned vf_wave_or(unsigned v) {
  for (int sh = 1; sh < 64; sh <<= 1) v |= (unsigned)__shfl_xor((int)v, sh, 64);
  return v;
}

// ---------------------------------------------------------------- pass A
template <bool VEC>
__global__ __launch_bounds__(VF_THREADS) void vf_stats_kernel(VfGeom g, const int32_t* __restrict__ qlab, const int32_t* __restrict__ rlab,
                                                               VfPart* __restrict__ part, int32_t* __restrict__ rowflags, int32_t* __restrict__ nanflag) {
  __shared__ VfPart s_part[VF_THREADS / 64];
  __shared__ unsigned s_bits[VF_THREADS / 64], s_nan[VF_THREADS / 64];
  long long c0 = 0, c1 = 0;
  double a0 = 0.0, a1 = 0.0, q0 = 0.0, q1 = 0.0;
  float mn0 = INFINITY, mn1 = INFINITY, mx0 = 0.f, mx1 = 0.f;
  unsigned bits = 0, nan = 0;                                  // bits: 2r = row r has an intra element, 2r + 1 = an inter element
  vf_walk<VEC>(g, qlab, rlab, [&](int r, float d, bool intra) {
    const float s = vf_s(d);
    const double sd = (double)s;
    nan |= (s != s) ? 1u : 0u;
    if (intra) {
      c0++; a0 += sd; q0 += sd * sd; mn0 = s < mn0 ? s : mn0; mx0 = s > mx0 ? s : mx0; bits |= 1u << (2 * r);
    } else {
      c1++; a1 += sd; q1 += sd * sd; mn1 = s < mn1 ? s : mn1; mx1 = s > mx1 ? s : mx1; bits |= 2u << (2 * r);
    }
  });
  c0 = vf_wave_sum(c0); c1 = vf_wave_sum(c1);
  a0 = vf_wave_sum(a0); a1 = vf_wave_sum(a1); q0 = vf_wave_sum(q0); q1 = vf_wave_sum(q1);
  mn0 = vf_wave_min(mn0); mn1 = vf_wave_min(mn1); mx0 = vf_wave_max(mx0); mx1 = vf_wave_max(mx1);
  bits = vf_wave_or(bits); nan = vf_wave_or(nan);
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  if (lane_id() == 0) {
    VfPart& p = s_part[wave];
    p.cnt[0] = c0; p.cnt[1] = c1; p.sum[0] = a0; p.sum[1] = a1; p.sum2[0] = q0; p.sum2[1] = q1;
    p.mn[0] = mn0; p.mn[1] = mn1; p.mx[0] = mx0; p.mx[1] = mx1;
    s_bits[wave] = bits; s_nan[wave] = nan;
  }
  __syncthreads();
  if (tid == 0) {
    VfPart t = s_part[0];
    for (int w = 1; w < VF_THREADS / 64; w++)
      for (int c = 0; c < 2; c++) {
        t.cnt[c] += s_part[w].cnt[c]; t.sum[c] += s_part[w].sum[c]; t.sum2[c] += s_part[w].sum2[c];
        t.mn[c] = fminf(t.mn[c], s_part[w].mn[c]); t.mx[c] = fmaxf(t.mx[c], s_part[w].mx[c]);
      }
    part[blockIdx.x] = t;
    if (s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3]) atomicOr(nanflag, 1);
  }
  if (tid < VF_ROWS) {
    const int i = (int)(blockIdx.x / g.nct) * VF_ROWS + tid;
    const unsigned b = ((s_bits[0] | s_bits[1] | s_bits[2] | s_bits[3]) >> (2 * tid)) & 3u;
    if (i < g.m && b) atomicOr(&rowflags[i], (int)b);
  }
}

__global__ __launch_bounds__(1024) void vf_stats_final_kernel(const VfPart* __restrict__ part, unsigned nwg, const int32_t* __restrict__ rowflags, int m,
                                                              const int32_t* __restrict__ nanflag, long long* __restrict__ counts,
                                                              double* __restrict__ sums, float* __restrict__ minmax, int32_t* __restrict__ status) {
  __shared__ VfPart s_part[16];
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  VfPart t;
  for (int c = 0; c < 2; c++) { t.cnt[c] = 0; t.sum[c] = 0.0; t.sum2[c] = 0.0; t.mn[c] = INFINITY; t.mx[c] = 0.f; }
  for (unsigned p = (unsigned)tid; p < nwg; p += 1024)
    for (int c = 0; c < 2; c++) {
      t.cnt[c] += part[p].cnt[c]; t.sum[c] += part[p].sum[c]; t.sum2[c] += part[p].sum2[c];
      t.mn[c] = fminf(t.mn[c], part[p].mn[c]); t.mx[c] = fmaxf(t.mx[c], part[p].mx[c]);
    }
  int bad = 0;
  for (int i = tid; i < m; i += 1024) bad |= rowflags[i] != 3;
  for (int c = 0; c < 2; c++) {
    t.cnt[c] = vf_wave_sum(t.cnt[c]); t.sum[c] = vf_wave_sum(t.sum[c]); t.sum2[c] = vf_wave_sum(t.sum2[c]);
    t.mn[c] = vf_wave_min(t.mn[c]); t.mx[c] = vf_wave_max(t.mx[c]);
  }
  if (lane_id() == 0) s_part[wave] = t;
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    t = s_part[0];
    for (int w = 1; w < 16; w++)
      for (int c = 0; c < 2; c++) {
        t.cnt[c] += s_part[w].cnt[c]; t.sum[c] += s_part[w].sum[c]; t.sum2[c] += s_part[w].sum2[c];
        t.mn[c] = fminf(t.mn[c], s_part[w].mn[c]); t.mx[c] = fmaxf(t.mx[c], s_part[w].mx[c]);
      }
    counts[0] = t.cnt[0]; counts[1] = t.cnt[1];
    sums[0] = t.sum[0]; sums[1] = t.sum2[0]; sums[2] = t.sum[1]; sums[3] = t.sum2[1];
    minmax[0] = t.mn[0]; minmax[1] = t.mx[0]; minmax[2] = t.mn[1]; minmax[3] = t.mx[1];
    status[0] = bad ? 1 : 0;
    status[1] = nanflag[0] ? 1 : 0;
  }
}

// ---------------------------------------------------------------- pass B
template <bool VEC>
__global__ __launch_bounds__(VF_THREADS) void vf_select_l0_kernel(VfGeom g, const int32_t* __restrict__ qlab, const int32_t* __restrict__ rlab,
                                                                   unsigned long long* __restrict__ ghist) {
  __shared__ unsigned s_h[VF_L0_BINS];
  for (int b = (int)threadIdx.x; b < VF_L0_BINS; b += VF_THREADS) s_h[b] = 0;
  __syncthreads();
  vf_walk<VEC>(g, qlab, rlab, [&](int, float d, bool intra) {
    if (!intra) atomicAdd(&s_h[vf_key(vf_s(d)) >> 20], 1u);
  });
  __syncthreads();
  for (int b = (int)threadIdx.x; b < VF_L0_BINS; b += VF_THREADS) {
    const unsigned c = s_h[b];
    if (c) atomicAdd(&ghist[b], (unsigned long long)c);
  }
}

template <bool VEC>
__global__ __launch_bounds__(VF_THREADS) void vf_select_lx_kernel(VfGeom g, const int32_t* __restrict__ qlab, const int32_t* __restrict__ rlab, int level,
                                                                   const VfSel* __restrict__ st, unsigned long long* __restrict__ ghist) {
  __shared__ unsigned s_pre[VF_MAXQ];
  __shared__ unsigned s_h[VF_MAXQ * VF_LX_BINS];
  const int nslot = (int)st->nslot;                             // 1 .. 64
  const int nb = 1 << vf_bits(level), pshift = vf_shift(level - 1), shift = vf_shift(level);
  if ((int)threadIdx.x < nslot) s_pre[threadIdx.x] = st->prefix[threadIdx.x];
  for (int b = (int)threadIdx.x; b < nslot * nb; b += VF_THREADS) s_h[b] = 0;
  __syncthreads();
  const unsigned plo = s_pre[0], phi = s_pre[nslot - 1];
  vf_walk<VEC>(g, qlab, rlab, [&](int, float d, bool intra) {
    if (intra) return;
    const unsigned key = vf_key(vf_s(d)), p = key >> pshift;
    if (p < plo || p > phi) return;
    int lo = 0, hi = nslot;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_pre[mid] < p) lo = mid + 1; else hi = mid;
    }
    if (lo < nslot && s_pre[lo] == p) atomicAdd(&s_h[lo * nb + (int)((key >> shift) & (unsigned)(nb - 1))], 1u);
  });
  __syncthreads();
  for (int b = (int)threadIdx.x; b < nslot * nb; b += VF_THREADS) {
    const unsigned c = s_h[b];
    if (c) atomicAdd(&ghist[b], (unsigned long long)c);
  }
}

// one workgroup of 64 threads, thread r = rank r: walk the level's histogram, extend the prefix, renumber the distinct prefixes
__global__ __launch_bounds__(64) void vf_select_scan_kernel(int level, VfRanks ranks, const unsigned long long* __restrict__ ghist, VfSel* __restrict__ st,
                                                            float* __restrict__ values, int32_t* __restrict__ status) {
  __shared__ unsigned long long s_h[VF_L0_BINS];
  __shared__ unsigned s_p[VF_MAXQ];
  __shared__ int s_first[VF_MAXQ];
  const int r = (int)threadIdx.x, nr = ranks.nr;
  const int nb = 1 << vf_bits(level);
  if (level == 0)
    for (int b = r; b < VF_L0_BINS; b += 64) s_h[b] = ghist[b];
  __syncthreads();
  unsigned P = 0;
  long long k = 0;
  int bad = 0;
  if (r < nr) {
    const unsigned slot = level == 0 ? 0u : st->slot[r];
    const unsigned base = level == 0 ? 0u : st->prefix[slot];
    k = level == 0 ? ranks.r[r] : st->krem[r];
    unsigned long long cum = 0, before = 0;
    int sel = -1;
    for (int b = 0; b < nb; b++) {
      const unsigned long long c = level == 0 ? s_h[b] : ghist[(size_t)slot * nb + b];
      if (sel < 0 && cum + c > (unsigned long long)k) { sel = b; before = cum; }
      cum += c;
    }
    if (sel < 0) { bad = 1; sel = 0; before = 0; k = 0; }       // rank >= number of inter elements (only possible at level 0)
    P = (base << vf_bits(level)) | (unsigned)sel;
    k -= (long long)before;
    s_p[r] = P;
  }
  bad = __syncthreads_or(bad | (level > 0 ? st->bad : 0));
  if (r < nr) {
    int first = 1;
    for (int q = 0; q < r; q++) first &= s_p[q] != P;
    s_first[r] = first;
  }
  __syncthreads();
  if (r < nr) {
    unsigned slot = 0;
    for (int q = 0; q < nr; q++) slot += (s_first[q] && s_p[q] < P) ? 1u : 0u;
    st->slot[r] = slot;
    st->prefix[slot] = P;                                       // every rank of a prefix writes the same value
    st->krem[r] = k;
    if (level == 3) values[r] = bad ? __uint_as_float(0x7fc00000u) : __uint_as_float(P);
  }
  if (r == 0) {
    unsigned ns = 0;
    for (int q = 0; q < nr; q++) ns += s_first[q] ? 1u : 0u;
    st->nslot = ns;
    st->bad = bad;
    if (level == 3) status[0] = bad;
  }
}

// ---------------------------------------------------------------- pass C
// bucket of an element = number of thresholds <= s (0 .. nt).  Buckets 0 and nt (below / not below every threshold: most of the block)
// are counted in registers, the others in LDS.  NaN elements count for the class totals only (every comparison with NaN is false).
template <bool VEC, bool SQ>
__global__ __launch_bounds__(VF_THREADS) void vf_count_kernel(VfGeom g, const int32_t* __restrict__ qlab, const int32_t* __restrict__ rlab, VfThr thr,
                                                               unsigned long long* __restrict__ gbins) {      // [2][VF_MAXQ + 1] buckets, then [2] totals
  __shared__ double s_t[VF_MAXQ];
  __shared__ unsigned s_h[2][VF_MAXQ + 1];
  __shared__ unsigned s_tot[2];
  const int nt = thr.nt, tid = (int)threadIdx.x;
  if (tid < nt) s_t[tid] = thr.t[tid];
  if (tid < 2 * (VF_MAXQ + 1)) (&s_h[0][0])[tid] = 0;
  if (tid < 2) s_tot[tid] = 0;
  __syncthreads();
  const double tlo = s_t[0], thi = s_t[nt - 1];
  unsigned lo0 = 0, lo1 = 0, hi0 = 0, hi1 = 0, n0 = 0, n1 = 0;
  vf_walk<VEC>(g, qlab, rlab, [&](int, float d, bool intra) {
    const double s = (double)(SQ ? vf_s(d) : d);
    if (intra) n0++; else n1++;
    if (s != s) return;
    if (s >= thi) { if (intra) hi0++; else hi1++; return; }
    if (s < tlo) { if (intra) lo0++; else lo1++; return; }
    int lo = 0, hi = nt;                                        // first k with t[k] > s
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_t[mid] <= s) lo = mid + 1; else hi = mid;
    }
    atomicAdd(&s_h[intra ? 0 : 1][lo], 1u);
  });
  lo0 = vf_wave_sum(lo0); lo1 = vf_wave_sum(lo1); hi0 = vf_wave_sum(hi0); hi1 = vf_wave_sum(hi1); n0 = vf_wave_sum(n0); n1 = vf_wave_sum(n1);
  if (lane_id() == 0) {
    if (lo0) atomicAdd(&s_h[0][0], lo0);
    if (lo1) atomicAdd(&s_h[1][0], lo1);
    if (hi0) atomicAdd(&s_h[0][nt], hi0);
    if (hi1) atomicAdd(&s_h[1][nt], hi1);
    atomicAdd(&s_tot[0], n0);
    atomicAdd(&s_tot[1], n1);
  }
  __syncthreads();
  if (tid < 2 * (VF_MAXQ + 1)) {
    const unsigned c = (&s_h[0][0])[tid];
    if (c) atomicAdd(&gbins[tid], (unsigned long long)c);
  }
  if (tid < 2 && s_tot[tid]) atomicAdd(&gbins[2 * (VF_MAXQ + 1) + tid], (unsigned long long)s_tot[tid]);
}

__global__ __launch_bounds__(64) void vf_count_final_kernel(VfThr thr, const unsigned long long* __restrict__ gbins, long long* __restrict__ counts,
                                                            long long* __restrict__ totals) {
  const int q = (int)threadIdx.x, nt = thr.nt;
  if (q < nt) {
    const int k = thr.pos[q];
    unsigned long long intra_lt = 0, inter_lt = 0, intra_ge = 0;
    for (int b = 0; b <= nt; b++) {
      const unsigned long long h0 = gbins[b], h1 = gbins[VF_MAXQ + 1 + b];
      if (b <= k) { intra_lt += h0; inter_lt += h1; } else intra_ge += h0;
    }
    counts[q] = (long long)intra_ge;
    counts[nt + q] = (long long)inter_lt;
    counts[2 * nt + q] = (long long)intra_lt;
  }
  if (q < 2) totals[q] = (long long)gbins[2 * (VF_MAXQ + 1) + q];
}

__global__ void vf_sqrt_kernel(const float* __restrict__ d, int n, float* __restrict__ s) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) s[i] = vf_s(d[i]);
}

}  // namespace ssg

using namespace ssg;

// workspace layout (bytes): [0, 64 * nwg) partials | rowflags int32[m] (padded to 8) | 8: nanflag | VfSel | histogram / bins 64 KiB
struct VfLayout { size_t nwg, off_rows, off_nan, off_sel, off_hist, total; };

static VfLayout vf_layout(int m, int n) {
  VfLayout l;
  const size_t slots = ((size_t)n + 3 + 3) / 4;                                   // misalignment k <= 3
  const size_t nct = (slots + VF_THREADS - 1) / VF_THREADS, nrc = ((size_t)m + VF_ROWS - 1) / VF_ROWS;
  l.nwg = nct * nrc;
  l.off_rows = l.nwg * sizeof(VfPart);
  l.off_nan = l.off_rows + (((size_t)m * 4 + 7) & ~(size_t)7);
  l.off_sel = l.off_nan + 8;
  l.off_hist = l.off_sel + ((sizeof(VfSel) + 7) & ~(size_t)7);
  l.total = l.off_hist + (size_t)VF_MAXQ * VF_LX_BINS * 8;
  return l;
}

static int vf_check(const char* fn, const float* D, int m, int n, size_t ld, const int32_t* qlab, const int32_t* rlab, const void* ws, size_t ws_bytes,
                    VfGeom* g) {
  if (m < 1 || n < 1) { ssg_set_error("%s: empty block m=%d n=%d", fn, m, n); return SSG_ERR_INVALID; }
  if (ld < (size_t)n) { ssg_set_error("%s: row pitch ld=%zu < n=%d", fn, ld, n); return SSG_ERR_INVALID; }
  const VfLayout l = vf_layout(m, n);
  if (l.nwg > 0x7fffffffull) { ssg_set_error("%s: m=%d n=%d needs %zu workgroups (> 2^31 - 1)", fn, m, n, l.nwg); return SSG_ERR_INVALID; }
  if (!D || !qlab || !rlab || !ws) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  if (((uintptr_t)D & 3) || ((uintptr_t)ws & 7)) { ssg_set_error("%s: D must be 4-byte and the workspace 8-byte aligned", fn); return SSG_ERR_INVALID; }
  if (ws_bytes < l.total) { ssg_set_error("%s: workspace of %zu bytes, ssg_verify_workspace_bytes(%d, %d) = %zu", fn, ws_bytes, m, n, l.total); return SSG_ERR_INVALID; }
  g->D = D; g->ld = ld; g->m = m; g->n = n;
  g->vec = (ld % 4 == 0) ? 1 : 0;
  g->k = g->vec ? (int)(((uintptr_t)D >> 2) & 3) : 0;
  g->nct = (unsigned)((((size_t)n + g->k + 3) / 4 + VF_THREADS - 1) / VF_THREADS);
  return SSG_OK;
}

static unsigned vf_grid(const VfGeom& g) { return g.nct * (unsigned)((g.m + VF_ROWS - 1) / VF_ROWS); }

extern "C" size_t ssg_verify_workspace_bytes(int m, int n) {
  if (m < 1 || n < 1) return 0;
  return vf_layout(m, n).total;
}

extern "C" int ssg_verify_stats_f32(const float* D, int m, int n, size_t ld, const int32_t* qlab, const int32_t* rlab, void* ws, size_t ws_bytes,
                                    int64_t* counts, double* sums, float* minmax, int32_t* status, hipStream_t stream) {
  const char* fn = "ssg_verify_stats_f32";
  VfGeom g;
  if (int rc = vf_check(fn, D, m, n, ld, qlab, rlab, ws, ws_bytes, &g)) return rc;
  if (!counts || !sums || !minmax || !status) { ssg_set_error("%s: NULL output", fn); return SSG_ERR_INVALID; }
  const VfLayout l = vf_layout(m, n);
  char* w = (char*)ws;
  VfPart* part = (VfPart*)w;
  int32_t* rowflags = (int32_t*)(w + l.off_rows);
  int32_t* nanflag = (int32_t*)(w + l.off_nan);
  SSG_HIP(hipMemsetAsync(rowflags, 0, l.off_sel - l.off_rows, stream));
  const unsigned grid = vf_grid(g);
  if (g.vec) hipLaunchKernelGGL(vf_stats_kernel<true>, dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, part, rowflags, nanflag);
  else hipLaunchKernelGGL(vf_stats_kernel<false>, dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, part, rowflags, nanflag);
  SSG_LAUNCH_CHECK("vf_stats_kernel");
  hipLaunchKernelGGL(vf_stats_final_kernel, dim3(1), dim3(1024), 0, stream, part, grid, rowflags, m, nanflag, (long long*)counts, sums, minmax, status);
  SSG_LAUNCH_CHECK("vf_stats_final_kernel");
  return SSG_OK;
}

extern "C" int ssg_verify_select_f32(const float* D, int m, int n, size_t ld, const int32_t* qlab, const int32_t* rlab, const int64_t* ranks_host, int nr,
                                     void* ws, size_t ws_bytes, float* values, int32_t* status, hipStream_t stream) {
  const char* fn = "ssg_verify_select_f32";
  VfGeom g;
  if (nr < 1 || nr > VF_MAXQ) { ssg_set_error("%s: %d ranks, 1 .. %d per call", fn, nr, VF_MAXQ); return SSG_ERR_INVALID; }
  if (!ranks_host) { ssg_set_error("%s: NULL ranks", fn); return SSG_ERR_INVALID; }
  VfRanks ranks;
  ranks.nr = nr;
  for (int r = 0; r < VF_MAXQ; r++) ranks.r[r] = r < nr ? (long long)ranks_host[r] : 0;
  for (int r = 0; r < nr; r++)
    if (ranks.r[r] < 0) { ssg_set_error("%s: rank[%d]=%lld is negative", fn, r, ranks.r[r]); return SSG_ERR_INVALID; }
  if (int rc = vf_check(fn, D, m, n, ld, qlab, rlab, ws, ws_bytes, &g)) return rc;
  if (!values || !status) { ssg_set_error("%s: NULL output", fn); return SSG_ERR_INVALID; }
  const VfLayout l = vf_layout(m, n);
  char* w = (char*)ws;
  VfSel* st = (VfSel*)(w + l.off_sel);
  unsigned long long* hist = (unsigned long long*)(w + l.off_hist);
  const size_t hist_bytes = (size_t)VF_MAXQ * VF_LX_BINS * 8;
  const unsigned grid = vf_grid(g);
  for (int level = 0; level < 4; level++) {
    SSG_HIP(hipMemsetAsync(hist, 0, hist_bytes, stream));
    if (level == 0) {
      if (g.vec) hipLaunchKernelGGL(vf_select_l0_kernel<true>, dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, hist);
      else hipLaunchKernelGGL(vf_select_l0_kernel<false>, dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, hist);
    } else {
      if (g.vec) hipLaunchKernelGGL(vf_select_lx_kernel<true>, dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, level, st, hist);
      else hipLaunchKernelGGL(vf_select_lx_kernel<false>, dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, level, st, hist);
    }
    SSG_LAUNCH_CHECK("vf_select kernel");
    hipLaunchKernelGGL(vf_select_scan_kernel, dim3(1), dim3(64), 0, stream, level, ranks, hist, st, values, status);
    SSG_LAUNCH_CHECK("vf_select_scan_kernel");
  }
  return SSG_OK;
}

extern "C" int ssg_verify_count_f32(const float* D, int m, int n, size_t ld, const int32_t* qlab, const int32_t* rlab, int is_sq, const double* thr_host,
                                    int nt, void* ws, size_t ws_bytes, int64_t* counts, int64_t* totals, hipStream_t stream) {
  const char* fn = "ssg_verify_count_f32";
  VfGeom g;
  if (nt < 1 || nt > VF_MAXQ) { ssg_set_error("%s: %d thresholds, 1 .. %d per call", fn, nt, VF_MAXQ); return SSG_ERR_INVALID; }
  if (!thr_host) { ssg_set_error("%s: NULL thresholds", fn); return SSG_ERR_INVALID; }
  for (int q = 0; q < nt; q++)
    if (thr_host[q] != thr_host[q]) { ssg_set_error("%s: threshold[%d] is NaN", fn, q); return SSG_ERR_INVALID; }
  if (int rc = vf_check(fn, D, m, n, ld, qlab, rlab, ws, ws_bytes, &g)) return rc;
  if (!counts || !totals) { ssg_set_error("%s: NULL output", fn); return SSG_ERR_INVALID; }
  VfThr thr;
  int order[VF_MAXQ];
  for (int q = 0; q < nt; q++) order[q] = q;
  std::stable_sort(order, order + nt, [&](int a, int b) { return thr_host[a] < thr_host[b]; });
  thr.nt = nt;
  for (int k = 0; k < VF_MAXQ; k++) { thr.t[k] = 0.0; thr.pos[k] = 0; }
  for (int k = 0; k < nt; k++) { thr.t[k] = thr_host[order[k]]; thr.pos[order[k]] = k; }
  // (equal thresholds need no care: bucket b holds the elements with exactly b thresholds <= s, so the buckets between the places of a
  // run of equal thresholds stay empty)
  const VfLayout l = vf_layout(m, n);
  unsigned long long* bins = (unsigned long long*)((char*)ws + l.off_hist);
  SSG_HIP(hipMemsetAsync(bins, 0, (2 * (VF_MAXQ + 1) + 2) * 8, stream));
  const unsigned grid = vf_grid(g);
  if (g.vec) {
    if (is_sq) hipLaunchKernelGGL((vf_count_kernel<true, true>), dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, thr, bins);
    else hipLaunchKernelGGL((vf_count_kernel<true, false>), dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, thr, bins);
  } else {
    if (is_sq) hipLaunchKernelGGL((vf_count_kernel<false, true>), dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, thr, bins);
    else hipLaunchKernelGGL((vf_count_kernel<false, false>), dim3(grid), dim3(VF_THREADS), 0, stream, g, qlab, rlab, thr, bins);
  }
  SSG_LAUNCH_CHECK("vf_count_kernel");
  hipLaunchKernelGGL(vf_count_final_kernel, dim3(1), dim3(64), 0, stream, thr, bins, (long long*)counts, (long long*)totals);
  SSG_LAUNCH_CHECK("vf_count_final_kernel");
  return SSG_OK;
}

extern "C" int ssg_selftest_verify_sqrt(const float* d, int n, float* s, hipStream_t stream) {
  if (n < 1 || !d || !s) { ssg_set_error("ssg_selftest_verify_sqrt: n=%d or NULL pointer", n); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(vf_sqrt_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d, n, s);
  SSG_LAUNCH_CHECK("vf_sqrt_kernel");
  return SSG_OK;
}
