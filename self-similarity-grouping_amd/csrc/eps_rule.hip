// eps_rule.hip -- K10 (epsilon rule).
//
// K10 replaces selftraining.py:289-293:
//   tri = triu(dist, 1); tri = tri[nonzero(tri)]; tri = sort(tri)
//   eps = tri[:round(rho * tri.size)].mean()
// as a 12-bit-digit radix select over the monotone u64 patterns of the (positive) float64
// distances, a compaction of everything at or below the selected digit, a bitonic sort of
// that small set (sort_u64.hip) and numpy's pairwise-summation mean -- bit-identical to np.mean.
// The fast path ("K10, fast path" below) replaces the radix select by a sampled threshold and ONE full pass, verified a posteriori.
#include "matview.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace ssg {

// ------------------------------------------------------------------ K10 histogram level
// hist[bin] += #{ (i<k), d != 0, (key >> (shift+width)) == prefix }, bin = (key>>shift) & mask.
// hist[4096] += number of non-zero strict-upper entries (only when count_nonzero != 0).
template <int MODE>
__global__ __launch_bounds__(256) void eps_hist_kernel(MatView mv, unsigned long long prefix, int shift, int width, int count_nonzero,
                                                       unsigned long long* __restrict__ hist) {
  __shared__ unsigned int lh[4096];
  __shared__ unsigned long long lnz;
  for (int b = (int)threadIdx.x; b < 4096; b += 256) lh[b] = 0;
  if (threadIdx.x == 0) lnz = 0;
  __syncthreads();
  const int lane = lane_id();
  const unsigned mask = (1u << width) - 1u;
  const bool anyprefix = (shift + width) >= 63;   // top level: no prefix to match
  unsigned long long nz = 0;
  for (int il = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); il < mv.nrows; il += (int)gridDim.x * 4) {
    const int gi = mv.row0 + il;
    RowStream rs(il, mv.N, mv.nrows);
    // strict upper triangle: columns k > gi only -> skip leading chunks
    int c0 = (rs.first + gi + 1) / 512;
    const hbits vi = MODE == 0 ? mv.v[gi] : (hbits)0;
    for (int cb = c0; cb < rs.nchunks; cb += PIPE) {
      RawChunk raw[PIPE];
      if (MODE != 2) {
#pragma unroll
        for (int u = 0; u < PIPE; u++) raw[u] = load_raw<MODE == 2 ? 1 : MODE>(mv, rs, cb + u, lane);
      }
#pragma unroll
      for (int u = 0; u < PIPE; u++) {
        const int c = cb + u;
        if (c >= rs.nchunks) break;
        double dv[8];
        if (MODE == 2) load_vals<MODE>(mv, rs, c, lane, gi, dv);
        else decode_raw<MODE == 2 ? 1 : MODE>(mv, raw[u], vi, dv);
        const int j0 = rs.col0(c, lane);
        int pbin = -1; unsigned pcnt = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = j0 + e;
          if (k > gi && k < mv.N) {
            const double d = dv[e];
            if (d != 0.0) {
              nz++;
              const unsigned long long key = (unsigned long long)__double_as_longlong(d);
              if (anyprefix || (key >> (shift + width)) == prefix) {
                const int bin = (int)((key >> shift) & mask);
                if (bin == pbin) pcnt++;
                else { if (pcnt) atomicAdd(&lh[pbin], pcnt); pbin = bin; pcnt = 1; }
              }
            }
          }
        }
        // the bulk of a row falls into one bin: one add per wave instead of 64
        const int fb = __shfl(pbin, 0, 64);
        if (__all(pbin == fb)) {
          unsigned tot = pcnt;
          for (int sh = 1; sh < 64; sh <<= 1) tot += (unsigned)__shfl_xor((int)tot, sh, 64);
          if (lane == 0 && fb >= 0 && tot) atomicAdd(&lh[fb], tot);
        } else if (pcnt) atomicAdd(&lh[pbin], pcnt);
      }
    }
  }
  for (int sh = 1; sh < 64; sh <<= 1) nz += (unsigned long long)__shfl_xor((long long)nz, sh, 64);
  if (lane == 0 && nz) atomicAdd(&lnz, nz);
  __syncthreads();
  for (int b = (int)threadIdx.x; b < 4096; b += 256) if (lh[b]) atomicAdd(&hist[b], (unsigned long long)lh[b]);
  if (threadIdx.x == 0 && count_nonzero && lnz) atomicAdd(&hist[4096], lnz);
}

// append every strict-upper non-zero key <= key_max to buf
template <int MODE>
__global__ __launch_bounds__(256) void eps_compact_kernel(MatView mv, unsigned long long key_max, unsigned long long* __restrict__ buf,
                                                          unsigned long long cap, unsigned long long* __restrict__ cursor) {
  __shared__ unsigned long long sbuf[4][STAGE_CAP];
  const int lane = lane_id();
  WaveStage<unsigned long long> st{sbuf[threadIdx.x >> 6], 0};
  for (int il = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); il < mv.nrows; il += (int)gridDim.x * 4) {
    const int gi = mv.row0 + il;
    RowStream rs(il, mv.N, mv.nrows);
    int c0 = (rs.first + gi + 1) / 512;
    const hbits vi = MODE == 0 ? mv.v[gi] : (hbits)0;
    for (int cb = c0; cb < rs.nchunks; cb += PIPE) {
      RawChunk raw[PIPE];
      if (MODE != 2) {
#pragma unroll
        for (int u = 0; u < PIPE; u++) raw[u] = load_raw<MODE == 2 ? 1 : MODE>(mv, rs, cb + u, lane);
      }
#pragma unroll
      for (int u = 0; u < PIPE; u++) {
        const int c = cb + u;
        if (c >= rs.nchunks) break;
        double dv[8];
        if (MODE == 2) load_vals<MODE>(mv, rs, c, lane, gi, dv);
        else decode_raw<MODE == 2 ? 1 : MODE>(mv, raw[u], vi, dv);
        const int j0 = rs.col0(c, lane);
        unsigned long long keys[8]; int n = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = j0 + e;
          keys[e] = ~0ULL;
          if (k > gi && k < mv.N) {
            const double d = dv[e];
            const unsigned long long key = (unsigned long long)__double_as_longlong(d);
            if (d != 0.0 && key <= key_max) { keys[e] = key; n++; }
          }
        }
        if (!__any(n > 0)) continue;
        int incl = n;
        for (int sh = 1; sh < 64; sh <<= 1) { const int o = __shfl_up(incl, sh, 64); if (lane >= sh) incl += o; }
        const int tot = __shfl(incl, 63, 64);
        int w = st.n + incl - n;
#pragma unroll
        for (int e = 0; e < 8; e++) if (keys[e] != ~0ULL) st.buf[w++] = keys[e];
        st.n += tot;
        if (st.n > STAGE_CAP - 512) st.flush(buf, cap, cursor, lane);
      }
    }
  }
  block_flush(st, buf, cap, cursor);
}

// ------------------------------------------------------------------ K10, fast path: sampled threshold + ONE full pass
// The radix select above costs two or three N^2 passes that each rebuild the float64 value of every element.  The fast path
// estimates the rho-quantile from a strided sample of rows (a few MB), turns it into a float32 threshold with a safety margin,
// and makes ONE pass over the strict upper triangle that (a) counts the exact zeros and (b) collects the exact float64 keys of
// the elements whose float32 SURROGATE value is below the threshold.  The host then sorts the collected keys and checks that
// the top-th smallest exact key lies below the threshold by more than the surrogate's error bound: in that case no
// uncollected element can be among the `top` smallest and the result is exactly the reference's; otherwise (a sample that
// underestimated the quantile) it falls back to the radix select.  Correctness never depends on the sample, only speed does.
//
// surrogate: float32 evaluation of the element (mode 0: jp + half(v_i+v_k)*lambda with float32 ops; modes 1/2: the value
// rounded to float32): |surrogate - exact| <= 4e-7 * (1 + |exact|) for the values that occur (final_dist < 4).
__device__ __forceinline__ int sur_bin(float x) {
  // 4096 bins over the float32 bit pattern: 16 binades [2^-14, 4) x 256 mantissa steps (0.4 % per bin); monotone in x >= 0
  const int b = (int)(__float_as_uint(x) >> 15) - 0x7100;
  return b < 0 ? 0 : (b > 4095 ? 4095 : b);
}
__device__ __forceinline__ float sur_bin_upper(int b) { return __uint_as_float((unsigned)(b + 1 + 0x7100) << 15); }   // exclusive upper edge of bin b

// raw half chunk -> 8 surrogate values (+ exact-zero mask for mode 0/1)
template <int MODE>
__device__ __forceinline__ void surrogate8(const MatView& mv, const RawChunk& r, hbits vi, float lam32, float sv[8], unsigned& zeromask) {
  const unsigned w[4] = {r.m.x, r.m.y, r.m.z, r.m.w}, vw[4] = {r.v.x, r.v.y, r.v.z, r.v.w};
  zeromask = 0;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const hbits raw = (hbits)((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
    if (MODE == 0) {
      const hbits s = h_add((hbits)((vw[e >> 1] >> ((e & 1) * 16)) & 0xffffu), vi);
      const float p = h2f(s) * lam32;
      sv[e] = h2f(raw) + p;
      // exact value 0 <=> J' == +-0 and half(v_i+v_k)*lambda == 0 (all terms are finite and the sum of two non-zero terms of
      // opposite sign is decided exactly below, on the rare candidates only)
      if ((raw & 0x7fffu) == 0 && ((s & 0x7fffu) == 0 || mv.lambda_value == 0.0)) zeromask |= 1u << e;
    } else {
      sv[e] = h2f(raw);
      if ((raw & 0x7fffu) == 0) zeromask |= 1u << e;
    }
  }
}

// sample histogram: local rows 0, stride, 2*stride, ...; strict upper triangle, exact zeros dropped; hist[4096] = sample size
// refine != nullptr: second level -- only the sample elements of coarse bin refine[2] are counted, in 1024 linear sub-bins of
// that bin's float range (hist[0..1023]); the coarse bins are 0.4 % wide, which on a dense value distribution is far more than
// the quantile margin and would blow the candidate set up
constexpr int SPARTS = 8;
// both selection levels for a 256-thread workgroup (the bodies of eps_select_kernel / eps_select2_kernel below, which stay the two-launch
// API): level 1 = first bin whose cumulative count reaches ceil(q * sample size), threshold = upper edge of the next bin, sel = {threshold
// bits, sample size, bin, sample elements below the bin, target}; level 2 = the sub-bin of coarse bin sel[2] where sel[3] + sub-bins reach
// sel[4], threshold = upper edge of the sub-bin after it.  `part` = 4097 words of LDS scratch.  Histogram words are read with agent-scope loads.
__device__ __forceinline__ void eps_select_block(const unsigned long long* __restrict__ hist, double q, unsigned long long* __restrict__ sel, bool level2,
                                                 unsigned int* part) {
  const int t = (int)threadIdx.x;
  // the histogram words were produced by device-scope atomics of workgroups on every XCD: read them past this CU's L1 and this XCD's L2
  // (sc0 sc1).  As plain buffer loads, not as atomic loads: hipcc waits for every relaxed atomic load before it issues the next one -- 16
  // dependent memory round trips per thread made the launch that carries the selection 45 us instead of 11 (rocprofv3, N = 16 000)
  typedef unsigned int v2u_ __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t hr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(hist), 0, 4097 * 8, 0x00020000);
  auto ld = [&](int b) -> unsigned long long {
    const v2u_ x = __builtin_amdgcn_raw_buffer_load_b64(hr, b * 8, 0, 17);
    return (unsigned long long)x[0] | ((unsigned long long)x[1] << 32);
  };
  const int nb = level2 ? 4 : 16, b0 = t * nb;                     // bins per thread: 1024 / 256 or 4096 / 256
  unsigned long long c[16], mine = 0;
#pragma unroll
  for (int u = 0; u < 16; u++) { c[u] = u < nb ? ld(b0 + u) : 0ull; mine += c[u]; }
  // exclusive prefix of the 256 per-thread sums (counts fit 32 bits: a sample holds < 2^32 elements)
  __syncthreads();
  part[t] = (unsigned int)mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned int add = t >= o ? part[t - o] : 0u;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  unsigned long long run = (unsigned long long)part[t] - mine;
  if (!level2) {
    const unsigned long long total = ld(4096);
    unsigned long long target = (unsigned long long)ceil(q * (double)total);
    if (target < 64) target = 64;
    __shared__ int bsel; __shared__ unsigned long long bbefore;
    if (t == 0) { bsel = 4096; bbefore = 0; }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const unsigned long long before = run;
      run += c[u];
      if (before < target && run >= target) { bsel = b0 + u; bbefore = before; }      // unique
    }
    __syncthreads();
    if (t == 0) {
      const int b = bsel;
      float thr = b >= 4094 ? __uint_as_float(0x7f800000u) : sur_bin_upper(b + 1);
      if (total == 0) thr = __uint_as_float(0x7f800000u);
      sel[0] = (unsigned long long)__float_as_uint(thr); sel[1] = total; sel[2] = (unsigned long long)b;
      sel[3] = b >= 4096 ? 0ull : bbefore; sel[4] = target;
    }
  } else {
    const int b = (int)sel[2];
    if (b < 1 || b >= 4094) return;                    // degenerate / open-ended bins keep the coarse threshold
    const unsigned long long before0 = sel[3], target = sel[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned long long excl = before0 + run, incl = excl + c[u];
      run += c[u];
      if (excl < target && incl >= target) {
        const float lo = sur_bin_upper(b - 1), hi = sur_bin_upper(b);
        const float thr = lo + (float)(b0 + u + 2) * ((hi - lo) * (1.f / 1024.f));
        sel[0] = (unsigned long long)__float_as_uint(thr < sur_bin_upper(b + 1) ? thr : sur_bin_upper(b + 1));
      }
    }
  }
}
template <int MODE>
__global__ __launch_bounds__(256) void eps_sample_hist_kernel(MatView mv, int stride, const unsigned long long* __restrict__ refine,
                                                              unsigned long long* __restrict__ hist, double q = 0.0, unsigned long long* __restrict__ sel = nullptr,
                                                              unsigned int* __restrict__ ticket = nullptr) {
  __shared__ unsigned int lh[4097];
  for (int b = (int)threadIdx.x; b < 4097; b += 256) lh[b] = 0;
  __syncthreads();
  const int lane = lane_id();
  const float lam32 = (float)mv.lambda_value;
  const int rbin = refine ? (int)refine[2] : -1;
  const float rlo = rbin > 0 ? sur_bin_upper(rbin - 1) : 0.f, rhi = rbin >= 0 ? sur_bin_upper(rbin) : 1.f;
  const float rinv = 1024.f / (rhi - rlo);
  const int nsamp = (mv.nrows + stride - 1) / stride;
  // a sample row is shared by SPARTS waves (chunks round-robin): 192 rows alone leave the launch at one wave per CU and latency-bound
  for (int widx = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); widx < nsamp * SPARTS; widx += (int)gridDim.x * 4) {
    const int sidx = widx / SPARTS, part = widx - sidx * SPARTS;
    const int il = sidx * stride, gi = mv.row0 + il;
    RowStream rs(il, mv.N, mv.nrows);
    const hbits vi = MODE == 0 ? mv.v[gi] : (hbits)0;
    unsigned cnt = 0;
    for (int c = (rs.first + gi + 1) / 512 + part; c < rs.nchunks; c += SPARTS) {
      float sv[8]; unsigned zm = 0;
      const int j0 = rs.col0(c, lane);
      if (MODE == 2) {
        double dv[8];
        load_vals<MODE>(mv, rs, c, lane, gi, dv);
#pragma unroll
        for (int e = 0; e < 8; e++) { sv[e] = (float)dv[e]; if (dv[e] == 0.0) zm |= 1u << e; }
      } else {
        const RawChunk raw = load_raw<MODE == 2 ? 1 : MODE>(mv, rs, c, lane);
        surrogate8<MODE == 2 ? 1 : MODE>(mv, raw, vi, lam32, sv, zm);
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int k = j0 + e;
        if (k > gi && k < mv.N && !((zm >> e) & 1u)) {
          const int b = sur_bin(sv[e]);
          if (!refine) { atomicAdd(&lh[b], 1u); cnt++; }
          else if (b == rbin) {
            int sb = (int)((sv[e] - rlo) * rinv);
            sb = sb < 0 ? 0 : (sb > 1023 ? 1023 : sb);
            atomicAdd(&lh[sb], 1u); cnt++;
          }
        }
      }
    }
    for (int sh = 1; sh < 64; sh <<= 1) cnt += (unsigned)__shfl_xor((int)cnt, sh, 64);
    if (lane == 0 && cnt) atomicAdd(&lh[4096], cnt);
  }
  __syncthreads();
  for (int b = (int)threadIdx.x; b < 4097; b += 256) if (lh[b]) atomicAdd(&hist[b], (unsigned long long)lh[b]);
  if (!sel) return;
  // ---- round 6: the threshold selection rides in this launch.  The workgroup that draws the last ticket has every other workgroup's
  // histogram atomics behind it (they are device-scope read-modify-writes at the memory side; the agent-scope loads of the selection
  // by-pass this CU's L1 and its XCD's L2) and runs what eps_select_kernel / eps_select2_kernel ran as launches of their own.
  // (no cache maintenance is involved: the histogram words are only ever touched by device-scope atomics and agent-scope loads, both
  // performed at the memory side -- a wave waits for the acknowledgement of its own atomics, the barrier collects the waves, lane 0 draws
  // the ticket.  __threadfence() here -- an L2 write-back + invalidate per thread -- cost more than the launches it saved.)
  __shared__ unsigned int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  eps_select_block(hist, q, sel, refine != nullptr, lh);
}

// one workgroup: first bin whose cumulative sample count reaches ceil(q * sample size); threshold = upper edge of the NEXT
// bin (one guard bin = 0.4 % in value).  out3 = {threshold as float bits, sample size, bin}; degenerate sample -> +inf threshold
__global__ __launch_bounds__(1024) void eps_select_kernel(const unsigned long long* __restrict__ hist, double q, unsigned long long* __restrict__ out3) {
  __shared__ unsigned long long part[1024];
  const int t = (int)threadIdx.x;
  unsigned long long c[4], s = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) { c[u] = hist[4 * t + u]; s += c[u]; }
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {             // Hillis-Steele inclusive scan
    const unsigned long long add = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  const unsigned long long total = hist[4096];
  unsigned long long target = (unsigned long long)ceil(q * (double)total);
  if (target < 64) target = 64;
  unsigned long long run = part[t] - s;              // exclusive prefix of this thread's four bins
  __shared__ int bsel;
  if (t == 0) bsel = 4096;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const unsigned long long before = run;
    run += c[u];
    if (before < target && run >= target) bsel = 4 * t + u;   // unique
  }
  __syncthreads();
  if (t == 0) {
    const int b = bsel;
    float thr = b >= 4094 ? __uint_as_float(0x7f800000u) : sur_bin_upper(b + 1);
    if (total == 0) thr = __uint_as_float(0x7f800000u);
    out3[0] = (unsigned long long)__float_as_uint(thr); out3[1] = total; out3[2] = (unsigned long long)b;
  }
  // for the refinement level: sample elements below the selected bin, and the target rank
#pragma unroll
  for (int u = 0; u < 4; u++) if (4 * t + u == bsel) out3[3] = part[t] - s + (u > 0 ? c[0] : 0) + (u > 1 ? c[1] : 0) + (u > 2 ? c[2] : 0);
  if (t == 0) { out3[4] = target; if (bsel >= 4096) out3[3] = 0; }
}

// level 2: hist2 = 1024 sub-bins of coarse bin sel[2]; threshold = upper edge of the sub-bin AFTER the one where the cumulative
// count (sel[3] + sub-bins) reaches the target sel[4] (one guard sub-bin, 4e-6 relative: ten times the surrogate error);
// overwrites sel[0] when the bin was usable
__global__ __launch_bounds__(1024) void eps_select2_kernel(const unsigned long long* __restrict__ hist2, unsigned long long* __restrict__ sel) {
  __shared__ unsigned long long part[1024];
  const int t = (int)threadIdx.x;
  const unsigned long long c = hist2[t];
  part[t] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long add = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  const int b = (int)sel[2];
  if (b < 1 || b >= 4094) return;                    // degenerate / open-ended bins keep the coarse threshold
  const unsigned long long before = sel[3], target = sel[4];
  const unsigned long long incl = before + part[t], excl = incl - c;
  if (excl < target && incl >= target) {
    const float lo = sur_bin_upper(b - 1), hi = sur_bin_upper(b);
    const float thr = lo + (float)(t + 2) * ((hi - lo) * (1.f / 1024.f));
    sel[0] = (unsigned long long)__float_as_uint(thr < sur_bin_upper(b + 1) ? thr : sur_bin_upper(b + 1));
  }
}

// the one full pass: exact float64 keys of the strict-upper non-zero elements whose surrogate is < *thr -> buf (cursor[0]);
// cursor[1] += number of exact zeros in the strict upper triangle
template <int MODE>
__global__ __launch_bounds__(256) void eps_compact_thr_kernel(MatView mv, const unsigned long long* __restrict__ thr3, unsigned long long* __restrict__ buf,
                                                              unsigned long long cap, unsigned long long* __restrict__ cursor,
                                                              const unsigned long long* __restrict__ gate, const unsigned char* __restrict__ rowmask) {
  // key stage (768 keys per wave: the generic path appends up to 512 at once) + candidate-column stage of the fast path (see below):
  // 33.4 KB per workgroup, four workgroups per CU
  constexpr int KCAP = 768, CCAP = 64 + 512;
#ifndef SSG_DENSE_PIPE
#define SSG_DENSE_PIPE 8
#endif
  constexpr int DPIPE = SSG_DENSE_PIPE;          // chunks in flight per wave in the fast path
  __shared__ unsigned long long sbuf[4][KCAP];
  __shared__ unsigned int cidx_s[4][CCAP];
  if (gate && *gate == 0ull) return;          // the sparse pass queued in front of this launch has done every row
  const int lane = lane_id();
  WaveStage<unsigned long long> st{sbuf[threadIdx.x >> 6], 0};
  unsigned int* cidx = cidx_s[threadIdx.x >> 6];
  int nci = 0;                                 // staged candidate columns of the current row (wave-uniform)
  const float thr = __uint_as_float((unsigned)thr3[0]);
  const float lam32 = (float)mv.lambda_value;
  unsigned long long zeros = 0;
  // generic chunk: per-element bounds, exact zero detection (row edges, unaligned rows, modes 1 / 2)
  auto generic_chunk = [&](const RowStream& rs, int c, int gi, hbits vi, const RawChunk* rawp) {
    const int j0 = rs.col0(c, lane);
    float sv[8]; unsigned zm = 0;
    double dv[8];
    RawChunk raw;
    if (MODE == 2) {
      load_vals<MODE>(mv, rs, c, lane, gi, dv);
#pragma unroll
      for (int e = 0; e < 8; e++) { sv[e] = (float)dv[e]; if (dv[e] == 0.0) zm |= 1u << e; }
    } else {
      raw = rawp ? *rawp : load_raw<MODE == 2 ? 1 : MODE>(mv, rs, c, lane);
      surrogate8<MODE == 2 ? 1 : MODE>(mv, raw, vi, lam32, sv, zm);
    }
    unsigned cand = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int k = j0 + e;
      if (k > gi && k < mv.N) {
        if ((zm >> e) & 1u) zeros++;
        else if (sv[e] < thr) cand |= 1u << e;
      }
    }
    if (!__any(cand != 0)) return;
    if (MODE != 2) decode_raw<MODE == 2 ? 1 : MODE>(mv, raw, vi, dv);   // exact float64 values of this chunk (rare path)
    unsigned long long keys[8]; int n = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      keys[e] = ~0ULL;
      if ((cand >> e) & 1u) {
        if (dv[e] != 0.0) { keys[e] = (unsigned long long)__double_as_longlong(dv[e]); n++; }
        else zeros++;
      }
    }
    int incl = n;
    for (int sh = 1; sh < 64; sh <<= 1) { const int o = __shfl_up(incl, sh, 64); if (lane >= sh) incl += o; }
    const int tot = __shfl(incl, 63, 64);
    int w = st.n + incl - n;
#pragma unroll
    for (int e = 0; e < 8; e++) if (keys[e] != ~0ULL) st.buf[w++] = keys[e];
    st.n += tot;
    if (st.n > KCAP - 512) st.flush(buf, cap, cursor, lane);
  };
  // the top `m` (<= 64) staged candidates (J' half | v_k half << 16) of a row -> exact float64 keys (exact zeros are counted, not kept) -> key stage
  auto finish = [&](const hbits* __restrict__ Mrow, hbits vi, int m) {
    (void)Mrow;
    unsigned long long key = ~0ULL; bool keep = false;
    if (lane < m) {
      const unsigned pk = cidx[nci - m + lane];
      const double d = final_dist_value((hbits)(pk & 0xffffu), vi, (hbits)(pk >> 16), mv.lambda_value);
      if (d != 0.0) { key = (unsigned long long)__double_as_longlong(d); keep = true; }
      else zeros++;
    }
    const uint64_t bm = __ballot(keep);
    if (keep) st.buf[st.n + __popcll(bm & lanemask_lt())] = key;
    st.n += __popcll(bm);
    nci -= m;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (st.n > KCAP - 512) st.flush(buf, cap, cursor, lane);
  };
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const bool fast_ok = MODE == 0 && (mv.N & 7) == 0 && thr > 0.f;
  // rows of the strict upper triangle get shorter linearly: a wave takes rows in complementary pairs (p, nrows-1-p), so every
  // wave streams the same number of elements (a handful of whole rows per wave would leave a 1.5-2x imbalance)
  const int npairs = (mv.nrows + 1) / 2;
  for (int pidx = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); pidx < npairs; pidx += (int)gridDim.x * 4)
  for (int hh = 0; hh < 2; hh++) {
    const int il = hh ? mv.nrows - 1 - pidx : pidx;
    if (hh && il == pidx) continue;                // odd row count: the middle row is its own partner
    if (rowmask && rowmask[il] == 0) continue;     // done through the sparse copy
    const int gi = mv.row0 + il;
    RowStream rs(il, mv.N, mv.nrows);
    const int c0 = (rs.first + gi + 1) / 512;
    const hbits vi = MODE == 0 ? mv.v[gi] : (hbits)0;
    if (fast_ok) {
      // N % 8 == 0: rows are 16-byte aligned.  The chunk holding the diagonal and a partial last chunk take the generic path;
      // every chunk in between lies entirely in the strict upper triangle: no bounds, packed half adds, and no zero test --
      // an exact zero has surrogate 0 (or J' alone when lambda == 0) < thr, so it is a candidate and is classified exactly below
      const hbits* M = reinterpret_cast<const hbits*>(mv.M) + (int64_t)il * mv.N;
      const _Float16 vi16 = __builtin_bit_cast(_Float16, vi);
      const h2 vi2 = {vi16, vi16};
      const int nfull = mv.N / 512;
      if (c0 < rs.nchunks) generic_chunk(rs, c0, gi, vi, nullptr);
      for (int cb = c0 + 1; cb < nfull; cb += DPIPE) {
        uint4 xjs[DPIPE], xvs[DPIPE];
#pragma unroll
        for (int u = 0; u < DPIPE; u++) {
          const int j0 = min(cb + u, nfull - 1) * 512 + lane * 8;
          xjs[u] = *reinterpret_cast<const uint4*>(M + j0);
          xvs[u] = *reinterpret_cast<const uint4*>(mv.v + j0);
        }
#pragma unroll
        for (int u = 0; u < DPIPE; u++) {
          const int c = cb + u;
          if (c >= nfull) break;
          const unsigned wj[4] = {xjs[u].x, xjs[u].y, xjs[u].z, xjs[u].w}, wv[4] = {xvs[u].x, xvs[u].y, xvs[u].z, xvs[u].w};
          unsigned cand = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const h2 s2 = __builtin_bit_cast(h2, wv[q]) + vi2;                 // half(v_k + v_i), two columns per instruction
            const h2 j2 = __builtin_bit_cast(h2, wj[q]);
            const float a = (float)j2.x + (float)s2.x * lam32, b = (float)j2.y + (float)s2.y * lam32;
            cand |= (a < thr ? 1u : 0u) << (2 * q) | (b < thr ? 1u : 0u) << (2 * q + 1);
          }
          // Round 6: at the 1.3 rho quantile about two chunks in three hold a candidate, so the "rare" path ran for most chunks -- and it
          // rebuilt the float64 value of all 8 x 64 elements of the chunk for that one candidate (the pass streamed at 2.4-2.9 TB/s
          // against 4.5-5.1 with a threshold nothing lies below).  Now a chunk only stages the two HALVES of each candidate (J' and v_k);
          // the exact float64 keys are built 64 candidates at a time, one per lane (`finish`).
          const int n = __popc(cand);
          const uint64_t bm = __ballot(n != 0);
          if (bm == 0) continue;
          // (staged: the two halves the key is made of -- J' and v_k --, not the column: `finish` needs no load)
          if (!__any(n > 1)) {
            // the usual case, one candidate in each of a few lanes: the slot is the lane's rank among them (two mbcnt instructions, no scan)
            if (n) {
              const int e = __ffs((int)cand) - 1, sh = (e & 1) * 16;
              const unsigned pj = e < 4 ? (e < 2 ? wj[0] : wj[1]) : (e < 6 ? wj[2] : wj[3]), pv = e < 4 ? (e < 2 ? wv[0] : wv[1]) : (e < 6 ? wv[2] : wv[3]);
              cidx[nci + __popcll(bm & lanemask_lt())] = ((pj >> sh) & 0xffffu) | (((pv >> sh) & 0xffffu) << 16);
            }
            nci += __popcll(bm);
          } else {
            int incl = n;
            for (int sh = 1; sh < 64; sh <<= 1) { const int o = __shfl_up(incl, sh, 64); if (lane >= sh) incl += o; }
            const int tot = __shfl(incl, 63, 64);
            int w = nci + incl - n;
#pragma unroll
            for (int e = 0; e < 8; e++)
              if ((cand >> e) & 1u) cidx[w++] = ((wj[e >> 1] >> ((e & 1) * 16)) & 0xffffu) | (((wv[e >> 1] >> ((e & 1) * 16)) & 0xffffu) << 16);
            nci += tot;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          while (nci >= 64) finish(M, vi, 64);
        }
      }
      if (nci) finish(M, vi, nci);                      // the row's last few candidates (vi is the row's)
      if (nfull * 512 < mv.N && nfull > c0) generic_chunk(rs, nfull, gi, vi, nullptr);
      continue;
    }
    for (int c = c0; c < rs.nchunks; c++) generic_chunk(rs, c, gi, vi, nullptr);
  }
  block_flush(st, buf, cap, cursor);
  for (int sh = 1; sh < 64; sh <<= 1) zeros += (unsigned long long)__shfl_xor((long long)zeros, sh, 64);
  if (lane == 0 && zeros) atomicAdd(&cursor[1], zeros);
}

// eps rule, the one full pass, on S: exact float64 keys of the strict-upper non-zero elements whose surrogate is < *thr -> buf
// (cursor[0]); cursor[1] += exact zeros.  A row is walked through S when no column outside S can be a candidate: the surrogate of such
// a column is >= J'(0) + half(v_i + vmin) * lambda in the very float operations the dense pass uses, so the test is exact.  Rows that
// fail it (and every row when S is unusable) get rowmask = 1 and raise cursor[2]: the dense pass queued behind this launch does them.
__global__ __launch_bounds__(256) void eps_compact_sparse_kernel(MatView mv, SparseView sv, const unsigned long long* __restrict__ thr3,
                                                                 unsigned long long* __restrict__ buf, unsigned long long cap,
                                                                 unsigned long long* __restrict__ cursor, unsigned char* __restrict__ rowmask) {
  __shared__ unsigned long long sbuf[4][SPARSE_STAGE];
  const int lane = lane_id();
  const float thr = __uint_as_float((unsigned)thr3[0]);
  const bool usable = thr > 0.f && sparse_usable(sv, mv);
  const hbits vmin = usable ? (hbits)*sv.vmin : (hbits)0;
  WaveStage<unsigned long long> st{sbuf[threadIdx.x >> 6], 0};
  const float lam32 = (float)mv.lambda_value;
  unsigned long long zeros = 0;
  bool anydense = false;
  for (int il = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); il < mv.nrows; il += (int)gridDim.x * 4) {
    const int gi = mv.row0 + il;
    const hbits vi = mv.v[gi];
    const bool rowok = usable && (h2f(sv.jp0) + h2f(h_add(vmin, vi)) * lam32 >= thr);
    if (lane == 0) rowmask[il] = rowok ? 0 : 1;
    if (!rowok) { anydense = true; continue; }
    for (int sg = 0; sg < sv.nseg; sg++) {
      const int64_t off = sv.seg_off[(int64_t)il * sv.nseg + sg];
      const int len = sv.seg_len[(int64_t)il * sv.nseg + sg];
      // SBATCH entries per lane in flight: the packed words first, then the gathers of v[k] they address (a segment is a few hundred
      // entries: one entry per lane and trip would make the row a chain of L2 round trips)
      for (int q0 = 0; q0 < len; q0 += 64 * SBATCH) {
        uint32_t e[SBATCH]; hbits vk[SBATCH];
#pragma unroll
        for (int u = 0; u < SBATCH; u++) { const int q = q0 + u * 64 + lane; e[u] = sv.pool[off + (q < len ? q : len - 1)]; }
#pragma unroll
        for (int u = 0; u < SBATCH; u++) vk[u] = mv.v[e[u] & 0x1ffffu];
#pragma unroll
        for (int u = 0; u < SBATCH; u++) {
          const int q = q0 + u * 64 + lane;
          if (q0 + u * 64 >= len) break;
          unsigned long long key = ~0ULL;
          const int k = (int)(e[u] & 0x1ffffu);
          if (q < len && k > gi) {
            const hbits jp = (hbits)(e[u] >> 17);
            const float sur = h2f(jp) + h2f(h_add(vk[u], vi)) * lam32;
            if (sur < thr) {           // (an exact zero has surrogate 0 < thr: it is always classified here)
              const double d = final_dist_value(jp, vi, vk[u], mv.lambda_value);
              if (d != 0.0) key = (unsigned long long)__double_as_longlong(d); else zeros++;
            }
          }
          const uint64_t bm = __ballot(key != ~0ULL);
          if (bm) {
            if (key != ~0ULL) st.buf[st.n + __popcll(bm & lanemask_lt())] = key;
            st.n += __popcll(bm);
            if (st.n > SPARSE_STAGE - 64) st.flush(buf, cap, cursor, lane);
          }
        }
      }
    }
  }
  block_flush(st, buf, cap, cursor);
  for (int sh = 1; sh < 64; sh <<= 1) zeros += (unsigned long long)__shfl_xor((long long)zeros, sh, 64);
  if (lane == 0 && zeros) atomicAdd(&cursor[1], zeros);
  if (lane == 0 && anydense) cursor[2] = 1ull;
}

// ------------------------------------------------------------------ numpy pairwise mean
// np.mean(x[:top]) = pairwise_sum(x, top) / top with numpy's recursion (blocks <= 128 summed
// with 8 accumulators, halves split at a multiple of 8).  The recursion tree depends on `top`
// only, so the host enumerates it once (leaves + internal nodes grouped by height) and one
// workgroup evaluates it: all leaves in parallel, then one tree level per barrier.
template <typename T>
__device__ T pw_leaf(const unsigned long long* keys, long long off, int n) {
  auto val = [&](long long i) -> T { return (T)__longlong_as_double((long long)keys[off + i]); };
  if (n < 8) { T r = (T)0; for (int i = 0; i < n; i++) r += val(i); return r; }
  T r[8]; int i;
  for (i = 0; i < 8; i++) r[i] = val(i);
  for (i = 8; i < n - (n % 8); i += 8) for (int j = 0; j < 8; j++) r[j] += val(i + j);
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) res += val(i);
  return res;
}
// the a-posteriori checks of the sampled eps rule (see eps_check_kernel, which runs them as a launch of its own): one thread
struct EpsCheckArgs {
  const unsigned long long* cursor = nullptr; const unsigned long long* thr3 = nullptr; double rho = 0.0; unsigned long long upper_total = 0; long long top_guess = 0;
  unsigned long long n_cap = 0; unsigned long long* status6 = nullptr; const unsigned long long* sort_fail = nullptr;
};
__device__ __forceinline__ void eps_check_one(const unsigned long long* __restrict__ sorted, const EpsCheckArgs& a, double* __restrict__ eps2) {
  const unsigned long long got = a.cursor[0], zeros = a.cursor[1];
  const long long count = (long long)(a.upper_total - zeros);
  const long long top = (long long)rint(a.rho * (double)count);
  const double thr = (double)__uint_as_float((unsigned)(a.thr3[0] & 0xffffffffull));
  bool ok = top == a.top_guess && top > 0 && got <= a.n_cap && got >= (unsigned long long)top && isfinite(thr) && !(a.sort_fail && *a.sort_fail);
  unsigned long long kb = 0;
  if (ok) {
    kb = sorted[top - 1];
    const double key_top = __longlong_as_double((long long)kb);
    ok = key_top < thr - 1e-6 * (1.0 + fabs(thr));
  }
  a.status6[0] = ok ? 1ull : 0ull; a.status6[1] = got; a.status6[2] = zeros; a.status6[3] = (unsigned long long)top; a.status6[4] = kb; a.status6[5] = a.thr3[0];
  if (!ok) eps2[0] = __longlong_as_double(0x7ff8000000000000ll);
}
// leaves of the pairwise tree, 8 lanes per leaf (one lane per accumulator of numpy's unrolled loop), 8 leaves per wave:
//   r[j] = a[j]; for i = 8, 16, ...: r[j] += a[i + j];  res = ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7));  res += a[tail...]
template <typename T>
__global__ __launch_bounds__(256) void eps_leaf_kernel(const unsigned long long* __restrict__ keys, int nleaves, const long long* __restrict__ leaf_off,
                                                       const int* __restrict__ leaf_n, T* __restrict__ val) {
  const int gl = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 3);      // leaf
  const int j = (int)(threadIdx.x & 7);
  const bool live = gl < nleaves;
  const long long off = live ? leaf_off[gl] : 0;
  const int n = live ? leaf_n[gl] : 0;
  auto a = [&](int i) -> T { return (T)__longlong_as_double((long long)keys[off + i]); };
  T res;
  if (n < 8) {
    res = (T)0;
    if (j == 0) for (int i = 0; i < n; i++) res += a(i);
  } else {
    const int nb = n - (n % 8);
    T r = a(j);
    for (int i = 8; i < nb; i += 8) r += a(i + j);
    // combine in numpy's order: lanes 2q, 2q+1 -> pairs, then pairs of pairs, then the two halves (xor shuffles inside the 8 lanes)
    T p = r + (T)__shfl_xor(r, 1, 64);         // lane even: r_j + r_{j+1} (addition is commutative, the operand order does not matter)
    T q = p + (T)__shfl_xor(p, 2, 64);         // lanes 0-3: (r0+r1)+(r2+r3); lanes 4-7: (r4+r5)+(r6+r7)
    res = q + (T)__shfl_xor(q, 4, 64);
    if (j == 0) for (int i = nb; i < n; i++) res += a(i);
  }
  if (live && j == 0) val[gl] = res;
}
// out[0] = eps as double; out[1] = half bits of eps (mode 1) as a double-held integer
template <typename T>
__global__ __launch_bounds__(1024) void eps_mean_kernel(const unsigned long long* __restrict__ keys, long long top, int nleaves, int nlevels,
                                                        const long long* __restrict__ leaf_off, const int* __restrict__ leaf_n,
                                                        const int* __restrict__ node_l, const int* __restrict__ node_r,
                                                        const int* __restrict__ level_ptr, T* __restrict__ val, double* __restrict__ out, EpsCheckArgs chk = EpsCheckArgs()) {
  (void)leaf_off; (void)leaf_n;        // the leaves were summed by eps_leaf_kernel
  for (int h = 0; h < nlevels; h++) {
    for (int x = level_ptr[h] + (int)threadIdx.x; x < level_ptr[h + 1]; x += (int)blockDim.x) val[nleaves + x] = val[node_l[x]] + val[node_r[x]];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int ninternal = level_ptr[nlevels];
    const T s = val[ninternal ? nleaves + ninternal - 1 : 0];   // the root is the last node of the last level
    if (sizeof(T) == 8) { out[0] = (double)s / (double)top; out[1] = 0.0; }
    else {
      const hbits e = d2h((double)s / (double)top);   // np.float32 scalar / np.intp -> float64 -> np.float16
      out[0] = (double)h2f(e); out[1] = (double)e;
    }
    if (chk.status6) eps_check_one(keys, chk, out);     // round 6: the a-posteriori checks in the same launch (ssg_eps_mean_check)
  }
}

}  // namespace ssg

using namespace ssg;

extern "C" int ssg_eps_hist(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value,
                            uint64_t prefix, int shift, int width, int count_nonzero, uint64_t* hist, hipStream_t stream) {
  int rc = check_view("ssg_eps_hist", M, v, N, row0, nrows, mode); if (rc) return rc;
  if (width <= 0 || width > 12 || shift < 0 || shift + width > 64) { ssg_set_error("ssg_eps_hist: bad digit"); return SSG_ERR_INVALID; }
#define SSG_HIST(MD) hipLaunchKernelGGL(eps_hist_kernel<MD>, dim3(stream_grid(nrows)), dim3(256), 0, stream, make_view(M, v, N, row0, nrows, mode, lambda_value), \
                     (unsigned long long)prefix, shift, width, count_nonzero, (unsigned long long*)hist)
  if (mode == 0) SSG_HIST(0); else if (mode == 1) SSG_HIST(1); else SSG_HIST(2);
#undef SSG_HIST
  SSG_LAUNCH_CHECK("eps_hist_kernel");
  return SSG_OK;
}

extern "C" int ssg_eps_compact(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value,
                               uint64_t key_max, uint64_t* buf, uint64_t cap, uint64_t* cursor, hipStream_t stream) {
  int rc = check_view("ssg_eps_compact", M, v, N, row0, nrows, mode); if (rc) return rc;
#define SSG_COMPACT(MD) hipLaunchKernelGGL(eps_compact_kernel<MD>, dim3(stream_grid(nrows)), dim3(256), 0, stream, make_view(M, v, N, row0, nrows, mode, lambda_value), \
                     (unsigned long long)key_max, (unsigned long long*)buf, (unsigned long long)cap, (unsigned long long*)cursor)
  if (mode == 0) SSG_COMPACT(0); else if (mode == 1) SSG_COMPACT(1); else SSG_COMPACT(2);
#undef SSG_COMPACT
  SSG_LAUNCH_CHECK("eps_compact_kernel");
  return SSG_OK;
}

// ---- K10 fast path (see eps_sample_hist_kernel): hist = 4097 uint64 zeroed by the caller; thr3 = 3 uint64 out
extern "C" int ssg_eps_sample_hist(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, int row_stride,
                                   const uint64_t* refine, uint64_t* hist, hipStream_t stream) {
  int rc = check_view("ssg_eps_sample_hist", M, v, N, row0, nrows, mode); if (rc) return rc;
  if (row_stride < 1) { ssg_set_error("ssg_eps_sample_hist: row_stride must be >= 1"); return SSG_ERR_INVALID; }
  const int nsamp = (nrows + row_stride - 1) / row_stride;
#define SSG_SH(MD) hipLaunchKernelGGL(eps_sample_hist_kernel<MD>, dim3(stream_grid(nsamp * SPARTS)), dim3(256), 0, stream, make_view(M, v, N, row0, nrows, mode, lambda_value), \
                     row_stride, (const unsigned long long*)refine, (unsigned long long*)hist)
  if (mode == 0) SSG_SH(0); else if (mode == 1) SSG_SH(1); else SSG_SH(2);
#undef SSG_SH
  SSG_LAUNCH_CHECK("eps_sample_hist_kernel");
  return SSG_OK;
}
// round 6: both sampling levels with their selections in TWO launches instead of four (the workgroup that finishes last selects).
// hist2x = 2 x 4097 words and tickets = 2 words, zeroed by the caller; thr5 receives what ssg_eps_select_threshold + ssg_eps_refine_threshold leave.
extern "C" int ssg_eps_sample_threshold(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, int row_stride,
                                        double quantile, uint64_t* hist2x, uint64_t* thr5, uint32_t* tickets2, hipStream_t stream) {
  int rc = check_view("ssg_eps_sample_threshold", M, v, N, row0, nrows, mode); if (rc) return rc;
  if (row_stride < 1 || !(quantile > 0.0) || !hist2x || !thr5 || !tickets2) { ssg_set_error("ssg_eps_sample_threshold: bad arguments"); return SSG_ERR_INVALID; }
  const int nsamp = (nrows + row_stride - 1) / row_stride;
  const MatView mv = make_view(M, v, N, row0, nrows, mode, lambda_value);
  const unsigned g = (unsigned)stream_grid(nsamp * SPARTS);
#define SSG_ST(MD, LVL) hipLaunchKernelGGL(eps_sample_hist_kernel<MD>, dim3(g), dim3(256), 0, stream, mv, row_stride, (LVL) ? (const unsigned long long*)thr5 : nullptr, \
                     (unsigned long long*)hist2x + (LVL) * 4097, quantile, (unsigned long long*)thr5, (unsigned int*)tickets2 + (LVL))
  for (int lvl = 0; lvl < 2; lvl++) { if (mode == 0) SSG_ST(0, lvl); else if (mode == 1) SSG_ST(1, lvl); else SSG_ST(2, lvl); }
#undef SSG_ST
  SSG_LAUNCH_CHECK("eps_sample_hist_kernel (+ selection)");
  return SSG_OK;
}
extern "C" int ssg_eps_select_threshold(const uint64_t* hist, double quantile, uint64_t* thr3, hipStream_t stream) {
  if (!(quantile > 0.0)) { ssg_set_error("ssg_eps_select_threshold: quantile must be positive"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(eps_select_kernel, dim3(1), dim3(1024), 0, stream, (const unsigned long long*)hist, quantile, (unsigned long long*)thr3);
  SSG_LAUNCH_CHECK("eps_select_kernel");
  return SSG_OK;
}
extern "C" int ssg_eps_refine_threshold(const uint64_t* hist2, uint64_t* thr5, hipStream_t stream) {
  hipLaunchKernelGGL(eps_select2_kernel, dim3(1), dim3(1024), 0, stream, (const unsigned long long*)hist2, (unsigned long long*)thr5);
  SSG_LAUNCH_CHECK("eps_select2_kernel");
  return SSG_OK;
}
extern "C" int ssg_eps_compact_below(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value,
                                     const uint64_t* thr3, uint64_t* buf, uint64_t cap, uint64_t* cursor2, hipStream_t stream) {
  int rc = check_view("ssg_eps_compact_below", M, v, N, row0, nrows, mode); if (rc) return rc;
#define SSG_CT(MD) hipLaunchKernelGGL(eps_compact_thr_kernel<MD>, dim3(stream_grid(nrows)), dim3(256), 0, stream, make_view(M, v, N, row0, nrows, mode, lambda_value), \
                     (const unsigned long long*)thr3, (unsigned long long*)buf, (unsigned long long)cap, (unsigned long long*)cursor2, (const unsigned long long*)nullptr, (const unsigned char*)nullptr)
  if (mode == 0) SSG_CT(0); else if (mode == 1) SSG_CT(1); else SSG_CT(2);
#undef SSG_CT
  SSG_LAUNCH_CHECK("eps_compact_thr_kernel");
  return SSG_OK;
}

// The same pass through the sparse copy S of J' (ssg_jaccard_rows2): cursor3 = {keys collected, exact zeros, dense pass needed}, zeroed by
// the caller; vmin = half bits of min(v) (ssg_half_min); rowmask = nrows bytes of workspace.  Two launches: the walk over S, which takes
// every row whose floor J'(0) + lambda * half(v_i + vmin) lies at or above the threshold and flags the others (all of them when S
// overflowed or lambda < 0), and the dense pass over the flagged rows, gated on cursor3[2] -- no host decision, no read-back in between.
extern "C" int ssg_eps_compact_below_s(const void* M, const uint16_t* v, int N, int row0, int nrows, double lambda_value, const uint64_t* thr3,
                                       uint64_t* buf, uint64_t cap, uint64_t* cursor3, const uint32_t* s_pool, const int64_t* seg_off,
                                       const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin, uint16_t jp0_half,
                                       uint8_t* rowmask, hipStream_t stream) {
  int rc = check_view("ssg_eps_compact_below_s", M, v, N, row0, nrows, 0); if (rc) return rc;
  if (!s_pool || !seg_off || !seg_len || nseg <= 0 || !s_cursor || !vmin || !rowmask) { ssg_set_error("ssg_eps_compact_below_s: no sparse copy"); return SSG_ERR_INVALID; }
  const MatView mv = make_view(M, v, N, row0, nrows, 0, lambda_value);
  hipLaunchKernelGGL(eps_compact_sparse_kernel, dim3(stream_grid(nrows)), dim3(256), 0, stream, mv, make_sparse(s_pool, seg_off, seg_len, nseg, s_cursor, vmin, jp0_half),
                     (const unsigned long long*)thr3, (unsigned long long*)buf, (unsigned long long)cap, (unsigned long long*)cursor3, rowmask);
  hipLaunchKernelGGL(eps_compact_thr_kernel<0>, dim3(stream_grid(nrows)), dim3(256), 0, stream, mv, (const unsigned long long*)thr3, (unsigned long long*)buf,
                     (unsigned long long)cap, (unsigned long long*)cursor3, (const unsigned long long*)(cursor3 + 2), (const unsigned char*)rowmask);
  SSG_LAUNCH_CHECK("eps_compact_sparse_kernel");
  return SSG_OK;
}

namespace ssg {
// smallest of N non-negative halves (bit order == value order), one workgroup
__global__ __launch_bounds__(1024) void half_min_kernel(const hbits* __restrict__ v, int N, uint32_t* __restrict__ out) {
  __shared__ unsigned smin[16];
  unsigned m = 0xffffu;
  for (int i = (int)threadIdx.x; i < N; i += 1024) { const unsigned x = v[i]; m = x < m ? x : m; }
  for (int sh = 1; sh < 64; sh <<= 1) { const unsigned o = (unsigned)__shfl_xor((int)m, sh, 64); m = o < m ? o : m; }
  if ((threadIdx.x & 63) == 0) smin[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) { for (int w = 1; w < 16; w++) m = smin[w] < m ? smin[w] : m; *out = m; }
}
}  // namespace ssg
// *out_bits = min_k v[k] as half bits (v >= 0: the source vector of rerank.py:38-40); the row floors of the sparse passes need it
extern "C" int ssg_half_min(const uint16_t* v, int N, uint32_t* out_bits, hipStream_t stream) {
  if (!v || N <= 0 || !out_bits) { ssg_set_error("ssg_half_min: bad arguments"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(ssg::half_min_kernel, dim3(1), dim3(1024), 0, stream, v, N, out_bits);
  SSG_LAUNCH_CHECK("half_min_kernel");
  return SSG_OK;
}

// The a-posteriori checks of the sampled eps rule (ssg_amd/cluster.py _eps_rule_sampled) on the device, one thread:
//   count = upper_total - zeros;  top = rint(rho * count) (np.round: half to even, selftraining.py:292) must equal the top_guess the
//   summation tree was built for;  every collected key fits (got <= n_cap), at least `top` were collected, the threshold is finite and
//   the top-th sorted key lies below it by the float32 surrogate's margin (=> the `top` smallest are all among the collected keys);
//   *sort_fail (the sample sort's word; may be null) is zero.
// status6 = {ok, got, zeros, top, bits of the top-th key, threshold bits};  eps2[0] (the mean ssg_eps_mean_run left there) is replaced
// by NaN when a check fails, so that a region query queued behind finds nothing and the caller falls back.
__global__ void eps_check_kernel(const unsigned long long* __restrict__ sorted, const unsigned long long* __restrict__ cursor, const unsigned long long* __restrict__ thr3,
                                 double rho, unsigned long long upper_total, long long top_guess, unsigned long long n_cap, double* __restrict__ eps2,
                                 unsigned long long* __restrict__ status6, const unsigned long long* __restrict__ sort_fail) {
  if (blockIdx.x || threadIdx.x) return;
  EpsCheckArgs a; a.cursor = cursor; a.thr3 = thr3; a.rho = rho; a.upper_total = upper_total; a.top_guess = top_guess; a.n_cap = n_cap; a.status6 = status6; a.sort_fail = sort_fail;
  eps_check_one(sorted, a, eps2);
}
extern "C" int ssg_eps_check(const uint64_t* sorted_keys, const uint64_t* cursor, const uint64_t* thr3, double rho, uint64_t upper_total, int64_t top_guess,
                             uint64_t n_cap, double* eps2, uint64_t* status6, const uint64_t* sort_fail, hipStream_t stream) {
  if (!sorted_keys || !cursor || !thr3 || !eps2 || !status6) { ssg_set_error("ssg_eps_check: null argument"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(eps_check_kernel, dim3(1), dim3(64), 0, stream, (const unsigned long long*)sorted_keys, (const unsigned long long*)cursor,
                     (const unsigned long long*)thr3, rho, (unsigned long long)upper_total, (long long)top_guess, (unsigned long long)n_cap, eps2,
                     (unsigned long long*)status6, (const unsigned long long*)sort_fail);
  SSG_LAUNCH_CHECK("eps_check_kernel");
  return SSG_OK;
}

// workspace bytes for ssg_eps_mean: recursion tables + node values for `top` summands
extern "C" size_t ssg_eps_mean_workspace_bytes(int64_t top) { const size_t nl = (size_t)(top / 32 + 64); return nl * 64 + 1024; }

namespace {
struct PwTree {
  std::vector<long long> leaf_off; std::vector<int> leaf_n, node_l, node_r, node_h, level_ptr;
  // returns node id (leaves: index; internal: nleaves + index) -- internal ids are remapped after sorting by height
  int build(long long off, long long n, std::vector<int>& il, std::vector<int>& ir, std::vector<int>& ih, int& height) {
    if (n <= 128) { leaf_off.push_back(off); leaf_n.push_back((int)n); height = 0; return -(int)leaf_off.size(); }   // leaf id = -(idx+1)
    long long n2 = n / 2; n2 -= n2 % 8;
    int hl, hr;
    const int l = build(off, n2, il, ir, ih, hl), r = build(off + n2, n - n2, il, ir, ih, hr);
    height = (hl > hr ? hl : hr) + 1;
    il.push_back(l); ir.push_back(r); ih.push_back(height);
    return (int)il.size() - 1;
  }
};
}  // namespace

namespace {
struct PwLayout { int L, I, hroot; size_t o_off, o_n, o_l, o_r, o_lp, o_val, need; std::vector<char> host; };
// numpy's summation tree for `top` summands (depends on top only) and its packed device layout.  np.add.reduce (hence np.mean) walks a
// contiguous array in chunks of its buffer size, 8192 elements: pairwise summation inside each chunk, the chunk sums added left to
// right -- a chain of internal nodes, one level each, on top of the chunk trees.
constexpr long long kNumpyBufsize = 8192;
static void pw_layout(int64_t top, PwLayout& out, bool with_tables) {
  PwTree t; std::vector<int> il, ir, ih; int hroot = 0;
  int acc = 0;
  for (long long off = 0; off < top; off += kNumpyBufsize) {
    int hc;
    const int c = t.build(off, std::min<long long>(kNumpyBufsize, top - off), il, ir, ih, hc);
    if (off == 0) { acc = c; hroot = hc; continue; }
    hroot = (hroot > hc ? hroot : hc) + 1;
    il.push_back(acc); ir.push_back(c); ih.push_back(hroot);
    acc = (int)il.size() - 1;
  }
  const int L = (int)t.leaf_off.size(), I = (int)il.size();
  out.L = L; out.I = I; out.hroot = hroot;
  // pack tables: leaf_off[L] i64 | leaf_n[L] | node_l[I] | node_r[I] | level_ptr[hroot+1] | val[(L+I)] (8 B each)
  out.o_off = 0; out.o_n = out.o_off + (size_t)L * 8; out.o_l = out.o_n + (size_t)L * 4; out.o_r = out.o_l + (size_t)I * 4; out.o_lp = out.o_r + (size_t)I * 4;
  out.o_val = out.o_lp + (size_t)(hroot + 1) * 4; out.o_val = (out.o_val + 15) & ~(size_t)15;
  out.need = out.o_val + (size_t)(L + I) * 8;
  if (!with_tables) return;
  // order internal nodes by height (stable), remap child references
  std::vector<int> order(I), pos(I);
  for (int i = 0; i < I; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ih[a] < ih[b]; });
  for (int i = 0; i < I; i++) pos[order[i]] = i;
  t.node_l.resize(I); t.node_r.resize(I); t.level_ptr.assign(hroot + 1, 0);
  auto ref = [&](int c) { return c < 0 ? (-c - 1) : (L + pos[c]); };
  for (int i = 0; i < I; i++) { const int o = order[i]; t.node_l[i] = ref(il[o]); t.node_r[i] = ref(ir[o]); t.level_ptr[ih[o]]++; }
  // level_ptr[h] currently counts nodes of height h (h>=1) at index h; turn into prefix offsets over levels 1..hroot
  std::vector<int> lp(hroot + 1, 0);
  for (int h = 1; h <= hroot; h++) lp[h] = lp[h - 1] + t.level_ptr[h];
  out.host.assign(out.o_val, 0);
  memcpy(out.host.data() + out.o_off, t.leaf_off.data(), (size_t)L * 8);
  memcpy(out.host.data() + out.o_n, t.leaf_n.data(), (size_t)L * 4);
  if (I) { memcpy(out.host.data() + out.o_l, t.node_l.data(), (size_t)I * 4); memcpy(out.host.data() + out.o_r, t.node_r.data(), (size_t)I * 4); }
  memcpy(out.host.data() + out.o_lp, lp.data(), (size_t)(hroot + 1) * 4);
}
}  // namespace

// Step 1 of ssg_eps_mean: upload the recursion tables for `top` into ws.  Blocks until the copy is done (the tables live in a
// local host buffer) -- call it while the stream is idle (right after `top` became known), not behind the sort.
extern "C" int ssg_eps_mean_prepare(int64_t top, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (top <= 0 || ws_bytes < ssg_eps_mean_workspace_bytes(top)) { ssg_set_error("ssg_eps_mean: top=%lld ws too small", (long long)top); return SSG_ERR_INVALID; }
  PwLayout lay; pw_layout(top, lay, true);
  if (lay.need > ws_bytes) { ssg_set_error("ssg_eps_mean: workspace %zu < %zu", ws_bytes, lay.need); return SSG_ERR_INVALID; }
  SSG_HIP(hipMemcpyAsync(ws, lay.host.data(), lay.o_val, hipMemcpyHostToDevice, stream));
  SSG_HIP(hipStreamSynchronize(stream));   // `lay.host` is a local buffer
  return SSG_OK;
}
// Step 2: the summation itself (asynchronous): leaves in parallel (8 lanes per leaf), then one workgroup walks the tree levels
static int eps_mean_run_impl(const uint64_t* sorted_keys, int64_t top, int mode, void* ws, size_t ws_bytes, double* out2, const EpsCheckArgs& chk, hipStream_t stream) {
  if (top <= 0 || ws_bytes < ssg_eps_mean_workspace_bytes(top)) { ssg_set_error("ssg_eps_mean: top=%lld ws too small", (long long)top); return SSG_ERR_INVALID; }
  PwLayout lay; pw_layout(top, lay, false);
  char* w = (char*)ws;
  const int L = lay.L, hroot = lay.hroot;
  const int lb = (L * 8 + 255) / 256;
  if (mode == 0) {
    hipLaunchKernelGGL(eps_leaf_kernel<double>, dim3(lb), dim3(256), 0, stream, (const unsigned long long*)sorted_keys, L, (const long long*)(w + lay.o_off),
                       (const int*)(w + lay.o_n), (double*)(w + lay.o_val));
    hipLaunchKernelGGL(eps_mean_kernel<double>, dim3(1), dim3(1024), 0, stream, (const unsigned long long*)sorted_keys, (long long)top, L, hroot,
                       (const long long*)(w + lay.o_off), (const int*)(w + lay.o_n), (const int*)(w + lay.o_l), (const int*)(w + lay.o_r),
                       (const int*)(w + lay.o_lp), (double*)(w + lay.o_val), out2, chk);
  } else {
    hipLaunchKernelGGL(eps_leaf_kernel<float>, dim3(lb), dim3(256), 0, stream, (const unsigned long long*)sorted_keys, L, (const long long*)(w + lay.o_off),
                       (const int*)(w + lay.o_n), (float*)(w + lay.o_val));
    hipLaunchKernelGGL(eps_mean_kernel<float>, dim3(1), dim3(1024), 0, stream, (const unsigned long long*)sorted_keys, (long long)top, L, hroot,
                       (const long long*)(w + lay.o_off), (const int*)(w + lay.o_n), (const int*)(w + lay.o_l), (const int*)(w + lay.o_r),
                       (const int*)(w + lay.o_lp), (float*)(w + lay.o_val), out2, chk);
  }
  SSG_LAUNCH_CHECK("eps_mean kernels");
  return SSG_OK;
}
extern "C" int ssg_eps_mean_run(const uint64_t* sorted_keys, int64_t top, int mode, void* ws, size_t ws_bytes, double* out2, hipStream_t stream) {
  return eps_mean_run_impl(sorted_keys, top, mode, ws, ws_bytes, out2, EpsCheckArgs(), stream);
}
// round 6: ssg_eps_mean_run + ssg_eps_check in the launches of the former (the tree kernel's last thread runs the checks)
extern "C" int ssg_eps_mean_check(const uint64_t* sorted_keys, int64_t top_guess, int mode, void* ws, size_t ws_bytes, double* eps2, const uint64_t* cursor,
                                  const uint64_t* thr3, double rho, uint64_t upper_total, uint64_t n_cap, uint64_t* status6, const uint64_t* sort_fail, hipStream_t stream) {
  if (!cursor || !thr3 || !status6 || !eps2) { ssg_set_error("ssg_eps_mean_check: null argument"); return SSG_ERR_INVALID; }
  EpsCheckArgs a; a.cursor = (const unsigned long long*)cursor; a.thr3 = (const unsigned long long*)thr3; a.rho = rho; a.upper_total = upper_total;
  a.top_guess = top_guess; a.n_cap = n_cap; a.status6 = (unsigned long long*)status6; a.sort_fail = (const unsigned long long*)sort_fail;
  return eps_mean_run_impl(sorted_keys, top_guess, mode, ws, ws_bytes, eps2, a, stream);
}
extern "C" int ssg_eps_mean(const uint64_t* sorted_keys, int64_t top, int mode, void* ws, size_t ws_bytes, double* out2, hipStream_t stream) {
  const int rc = ssg_eps_mean_prepare(top, ws, ws_bytes, stream);
  return rc ? rc : ssg_eps_mean_run(sorted_keys, top, mode, ws, ws_bytes, out2, stream);
}
