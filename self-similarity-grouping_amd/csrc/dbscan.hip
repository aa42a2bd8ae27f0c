// dbscan.hip -- K11 (DBSCAN region query), K12 (connected components).
//
// K11/K12 replace sklearn 1.7.2 DBSCAN(eps, min_samples, metric='precomputed').fit_predict
// (selftraining.py:295,306): neighbourhood = {k : d[i,k] <= eps} row-wise, core = count >=
// min_samples, clusters = connected components of core-core edges numbered by their
// smallest core index (== dbscan_inner's visiting order), border points take the smallest
// cluster id among their core neighbours, everything else is -1.
#include "matview.h"

namespace ssg {

// ------------------------------------------------------------------ K11 region query
// cnt[il] = #{k : d(i,k) <= eps} (self included when d(i,i) <= eps);  edges (i,k) incl. self hits.
struct Edge { int i, k; };

// append the hit columns (bit e of hitmask -> column j0+e) of this wave to its LDS stage (out of line: rare)
__device__ __forceinline__ int rq_append(WaveStage<Edge>& st, unsigned hitmask, int j0, int gi, Edge* eout, unsigned long long cap,
                                                   unsigned long long* cursor) {
  const int lane = lane_id();
  const uint64_t lt = lanemask_lt();
  int added = 0;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const bool h = (hitmask >> e) & 1u;
    const uint64_t m = __ballot(h);
    if (h) { Edge& x = st.buf[st.n + added + __popcll(m & lt)]; x.i = gi; x.k = j0 + e; }
    added += __popcll(m);
  }
  st.n += added;
  if (st.n > STAGE_CAP - 512) st.flush(eout, cap, cursor, lane);
  return added;
}

// generic chunk (row edges, unaligned rows, plain matrices): exact value of every element
template <int MODE>
__device__ __forceinline__ unsigned rq_generic_chunk(const MatView& mv, const RowStream& rs, int c, int lane, int gi, double eps) {
  double dv[8];
  load_vals<MODE>(mv, rs, c, lane, gi, dv);
  const int j0 = rs.col0(c, lane);
  unsigned hitmask = 0;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int k = j0 + e;
    if (k >= 0 && k < mv.N && dv[e] <= eps) hitmask |= 1u << e;
  }
  return hitmask;
}

// exact decision for the elements flagged by the packed-half prefilter (mode 0)
__device__ __forceinline__ unsigned rq_decide(const MatView& mv, unsigned flags, const uint4& xj, const uint4& xv, int gi, double eps) {
  const unsigned wj[4] = {xj.x, xj.y, xj.z, xj.w}, wv[4] = {xv.x, xv.y, xv.z, xv.w};
  const hbits vi = mv.v[gi];
  unsigned hitmask = 0;
  while (flags) {
    const int e = __ffs((int)flags) - 1;
    flags &= flags - 1;
    const unsigned a = e < 2 ? wj[0] : e < 4 ? wj[1] : e < 6 ? wj[2] : wj[3], b = e < 2 ? wv[0] : e < 4 ? wv[1] : e < 6 ? wv[2] : wv[3];
    const hbits jp = (hbits)((a >> ((e & 1) * 16)) & 0xffffu), vk = (hbits)((b >> ((e & 1) * 16)) & 0xffffu);
    if (final_dist_value(jp, vi, vk, mv.lambda_value) <= eps) hitmask |= 1u << e;    // exact, rerank.py:122
  }
  return hitmask;
}

template <int MODE>
__global__ __launch_bounds__(256) void region_query_kernel(MatView mv, double eps_arg, int32_t* __restrict__ cnt, int32_t* __restrict__ edges,
                                                           unsigned long long cap, unsigned long long* __restrict__ cursor,
                                                           const unsigned long long* __restrict__ gate, const unsigned char* __restrict__ rowmask,
                                                           const double* __restrict__ eps_dev) {
  __shared__ Edge sbuf[4][STAGE_CAP];
  if (gate && *gate == 0ull) return;          // the sparse pass queued in front of this launch has done every row
  const double eps = eps_dev ? *eps_dev : eps_arg;     // round 5: eps left on the device by the eps rule queued in front (NaN = "no eps": no hit)
  const int lane = lane_id();
  WaveStage<Edge> st{sbuf[threadIdx.x >> 6], 0};
  Edge* eout = reinterpret_cast<Edge*>(edges);
  // mode-0 prefilter in packed half math (2 elements per instruction): d16 = half(v_i+v_k)*half(lambda) + J' is
  // within `band` of the exact float64 value, so only elements with d16 < eps + band can be hits; those (a
  // handful per row) are decided exactly.  half(v_i + v_k) with the native half add equals numpy's
  // float32-add-then-round for every pair of halves.
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const float bandf = 0.0078125f * (1.f + fabsf((float)eps) + fabsf((float)mv.lambda_value));   // >= 2^-9*lambda*|s| + 3*2^-11*|d| with margin
  const _Float16 thr16 = (_Float16)((float)eps + bandf + 0.002f * (1.f + fabsf((float)eps)));   // margin also covers the rounding of the threshold itself
  const h2 thr2 = {thr16, thr16};
  const h2 lam2 = {(_Float16)(float)mv.lambda_value, (_Float16)(float)mv.lambda_value};
  const bool fast_ok = MODE == 0 && (mv.N & 7) == 0 && (float)eps < 30000.f && fabsf((float)mv.lambda_value) < 16.f;
  for (int il = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); il < mv.nrows; il += (int)gridDim.x * 4) {
    if (rowmask && rowmask[il] == 0) continue;     // done through the sparse copy
    const int gi = mv.row0 + il;
    RowStream rs(il, mv.N, mv.nrows);
    int rowcnt = 0;
    if (fast_ok) {
      // N % 8 == 0: every row starts on a 16-byte boundary, all chunks are aligned; the last one may be partial
      const hbits* M = reinterpret_cast<const hbits*>(mv.M) + (int64_t)il * mv.N;
      const _Float16 vi16 = __builtin_bit_cast(_Float16, mv.v[gi]);
      const h2 vi2 = {vi16, vi16};
      const int nfull = mv.N / 512;
      for (int cb = 0; cb < nfull; cb += PIPE) {
        uint4 xjs[PIPE], xvs[PIPE];
#pragma unroll
        for (int u = 0; u < PIPE; u++) {
          const int j0 = min(cb + u, nfull - 1) * 512 + lane * 8;       // clamped: the loads of a short tail are repeated, never out of range
          xjs[u] = *reinterpret_cast<const uint4*>(M + j0);
          xvs[u] = *reinterpret_cast<const uint4*>(mv.v + j0);
        }
#pragma unroll
        for (int u = 0; u < PIPE; u++) {
          const int c = cb + u;
          if (c >= nfull) break;
          const int j0 = c * 512 + lane * 8;
          const uint4 xj = xjs[u], xv = xvs[u];
          const unsigned wj[4] = {xj.x, xj.y, xj.z, xj.w}, wv[4] = {xv.x, xv.y, xv.z, xv.w};
          unsigned flags = 0;   // bit e set: element e may be <= eps
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const h2 s2 = __builtin_bit_cast(h2, wv[q]) + vi2;
            const h2 d2 = s2 * lam2 + __builtin_bit_cast(h2, wj[q]);
            const unsigned sg = __builtin_bit_cast(unsigned, (h2)(d2 - thr2));     // sign bit set <=> d16 < thr (NaNs never hit)
            flags |= ((sg >> 15) & 1u) << (2 * q) | ((sg >> 31) & 1u) << (2 * q + 1);
          }
          if (!__any(flags != 0)) continue;                         // the common case: one branch per KiB
          const unsigned hitmask = rq_decide(mv, flags, xj, xv, gi, eps);
          if (__any(hitmask != 0)) rowcnt += rq_append(st, hitmask, j0, gi, eout, cap, cursor);
        }
      }
      if (nfull * 512 < mv.N) {
        const unsigned hitmask = rq_generic_chunk<MODE>(mv, rs, nfull, lane, gi, eps);
        if (__any(hitmask != 0)) rowcnt += rq_append(st, hitmask, rs.col0(nfull, lane), gi, eout, cap, cursor);
      }
    } else {
      for (int c = 0; c < rs.nchunks; c++) {
        const unsigned hitmask = rq_generic_chunk<MODE>(mv, rs, c, lane, gi, eps);
        if (__any(hitmask != 0)) rowcnt += rq_append(st, hitmask, rs.col0(c, lane), gi, eout, cap, cursor);
      }
    }
    if (lane == 0) cnt[il] = rowcnt;
  }
  block_flush(st, eout, cap, cursor);
}

// region query on S: row i is walked through S when floor_i = f64(J'(0)) + f64(half(v_i + vmin)) * lambda > eps (no column outside S can
// be a neighbour then); other rows (all rows when S is unusable) get rowmask = 1 and raise cursor[1] for the dense pass behind this launch
__global__ __launch_bounds__(256) void region_query_sparse_kernel(MatView mv, SparseView sv, double eps_arg, int32_t* __restrict__ cnt, int32_t* __restrict__ edges,
                                                                  unsigned long long cap, unsigned long long* __restrict__ cursor,
                                                                  unsigned char* __restrict__ rowmask, const double* __restrict__ eps_dev) {
  __shared__ Edge sbuf[4][SPARSE_STAGE];
  const double eps = eps_dev ? *eps_dev : eps_arg;
  const int lane = lane_id();
  WaveStage<Edge> st{sbuf[threadIdx.x >> 6], 0};
  Edge* eout = reinterpret_cast<Edge*>(edges);
  const bool usable = sparse_usable(sv, mv);
  const hbits vmin = usable ? (hbits)*sv.vmin : (hbits)0;
  bool anydense = false;
  for (int il = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); il < mv.nrows; il += (int)gridDim.x * 4) {
    const int gi = mv.row0 + il;
    const hbits vi = mv.v[gi];
    const bool rowok = usable && final_dist_value(sv.jp0, vi, vmin, mv.lambda_value) > eps;
    if (lane == 0) rowmask[il] = rowok ? 0 : 1;
    if (!rowok) { anydense = true; continue; }
    int rowcnt = 0;
    for (int sg = 0; sg < sv.nseg; sg++) {
      const int64_t off = sv.seg_off[(int64_t)il * sv.nseg + sg];
      const int len = sv.seg_len[(int64_t)il * sv.nseg + sg];
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
          const int k = (int)(e[u] & 0x1ffffu);
          const bool hit = q < len && final_dist_value((hbits)(e[u] >> 17), vi, vk[u], mv.lambda_value) <= eps;     // exact, rerank.py:122
          const uint64_t bm = __ballot(hit);
          if (bm) {
            if (hit) { Edge ed; ed.i = gi; ed.k = k; st.buf[st.n + __popcll(bm & lanemask_lt())] = ed; }
            st.n += __popcll(bm); rowcnt += __popcll(bm);
            if (st.n > SPARSE_STAGE - 64) st.flush(eout, cap, cursor, lane);
          }
        }
      }
    }
    if (lane == 0) cnt[il] = rowcnt;
  }
  block_flush(st, eout, cap, cursor);
  if (lane == 0 && anydense) cursor[1] = 1ull;
}

// ------------------------------------------------------------------ K12 union-find
__device__ __forceinline__ int uf_load(int* parent, int x) { return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ int uf_find(int* parent, int x) {
  for (;;) {
    const int p = uf_load(parent, x);
    if (p == x) return x;
    const int gp = uf_load(parent, p);
    if (gp != p) atomicMin(&parent[x], gp);   // path halving; parents only ever decrease
    x = p;
  }
}
__device__ void uf_union(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a); b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    if (atomicCAS(&parent[b], b, a) == b) return;   // hook the larger root under the smaller
  }
}
__global__ void cc_init_kernel(const int32_t* __restrict__ cnt, int N, int min_samples, int* __restrict__ parent, int* __restrict__ lab) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < N) { parent[i] = i; lab[i] = 0x7fffffff; (void)cnt; (void)min_samples; }
}
// The region query emits a row's edges (i, k1), (i, k2), ... next to each other, so a wave holds runs of lanes with the same i.  The lanes
// of a run agree on m = min(k1, k2, ...) over the run's core-core edges (a segmented min: 12 shuffles); `first` marks the run's first lane.
__device__ __forceinline__ void cc_run_min(const int32_t* __restrict__ edges, unsigned long long e, unsigned long long ne, const int32_t* __restrict__ cnt,
                                           int min_samples, int lane, int& i, int& k, bool& valid, int& m, bool& first) {
  i = -1 - lane; k = 0x7fffffff; valid = false;                                   // (idle lanes: a run of their own)
  if (e < ne) {
    i = edges[2 * e]; const int kk = edges[2 * e + 1];
    valid = i != kk && cnt[i] >= min_samples && cnt[kk] >= min_samples;
    if (valid) k = kk;
  }
  m = k;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int oi = __shfl_up(i, d, 64), om = __shfl_up(m, d, 64);
    if (lane >= d && oi == i) m = om < m ? om : m;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int oi = __shfl_down(i, d, 64), om = __shfl_down(m, d, 64);
    if (lane + d < 64 && oi == i) m = om < m ? om : m;
  }
  const int pi = __shfl_up(i, 1, 64);
  first = lane == 0 || pi != i;
}
// Pass 1 (round 5): every core point is hooked under its smallest core neighbour with ONE fire-and-forget atomicMin per run -- no find,
// no compare-and-swap, no dependent chain of device-scope accesses (each is ~1.5 us on this part: the L2s of the 8 XCDs are not coherent
// with each other, a device-scope access goes out to the fabric).  parent[i] <= i stays a valid forest inside i's component; a clique --
// what a DBSCAN cluster mostly is -- ends with every member pointing at its smallest one.
__global__ void cc_hook_kernel(const int32_t* __restrict__ edges, unsigned long long ne, const unsigned long long* __restrict__ ne_dev,
                               const int32_t* __restrict__ cnt, int min_samples, int* __restrict__ parent) {
  if (ne_dev) { const unsigned long long d = *ne_dev; ne = d < ne ? d : ne; }     // device-side count (region query cursor), capped by the capacity
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long eb = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x - lane; eb < ne; eb += stride) {     // (wave-uniform trip count)
    int i, k, m; bool valid, first;
    cc_run_min(edges, eb + lane, ne, cnt, min_samples, lane, i, k, valid, m, first);
    if (first && m < i) atomicMin(&parent[i], m);                                  // (m < i implies the run holds a core-core edge, so i is core)
  }
}
// Pass 2: the union-find proper, for the edges pass 1 left open.  Two rounds of plain loads (an ancestor read a moment too early is still
// an ancestor in the same component) show for nearly every edge that both ends already hang under the same point; the rest is united
// with the lock-free find / compare-and-swap above.  (Before pass 1 existed every edge paid two finds and a compare-and-swap, the lanes
// of a run with k < i one winner at a time: 77 us at N = 16 000; hooking the run's k to the run's minimum instead: 60 us.)
__global__ void cc_union_kernel(const int32_t* __restrict__ edges, unsigned long long ne, const unsigned long long* __restrict__ ne_dev,
                                const int32_t* __restrict__ cnt, int min_samples,
                                int* __restrict__ parent) {
  if (ne_dev) { const unsigned long long d = *ne_dev; ne = d < ne ? d : ne; }
  for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (unsigned long long)gridDim.x * blockDim.x) {
    const int i = edges[2 * e], k = edges[2 * e + 1];
    if (i == k || cnt[i] < min_samples || cnt[k] < min_samples) continue;
    const int hi = parent[i], hk = parent[k];
    if (hi == hk) continue;
    const int gi = parent[hi], gk = parent[hk];
    if (gi != gk) uf_union(parent, gi, gk);
  }
}
// rootflag[i] = 1 iff i is a core point that is the root (= smallest index) of its component
__global__ void cc_flatten_kernel(const int32_t* __restrict__ cnt, int N, int min_samples, int* __restrict__ parent, int32_t* __restrict__ rootflag) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= N) return;
  int r = i;
  if (cnt[i] >= min_samples) { r = uf_find(parent, i); parent[i] = r; }
  rootflag[i] = (cnt[i] >= min_samples && r == i) ? 1 : 0;
}
__global__ void cc_label_core_kernel(const int32_t* __restrict__ cnt, int N, int min_samples, const int* __restrict__ parent,
                                     const int64_t* __restrict__ rootid, int* __restrict__ lab) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < N && cnt[i] >= min_samples) lab[i] = (int)rootid[parent[i]];
}
// border points take the smallest label among their core neighbours; the same launch labels the core points (disjoint entries of lab)
__global__ void cc_border_kernel(const int32_t* __restrict__ edges, unsigned long long ne, const unsigned long long* __restrict__ ne_dev,
                                 const int32_t* __restrict__ cnt, int min_samples,
                                 const int* __restrict__ parent, const int64_t* __restrict__ rootid, int* __restrict__ lab, int N) {
  if (ne_dev) { const unsigned long long d = *ne_dev; ne = d < ne ? d : ne; }
  const unsigned long long gid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = gid; i < (unsigned long long)N; i += stride)
    if (cnt[i] >= min_samples) lab[i] = (int)rootid[parent[i]];
  for (unsigned long long e = gid; e < ne; e += stride) {
    const int i = edges[2 * e], k = edges[2 * e + 1];
    if (cnt[i] >= min_samples && cnt[k] < min_samples) atomicMin(&lab[k], (int)rootid[parent[i]]);
  }
}
__global__ void cc_finalize_kernel(const int* __restrict__ lab, int N, int64_t* __restrict__ labels) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < N) labels[i] = lab[i] == 0x7fffffff ? -1 : (int64_t)lab[i];
}

}  // namespace ssg

using namespace ssg;
// exscan_kernel (exclusive scan that also clears its input) comes from jaccard.hip: the
// library is built as one translation unit (ssg_hip.hip).

static int region_query_impl(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, double eps, const double* eps_dev,
                             int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor, hipStream_t stream) {
  int rc = check_view("ssg_region_query", M, v, N, row0, nrows, mode); if (rc) return rc;
#define SSG_RQ(MD) hipLaunchKernelGGL(region_query_kernel<MD>, dim3(stream_grid(nrows)), dim3(256), 0, stream, make_view(M, v, N, row0, nrows, mode, lambda_value), eps, \
                     cnt, edges, (unsigned long long)cap_edges, (unsigned long long*)cursor, (const unsigned long long*)nullptr, (const unsigned char*)nullptr, eps_dev)
  if (mode == 0) SSG_RQ(0); else if (mode == 1) SSG_RQ(1); else SSG_RQ(2);
#undef SSG_RQ
  SSG_LAUNCH_CHECK("region_query_kernel");
  return SSG_OK;
}
extern "C" int ssg_region_query(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, double eps,
                                int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor, hipStream_t stream) {
  return region_query_impl(M, v, N, row0, nrows, mode, lambda_value, eps, nullptr, cnt, edges, cap_edges, cursor, stream);
}
// round 5: eps is read from device memory (what ssg_eps_check left there), so that eps rule -> region query -> components run back
// to back without the host seeing eps in between; a NaN there means "the eps rule's fast path did not verify": no hit, the caller redoes
extern "C" int ssg_region_query_dev(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, const double* eps_dev,
                                    int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor, hipStream_t stream) {
  if (!eps_dev) { ssg_set_error("ssg_region_query_dev: null eps"); return SSG_ERR_INVALID; }
  return region_query_impl(M, v, N, row0, nrows, mode, lambda_value, 0.0, eps_dev, cnt, edges, cap_edges, cursor, stream);
}

// Region query through the sparse copy S of J': cursor2 = {edges counted, dense pass needed} zeroed by the caller, rowmask = nrows bytes
// of workspace.  Row i goes through S when J'(0) + lambda * half(v_i + vmin) > eps; the other rows (all of them when S overflowed) are
// flagged and done by the dense pass queued behind, gated on cursor2[1].  Same outputs as ssg_region_query.
static int region_query_s_impl(const void* M, const uint16_t* v, int N, int row0, int nrows, double lambda_value, double eps, const double* eps_dev,
                               const uint32_t* s_pool, const int64_t* seg_off, const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin,
                               uint16_t jp0_half, uint8_t* rowmask, int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor2, hipStream_t stream) {
  int rc = check_view("ssg_region_query_s", M, v, N, row0, nrows, 0); if (rc) return rc;
  if (!s_pool || !seg_off || !seg_len || nseg <= 0 || !s_cursor || !vmin || !rowmask) { ssg_set_error("ssg_region_query_s: no sparse copy"); return SSG_ERR_INVALID; }
  const MatView mv = make_view(M, v, N, row0, nrows, 0, lambda_value);
  hipLaunchKernelGGL(region_query_sparse_kernel, dim3(stream_grid(nrows)), dim3(256), 0, stream, mv, make_sparse(s_pool, seg_off, seg_len, nseg, s_cursor, vmin, jp0_half),
                     eps, cnt, edges, (unsigned long long)cap_edges, (unsigned long long*)cursor2, rowmask, eps_dev);
  hipLaunchKernelGGL(region_query_kernel<0>, dim3(stream_grid(nrows)), dim3(256), 0, stream, mv, eps, cnt, edges, (unsigned long long)cap_edges,
                     (unsigned long long*)cursor2, (const unsigned long long*)(cursor2 + 1), (const unsigned char*)rowmask, eps_dev);
  SSG_LAUNCH_CHECK("region_query_sparse_kernel");
  return SSG_OK;
}
extern "C" int ssg_region_query_s(const void* M, const uint16_t* v, int N, int row0, int nrows, double lambda_value, double eps, const uint32_t* s_pool,
                                  const int64_t* seg_off, const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin,
                                  uint16_t jp0_half, uint8_t* rowmask, int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor2,
                                  hipStream_t stream) {
  return region_query_s_impl(M, v, N, row0, nrows, lambda_value, eps, nullptr, s_pool, seg_off, seg_len, nseg, s_cursor, vmin, jp0_half, rowmask, cnt, edges, cap_edges,
                             cursor2, stream);
}
extern "C" int ssg_region_query_s_dev(const void* M, const uint16_t* v, int N, int row0, int nrows, double lambda_value, const double* eps_dev, const uint32_t* s_pool,
                                      const int64_t* seg_off, const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin,
                                      uint16_t jp0_half, uint8_t* rowmask, int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor2,
                                      hipStream_t stream) {
  if (!eps_dev) { ssg_set_error("ssg_region_query_s_dev: null eps"); return SSG_ERR_INVALID; }
  return region_query_s_impl(M, v, N, row0, nrows, lambda_value, 0.0, eps_dev, s_pool, seg_off, seg_len, nseg, s_cursor, vmin, jp0_half, rowmask, cnt, edges, cap_edges,
                             cursor2, stream);
}

// workspace: parent[N] int32 | lab[N] int32 | rootflag[N] int32 | rootid[N+1] int64
extern "C" size_t ssg_dbscan_cc_workspace_bytes(int N) { return (size_t)N * 12 + ((size_t)N + 1) * 8 + 64; }

static int dbscan_cc_impl(const int32_t* cnt, const int32_t* edges, uint64_t nedges, const unsigned long long* ne_dev, int N, int min_samples, void* ws,
                          size_t ws_bytes, int64_t* labels, hipStream_t stream) {
  if (N <= 0 || ws_bytes < ssg_dbscan_cc_workspace_bytes(N)) { ssg_set_error("ssg_dbscan_cc: workspace too small"); return SSG_ERR_INVALID; }
  int* parent = (int*)ws; int* lab = parent + N; int32_t* rootflag = lab + N;
  int64_t* rootid = (int64_t*)(((uintptr_t)(rootflag + N) + 15) & ~(uintptr_t)15);
  const int nb = (N + 255) / 256;
  const int eb = nedges ? (int)((nedges + 255) / 256 < 8192 ? (nedges + 255) / 256 : 8192) : 1;
  hipLaunchKernelGGL(cc_init_kernel, dim3(nb), dim3(256), 0, stream, cnt, N, min_samples, parent, lab);
  if (nedges) {
    hipLaunchKernelGGL(cc_hook_kernel, dim3(eb), dim3(256), 0, stream, edges, (unsigned long long)nedges, ne_dev, cnt, min_samples, parent);
    hipLaunchKernelGGL(cc_union_kernel, dim3(eb), dim3(256), 0, stream, edges, (unsigned long long)nedges, ne_dev, cnt, min_samples, parent);
  }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(nb), dim3(256), 0, stream, cnt, N, min_samples, parent, rootflag);
  hipLaunchKernelGGL(exscan_kernel, dim3(1), dim3(1024), 0, stream, rootflag, N, rootid);
  if (nedges) hipLaunchKernelGGL(cc_border_kernel, dim3(eb > nb ? eb : nb), dim3(256), 0, stream, edges, (unsigned long long)nedges, ne_dev, cnt, min_samples, parent, rootid, lab, N);
  else hipLaunchKernelGGL(cc_label_core_kernel, dim3(nb), dim3(256), 0, stream, cnt, N, min_samples, parent, rootid, lab);
  // labels == NULL (round 6): the caller reads lab = (int32*)ws + N itself (0x7fffffff = noise) -- one launch less in a chain that reads the workspace back anyway
  if (labels) hipLaunchKernelGGL(cc_finalize_kernel, dim3(nb), dim3(256), 0, stream, lab, N, labels);
  SSG_LAUNCH_CHECK("dbscan_cc");
  return SSG_OK;
}

extern "C" int ssg_dbscan_cc(const int32_t* cnt, const int32_t* edges, uint64_t nedges, int N, int min_samples, void* ws, size_t ws_bytes,
                             int64_t* labels, hipStream_t stream) {
  return dbscan_cc_impl(cnt, edges, nedges, nullptr, N, min_samples, ws, ws_bytes, labels, stream);
}
// the same with the edge count left on the device: edges holds min(*nedges_dev, cap_edges) entries (the region query's cursor
// and capacity), so region query -> components -> labels runs without a host round trip in between
extern "C" int ssg_dbscan_cc_dev(const int32_t* cnt, const int32_t* edges, const uint64_t* nedges_dev, uint64_t cap_edges, int N, int min_samples,
                                 void* ws, size_t ws_bytes, int64_t* labels, hipStream_t stream) {
  if (!nedges_dev) { ssg_set_error("ssg_dbscan_cc_dev: null edge counter"); return SSG_ERR_INVALID; }
  return dbscan_cc_impl(cnt, edges, cap_edges, (const unsigned long long*)nedges_dev, N, min_samples, ws, ws_bytes, labels, stream);
}
