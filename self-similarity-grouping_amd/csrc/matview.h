// matview.h -- what the matrix passes of the eps rule (eps_rule.hip) and of DBSCAN (dbscan.hip) share: the view of the distance
// matrix, the row streaming, the per-wave LDS staging of results, the view of the sparse copy S of J', and the host helpers that
// build the views and size the persistent grid.
//
// The matrix is never materialised in f64: mode 0 rebuilds final_dist from the compact
// half J' and the source vector v (reid/rerank.py:122), mode 1 reads a plain half matrix
// (the no-rerank euclidean_dist).  All matrix passes are HBM-read-bound (2 bytes/entry).
#pragma once
#include "ssg_common.h"

namespace ssg {

struct MatView {
  const void* M;       // [nrows, N] rows of this row block: half (mode 0/1) or double (mode 2)
  const hbits* v;      // [N] source vector (mode 0) or null
  int N, row0, nrows, mode;
  double lambda_value;
};

// Row streaming shared by the matrix passes: one wave per row, 8 consecutive elements per
// lane per chunk (16 B of half / 64 B of double), chunks aligned to 8 elements of the block.
struct RowStream {
  int64_t total, al; int first, nchunks;
  __device__ __forceinline__ RowStream(int row, int N, int nrows) {
    total = (int64_t)nrows * N;
    const int64_t base = (int64_t)row * N;
    al = base & ~(int64_t)7; first = (int)(base - al); nchunks = (first + N + 511) / 512;
  }
  __device__ __forceinline__ int col0(int c, int lane) const { return c * 512 + lane * 8 - first; }
};

// d[e] = value of column col0+e of row gi (garbage for columns outside [0,N): callers mask)
template <int MODE>
__device__ __forceinline__ void load_vals(const MatView& mv, const RowStream& rs, int c, int lane, int gi, double d[8]) {
  const int64_t off = rs.al + (int64_t)c * 512 + lane * 8;
  if (MODE == 2) {
    const double* M = reinterpret_cast<const double*>(mv.M);
    if (off + 8 <= rs.total) {
#pragma unroll
      for (int q = 0; q < 4; q++) { const double2 t = *reinterpret_cast<const double2*>(M + off + 2 * q); d[2 * q] = t.x; d[2 * q + 1] = t.y; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) d[e] = (off + e < rs.total) ? M[off + e] : 0.0;
    }
    return;
  }
  const hbits* M = reinterpret_cast<const hbits*>(mv.M);
  unsigned w[4] = {0, 0, 0, 0};
  if (off + 8 <= rs.total) { const uint4 x = *reinterpret_cast<const uint4*>(M + off); w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w; }
  else if (off < rs.total) {
#pragma unroll
    for (int e = 0; e < 8; e++) if (off + e < rs.total) w[e >> 1] |= (unsigned)M[off + e] << ((e & 1) * 16);
  }
  const int j0 = rs.col0(c, lane);
  unsigned vw[4] = {0, 0, 0, 0};   // v[j0 .. j0+7] (mode 0)
  if (MODE == 0) {
    if (j0 >= 0 && j0 + 8 <= mv.N && (j0 & 7) == 0) {   // rows start on 16-byte boundaries when N % 8 == 0: one load
      const uint4 x = *reinterpret_cast<const uint4*>(mv.v + j0); vw[0] = x.x; vw[1] = x.y; vw[2] = x.z; vw[3] = x.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) { const int k = j0 + e; if (k >= 0 && k < mv.N) vw[e >> 1] |= (unsigned)mv.v[k] << ((e & 1) * 16); }
    }
  }
  const hbits vi = MODE == 0 ? mv.v[gi] : (hbits)0;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const hbits raw = (hbits)((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
    if (MODE == 0) d[e] = final_dist_value(raw, vi, (hbits)((vw[e >> 1] >> ((e & 1) * 16)) & 0xffffu), mv.lambda_value);
    else d[e] = (double)h2f(raw);
  }
}

// The same in two steps for the half modes, so that a streaming loop can keep several chunks' loads in flight before it
// decodes the first one (one 1 KiB load per wave at a time leaves the pass latency-bound at ~2.3 TB/s).
struct RawChunk { uint4 m, v; };
template <int MODE>
__device__ __forceinline__ RawChunk load_raw(const MatView& mv, const RowStream& rs, int c, int lane) {
  static_assert(MODE == 0 || MODE == 1, "half matrices only");
  RawChunk r; r.m = make_uint4(0, 0, 0, 0); r.v = make_uint4(0, 0, 0, 0);
  const int64_t off = rs.al + (int64_t)c * 512 + lane * 8;
  const hbits* M = reinterpret_cast<const hbits*>(mv.M);
  if (c < rs.nchunks) {
    if (off + 8 <= rs.total) r.m = *reinterpret_cast<const uint4*>(M + off);
    else if (off < rs.total) {
      unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < 8; e++) if (off + e < rs.total) w[e >> 1] |= (unsigned)M[off + e] << ((e & 1) * 16);
      r.m = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (MODE == 0) {
      const int j0 = rs.col0(c, lane);
      if (j0 >= 0 && j0 + 8 <= mv.N && (j0 & 7) == 0) r.v = *reinterpret_cast<const uint4*>(mv.v + j0);
      else {
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; e++) { const int k = j0 + e; if (k >= 0 && k < mv.N) w[e >> 1] |= (unsigned)mv.v[k] << ((e & 1) * 16); }
        r.v = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
  return r;
}
template <int MODE>
__device__ __forceinline__ void decode_raw(const MatView& mv, const RawChunk& r, hbits vi, double d[8]) {
  const unsigned w[4] = {r.m.x, r.m.y, r.m.z, r.m.w}, vw[4] = {r.v.x, r.v.y, r.v.z, r.v.w};
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const hbits raw = (hbits)((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
    if (MODE == 0) d[e] = final_dist_value(raw, vi, (hbits)((vw[e >> 1] >> ((e & 1) * 16)) & 0xffffu), mv.lambda_value);
    else d[e] = (double)h2f(raw);
  }
}
constexpr int PIPE = 4;     // chunks (4 KiB of the matrix per wave) in flight in the streaming passes

// Per-wave staging buffer in LDS: results are appended with ballot prefix sums and flushed to a
// global list with ONE cursor atomic per ~512 entries (a per-chunk atomic on one word saturates
// at ~90 ops/us and was the bottleneck of the first version).
constexpr int STAGE_CAP = 1024;
template <typename T>
struct WaveStage {
  T* buf; int n;
  __device__ __forceinline__ void flush(T* __restrict__ out, unsigned long long cap, unsigned long long* __restrict__ cursor, int lane) {
    if (n == 0) return;
    unsigned long long basep = 0;
    if (lane == 0) basep = atomicAdd(cursor, (unsigned long long)n);
    basep = (unsigned long long)__shfl((long long)basep, 0, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int x = lane; x < n; x += 64) if (basep + x < cap) out[basep + x] = buf[x];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    n = 0;
  }
};

// Final flush of a workgroup's four wave stages with ONE cursor atomic (the sparse passes end with a few dozen staged entries per wave:
// a returning atomic per wave on one word -- ~90 per us -- was their whole run time, 5120 waves = 57 us).  Every thread of the block calls it.
template <typename T>
__device__ __forceinline__ void block_flush(WaveStage<T>& st, T* __restrict__ out, unsigned long long cap, unsigned long long* __restrict__ cursor) {
  __shared__ unsigned long long bf_base;
  __shared__ int bf_n[4];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) bf_n[wave] = st.n;
  __syncthreads();
  if (threadIdx.x == 0) { const int tot = bf_n[0] + bf_n[1] + bf_n[2] + bf_n[3]; bf_base = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull; }
  __syncthreads();
  unsigned long long basep = bf_base;
  for (int w = 0; w < wave; w++) basep += (unsigned long long)bf_n[w];
  for (int x = lane; x < st.n; x += 64) if (basep + x < cap) out[basep + x] = st.buf[x];
  st.n = 0;
}

// ------------------------------------------------------------------ round 4: the sparse copy S of J' (jaccard.hip, second generation)
// S holds, per (row, column chunk), the packed words (J' << 17 | column) of every column the row's Jaccard walk touched; every other
// column of the row holds the constant J'(0) = half(1 - lambda), the LARGEST value J' takes.  final_dist = J' + lambda * half(v_i + v_k)
// with v >= 0 and lambda >= 0, so an entry of row i outside S is >= J'(0) + lambda * half(v_i + min_k v_k) =: floor_i (every operation in
// that expression is monotone in v_k): while the bound a pass asks about stays below floor_i, only S can hold what it looks for in
// row i -- a few hundred entries instead of N.  The decision is taken PER ROW on the device: rows whose floor is too low (and all
// rows when S is incomplete) are flagged in a row mask and done by the dense pass queued behind the sparse one.
constexpr int SBATCH = 4;
constexpr int SPARSE_STAGE = 256;        // per-wave staging entries of the sparse passes (a row yields a handful of keys / edges)
struct SparseView {
  const uint32_t* pool; const int64_t* seg_off; const int32_t* seg_len; int nseg;
  const unsigned long long* s_cursor;      // [1] != 0: a segment did not fit, S is unusable
  const uint32_t* vmin;                    // half bits of min_k v_k
  hbits jp0;                               // J'(0)
};
// Can S be used at all?  (all lanes agree)
__device__ __forceinline__ bool sparse_usable(const SparseView& sv, const MatView& mv) {
  return sv.pool && mv.mode == 0 && sv.s_cursor[1] == 0ull && mv.lambda_value >= 0.0 && (sv.jp0 & 0x7fffu) != 0 && (sv.jp0 & 0x7fffu) < 0x7c00u &&
         (sv.jp0 & 0x8000u) == 0;
}

}  // namespace ssg

using namespace ssg;

static MatView make_view(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value) {
  MatView mv; mv.M = M; mv.v = v; mv.N = N; mv.row0 = row0; mv.nrows = nrows; mv.mode = mode; mv.lambda_value = lambda_value;
  return mv;
}
static int check_view(const char* fn, const void* M, const uint16_t* v, int N, int row0, int nrows, int mode) {
  if (!M || N <= 0 || nrows <= 0 || row0 < 0 || row0 + nrows > N || mode < 0 || mode > 2 || (mode == 0 && !v)) {
    ssg_set_error("%s: bad matrix view (N=%d row0=%d nrows=%d mode=%d)", fn, N, row0, nrows, mode);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}
// Persistent grid: ~5 workgroups per CU.  Every wave walks many rows and publishes its staged results with one
// cursor atomic per ~500 entries; one wave per row meant N cursor / histogram atomics on a single word
// (one word saturates at ~90 atomics/us: 16 000 rows = 0.18 ms of pure serialisation).
// The grid is then trimmed so that every wave walks the SAME number of rows: 16 000 rows on 5120 waves are 3.1 rows per wave, i.e.
// most waves finish after 3 rows and wait for the ones that got 4 (region query 0.18 ms); 4000 waves x exactly 4 rows: 0.15 ms.
static int stream_grid(int nrows) {
  constexpr int cap = 1280;
  const int b = (nrows + 3) / 4;                        // one row per wave, four waves per workgroup
  if (b <= cap) return b;
  const int per_wave = (nrows + 4 * cap - 1) / (4 * cap);          // rows per wave at the cap
  return (nrows + 4 * per_wave - 1) / (4 * per_wave);
}

static SparseView make_sparse(const uint32_t* pool, const int64_t* seg_off, const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin,
                              uint16_t jp0) {
  SparseView sv; sv.pool = pool; sv.seg_off = seg_off; sv.seg_len = seg_len; sv.nseg = nseg; sv.s_cursor = (const unsigned long long*)s_cursor; sv.vmin = vmin; sv.jp0 = jp0;
  return sv;
}
