// sort_u64.hip -- the general u64 sorts behind the eps rule (eps_rule.hip sorts the compacted float64 keys of K10 with them) and the
// concatenation of fixed-capacity segments the sharded chain feeds them with:
//   ssg_sort_u64 / ssg_sort_u64_dev      one bitonic network, its length given by the host or left on the device by the pass in front;
//   ssg_samplesort_u64_dev / _big_dev    sample sort of a device-sized list in two geometries (1023 / 4095 splitters);
//   ssg_fill_u64, ssg_concat_segments_u64.
#include "ssg_common.h"

namespace ssg {

// ------------------------------------------------------------------ bitonic sort (u64, ascending)
constexpr int SORT_CH = 2048;
__device__ __forceinline__ void cswap(unsigned long long& a, unsigned long long& b, bool up) {
  if ((a > b) == up) { const unsigned long long t = a; a = b; b = t; }
}
// ---- round 5: the eps rule without a host round trip between its full pass and the mean -------------------------------------------
// The number of collected keys stays on the device (cursor[0] of the compaction pass).  The sort network is LAUNCHED for the capacity
// n_cap (a power of two) but every kernel works on n_eff = the power of two >= max(*n_dev, SORT_CH) only: merge levels k > n_eff and
// workgroups past n_eff exit at once (a handful of empty launches of ~2 us instead of a blocking read + a restart of the launch queue).
__device__ __forceinline__ unsigned long long sort_n_eff(const unsigned long long* n_dev, unsigned long long n_cap) {
  unsigned long long n = *n_dev, e = (unsigned long long)SORT_CH;
  if (n > n_cap) n = n_cap;                     // (overflow of the compaction buffer: the check kernel reports it, the result is discarded)
  while (e < n) e <<= 1;
  return e;
}
// The kernels below exist once.  DEV = true: the length is n_eff as above (ssg_sort_u64_dev); DEV = false: the host knows the length, it is
// n_cap itself and n_dev is not read (ssg_sort_u64, ssg_fill_u64).
// p[n0 .. n1) = v with n0 = min(*n_dev, n_cap), n1 = n_eff (DEV) or n0 = 0, n1 = n_cap
template <bool DEV>
__global__ void fill_u64_kernel(unsigned long long* p, const unsigned long long* __restrict__ n_dev, unsigned long long n_cap, unsigned long long v) {
  const unsigned long long n1 = DEV ? sort_n_eff(n_dev, n_cap) : n_cap;
  unsigned long long n0 = 0;
  if (DEV) { n0 = *n_dev; if (n0 > n_cap) n0 = n_cap; }
  for (unsigned long long i = n0 + blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n1; i += (unsigned long long)gridDim.x * blockDim.x) p[i] = v;
}
// k_lo..k_hi: run all (k, j) stages with j < SORT_CH inside LDS.  For k <= SORT_CH this is a full
// local sort; for k > SORT_CH only the tail j = SORT_CH/2 .. 1 of stage k.
template <bool DEV>
__global__ __launch_bounds__(1024) void bitonic_local_kernel(unsigned long long* __restrict__ a, unsigned long long k_first, unsigned long long k_last,
                                                             const unsigned long long* __restrict__ n_dev, unsigned long long n_cap) {
  __shared__ unsigned long long s[SORT_CH];
  const unsigned long long n_eff = DEV ? sort_n_eff(n_dev, n_cap) : n_cap;
  const unsigned long long g0 = (unsigned long long)blockIdx.x * SORT_CH;
  if (g0 >= n_eff || k_first > n_eff) return;           // (uniform per workgroup)
  const int t = (int)threadIdx.x;
  s[t] = a[g0 + t]; s[t + 1024] = a[g0 + t + 1024];
  __syncthreads();
  for (unsigned long long k = k_first; k <= k_last; k <<= 1) {
    for (unsigned long long j = (k >> 1) < (unsigned long long)(SORT_CH / 2) ? (k >> 1) : (unsigned long long)(SORT_CH / 2); j > 0; j >>= 1) {
      // thread t handles the pair (i, i^j) with i = the t-th index whose j bit is clear
      const unsigned long long i = ((unsigned long long)t / j) * (2 * j) + ((unsigned long long)t % j);
      const bool up = (((g0 + i) & k) == 0);
      unsigned long long x = s[i], y = s[i + j];
      cswap(x, y, up);
      s[i] = x; s[i + j] = y;
      __syncthreads();
    }
  }
  a[g0 + t] = s[t]; a[g0 + t + 1024] = s[t + 1024];
}
// NS consecutive global stages (strides j, j/2, .. j >> (NS-1), all >= SORT_CH) of merge level k in ONE launch: a thread holds the 2^NS
// elements whose indices differ only in those stride bits, so every compare-exchange of the NS stages stays inside its registers
// (round 4: one launch per stage was 36 launches of ~3 us for 2^19 keys; three stages per launch make it 15).  k >= 2j, so the
// sort direction is the same for all of a thread's elements.
template <bool DEV, int NS>
__global__ __launch_bounds__(256) void bitonic_global_kernel(unsigned long long* __restrict__ a, unsigned long long k, unsigned long long j,
                                                             const unsigned long long* __restrict__ n_dev, unsigned long long n_cap) {
  constexpr int NE = 1 << NS;
  const unsigned long long n_eff = DEV ? sort_n_eff(n_dev, n_cap) : n_cap;
  if (k > n_eff) return;
  const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_eff / NE) return;
  const unsigned long long jl = j >> (NS - 1);                  // smallest stride of this launch
  const unsigned long long base = (t / jl) * (NE * jl) + (t % jl);
  const bool up = ((base & k) == 0);
  unsigned long long e[NE];
#pragma unroll
  for (int b = 0; b < NE; b++) e[b] = a[base + (unsigned long long)b * jl];
#pragma unroll
  for (int s = NS - 1; s >= 0; s--) {                           // stride jl << s
#pragma unroll
    for (int b = 0; b < NE; b++)
      if (!(b & (1 << s))) cswap(e[b], e[b | (1 << s)], up);
  }
#pragma unroll
  for (int b = 0; b < NE; b++) a[base + (unsigned long long)b * jl] = e[b];
}

}  // namespace ssg

using namespace ssg;

// the network's launches for a buffer of n entries (a power of two >= SORT_CH); nd = the device count (DEV) or null
template <bool DEV>
static void bitonic_launch(unsigned long long* a, unsigned long long n, const unsigned long long* nd, hipStream_t stream) {
  hipLaunchKernelGGL(bitonic_local_kernel<DEV>, dim3((unsigned)(n / SORT_CH)), dim3(1024), 0, stream, a, 2ULL, (unsigned long long)SORT_CH, nd, n);
  for (unsigned long long k = 2ULL * SORT_CH; k <= n; k <<= 1) {
    unsigned long long j = k >> 1;
    while (j >= (unsigned long long)SORT_CH) {                  // global stages j, j/2, ... SORT_CH: three per launch while they last
      int ns = 0;
      for (unsigned long long q = j; q >= (unsigned long long)SORT_CH && ns < 3; q >>= 1) ns++;
      const unsigned long long thr = n >> ns;
      const unsigned blocks = (unsigned)((thr + 255) / 256);
      if (ns == 3) hipLaunchKernelGGL((bitonic_global_kernel<DEV, 3>), dim3(blocks), dim3(256), 0, stream, a, k, j, nd, n);
      else if (ns == 2) hipLaunchKernelGGL((bitonic_global_kernel<DEV, 2>), dim3(blocks), dim3(256), 0, stream, a, k, j, nd, n);
      else hipLaunchKernelGGL((bitonic_global_kernel<DEV, 1>), dim3(blocks), dim3(256), 0, stream, a, k, j, nd, n);
      j >>= ns;
    }
    hipLaunchKernelGGL(bitonic_local_kernel<DEV>, dim3((unsigned)(n / SORT_CH)), dim3(1024), 0, stream, a, k, k, nd, n);
  }
}

// ascending sort of buf[0..n) (n = power of two >= 2048; pad with ~0)
extern "C" int ssg_sort_u64(uint64_t* buf, uint64_t n, hipStream_t stream) {
  if (n < (uint64_t)SORT_CH || (n & (n - 1))) { ssg_set_error("ssg_sort_u64: n must be a power of two >= %d", SORT_CH); return SSG_ERR_INVALID; }
  bitonic_launch<false>((unsigned long long*)buf, n, nullptr, stream);
  SSG_LAUNCH_CHECK("bitonic sort");
  return SSG_OK;
}

extern "C" int ssg_fill_u64(uint64_t* buf, uint64_t n0, uint64_t n1, uint64_t value, hipStream_t stream) {
  if (n1 > n0) hipLaunchKernelGGL(fill_u64_kernel<false>, dim3(256), dim3(256), 0, stream, (unsigned long long*)buf + n0, (const unsigned long long*)nullptr,
                                  (unsigned long long)(n1 - n0), (unsigned long long)value);
  SSG_LAUNCH_CHECK("fill_u64_kernel");
  return SSG_OK;
}

// ascending sort of buf[0 .. *n_dev) inside a buffer of n_cap entries (n_cap = power of two >= 2048); entries [*n_dev, n_eff) are
// overwritten with ~0 first.  After the call buf[0 .. *n_dev) is sorted (when *n_dev <= n_cap).
extern "C" int ssg_sort_u64_dev(uint64_t* buf, uint64_t n_cap, const uint64_t* n_dev, hipStream_t stream) {
  if (n_cap < (uint64_t)SORT_CH || (n_cap & (n_cap - 1)) || !n_dev) { ssg_set_error("ssg_sort_u64_dev: n_cap must be a power of two >= %d, n_dev non-null", SORT_CH); return SSG_ERR_INVALID; }
  unsigned long long* a = (unsigned long long*)buf;
  const unsigned long long* nd = (const unsigned long long*)n_dev;
  hipLaunchKernelGGL(fill_u64_kernel<true>, dim3(256), dim3(256), 0, stream, a, nd, (unsigned long long)n_cap, ~0ULL);
  bitonic_launch<true>(a, n_cap, nd, stream);
  SSG_LAUNCH_CHECK("bitonic sort (device-sized)");
  return SSG_OK;
}

// ---- round 6: fixed-capacity segments (the all-gathered candidate / edge buffers of the ranks) -> one list, counts left on the device ----
// Segment s holds min(counts[s * count_stride], seg_cap) valid 8-byte items at in + s * seg_stride; they go to out back to back in segment
// order.  total2[0] = the number written, total2[1] = 1 when a segment's count exceeded seg_cap (its owner's buffer overflowed: the caller's
// check must fail).  One workgroup per (segment, 4096-item chunk); every workgroup re-derives its segment's base from the <= 64 counts.
namespace ssg {
__global__ __launch_bounds__(256) void concat_segments_kernel(const unsigned long long* __restrict__ in, int nseg, unsigned long long seg_cap,
                                                              unsigned long long seg_stride, const unsigned long long* __restrict__ counts, int count_stride,
                                                              unsigned long long* __restrict__ out, unsigned long long* __restrict__ total2, int chunks_per_seg) {
  const int s = (int)blockIdx.x / chunks_per_seg, ch = (int)blockIdx.x % chunks_per_seg;
  unsigned long long base = 0, mine = 0, over = 0, sum = 0;
  for (int r = 0; r < nseg; r++) {
    unsigned long long c = counts[(size_t)r * count_stride];
    if (c > seg_cap) { c = seg_cap; over = 1; }
    if (r < s) base += c;
    if (r == s) mine = c;
    sum += c;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { total2[0] = sum; total2[1] = over; }
  const unsigned long long i0 = (unsigned long long)ch * 4096;
  const unsigned long long* src = in + (size_t)s * seg_stride;
#pragma unroll 4
  for (unsigned long long i = i0 + threadIdx.x; i < i0 + 4096 && i < mine; i += 256) out[base + i] = src[i];
}
}  // namespace ssg
extern "C" int ssg_concat_segments_u64(const uint64_t* in, int nseg, uint64_t seg_cap, uint64_t seg_stride, const uint64_t* counts, int count_stride,
                                       uint64_t* out, uint64_t* total2, hipStream_t stream) {
  if (!in || !counts || !out || !total2 || nseg <= 0 || nseg > 4096 || seg_stride < seg_cap || count_stride < 1) {
    ssg_set_error("ssg_concat_segments_u64: bad arguments (nseg=%d)", nseg);
    return SSG_ERR_INVALID;
  }
  const int cps = (int)((seg_cap + 4095) / 4096) > 0 ? (int)((seg_cap + 4095) / 4096) : 1;
  hipLaunchKernelGGL(ssg::concat_segments_kernel, dim3((unsigned)(nseg * cps)), dim3(256), 0, stream, (const unsigned long long*)in, nseg, (unsigned long long)seg_cap,
                     (unsigned long long)seg_stride, (const unsigned long long*)counts, count_stride, (unsigned long long*)out, (unsigned long long*)total2, cps);
  SSG_LAUNCH_CHECK("concat_segments_kernel");
  return SSG_OK;
}

// ---- round 5: sample sort of the device-sized key list -------------------------------------------------------------------------------
// The bitonic network above costs 25 launches (0.15 ms of 4..9 us kernels + their dispatch gaps) for the ~2.7e5 candidates of the eps rule
// at N = 16 000 -- a third of the whole eps rule + DBSCAN chain.  Five launches instead:
//   1. one workgroup sorts a strided sample of 4096 keys in LDS and keeps every 4th as a splitter (1023 of them);
//   2. every workgroup of 4096 keys finds each key's bucket by a 10-step lower bound over the splitters in LDS and counts per bucket:
//      bucket = 2 * #(splitters < key) + (key == that splitter) -- keys EQUAL to a splitter get a bucket of their own (odd numbers), so
//      any number of duplicates (half-valued distances: a few hundred distinct keys) stays out of the buckets that need sorting; the
//      workgroup reserves its share of every bucket with one returning atomic per non-empty bucket (the order inside a bucket is free);
//   3. one workgroup scans the 2048 bucket totals into offsets;
//   4. the keys are scattered to their bucket's range (LDS cursors on top of the reserved bases);
//   5. one workgroup per bucket sorts its keys in LDS (bitonic on the next power of two: ~260 keys at 4x oversampling) and writes them
//      back.  Buckets over 2048 keys are ranked out of global memory (slow, exact); over 16384: *fail = 1.
// (First version, measured: ranking every key against the whole bucket in LDS = 73 us of dependent LDS reads, the sample's bitonic
//  network with integer divisions in its index arithmetic = 51 us, a (workgroup x bucket) count matrix scanned by one workgroup = 17 us:
//  171 us, slower than the network it was to replace.)
// Two geometries (round 6): LB = 10 -- 1023 splitters out of a sorted sample of 4096 keys, chunks of 4096 keys per counting workgroup,
// sorting buckets of up to 2048 keys (256 threads) -- while the expected number of keys stays below ~4e5 (LDS-sized buckets with a 4x
// margin); LB = 12 -- 4095 splitters out of a sample of 16 384, chunks of 16 384, buckets of up to 16 384 keys in 128 KB of LDS (1024
// threads, up to 16 keys per thread in registers) -- up to ~2.4e7 keys (N = 128 000: 1.7e7 candidates, 4.1 k per bucket on average), where
// the bitonic network over the whole array took 7.1 ms.
template <int LB> struct SsCfg {
  static constexpr int NSLOT = 1 << LB, NSPLIT = NSLOT - 1, NBK = 2 * NSLOT, SAMPLE = 4 * NSLOT, CHUNK = LB == 10 ? 4096 : 16384;
  static constexpr int CAP = LB == 10 ? 2048 : 16384, NTB = LB == 10 ? 256 : 1024;     // largest bucket sorted in LDS, threads of the bucket sort
  static constexpr int CAP_GLOBAL = 16384;                                              // LB = 10: ranked out of global memory up to here; beyond: fail
};
struct SsWs { unsigned long long* tmp; unsigned long long* split; unsigned int* cmat; unsigned int* gcount; unsigned int* off; unsigned short* bid; };
template <int LB>
static size_t ss_layout(uint64_t n_cap, char* base, SsWs* w) {
  using C = SsCfg<LB>;
  size_t o = 0;
  const size_t G = (size_t)((n_cap + C::CHUNK - 1) / C::CHUNK);
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  const size_t a_tmp = take((size_t)n_cap * 8), a_split = take((size_t)C::NSLOT * 8), a_cmat = take(G * C::NBK * 4), a_gc = take((size_t)C::NBK * 4),
               a_off = take(((size_t)C::NBK + 1) * 4), a_bid = take((size_t)n_cap * 2);
  if (w) {
    w->tmp = (unsigned long long*)(base + a_tmp); w->split = (unsigned long long*)(base + a_split); w->cmat = (unsigned int*)(base + a_cmat);
    w->gcount = (unsigned int*)(base + a_gc); w->off = (unsigned int*)(base + a_off); w->bid = (unsigned short*)(base + a_bid);
  }
  return o;
}
__device__ __forceinline__ unsigned long long ss_count_of(const unsigned long long* n_dev, unsigned long long n_cap) {
  const unsigned long long n = *n_dev;
  return n > n_cap ? n_cap : n;
}
// One bitonic network over M = E * NT keys, E consecutive keys per thread IN REGISTERS (key index e = t * E + r).  A compare-exchange
// partner at distance j sits in the same thread (j < E), in the same wave (j < 64 E: one 64-bit shuffle) or in another wave (LDS, two
// barriers) -- 10 of the 78 steps of a 4096-key network go through LDS instead of all of them (the all-LDS version was bound by LDS
// traffic: 40 us for the sample, 21 us for the buckets).  After the call key e of the sorted order is v[e - t * E] of thread e / E.
template <int E, int NT>
__device__ __forceinline__ void ss_bitonic_reg(unsigned long long (&v)[E], unsigned long long* s, int t) {
  constexpr int M = E * NT, WSPAN = 64 * E;
  const int e0 = t * E;
  for (int k = 2; k <= M; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j < E) {
#pragma unroll
        for (int jj = 1; jj < E; jj <<= 1)
          if (j == jj) {
#pragma unroll
            for (int r = 0; r < E; r++)
              if (!(r & jj)) cswap(v[r], v[r | jj], ((e0 + r) & k) == 0);
          }
      } else {
        unsigned long long pv[E];
        if (j < WSPAN) {
          const int lx = j / E;
#pragma unroll
          for (int r = 0; r < E; r++) pv[r] = __shfl_xor(v[r], lx, 64);
        } else {
#pragma unroll
          for (int r = 0; r < E; r++) s[e0 + r] = v[r];
          __syncthreads();
#pragma unroll
          for (int r = 0; r < E; r++) pv[r] = s[(e0 + r) ^ j];
          __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < E; r++) {
          const int e = e0 + r;
          const bool take_min = (((e & j) == 0) == ((e & k) == 0));      // the lower key of an ascending pair, the upper one of a descending pair
          const unsigned long long a = v[r], b = pv[r];
          v[r] = take_min ? (a < b ? a : b) : (a < b ? b : a);
        }
      }
    }
}
template <int LB>
__global__ __launch_bounds__(1024) void ss_splitters_kernel(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ n_dev, unsigned long long n_cap,
                                                            unsigned long long* __restrict__ split, unsigned int* __restrict__ gcount,
                                                            unsigned long long* __restrict__ fail) {
  using C = SsCfg<LB>;
  constexpr int E = C::SAMPLE / 1024;
  __shared__ unsigned long long s[C::SAMPLE];
  const unsigned long long n = ss_count_of(n_dev, n_cap);
  const int t = (int)threadIdx.x;
  if (t == 0) *fail = 0ull;
  for (int q = t; q < C::NBK; q += 1024) gcount[q] = 0u;
  if (n == 0) return;
  unsigned long long v[E];
#pragma unroll
  for (int r = 0; r < E; r++) v[r] = a[((unsigned long long)(E * t + r) * n) >> (LB + 2)];        // (n < 2^31, sample index < 2^14)
  ss_bitonic_reg<E, 1024>(v, s, t);
  // sorted sample keys 3, 7, 11, ...: with E keys per thread the splitters of thread t are its keys 3, 7, ... (E = 4: one, E = 16: four)
#pragma unroll
  for (int r = 3; r < E; r += 4) { const int q = (E * t + r) >> 2; if (q < C::NSPLIT) split[q] = v[r]; }
}
// sp: NSLOT entries in LDS, the NSPLIT splitters ascending + ~0
template <int NSLOT>
__device__ __forceinline__ int ss_bucket(const unsigned long long* sp, unsigned long long key) {
  int lo = 0;
#pragma unroll
  for (int step = NSLOT / 2; step > 0; step >>= 1) lo += (sp[lo + step - 1] < key) ? step : 0;
  return 2 * lo + (sp[lo] == key ? 1 : 0);
}
template <int LB>
__global__ __launch_bounds__(256) void ss_count_kernel(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ n_dev, unsigned long long n_cap,
                                                       const unsigned long long* __restrict__ split, unsigned int* __restrict__ gcount,
                                                       unsigned int* __restrict__ cmat, unsigned short* __restrict__ bid) {
  using C = SsCfg<LB>;
  __shared__ unsigned long long sp[C::NSLOT];
  __shared__ unsigned int cn[C::NBK];
  const unsigned long long n = ss_count_of(n_dev, n_cap);
  const unsigned long long g0 = (unsigned long long)blockIdx.x * C::CHUNK;
  if (g0 >= n) return;
  const int t = (int)threadIdx.x;
  for (int q = t; q < C::NSLOT; q += 256) sp[q] = q < C::NSPLIT ? split[q] : ~0ull;
  for (int q = t; q < C::NBK; q += 256) cn[q] = 0u;
  __syncthreads();
  for (int u = 0; u < C::CHUNK / 256; u += 4) {
    unsigned long long key[4]; int b[4];
#pragma unroll
    for (int v = 0; v < 4; v++) { const unsigned long long idx = g0 + (unsigned long long)(u + v) * 256 + t; key[v] = a[idx < n ? idx : n - 1]; }
#pragma unroll
    for (int v = 0; v < 4; v++) b[v] = ss_bucket<C::NSLOT>(sp, key[v]);
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const unsigned long long idx = g0 + (unsigned long long)(u + v) * 256 + t;
      if (idx < n) { atomicAdd(&cn[b[v]], 1u); bid[idx] = (unsigned short)b[v]; }
    }
  }
  __syncthreads();
  for (int q = t; q < C::NBK; q += 256) {
    const unsigned int c = cn[q];
    cmat[(size_t)blockIdx.x * C::NBK + q] = c ? atomicAdd(&gcount[q], c) : 0u;       // this workgroup's base inside bucket q
  }
}
// (round 6: every workgroup scans the bucket counts itself -- NBK / 256 per thread + a 256-entry LDS scan, ~1 us -- instead of waiting for a
//  one-workgroup scan launch in between; workgroup 0 also leaves the offsets in `off` for the bucket sort)
template <int LB>
__global__ __launch_bounds__(256) void ss_scatter_kernel(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ n_dev, unsigned long long n_cap,
                                                         const unsigned int* __restrict__ cmat, const unsigned int* __restrict__ gcount, unsigned int* __restrict__ off,
                                                         const unsigned short* __restrict__ bid, unsigned long long* __restrict__ tmp) {
  using C = SsCfg<LB>;
  constexpr int PT = C::NBK / 256;                      // bucket counts per thread: 8 or 32
  __shared__ unsigned int cur[C::NBK];
  __shared__ unsigned int psum[256];
  const unsigned long long n = ss_count_of(n_dev, n_cap);
  const unsigned long long g0 = (unsigned long long)blockIdx.x * C::CHUNK;
  if (g0 >= n && blockIdx.x != 0) return;
  const int t = (int)threadIdx.x;
  unsigned int mine = 0;
  for (int u = 0; u < PT; u++) mine += gcount[PT * t + u];
  psum[t] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned int add = t >= o ? psum[t - o] : 0u;
    __syncthreads();
    psum[t] += add;
    __syncthreads();
  }
  unsigned int run = psum[t] - mine;
  for (int u = 0; u < PT; u++) {
    const unsigned int gc = gcount[PT * t + u];
    cur[PT * t + u] = run + (g0 < n ? cmat[(size_t)blockIdx.x * C::NBK + PT * t + u] : 0u);
    if (blockIdx.x == 0) off[PT * t + u] = run;
    run += gc;
  }
  if (blockIdx.x == 0 && t == 255) off[C::NBK] = run;
  if (g0 >= n) return;                      // (workgroup 0 of an empty input: only the offsets)
  __syncthreads();
  for (int u = 0; u < C::CHUNK / 256; u += 4) {
    unsigned long long key[4]; int b[4];
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const unsigned long long idx = g0 + (unsigned long long)(u + v) * 256 + t, ic = idx < n ? idx : n - 1;
      key[v] = a[ic]; b[v] = (int)bid[ic];
    }
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const unsigned long long idx = g0 + (unsigned long long)(u + v) * 256 + t;
      if (idx < n) tmp[atomicAdd(&cur[b[v]], 1u)] = key[v];
    }
  }
}
template <int LB>
__global__ __launch_bounds__(SsCfg<LB>::NTB) void ss_bucket_sort_kernel(const unsigned long long* __restrict__ tmp, const unsigned int* __restrict__ off,
                                                                        unsigned long long* __restrict__ out, unsigned long long* __restrict__ fail) {
  using C = SsCfg<LB>;
  constexpr int NTB = C::NTB;
  __shared__ unsigned long long s[C::CAP];
  const int b = (int)blockIdx.x, t = (int)threadIdx.x;
  const unsigned int s0 = off[b];
  const int len = (int)(off[b + 1] - s0);
  if (len <= 0) return;
  const bool hopeless = LB == 10 ? len > C::CAP_GLOBAL : len > C::CAP;
  if ((b & 1) || len == 1 || hopeless) {                             // all keys equal (a splitter's own bucket) / one key / hopeless: copy
    for (int q = t; q < len; q += NTB) out[s0 + q] = tmp[s0 + q];
    if (!(b & 1) && hopeless && t == 0) atomicOr(fail, 1ull);
    return;
  }
  if (len <= C::CAP) {
    // NTB * E keys (E = the power of two that holds the bucket), padded with ~0, the network in registers
#define SS_BUCKET(E_)                                                                                          \
    {                                                                                                          \
      unsigned long long v[E_];                                                                                \
      _Pragma("unroll") for (int r = 0; r < E_; r++) { const int e = t * E_ + r; v[r] = e < len ? tmp[s0 + e] : ~0ull; } \
      ss_bitonic_reg<E_, NTB>(v, s, t);                                                                        \
      _Pragma("unroll") for (int r = 0; r < E_; r++) { const int e = t * E_ + r; if (e < len) out[s0 + e] = v[r]; }      \
    }
    if (len <= NTB) SS_BUCKET(1) else if (len <= 2 * NTB) SS_BUCKET(2) else if (len <= 4 * NTB) SS_BUCKET(4) else if (len <= 8 * NTB) SS_BUCKET(8)
    else if constexpr (C::CAP >= 16 * NTB) SS_BUCKET(16)
#undef SS_BUCKET
    return;
  }
  for (int q = t; q < len; q += NTB) {                                // (LB = 10) an oversized bucket: every key ranked against the bucket out of global memory
    const unsigned long long key = tmp[s0 + q];
    int rank = 0;
    for (int j = 0; j < len; j++) { const unsigned long long kj = tmp[s0 + j]; rank += (kj < key || (kj == key && j < q)) ? 1 : 0; }
    out[s0 + rank] = key;
  }
}
template <int LB>
static int samplesort_impl(uint64_t* buf, uint64_t n_cap, const uint64_t* n_dev, void* ws, size_t ws_bytes, uint64_t* fail, hipStream_t stream) {
  using C = SsCfg<LB>;
  SsWs w;
  if (ss_layout<LB>(n_cap, (char*)ws, &w) > ws_bytes) { ssg_set_error("sample sort: workspace too small"); return SSG_ERR_INVALID; }
  unsigned long long* a = (unsigned long long*)buf;
  const unsigned long long* nd = (const unsigned long long*)n_dev;
  const unsigned G = (unsigned)((n_cap + C::CHUNK - 1) / C::CHUNK);
  hipLaunchKernelGGL(ss_splitters_kernel<LB>, dim3(1), dim3(1024), 0, stream, a, nd, (unsigned long long)n_cap, w.split, w.gcount, (unsigned long long*)fail);
  hipLaunchKernelGGL(ss_count_kernel<LB>, dim3(G), dim3(256), 0, stream, a, nd, (unsigned long long)n_cap, (const unsigned long long*)w.split, w.gcount, w.cmat, w.bid);
  hipLaunchKernelGGL(ss_scatter_kernel<LB>, dim3(G), dim3(256), 0, stream, a, nd, (unsigned long long)n_cap, w.cmat, (const unsigned int*)w.gcount, w.off, w.bid, w.tmp);
  hipLaunchKernelGGL(ss_bucket_sort_kernel<LB>, dim3(C::NBK), dim3(C::NTB), 0, stream, w.tmp, w.off, a, (unsigned long long*)fail);
  SSG_LAUNCH_CHECK("sample sort (device-sized)");
  return SSG_OK;
}
extern "C" size_t ssg_samplesort_u64_workspace_bytes(uint64_t n_cap) { return ss_layout<10>(n_cap, nullptr, nullptr); }
// ascending sort of buf[0 .. min(*n_dev, n_cap)) in place (through ws); *fail = 1 when a bucket could not be sorted (more than 16384 keys
// strictly between two neighbouring splitters: the sample missed the distribution) -- buf then holds a permutation of the keys, not sorted.
extern "C" int ssg_samplesort_u64_dev(uint64_t* buf, uint64_t n_cap, const uint64_t* n_dev, void* ws, size_t ws_bytes, uint64_t* fail, hipStream_t stream) {
  if (!buf || !n_dev || !ws || !fail || n_cap == 0 || n_cap > (1ull << 31)) { ssg_set_error("ssg_samplesort_u64_dev: bad arguments"); return SSG_ERR_INVALID; }
  return samplesort_impl<10>(buf, n_cap, n_dev, ws, ws_bytes, fail, stream);
}
// round 6: the LB = 12 geometry (see above) for 4e5 .. 2.4e7 expected keys; same contract, its own workspace size
extern "C" size_t ssg_samplesort_u64_big_workspace_bytes(uint64_t n_cap) { return ss_layout<12>(n_cap, nullptr, nullptr); }
extern "C" int ssg_samplesort_u64_big_dev(uint64_t* buf, uint64_t n_cap, const uint64_t* n_dev, void* ws, size_t ws_bytes, uint64_t* fail, hipStream_t stream) {
  if (!buf || !n_dev || !ws || !fail || n_cap == 0 || n_cap > (1ull << 31)) { ssg_set_error("ssg_samplesort_u64_big_dev: bad arguments"); return SSG_ERR_INVALID; }
  return samplesort_impl<12>(buf, n_cap, n_dev, ws, ws_bytes, fail, stream);
}
