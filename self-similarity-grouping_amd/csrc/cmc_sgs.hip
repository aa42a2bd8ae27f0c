// cmc_sgs.hip -- the single-gallery-shot CMC protocol ('cuhk03': reid/evaluation_metrics/ranking.py:10-16,53-66 with
// single_gallery_shot=True) on a query x gallery float32 distance block.
//
// For every query the reference argsorts the row, groups the valid gallery entries by identity and then, ten times, draws ONE entry
// per identity with np.random.choice and credits the bin k = number of OTHER identities whose drawn entry is ranked before the drawn
// entry of the query's own identity.  np.random.choice(list of s entries) is the legacy randint(0, s): s == 1 consumes no word,
// otherwise successive 32-bit MT19937 words w are masked with mask = 2^bit_length(s-1) - 1 and the first w & mask <= s - 1 is the
// choice.  The identities are visited in order of first appearance along the ranking, the entries of one identity are in rank order,
// so choice c picks the identity's c-th best entry.  The host draws the words from a copy of the caller's stream (ssg_amd/ranking.py)
// and uploads them; three stages replay the loop, the order being (distance, gallery index) encoded as u64 key = orderable float
// bits << 32 | index:
//   groups (one workgroup per query)   valid mask, counting pass by dense identity, every identity's keys ascending, the identities
//                                      ordered by their smallest key (the register/LDS bitonic network of sort_u64.hip), the list of
//                                      identities with more than one entry in that order.  The row itself is never sorted and never
//                                      held in LDS (131 072 keys are 1 MiB);
//   draws  (ONE wave)                  queries -> 10 repeats -> identities with more than one entry: the masked-rejection rule on the
//                                      word stream.  Where a draw reads its word depends on every rejection before it, so this
//                                      stage is serial by nature and latency-bound (every step waits for its LDS reads and then for a
//                                      chain of scalar instructions on one wave; 85-89 % of a call, profiles/cmc_sgs_times.txt); a step tests 64
//                                      consecutive draws against the words they would read after 0 .. 7 rejections, one ballot each,
//                                      and commits draws up to the eighth reject.  When the words run out it stores where it
//                                      stopped and sets a flag; the next launch resumes there;
//   counts (one workgroup per query x repeat)   k = number of identities whose chosen key is below the chosen key of the query's own.
#include "ssg_common.h"

namespace ssg {

constexpr int SGS_MAX_N = 131072, SGS_MAX_G = 16384, SGS_MAX_GROUP = 16384, SGS_REPEAT = 10;
constexpr int SGS_WIN = 4096;          // words of the stream the draw stage keeps in LDS
constexpr int SGS_SHIFTS = 8;         // rejections the draw stage resolves per step

// one chunk of mq queries: tmp / keys [mq, n] (keys: the valid entries, identity after identity, each ascending), goff [mq, G + 1]
// (where identity g starts in the query's keys), multi [mq, G] (identity << 16 | size - 1 of the identities with size > 1, in order of
// first appearance), nmulti [mq] (their number; 0 for a query without a valid true match), trueid [mq] (the query's dense identity, -1
// likewise), choice [mq, 10, G] (the drawn entry of an identity with size > 1)
struct SgsWs { unsigned long long* tmp; unsigned long long* keys; int* goff; unsigned* multi; int* nmulti; int* trueid; unsigned short* choice; };

__device__ __forceinline__ unsigned long long sgs_key(float x, int j) {
  unsigned u = __float_as_uint(x + 0.0f);                                       // -0 -> +0: equal distances, ordered by index
  u = (x != x) ? 0xffffffffu : (u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));   // NaN last, like numpy's sorts
  return ((unsigned long long)u << 32) | (unsigned)j;
}

// exclusive scan of one int per thread over the 1024 threads of the workgroup (sc: 1024 ints of LDS); *total = the sum
__device__ __forceinline__ int sgs_block_scan(int mine, int* sc, int t, int* total) {
  sc[t] = mine;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int add = t >= o ? sc[t - o] : 0;
    __syncthreads();
    sc[t] += add;
    __syncthreads();
  }
  const int incl = sc[t];
  *total = sc[1023];
  __syncthreads();
  return incl - mine;
}

// the identities by their smallest key (E * 1024 >= G slots, ~0 for an identity without a valid entry), then the ordered list of those
// with more than one entry
template <int E>
__device__ __forceinline__ void sgs_order_groups(const unsigned long long* keys, const int* goff, const int* __restrict__ gden,
                                                 int G, unsigned long long* sbuf, int* sc, unsigned* __restrict__ multi, int t, int* n_multi) {
  unsigned long long v[E];
#pragma unroll
  for (int r = 0; r < E; r++) {
    const int g = t * E + r;
    v[r] = ~0ull;
    if (g < G) { const int a = goff[g]; if (goff[g + 1] > a) v[r] = keys[a]; }
  }
  __syncthreads();                                   // sbuf held the counters until here
  ss_bitonic_reg<E, 1024>(v, sbuf, t);
  unsigned ent[E];
  int mine = 0;
#pragma unroll
  for (int r = 0; r < E; r++) {
    ent[r] = 0u;
    if (v[r] != ~0ull) {
      const int g = gden[(unsigned)v[r]];
      const int s = goff[g + 1] - goff[g];
      if (s > 1) { ent[r] = ((unsigned)g << 16) | (unsigned)(s - 1 < 0xffff ? s - 1 : 0xffff); mine++; }      // (s <= 16 384 by the caller's check)
    }
  }
  int pos = sgs_block_scan(mine, sc, t, n_multi);
#pragma unroll
  for (int r = 0; r < E; r++)
    if (ent[r]) multi[pos++] = ent[r];
}

__global__ __launch_bounds__(1024) void sgs_groups_kernel(const float* __restrict__ dist, int64_t ld, int n, const int* __restrict__ qid,
                                                          const int* __restrict__ qcam, const int* __restrict__ qden, const int* __restrict__ gid,
                                                          const int* __restrict__ gcam, const int* __restrict__ gden, int G, int separate_cams, SgsWs w) {
  __shared__ unsigned long long sbuf[SGS_MAX_G];      // 128 KiB: the counters and cursors of the identities, later the network's exchange buffer
  __shared__ int sc[1024];
  int* cnt = (int*)sbuf;                              // [G] valid entries of identity g
  int* cur = cnt + SGS_MAX_G;                         // [G] scatter cursor; after the scatter: the END of identity g
  const int q = (int)blockIdx.x, t = (int)threadIdx.x;
  const float* row = dist + (int64_t)q * ld;
  unsigned long long* tmp = w.tmp + (size_t)q * n;
  unsigned long long* keys = w.keys + (size_t)q * n;
  int* goff = w.goff + (size_t)q * (G + 1);
  const int myid = qid[q], mycam = qcam[q];
  // valid gallery entry (ranking.py:47-51): different identity or different camera; 'separate camera set': different camera only.
  // An identity outside [0, G) cannot come from the host wrapper; such an entry is left out instead of indexing with it.
  auto dense_of = [&](int j) -> int {
    const bool diffcam = gcam[j] != mycam;
    const bool ok = separate_cams ? diffcam : (gid[j] != myid || diffcam);
    const int g = gden[j];
    return (ok && (unsigned)g < (unsigned)G) ? g : -1;
  };
  for (int g = t; g < G; g += 1024) cnt[g] = 0;
  __syncthreads();
  for (int j = t; j < n; j += 1024) { const int g = dense_of(j); if (g >= 0) atomicAdd(&cnt[g], 1); }
  __syncthreads();
  const int PT = (G + 1023) / 1024;                   // identities per thread of the scan
  int mine = 0;
  for (int u = 0; u < PT; u++) { const int g = t * PT + u; if (g < G) mine += cnt[g]; }
  int total;
  int run = sgs_block_scan(mine, sc, t, &total);
  for (int u = 0; u < PT; u++) {
    const int g = t * PT + u;
    if (g < G) { goff[g] = run; cur[g] = run; run += cnt[g]; }
  }
  if (t == 0) goff[G] = total;
  __syncthreads();
  for (int j = t; j < n; j += 1024) { const int g = dense_of(j); if (g >= 0) tmp[atomicAdd(&cur[g], 1)] = sgs_key(row[j], j); }
  __syncthreads();
  // every identity's keys ascending: each key counts the smaller keys of its identity (keys are distinct: they carry the index).
  // Tens of entries for a person; the junk / distractor identities of a raw Market list have thousands, read through the caches.
  for (int e = t; e < total; e += 1024) {
    const unsigned long long key = tmp[e];
    const int g = gden[(unsigned)key];
    const int end = cur[g], beg = end - cnt[g];
    int r = 0;
    for (int u = beg; u < end; u++) r += tmp[u] < key ? 1 : 0;
    keys[beg + r] = key;
  }
  __syncthreads();
  int nm;
  unsigned* multi = w.multi + (size_t)q * G;
  if (G <= 1024) sgs_order_groups<1>(keys, goff, gden, G, sbuf, sc, multi, t, &nm);
  else if (G <= 2048) sgs_order_groups<2>(keys, goff, gden, G, sbuf, sc, multi, t, &nm);
  else if (G <= 4096) sgs_order_groups<4>(keys, goff, gden, G, sbuf, sc, multi, t, &nm);
  else if (G <= 8192) sgs_order_groups<8>(keys, goff, gden, G, sbuf, sc, multi, t, &nm);
  else sgs_order_groups<16>(keys, goff, gden, G, sbuf, sc, multi, t, &nm);
  if (t == 0) {
    const int tq = qden[q];
    const bool ok = (unsigned)tq < (unsigned)G && goff[tq + 1] > goff[tq];       // a query without a valid true match is skipped and draws nothing (ranking.py:52)
    w.nmulti[q] = ok ? nm : 0;
    w.trueid[q] = ok ? tq : -1;
  }
}

// state[0] = words of the stream consumed so far (carried from chunk to chunk), state[1] / state[2] = the query of this chunk and the
// draw inside it (repeat * nmulti + position) to go on with, state[3] = 1 when the supplied words [word_base, word_base + nwords)
// ran out before the chunk was done.  One wave; every branch below is uniform (it depends on ballots and on shared values only).
__global__ __launch_bounds__(64) void sgs_draws_kernel(SgsWs w, int mq, int G, const unsigned* __restrict__ words, unsigned long long word_base,
                                                       unsigned long long nwords, unsigned long long* __restrict__ state) {
  __shared__ unsigned sm_multi[SGS_MAX_G];
  __shared__ unsigned sm_w[SGS_WIN];
  const int lane = (int)threadIdx.x;
  unsigned long long cursor = state[0];
  int q = (int)state[1];
  int t = (int)state[2];
  if (cursor < word_base) cursor = word_base;          // (cannot happen: the host uploads the stream from the cursor on)
  unsigned long long cur = cursor - word_base;         // position inside words[]
  unsigned long long win0 = 0, win1 = 0;               // sm_w holds words[win0 .. win1)
  bool out_of_words = false;
  for (; q < mq && !out_of_words; q++, t = 0) {
    const int nm = w.nmulti[q];
    const int total = nm * SGS_REPEAT;                   // <= 163 840
    if (t >= total) continue;
    __syncthreads();
    for (int u = lane; u < nm; u += 64) sm_multi[u] = w.multi[(size_t)q * G + u];
    __syncthreads();
    unsigned short* choice = w.choice + (size_t)q * SGS_REPEAT * G;
    int t_rep = t / nm, t_pos = t % nm;                  // the draw t: repeat and position in the query's list
    while (t < total) {
      if (cur + 64 + SGS_SHIFTS > win1 && win1 < nwords) {   // the window ends inside the words this step may read and the stream goes on: move it up
        __syncthreads();
        win0 = cur;
        win1 = nwords - cur < (unsigned long long)SGS_WIN ? nwords : cur + SGS_WIN;
        for (unsigned long long u = win0 + lane; u < win1; u += 64) sm_w[u - win0] = words[u];
        __syncthreads();
      }
      const bool active = t + lane < total;
      int rep = t_rep, pos = t_pos + lane;
      if (pos >= nm) { rep += pos / nm; pos %= nm; }
      const unsigned ent = active ? sm_multi[pos] : 1u;
      const unsigned rng = ent & 0xffffu, g = ent >> 16;                 // rng = size - 1 >= 1
      const unsigned mask = (2u << (31 - __clz((int)rng))) - 1u;          // 2^bit_length(rng) - 1
      // After r rejections draw i reads word i + r.  Test every draw under the shifts r = 0 .. SGS_SHIFTS-1 at once (ok[r]: the lanes whose
      // draw accepts its word under shift r), then walk the rejections with scalar work only: under shift r the draws from `done` up to the
      // first lane that does not accept are committed; that lane's word is consumed and it, and every draw behind it, moves on to shift r + 1.
      const int off = (int)(cur - win0), avail = (int)(win1 - cur);      // words left in the window: all there are when it is shorter than a step reads
      unsigned v[SGS_SHIFTS];
      unsigned long long ok[SGS_SHIFTS];
#pragma unroll
      for (int r = 0; r < SGS_SHIFTS; r++) {
        const bool have = lane + r < avail;
        v[r] = (have ? sm_w[off + lane + r] : 0u) & mask;
        ok[r] = __ballot(active && have && v[r] <= rng);
      }
      const unsigned long long act = __ballot(active);
      const int nact = __popcll(act);
      int done = 0, used = 0;                            // draws committed, rejected words consumed
      bool stop = false;
      unsigned mine = 0;
#pragma unroll
      for (int r = 0; r < SGS_SHIFTS; r++) {
        if (!stop) {
          const unsigned long long rej = ~ok[r] & act & (~0ull << done);      // (done < nact <= 64 here)
          const int f = rej ? __builtin_ctzll(rej) : nact;
          if (lane >= done && lane < f) mine = v[r];
          done = f;
          if (done >= nact) stop = true;
          else if (done + r >= avail) { stop = true; out_of_words = true; }    // no word left for this draw: stop here, never guess
          else used = r + 1;                                                    // a rejected word is consumed too; the same draw takes the next one
        }
      }
      if (lane < done) choice[(size_t)rep * G + g] = (unsigned short)mine;
      t += done;
      cur += done + used;
      t_pos += done;
      while (t_pos >= nm) { t_pos -= nm; t_rep++; }
      if (out_of_words) break;
    }
    if (out_of_words) break;
  }
  if (lane == 0) {
    state[0] = word_base + cur;
    state[1] = (unsigned long long)q;
    state[2] = (unsigned long long)(out_of_words ? t : 0);
    state[3] = out_of_words ? 1ull : 0ull;
  }
}

__global__ __launch_bounds__(256) void sgs_counts_kernel(SgsWs w, int n, int G, int* __restrict__ kout) {
  __shared__ int acc;
  const int q = (int)blockIdx.x / SGS_REPEAT, rep = (int)blockIdx.x % SGS_REPEAT, t = (int)threadIdx.x;
  const int tq = w.trueid[q];
  if (tq < 0) { if (t == 0) kout[blockIdx.x] = -1; return; }
  const unsigned long long* keys = w.keys + (size_t)q * n;
  const int* goff = w.goff + (size_t)q * (G + 1);
  const unsigned short* choice = w.choice + ((size_t)q * SGS_REPEAT + rep) * G;
  auto chosen = [&](int g, int a, int s) { return keys[a + (s > 1 ? (int)choice[g] : 0)]; };
  if (t == 0) acc = 0;
  __syncthreads();
  const int ta = goff[tq];
  const unsigned long long tk = chosen(tq, ta, goff[tq + 1] - ta);
  int mine = 0;
  for (int g = t; g < G; g += 256) {
    const int a = goff[g], s = goff[g + 1] - a;
    if (s > 0 && g != tq) mine += chosen(g, a, s) < tk ? 1 : 0;
  }
  atomicAdd(&acc, mine);
  __syncthreads();
  if (t == 0) kout[blockIdx.x] = acc;
}

}  // namespace ssg

using namespace ssg;

static size_t sgs_layout(int mq, int n, int G, char* base, SgsWs* w) {
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  const size_t a_tmp = take((size_t)mq * n * 8), a_keys = take((size_t)mq * n * 8), a_goff = take((size_t)mq * (G + 1) * 4),
               a_multi = take((size_t)mq * G * 4), a_nm = take((size_t)mq * 4), a_true = take((size_t)mq * 4),
               a_choice = take((size_t)mq * SGS_REPEAT * G * 2);
  if (w) {
    w->tmp = (unsigned long long*)(base + a_tmp); w->keys = (unsigned long long*)(base + a_keys); w->goff = (int*)(base + a_goff);
    w->multi = (unsigned*)(base + a_multi); w->nmulti = (int*)(base + a_nm); w->trueid = (int*)(base + a_true);
    w->choice = (unsigned short*)(base + a_choice);
  }
  return o;
}
static int sgs_check(const char* who, int mq, int n, int G, const void* ws, size_t ws_bytes, SgsWs* w) {
  if (mq <= 0 || n <= 0 || G <= 0) { ssg_set_error("%s: bad shape mq=%d n=%d G=%d", who, mq, n, G); return SSG_ERR_INVALID; }
  if (n > SGS_MAX_N) { ssg_set_error("%s: n=%d gallery entries, at most %d", who, n, SGS_MAX_N); return SSG_ERR_INVALID; }
  if (G > SGS_MAX_G) { ssg_set_error("%s: G=%d gallery identities, at most %d", who, G, SGS_MAX_G); return SSG_ERR_INVALID; }
  if (!ws || ((uintptr_t)ws & 7) || sgs_layout(mq, n, G, (char*)ws, w) > ws_bytes) {
    ssg_set_error("%s: workspace missing, misaligned or smaller than ssg_cmc_sgs_workspace_bytes(%d, %d, %d)", who, mq, n, G);
    return SSG_ERR_INVALID;
  }
  return SSG_OK;
}

extern "C" size_t ssg_cmc_sgs_workspace_bytes(int mq, int n, int G) {
  if (mq <= 0 || n <= 0 || G <= 0 || n > SGS_MAX_N || G > SGS_MAX_G) return 0;
  return sgs_layout(mq, n, G, nullptr, nullptr);
}
extern "C" int ssg_cmc_sgs_max_group() { return SGS_MAX_GROUP; }

// stage 1 for the mq queries of one chunk (dist, qid, qcam, qden point at the chunk's first query).  gden [n] = dense gallery identity
// 0..G-1 (np.unique's inverse), qden [mq] = the dense identity of the query's id or -1 when the gallery does not hold it.  No identity
// may have more than 16 384 gallery entries (the caller checks: its choice is stored in 16 bits).
extern "C" int ssg_cmc_sgs_groups(const float* dist, int mq, int n, int64_t ld, const int32_t* qid, const int32_t* qcam, const int32_t* qden,
                                  const int32_t* gid, const int32_t* gcam, const int32_t* gden, int G, int separate_cams, void* ws, size_t ws_bytes,
                                  hipStream_t stream) {
  SgsWs w;
  const int rc = sgs_check("ssg_cmc_sgs_groups", mq, n, G, ws, ws_bytes, &w);
  if (rc) return rc;
  if (ld < n || !dist || !qid || !qcam || !qden || !gid || !gcam || !gden) {
    ssg_set_error("ssg_cmc_sgs_groups: null argument or row pitch ld=%lld < n=%d", (long long)ld, n);
    return SSG_ERR_INVALID;
  }
  hipLaunchKernelGGL(sgs_groups_kernel, dim3(mq), dim3(1024), 0, stream, dist, ld, n, qid, qcam, qden, gid, gcam, gden, G, separate_cams, w);
  SSG_LAUNCH_CHECK("sgs_groups_kernel");
  return SSG_OK;
}

// stage 2: words [nwords] = the 32-bit words word_base, word_base + 1, ... of the stream; state [4] as described at the kernel (the
// caller zeroes state[1..3] before the first launch of a chunk and relaunches with more words while state[3] is set).
extern "C" int ssg_cmc_sgs_draws(void* ws, size_t ws_bytes, int mq, int n, int G, const uint32_t* words, uint64_t word_base, uint64_t nwords,
                                 uint64_t* state, hipStream_t stream) {
  SgsWs w;
  const int rc = sgs_check("ssg_cmc_sgs_draws", mq, n, G, ws, ws_bytes, &w);
  if (rc) return rc;
  if (!state || (nwords && !words)) { ssg_set_error("ssg_cmc_sgs_draws: null state, or nwords=%llu without words", (unsigned long long)nwords); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(sgs_draws_kernel, dim3(1), dim3(64), 0, stream, w, mq, G, (const unsigned*)words, (unsigned long long)word_base,
                     (unsigned long long)nwords, (unsigned long long*)state);
  SSG_LAUNCH_CHECK("sgs_draws_kernel");
  return SSG_OK;
}

// stage 3: k [mq, 10] = per (query, repeat) the bin the reference credits, -1 for a query without a valid true match
extern "C" int ssg_cmc_sgs_counts(const void* ws, size_t ws_bytes, int mq, int n, int G, int32_t* k, hipStream_t stream) {
  SgsWs w;
  const int rc = sgs_check("ssg_cmc_sgs_counts", mq, n, G, ws, ws_bytes, &w);
  if (rc) return rc;
  if (!k) { ssg_set_error("ssg_cmc_sgs_counts: k is null"); return SSG_ERR_INVALID; }
  hipLaunchKernelGGL(sgs_counts_kernel, dim3((unsigned)mq * SGS_REPEAT), dim3(256), 0, stream, w, n, G, k);
  SSG_LAUNCH_CHECK("sgs_counts_kernel");
  return SSG_OK;
}
