/*
 * ssg_hip.h -- C ABI of libssg_hip.so: the MI355X (gfx950) kernels behind the SSG
 * pseudo-label grouping hot path (extract -> N x N re-rank -> eps -> DBSCAN).
 *
 * The reference (SHI-Labs/Self-Similarity-Grouping) has no FFI layer: its boundary for this
 * path is the Python call surface of selftraining.py / reid/.  This header is what a ctypes
 * stub in that Python binds (INTEGRATION.md shows the stub); every entry point names the
 * reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller (PyTorch
 *     or any HIP allocator) owns all buffers including workspaces;
 *   - calls are asynchronous on `stream` (a hipStream_t, 0 = default stream), re-entrant,
 *     and keep no global state;
 *   - return value: SSG_OK (0) or a negative SSG_ERR_* code; ssg_last_error() gives the
 *     message (thread-local).  No C++ exception crosses the boundary;
 *   - "half" = IEEE binary16 stored as uint16_t bit patterns; arithmetic on it follows
 *     numpy's half loops (float32 op + round-to-nearest-even), see DESIGN.md;
 *   - row-block arguments (row0, nrows) address rows [row0, row0+nrows) of an N-row
 *     problem: one GPU of a row-sharded job passes its own block, a single GPU passes
 *     (0, N).
 */
#ifndef SSG_HIP_H
#define SSG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ssg_stream_t; /* == hipStream_t */

#define SSG_OK 0
#define SSG_ERR_INVALID (-1)  /* bad argument / shape */
#define SSG_ERR_HIP (-2)      /* HIP runtime error */
#define SSG_ERR_OVERFLOW (-3) /* caller-provided capacity exceeded */
#define SSG_ERR_NAN (-4)

const char* ssg_last_error(void);
int ssg_version(void);
/* half(x) with one rounding; used for the weak python scalar (1-lambda) of rerank.py:122 */
uint16_t ssg_double_to_half_bits(double d);

/* ---- K3/K4 pairwise distance (replaces scipy cdist in reid/rerank.py:36-37,61-62) ------ */
/* Value ranges of the two feature sets in one launch: out4 (device, 4 floats) = [max|a|, max|b|, max row norm of a, max row norm of b];
 * the norms are float32 upper bounds (inflated by 1e-5).  a [rows_a,d], b [rows_b,d] or NULL.  The host picks the digit count of
 * ssg_gram_i8_encode and the tolerance / operand scales of ssg_source_rowmin_filtered* from them (one read-back). */
int ssg_range_stats_f32(const float* a, int rows_a, const float* b, int rows_b, int d, float* out4, ssg_stream_t stream);
/* norms[i] = sum_k x[i,k]^2 in float64, accumulated exactly like the Gram kernel.
 * round_to_half != 0 first rounds x to half (rerank.py:33 feat = astype(float16)). */
int ssg_row_norms_f64(const float* x, int n, int d, int round_to_half, double* norms, ssg_stream_t stream);
/* D[il, j] = half(half(sqrt(|f16(x_i) - f16(x_j)|^2))^2) for rows i = row0+il (rerank.py:33,61-62)
 * rowmax[il] = max_j D[il, j] as half bits in a uint32 (rerank.py:68 max(original_dist, axis=0)).
 * x [N,d] f32 row-major, d % 4 == 0; norms from ssg_row_norms_f64(x, N, d, 1).
 * memory_save != 0: the reference's MemorySave=True branch (rerank.py:49-59) D = half(sqrt(.)^2), squared in float64 and rounded
 * once (Minibatch only chunks the rows there and does not change a value). */
int ssg_sqdist_self_f16(const float* x, const double* norms, int N, int d, int row0, int nrows, int memory_save, uint16_t* D, uint32_t* rowmax,
                        ssg_stream_t stream);
/* The same matrix as an EXACT integer Gram on the int8 matrix cores (csrc/gram_i8.hip): for half-rounded features in
 * [-1, 1] (L2-normalised embeddings) feat*2^24 is an integer and scipy's float64 squared distance is exact, so
 * d2*2^48 = |X_i|^2 + |X_j|^2 - 2<X_i,X_j> as an integer, with the dot product on v_mfma_i32_32x32x32_i8 over ndigits balanced
 * radix-256 digits (3: -0.50195 <= feat <= 0.4978, 9 digit products; 4: |feat| <= 1, 16), gives the identical value.
 * The integer is exact for every admitted input: up to 4 d * 2^48 = 2^64 at d = 16384, combined modulo 2^64 (2^64 itself saturates;
 * half holds nothing above 65504 anyway).  For d2 < 32 D is the reference's bit for bit; beyond, it is sqrt -> half -> square -> half
 * of the correctly rounded float64 of that exact integer, where scipy's running float64 sum may round differently in the last bit.
 * ssg_gram_i8_encode writes the digits (ssg_gram_i8_encoded_bytes bytes: whole 64-row panels, layout [row / 64][k block][row % 64]
 * [digit][32] since round 4 -- opaque to the caller, consumed by ssg_sqdist_self_i8 only) and the exact int64 norms and sets *flag when a
 * feature does not fit (caller zeroes *flag first and falls back to ssg_sqdist_self_f16 when it is set;
 * ssg_sqdist_self_i8 itself does nothing in that case).  d <= 16384. */
size_t ssg_gram_i8_encoded_bytes(int n, int d, int ndigits);
int ssg_gram_i8_encode(const float* x, int n, int d, int ndigits, void* E, int64_t* norms, int32_t* flag, ssg_stream_t stream);
int ssg_sqdist_self_i8(const void* E, const int64_t* norms, int N, int d, int ndigits, int row0, int nrows, int memory_save, uint16_t* D,
                       uint32_t* rowmax,
                       const int32_t* flag, ssg_stream_t stream);
/* rowmin[i] = min_s half(cdist(tgt_i, src_s)^2) as half bits in uint32 (rerank.py:36-37,39) */
int ssg_source_rowmin_f16(const float* tgt, const double* ntgt, const float* src, const double* nsrc, int nrows, int Ns, int d,
                          uint32_t* rowmin, ssg_stream_t stream);
/* Same result by filter-and-refine: a float32 MFMA pass bounds every target-source distance per row and
 * 8-source granule, float64 re-evaluates only the granules within `tol` of the row's bound (tol >= float32
 * error of the bound).  src has Ns_pad rows (rows >= Ns padding), d % 32 == 0, Ns_pad % 128 == 0;
 * ws = nrows + Ns_pad + nrows*Ns_pad/8 floats (row norms + the per-row bounds of every 8-source granule).
 * scale_t, scale_s > 0: the bound pass runs on the fp16 matrix cores over split-half (h8l8) copies of
 * tgt*scale_t and src*scale_s (powers of two with max|x|*scale < 65504; ws grows by (nrows + Ns_pad)*d floats)
 * and tol must cover that pass's error; 0 = float32 MFMA bound pass. */
int ssg_source_rowmin_filtered(const float* tgt, const float* src, int nrows, int Ns, int Ns_pad, int d, float tol, float scale_t,
                               float scale_s, float* ws, uint32_t* rowmin, ssg_stream_t stream);
/* The same with the bound pass as a plain fp16 GEMM (csrc/source_bound.hip: half copies of tgt*scale_t and src*scale_s, one
 * v_mfma_f32_32x32x16_f16 product per term, 2 bytes per operand element instead of 4); tol must additionally cover 2^-10 |x||y| per
 * dot product -- a few more granules are re-evaluated in float64, the result is the same.  Needs scale_t, scale_s > 0 (runs the
 * three-product pass otherwise); ws as for ssg_source_rowmin_filtered with the split copies. */
int ssg_source_rowmin_filtered1(const float* tgt, const float* src, int nrows, int Ns, int Ns_pad, int d, float tol, float scale_t,
                                float scale_s, float* ws, uint32_t* rowmin, ssg_stream_t stream);
/* v = half(1-exp(-rowmin)); *max_bits = max(v); v /= max(v)   (rerank.py:38-40).  A zero
 * max means the reference would produce NaNs (0/0): the caller must raise. */
int ssg_source_vec_finish(const uint32_t* rowmin, int N, uint16_t* v, uint32_t* max_bits, ssg_stream_t stream);

/* ---- K5 ranking (replaces np.argsort in reid/rerank.py:68-70) --------------------------- */
/* rank[il, 0:K] = the K smallest of half(D[il,:]/rowmax[il]) in (value, column) order
 * (== np.argsort(kind='stable'); opt-in rank_mode='stable'). K <= 64 */
int ssg_topk_rank(const uint16_t* D, const uint32_t* rowmax, int N, int nrows, int K, int32_t* rank, ssg_stream_t stream);
/* The same K columns in the order of the UNMODIFIED reference: np.argsort's default kind (rerank.py:70) is numpy's unstable
 * introsort on an index array (npysort aquicksort_<half>: median-of-3 Hoare partition, insertion sort below 17 entries,
 * heapsort past the depth budget), so the column of equal keys depends on the whole partition sequence.  One workgroup per
 * row replays exactly the partitions that reach columns [0,K) (csrc/topk_intro.hip).  2 <= N <= 131072, K <= 64.
 * Two launches: a workgroup per row runs the partitions of ranges longer than 2048 entries (SSG_INTRO_TAILN; 0 = one launch,
 * the round-2 kernel) and hands the shorter ranges that still intersect [0, K) to a one-wave-per-row tail kernel through ws.
 * ws: ssg_topk_rank_introsort_ws_bytes(N, nrows) bytes = the hand-over records (about 9 KB per row) plus, for rows that do not fit
 * in LDS (N > ~36 k), the global arena.  A caller that passes ssg_topk_rank_introsort_arena_bytes(N, nrows) bytes selects the
 * global-arena variant for any N (parity tests).  ws == NULL / fewer bytes than the hand-over records (the pre-round-3 calling
 * convention for LDS-resident rows) is accepted: the replay then runs unsplit in one launch (slower); only the arena is mandatory. */
size_t ssg_topk_rank_introsort_ws_bytes(int N, int nrows);
/* round 6 (test / diagnostic surface): byte offset, inside a workspace of ssg_topk_rank_introsort_arena_bytes(N, nrows) bytes, of the per-row
 * int32 flags of the streamed replay (1 = the row was handed to the in-place kernel: a pivot landed inside [0, K)); (size_t)-1 when the
 * streamed kernel does not run for this N.  Valid after the call that used the workspace. */
size_t ssg_topk_rank_introsort_flags_offset(int N, int nrows);
size_t ssg_topk_rank_introsort_arena_bytes(int N, int nrows);
int ssg_topk_rank_introsort(const uint16_t* D, const uint32_t* rowmax, int N, int nrows, int K, int32_t* rank, void* ws, size_t ws_bytes,
                            ssg_stream_t stream);

/* ---- K6 k-reciprocal encoding (reid/rerank.py:74-92) ------------------------------------ */
int ssg_krecip_row_capacity(int k1); /* entries per sparse V row: (k1+1)*(round(k1/2)+2) */
/* rank is the FULL [N,K] table; D/rowmax and the outputs cover rows [row0,row0+nrows).
 * Output: sparse rows sorted by column: v_idx/v_val [nrows,cap], v_nnz [nrows]. */
int ssg_krecip(const uint16_t* D, const uint32_t* rowmax, const int32_t* rank, int N, int row0, int nrows, int K, int k1, int cap,
               int32_t* v_idx, uint16_t* v_val, int32_t* v_nnz, ssg_stream_t stream);

/* ---- K7 local query expansion (reid/rerank.py:94-99) ------------------------------------ */
/* v_* are FULL [N,capV] tables; max_nnz = an upper bound of the V rows the k2 neighbours of these rows have (sizes the LDS staging:
 * max(v_nnz) read back, or a GUESS); q_* cover rows [row0,row0+nrows) with row stride capQ >= k2*max_nnz.
 * overflow (device int32 [2], zeroed by the caller, may be NULL; round 4): [0] = the longest V row met when one exceeds max_nnz (that
 * row of q_* is then truncated, never written out of bounds), [1] = the longest V row met at all -- lets the caller run on a guessed
 * max_nnz without a host round trip, redo the rare miss and size its next guess.
 * One wave stages the min(k2, N, K) V rows of a row in LDS (about 10 bytes per entry of max_nnz each): the call runs 4, 2 or 1 rows per
 * workgroup, whatever fits 160 KB -- ssg_query_expand_rows_per_group tells which, 0 when one row alone does not fit (k2 = 64 fits rows
 * of up to 255 entries); the call then returns SSG_ERR_INVALID. */
int ssg_query_expand_rows_per_group(int N, int K, int k2, int max_nnz);
int ssg_query_expand(const int32_t* v_idx, const uint16_t* v_val, const int32_t* v_nnz, const int32_t* rank, int N, int row0, int nrows,
                     int K, int k2, int capV, int capQ, int max_nnz, int32_t* q_idx, uint16_t* q_val, int32_t* q_nnz, int32_t* overflow,
                     ssg_stream_t stream);

/* ---- K8 inverted index (reid/rerank.py:101-103) ------------------------------------------ */
/* colcnt [ncols] int32 scratch, colptr [ncols+1] int64, inv_row/inv_val >= sum(q_nnz) entries */
int ssg_invert_index(const int32_t* q_idx, const uint16_t* q_val, const int32_t* q_nnz, int nrows, int ncols, int capQ, int32_t* colcnt,
                     int64_t* colptr, int32_t* inv_row, uint16_t* inv_val, ssg_stream_t stream);

/* ---- K9 Jaccard distance (reid/rerank.py:105-122) ---------------------------------------- */
/* Jp[il,k] = half(clamp(1 - t/(2-t)) * half(1-lambda)); q_* are FULL tables; inv_nnz = colptr[N];
 * colmeta = caller workspace of 2*nrows*capQ int32. */
int ssg_jaccard_rows(const int32_t* q_idx, const uint16_t* q_val, const int32_t* q_nnz, int capQ, const int64_t* colptr,
                     const int32_t* inv_row, const uint16_t* inv_val, int64_t inv_nnz, int32_t* colmeta, int N, int row0, int nrows,
                     uint16_t one_minus_lambda_half, uint16_t* Jp, ssg_stream_t stream);
/* Second generation (round 4): the same J' rows with every line written once, plus a SPARSE copy S of the columns the row's walk
 * touched -- every other column holds the constant J'(0) = half(1 - lambda), the largest value of the row.  s_pool [s_cap] uint32 =
 * packed (J' << 17 | column); seg_off / seg_len [nrows * ssg_jaccard_segments(N)] = the segment of every (row, 32768-column chunk);
 * s_cursor [2] uint64 (zeroed by the call): entries allocated, and 1 when a segment did not fit (S unusable: consumers go dense).
 * s_pool == NULL: J' only.  ssg_eps_compact_below_s / ssg_region_query_s are the passes that walk S instead of the N x N matrix. */
int ssg_jaccard_segments(int N);
int ssg_jaccard_rows2(const int32_t* q_idx, const uint16_t* q_val, const int32_t* q_nnz, int capQ, const int64_t* colptr,
                      const int32_t* inv_row, const uint16_t* inv_val, int64_t inv_nnz, int32_t* colmeta, int N, int row0, int nrows,
                      uint16_t one_minus_lambda_half, uint16_t* Jp, uint32_t* s_pool, uint64_t s_cap, uint64_t* s_cursor, int64_t* seg_off,
                      int32_t* seg_len, ssg_stream_t stream);
/* API materialisation of final_dist (rerank.py:122): out[il,k] = f64(Jp) + f64(half(v_i+v_k))*lambda */
int ssg_final_dist_f64(const uint16_t* Jp, const uint16_t* v, int N, int row0, int nrows, double lambda_value, double* out,
                       ssg_stream_t stream);

/* ---- K10 epsilon rule (selftraining.py:289-293) ------------------------------------------ */
/* Matrix view for K10/K11 (M is [nrows,N] row-major): mode 0 = half Jp + v + lambda -> the
 * final_dist values of rerank.py:122; mode 1 = plain half matrix (no-rerank euclidean_dist);
 * mode 2 = plain float64 matrix (any precomputed distance, the sklearn drop-in case). */
/* One radix level over the strict upper triangle, zeros dropped: hist[bin] (uint64[4097]) +=
 * count of keys whose bits above (shift+width) equal prefix; hist[4096] += non-zero count. */
int ssg_eps_hist(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, uint64_t prefix,
                 int shift, int width, int count_nonzero, uint64_t* hist, ssg_stream_t stream);
/* buf[cursor++] = key for every strict-upper non-zero key <= key_max (writes beyond cap dropped) */
int ssg_eps_compact(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, uint64_t key_max,
                    uint64_t* buf, uint64_t cap, uint64_t* cursor, ssg_stream_t stream);
/* Fast path of the epsilon rule: (1) float32-surrogate histogram (4096 bins over the float bit pattern, hist[4096] = sample size;
 * hist = 4097 uint64 zeroed by the caller) of every row_stride-th local row's strict-upper non-zero elements; (2) threshold =
 * upper edge of the bin after the one where the cumulative count reaches quantile * sample size -> thr3 = {float bits, sample
 * size, bin}; (3) ONE pass over the block: exact float64 keys of the strict-upper non-zero elements whose surrogate is below the
 * threshold -> buf (cursor2[0] counts them, writes beyond cap dropped), cursor2[1] += exact zeros.  The caller sorts, and accepts
 * the result only if the top-th smallest key is below the threshold by more than the surrogate error (else: the radix select). */
int ssg_eps_sample_hist(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, int row_stride,
                        const uint64_t* refine, uint64_t* hist, ssg_stream_t stream);
/* thr = 5 uint64: {threshold float bits, sample size, selected coarse bin, sample elements below that bin, target rank} */
/* round 6: both sampling levels AND their selections in two launches (instead of four): the workgroup that finishes a level last selects.
 * hist2x = 2 x 4097 words and tickets2 = 2 words, zeroed by the caller; thr5 (5 words) ends up as ssg_eps_select_threshold followed by
 * ssg_eps_refine_threshold leave it (the separate calls remain: the sharded two-call form all-reduces the histograms in between) */
int ssg_eps_sample_threshold(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, int row_stride,
                             double quantile, uint64_t* hist2x, uint64_t* thr5, uint32_t* tickets2, ssg_stream_t stream);
int ssg_eps_select_threshold(const uint64_t* hist, double quantile, uint64_t* thr3, ssg_stream_t stream);
/* second level: ssg_eps_sample_hist(..., refine = thr, hist2) counts the sample elements of the selected coarse bin in 1024 linear
 * sub-bins (hist2 zeroed by the caller); this replaces thr[0] by the sub-bin edge (one guard sub-bin) */
int ssg_eps_refine_threshold(const uint64_t* hist2, uint64_t* thr, ssg_stream_t stream);
int ssg_eps_compact_below(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value,
                          const uint64_t* thr3, uint64_t* buf, uint64_t cap, uint64_t* cursor2, ssg_stream_t stream);
/* the same pass through the sparse copy S (mode 0 handles only): cursor3 = {keys collected, exact zeros, dense pass needed} zeroed by
 * the caller, vmin = ssg_half_min(v), rowmask = nrows bytes of workspace.  Row i is walked through S when its floor
 * J'(0) + lambda * half(v_i + vmin) -- a lower bound of every column outside S -- lies at or above the threshold; the other rows (all
 * of them when S overflowed or lambda < 0) are flagged in rowmask and done by the dense pass queued behind (inside this call), gated on
 * cursor3[2] -- decided on the device, no read-back in between */
int ssg_eps_compact_below_s(const void* M, const uint16_t* v, int N, int row0, int nrows, double lambda_value, const uint64_t* thr3,
                            uint64_t* buf, uint64_t cap, uint64_t* cursor3, const uint32_t* s_pool, const int64_t* seg_off,
                            const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin, uint16_t jp0_half,
                            uint8_t* rowmask, ssg_stream_t stream);
/* *out_bits = the smallest of N non-negative halves (the source vector v of rerank.py:38-40) as half bits */
int ssg_half_min(const uint16_t* v, int N, uint32_t* out_bits, ssg_stream_t stream);
int ssg_fill_u64(uint64_t* buf, uint64_t n0, uint64_t n1, uint64_t value, ssg_stream_t stream);
int ssg_sort_u64(uint64_t* buf, uint64_t n_pow2, ssg_stream_t stream); /* ascending, n = 2^k >= 2048 */
/* round 5: the same sort with the number of keys left on the device (*n_dev, the compaction pass's cursor word): the network is launched
 * for the capacity n_cap (2^k >= 2048) but works on the power of two >= max(*n_dev, 2048) only; [*n_dev, that) is filled with ~0 first */
int ssg_sort_u64_dev(uint64_t* buf, uint64_t n_cap, const uint64_t* n_dev, ssg_stream_t stream);
/* round 5: the a-posteriori checks of the sampled eps rule on the device (selftraining.py:289-293 stays exact): top = rint(rho * (upper_total -
 * cursor[1])) == top_guess (the tree ssg_eps_mean_run summed), cursor[0] <= n_cap keys collected, >= top of them, the top-th sorted key below
 * the float32 threshold thr3[0] by its margin.  status6 = {ok, got, zeros, top, top-th key bits, threshold bits}; on failure eps2[0] := NaN */
int ssg_eps_check(const uint64_t* sorted_keys, const uint64_t* cursor, const uint64_t* thr3, double rho, uint64_t upper_total, int64_t top_guess,
                  uint64_t n_cap, double* eps2, uint64_t* status6, const uint64_t* sort_fail, ssg_stream_t stream);   /* sort_fail: nullable, ssg_samplesort_u64_dev's word */
/* round 5: the same device-sized ascending sort in 5 launches instead of 25 (sample sort: 1023 splitters out of a sorted sample of 4096 keys,
 * buckets ranked in LDS; keys equal to a splitter get their own bucket, so duplicates cost nothing).  In place through ws (any n_cap >= 1);
 * *fail = 1 when a bucket between two splitters holds more than 16384 keys (buf is then a permutation of the keys, not sorted) */
size_t ssg_samplesort_u64_workspace_bytes(uint64_t n_cap);
int ssg_samplesort_u64_dev(uint64_t* buf, uint64_t n_cap, const uint64_t* n_dev, void* ws, size_t ws_bytes, uint64_t* fail, ssg_stream_t stream);
/* round 6: a second geometry of the same sort for 4e5 .. 2.4e7 expected keys (4095 splitters out of a sorted sample of 16 384 keys, sorting
 * buckets of up to 16 384 keys in 128 KB of LDS, 1024 threads): N = 128 000 collects 1.7e7 candidates, where the bitonic network over the
 * whole array took 7.1 ms.  Same contract as ssg_samplesort_u64_dev (*fail = 1: a bucket beyond 16 384 keys), its own workspace size. */
size_t ssg_samplesort_u64_big_workspace_bytes(uint64_t n_cap);
int ssg_samplesort_u64_big_dev(uint64_t* buf, uint64_t n_cap, const uint64_t* n_dev, void* ws, size_t ws_bytes, uint64_t* fail, ssg_stream_t stream);
size_t ssg_eps_mean_workspace_bytes(int64_t top);
/* out2[0] = mean of the first `top` sorted keys with numpy's pairwise summation (mode 0: f64;
 * mode 1: float32 sum of half values -> half, out2[1] = its bits) */
int ssg_eps_mean(const uint64_t* sorted_keys, int64_t top, int mode, void* ws, size_t ws_bytes, double* out2, ssg_stream_t stream);
/* the same in two steps: _prepare uploads the recursion tables of numpy's pairwise tree for `top` summands (blocks until the copy is
 * done: call it while the stream is idle), _run launches the summation asynchronously.  ssg_eps_mean = prepare + run. */
int ssg_eps_mean_prepare(int64_t top, void* ws, size_t ws_bytes, ssg_stream_t stream);
int ssg_eps_mean_run(const uint64_t* sorted_keys, int64_t top, int mode, void* ws, size_t ws_bytes, double* out2, ssg_stream_t stream);
/* round 6: ssg_eps_mean_run followed by ssg_eps_check without the check's own launch (same arguments as the two calls; eps2 = out2) */
int ssg_eps_mean_check(const uint64_t* sorted_keys, int64_t top_guess, int mode, void* ws, size_t ws_bytes, double* eps2, const uint64_t* cursor,
                       const uint64_t* thr3, double rho, uint64_t upper_total, uint64_t n_cap, uint64_t* status6, const uint64_t* sort_fail, ssg_stream_t stream);

/* ---- K11/K12 DBSCAN (selftraining.py:295,306; sklearn 1.7.2 DBSCAN precomputed) ---------- */
/* cnt[il] = |{k: d(i,k) <= eps}|; edges[2e],[2e+1] = (i,k) for every hit (cursor counts all) */
int ssg_region_query(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, double eps,
                     int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor, ssg_stream_t stream);
/* the same through S, row by row: row i through S when J'(0) + lambda * half(v_i + vmin) > eps, the dense scan (queued behind, gated on
 * cursor2[1]) for the rows flagged in rowmask.  cursor2 = {edges counted, dense pass needed}, zeroed by the caller. */
int ssg_region_query_s(const void* M, const uint16_t* v, int N, int row0, int nrows, double lambda_value, double eps, const uint32_t* s_pool,
                       const int64_t* seg_off, const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin,
                       uint16_t jp0_half, uint8_t* rowmask, int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor2,
                       ssg_stream_t stream);
/* round 5: both region queries with eps read from device memory (*eps_dev, e.g. out2[0] of ssg_eps_mean_run after ssg_eps_check): the eps rule,
 * the region query and the components run back to back, the host reads eps with the labels.  *eps_dev = NaN: no hit */
int ssg_region_query_dev(const void* M, const uint16_t* v, int N, int row0, int nrows, int mode, double lambda_value, const double* eps_dev,
                         int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor, ssg_stream_t stream);
int ssg_region_query_s_dev(const void* M, const uint16_t* v, int N, int row0, int nrows, double lambda_value, const double* eps_dev, const uint32_t* s_pool,
                           const int64_t* seg_off, const int32_t* seg_len, int nseg, const uint64_t* s_cursor, const uint32_t* vmin,
                           uint16_t jp0_half, uint8_t* rowmask, int32_t* cnt, int32_t* edges, uint64_t cap_edges, uint64_t* cursor2,
                           ssg_stream_t stream);
/* round 6 (sharded eps rule + DBSCAN as one device chain): nseg fixed-capacity segments of 8-byte items -- the all-gathered
 * candidate-key or edge buffers of the ranks; segment s holds min(counts[s * count_stride], seg_cap) valid items at in + s * seg_stride -- are
 * written to `out` back to back in segment order without the host seeing the counts.  total2[0] = items written, total2[1] = 1 when a
 * segment's count exceeded seg_cap (its owner's buffer overflowed).  out holds nseg * seg_cap items. */
int ssg_concat_segments_u64(const uint64_t* in, int nseg, uint64_t seg_cap, uint64_t seg_stride, const uint64_t* counts, int count_stride,
                            uint64_t* out, uint64_t* total2, ssg_stream_t stream);
size_t ssg_dbscan_cc_workspace_bytes(int N);
/* cnt is the FULL [N] table, edges the concatenated edge list: labels[N] int64, -1 = noise */
int ssg_dbscan_cc(const int32_t* cnt, const int32_t* edges, uint64_t nedges, int N, int min_samples, void* ws, size_t ws_bytes,
                  int64_t* labels, ssg_stream_t stream);
/* the same with the edge count left on the device (the region query's cursor; min(*nedges_dev, cap_edges) edges are read): no host
 * round trip between region query and labels.  labels may be NULL (round 6): the int64 conversion launch is skipped and the caller reads
 * the labels as int32 from the workspace itself -- lab = (int32_t*)ws + N, 0x7fffffff = noise (ws: parent[N] | lab[N] | ...) */
int ssg_dbscan_cc_dev(const int32_t* cnt, const int32_t* edges, const uint64_t* nedges_dev, uint64_t cap_edges, int N, int min_samples,
                      void* ws, size_t ws_bytes, int64_t* labels, ssg_stream_t stream);

/* ---- K1/K2 ResNet-50 embedding forward (reid/models/resnet.py:86-111, reid/evaluators.py:18-60) */
/* Conv2d with eval-BatchNorm folded into (w, bias) + optional residual add + optional ReLU, NHWC
 * float32 on the fp32 matrix cores.  in [B,H,W,Cin]; w [Cout][Kpad], k = ((c/32)*KH*KW + r*KW+s)*32 + c%32
 * (32-channel chunks outermost: the taps of a chunk re-read cached pixels; stem: k = (r*KW+s)*4 + c), rows
 * zero-padded to Kpad (multiple of 32); res/out [B,OH,OW,Cout].  Cin % 32 == 0 or Cin == 4 (stem:
 * RGB0 pixels, Kpad = 32*ceil(KH*KW/8)); Cout % 64 == 0.  (cuDNN conv+BN+ReLU of base.py:57-93) */
int ssg_conv2d_nhwc_f32(const float* in, const float* w, const float* bias, const float* res, float* out, int B, int H, int W, int Cin,
                        int Cout, int KH, int KW, int stride, int pad, int relu, ssg_stream_t stream);
/* Bottleneck tail with a downsample branch (base.py:75-90) as one GEMM over the concatenated K:
 * out = relu(conv3(in) + downsample(in2) + bias); w [Cout][Cin+Cin2], bias = folded b3 + b_ds;
 * in [B,H,W,Cin] (1x1 stride 1), in2 [B,H2,W2,Cin2] sampled at (oh*stride2, ow*stride2). */
int ssg_conv1x1_dual_nhwc_f32(const float* in, const float* in2, const float* w, const float* bias, float* out, int B, int H, int W, int Cin,
                              int H2, int W2, int Cin2, int stride2, int Cout, int relu, ssg_stream_t stream);
/* Same two layers with the fp32 values carried as SPLIT HALVES ("h8l8": per 8 consecutive channels 32 bytes =
 * [8 x half hi][8 x half lo], hi = half(v), lo = half(v - hi); same 4 bytes per value and same addressing as
 * fp32).  flags & SSG_CONV_IN_SPLIT: in (in2) and w are h8l8, w pre-multiplied by 1/acc_scale (a power of two
 * that lifts small weights out of the half subnormals); the GEMM then runs on v_mfma_f32_32x32x16_f16 as
 * xh*wh + xh*wl + xl*wh with fp32 accumulation (half x half products are exact in fp32, the dropped xl*wl is
 * < 2^-22 |x*w|): fp32-class results at 3/16 of the fp32-MFMA cost.  flags & SSG_CONV_OUT_SPLIT: out and res
 * are h8l8 (values must stay below 65504).  flags = 0 is exactly ssg_conv2d_nhwc_f32. */
#define SSG_CONV_IN_SPLIT 1
#define SSG_CONV_OUT_SPLIT 2
/* ch_scale (nullable): per-output-channel factor applied to the accumulator (after acc_scale) before the bias -- the split path
 * pre-multiplies every weight ROW by its own power of two, so folded checkpoints whose per-channel BN scales span orders of
 * magnitude keep all their bits.  overflow (nullable): *overflow is set to 1 when a value that does not fit the split-half
 * output format (|v| >= 65520 or NaN) is written; the caller zeroes it, reads it after the forward and falls back to fp32. */
int ssg_conv2d_nhwc_x(const void* in, const void* w, const float* bias, const void* res, void* out, int B, int H, int W, int Cin,
                      int Cout, int KH, int KW, int stride, int pad, int relu, int flags, float acc_scale, const float* ch_scale,
                      int32_t* overflow, ssg_stream_t stream);
int ssg_conv1x1_dual_nhwc_x(const void* in, const void* in2, const void* w, const float* bias, void* out, int B, int H, int W, int Cin,
                            int H2, int W2, int Cin2, int stride2, int Cout, int relu, int flags, float acc_scale, const float* ch_scale,
                            int32_t* overflow, ssg_stream_t stream);
/* Tiled weights.  The LDS-DMA kernel behind the two entry points above streams its weight stages 16 rows x 64 bytes at a time; from the
 * row-major w that is half a cache line per row.  ssg_conv_weights_tile writes the same containers k-tile-major:
 * wt [Cout/128][Kpad/16][128 rows][64 B], slot pc (16 bytes) of row r holding the row's chunk pc ^ ((r >> 2) & 3) of that k-tile, so that
 * every DMA instruction reads 1 KB contiguous.  Returns 1 when wt was written, 0 when the shape has no tiled form (Cout % 128 or
 * Kpad % 16, see ssg_conv_weights_tile_supported; nothing is written), negative on error.  wt: Cout * Kpad containers, not overlapping w.
 * The _xt entry points are the _x ones plus that pointer (NULL = row-major everywhere); only the three-product LDS-DMA launches read it,
 * w stays required, and the result is bit-identical either way.  flags & SSG_CONV_W_TILED hands the same copy to the _x entry points
 * without the pointer: it then lies right behind w (wt == (float*)w + Cout * Kpad). */
#define SSG_CONV_W_TILED 4
int ssg_conv_weights_tile_supported(int Cout, int Kpad);
int ssg_conv_weights_tile(const void* w, int Cout, int Kpad, void* wt, ssg_stream_t stream);
int ssg_conv2d_nhwc_xt(const void* in, const void* w, const void* wt, const float* bias, const void* res, void* out, int B, int H, int W, int Cin,
                       int Cout, int KH, int KW, int stride, int pad, int relu, int flags, float acc_scale, const float* ch_scale,
                       int32_t* overflow, ssg_stream_t stream);
int ssg_conv1x1_dual_nhwc_xt(const void* in, const void* in2, const void* w, const void* wt, const float* bias, void* out, int B, int H, int W, int Cin,
                             int H2, int W2, int Cin2, int stride2, int Cout, int relu, int flags, float acc_scale, const float* ch_scale,
                             int32_t* overflow, ssg_stream_t stream);
/* One identity bottleneck block (base.py:57-90 without a downsample branch, stride 1) in ONE launch, split-half tensors:
 * out = relu(conv3(relu(conv2_3x3(relu(conv1(x))))) + x).  x / out [B,H,W,C] h8l8 (out must not alias x); w1 [MID][C],
 * w2 [MID][9*MID] (k = (32-channel chunk, tap, channel)), w3 [C][MID] as ssg_conv2d_nhwc_x takes them, rows pre-multiplied by
 * powers of two that cs1/cs2/cs3 undo; b* fp32 folded BatchNorm biases.  Bit-identical to the three ssg_conv2d_nhwc_x launches;
 * the two MID-channel intermediates stay in LDS.  ssg_bottleneck_supported() tells which block shapes have a kernel
 * (layer1 of ResNet-50 at 256x128 input: H x 32 x 256, MID 64; CIN == C for the identity block, CIN = 64 for the first block).
 * ssg_bottleneck_ds_nhwc_x: the block with a stride-1 downsample branch, out = relu(conv3(...) + downsample(x)); x [B,H,W,CIN],
 * w3cat [C][MID + CIN] = conv3 | downsample weights along K and b3 = b3 + b_ds, as ssg_conv1x1_dual_nhwc_x takes them. */
int ssg_bottleneck_supported(int H, int W, int CIN, int C, int MID);
int ssg_bottleneck_nhwc_x(const void* x, const void* w1, const float* b1, const float* cs1, const void* w2, const float* b2, const float* cs2,
                          const void* w3, const float* b3, const float* cs3, void* out, int B, int H, int W, int C, int MID,
                          int32_t* overflow, ssg_stream_t stream);
int ssg_bottleneck_ds_nhwc_x(const void* x, const void* w1, const float* b1, const float* cs1, const void* w2, const float* b2, const float* cs2,
                             const void* w3cat, const float* b3, const float* cs3, void* out, int B, int H, int W, int CIN, int C, int MID,
                             int32_t* overflow, ssg_stream_t stream);
/* Next-conv instance of the layer1 identity block: the 1x1 convolution that opens the FOLLOWING block (layer2's entry conv1) rides in
 * this block's epilogue, so its launch -- a read of all of `out` -- goes away.  ssg_bottleneck_attach_next stores a descriptor in a
 * thread-local slot; this thread's next ssg_bottleneck_nhwc_x call consumes and clears it, whether it succeeds or not, and also writes
 *   y1n [B,H,W,MIDN] = relu(conv1_next(out)): w1n [MIDN][C] h8l8 row-major, rows pre-multiplied by the powers of two cs1n undoes, b1n fp32;
 *                      bit-identical to ssg_conv2d_nhwc_x(out, w1n, ...);
 *   out_s2 [B,H/2,W/2,C] = out[:, ::2, ::2] (all a stride-2 downsample branch reads of `out`).
 * y1n, out_s2 and that call's `out` may each be null (not written).  With a descriptor attached, a shape without
 * ssg_bottleneck_next_supported (1 for H % 4 == 0, W 32, C 256, MID 64, MIDN 128) is SSG_ERR_INVALID, never a plain launch.
 * ssg_bottleneck_next_enabled: the routing switch SSG_BN_L1_NEXT (0 | 1, read per call; unset: the library's compile-time default),
 * SSG_ERR_INVALID for any other value. */
int ssg_bottleneck_next_supported(int H, int W, int C, int MID, int MIDN);
int ssg_bottleneck_next_enabled(void);
int ssg_bottleneck_attach_next(const void* w1n, const float* b1n, const float* cs1n, void* y1n, void* out_s2, int MIDN);
/* One identity BasicBlock of ResNet-18 / ResNet-34 (base.py:25-54 without a downsample branch, stride 1) in ONE launch, split-half
 * tensors: out = relu(conv2_3x3(relu(conv1_3x3(x) + b1)) + b2 + x).  x / out [B,H,W,C] h8l8 (out must not alias x); w1 / w2 [C][9*C]
 * (k = (32-channel chunk, tap, channel)) as ssg_conv2d_nhwc_x takes them, rows pre-multiplied by powers of two that cs1 / cs2 undo;
 * b* fp32 folded BatchNorm biases.  Bit-identical to the two ssg_conv2d_nhwc_x launches (the range flag included: it goes up for
 * the intermediate as well as for the output); the C-channel intermediate stays in LDS and x is read from HBM once.
 * ssg_basicblock_supported(): W == 32, C == 64, H % 4 == 0 (layer1 of both networks at 128-wide input); any other shape is refused
 * before a launch. */
int ssg_basicblock_supported(int H, int W, int C);
int ssg_basicblock_nhwc_x(const void* x, const void* w1, const float* b1, const float* cs1, const void* w2, const float* b2, const float* cs2,
                          void* out, int B, int H, int W, int C, int32_t* overflow, ssg_stream_t stream);
/* The stem in ONE launch (base.py:101-105 conv1 + bn1 + relu + maxpool, with the fliplr of evaluators.py:12-16 folded into the
 * image read): images [B,3,H,W] float32 NCHW -> out [B,H/4,W/4,64] h8l8.  w [64][224] / bias / ch_scale: the stem weights as
 * ssg_conv2d_nhwc_x takes them (Cin = 4 "h4l4" layout).  Bit-identical to ssg_nchw_to_nhwc4_h4l4 + ssg_conv2d_nhwc_x +
 * ssg_maxpool3x3s2_h8l8; the 64-channel stem map never reaches HBM.  ssg_stem_pool_supported(): W == 128, H % 4 == 0. */
int ssg_stem_pool_supported(int H, int W);
int ssg_stem_pool_nchw_x(const float* images, int flip, const void* w, const float* bias, const float* ch_scale, void* out, int B, int H, int W,
                         int32_t* overflow, ssg_stream_t stream);
/* stem input for the split path: [B,3,H,W] NCHW fp32 -> [B,H,W] pixels of 16 bytes [4 x half hi][4 x half lo] ("h4l4",
 * 4th channel 0); ssg_conv2d_nhwc_x with Cin = 4 and SSG_CONV_IN_SPLIT takes these, with w in the same per-tap layout */
int ssg_nchw_to_nhwc4_h4l4(const float* in, void* out, int B, int H, int W, int flip, ssg_stream_t stream);
/* MaxPool2d(3,2,1) and the global/stripe average pool on h8l8 maps (the averages come out as fp32) */
int ssg_maxpool3x3s2_h8l8(const void* in, void* out, int B, int H, int W, int C, ssg_stream_t stream);
int ssg_gap_stripes_h8l8(const void* in, float* out, int B, int H, int W, int C, int num_split, ssg_stream_t stream);
/* fp32 [n] -> h8l8 of (in * scale), and h8l8 -> fp32 (times scale); n % 8 == 0 */
int ssg_h8l8_encode(const float* in, void* out, int64_t n, float scale, ssg_stream_t stream);
int ssg_h8l8_decode(const void* in, float* out, int64_t n, float scale, ssg_stream_t stream);
/* float32 squared-L2 block (reid/evaluators.py:63-85 pairwise_distance) on the fp32 matrix cores:
 * out[i,j] = |x_i|^2 + |y_j|^2 - 2<x_i,y_j>; self_form != 0 gives the reference's query=None form
 * 2|x_i|^2 - 2<x_i,y_j> (:64-72).  x [m,d], y [n,d], out [m,n]; d % 32 == 0, n % 64 == 0; ws = m+n floats. */
int ssg_pairwise_sqdist_f32(const float* x, const float* y, int m, int n, int d, int self_form, float* ws, float* out, ssg_stream_t stream);
/* [B,3,H,W] NCHW -> [B,H,W,4] NHWC (4th channel 0); flip != 0 mirrors W (evaluators.py:12-16 fliplr) */
int ssg_nchw_to_nhwc4(const float* in, float* out, int B, int H, int W, int flip, ssg_stream_t stream);
/* MaxPool2d(3, stride 2, padding 1) on NHWC (base.py:105) */
int ssg_maxpool3x3s2_nhwc(const float* in, float* out, int B, int H, int W, int C, ssg_stream_t stream);
/* out[s][b][c]: s=0 global average pool, s=1..S the S horizontal stripes (resnet.py:93-111) */
int ssg_gap_stripes(const float* in, float* out, int B, int H, int W, int C, int num_split, ssg_stream_t stream);
/* out = (a+b)/||a+b||_2 per row (evaluators.py:31-35: original + flipped features, L2 norm); out may alias neither a nor b */
int ssg_flip_sum_l2norm(const float* a, const float* b, float* out, int rows, int C, ssg_stream_t stream);

/* ---- kNN-set Jaccard re-ranking variant (reid/rerank_plain.py:125-178 re_ranking; shares K3/K4 with rerank.py) */
/* A_i = { j != i : D[i,j] <= k-th smallest of row i } (:165-170).  rank = ssg_topk_rank of the same rows with rowmax = half(1)
 * everywhere and K = k; a_idx/a_val [nrows, cap] (a_val = half 1: feed ssg_invert_index), a_nnz [nrows]; *overflow = rows
 * with more than cap members. */
int ssg_knn_sets(const uint16_t* D, const int32_t* rank, int N, int row0, int nrows, int K, int cap, int32_t* a_idx, uint16_t* a_val,
                 int32_t* a_nnz, int32_t* overflow, ssg_stream_t stream);
/* J'[i,k] = half(half(|A_i xor A_k| / |A_i or A_k|) * half(1-lambda)) (scipy cdist 'jaccard' on booleans, :173-175; 0 for
 * two empty sets) for rows [row0,row0+nrows); a_idx/a_nnz cover all N rows, colptr/inv_row = ssg_invert_index of them. */
int ssg_set_jaccard_rows(const int32_t* a_idx, const int32_t* a_nnz, int capA, const int64_t* colptr, const int32_t* inv_row, int N, int row0,
                         int nrows, uint16_t one_minus_lambda_half, uint16_t* Jp, ssg_stream_t stream);

/* ---- Hausdorff re-ranking variant (reid/rerank_hausdorff.py:7-65 re_ranking; csrc/hausdorff.hip; shares the half original distance
 * and the kNN sets -- ssg_knn_sets -- with the kNN-set variant).  Everything below is float64 on the vector ALU with no fused
 * multiply-add, in the one order scipy's cdist and directed_hausdorff use, so the results are the reference's bit for bit. */
/* out[i, j] = s or sqrt(s) (take_sqrt != 0, correctly rounded) for x [m, d], y [n, d] float32, out float64 at row pitch ld >= n
 * (elements):  s = 0; for c = 0 .. d-1: t = f64(x[i,c]) - f64(y[j,c]); s = s + t * t.  Any m, n, d >= 1. */
int ssg_seqdist_f64(const float* x, int m, const float* y, int n, int d, int take_sqrt, double* out, int64_t ld, ssg_stream_t stream);
/* the same for y = x: only the 64 x 64 tiles on or above the diagonal are computed, the others are their mirror images
 * ((a-b)^2 == (b-a)^2 bit for bit): out is exactly symmetric with a zero diagonal */
int ssg_seqdist_self_f64(const float* x, int n, int d, int take_sqrt, double* out, int64_t ld, ssg_stream_t stream);
/* rowmin[i] = min_j s[i, j] (the squared sum; the m x n block is never written) */
int ssg_seqdist_rowmin_f64(const float* x, int m, const float* y, int n, int d, double* rowmin, ssg_stream_t stream);
/* vec = sqrt(rowmin); *vmax = max(vec); vec = vec / max(vec)  (:14-15).  *vmax == 0: the reference divides 0/0, the caller must raise. */
int ssg_hausdorff_source_finish(const double* rowmin, int N, double* vec, double* vmax, ssg_stream_t stream);
/* Directed distances G[i, j] = max_{b in S_j} min_{a in S_i} E[a, b] for rows i in [row0, row0+nrows) of the full N x N matrix G
 * (G[i, i] = 0).  E [N, N] float64 MUST be exactly symmetric (ssg_seqdist_self_f64); a_idx [N, cap] / a_nnz [N] = the sets of all N
 * rows as ssg_knn_sets writes them (non-empty; an empty S_j gives 0).  The table is trusted, not
 * validated: a_nnz is clamped to cap and an index outside [0, N) is skipped so that a damaged table cannot read out of bounds, but
 * the result is then meaningless and no error is reported.  ws: ssg_hausdorff_workspace_bytes(N, nrows) bytes.
 * N * N < 2^31. */
size_t ssg_hausdorff_workspace_bytes(int N, int nrows);
int ssg_hausdorff_directed_rows(const double* E, const int32_t* a_idx, const int32_t* a_nnz, int cap, int N, int row0, int nrows, double* G,
                                void* ws, size_t ws_bytes, ssg_stream_t stream);
/* H = max(G, G^T) in place once every row of G is there (:57-58: the other direction of the pair (i, j) is G[j, i] because E is
 * symmetric); *hmax = max(H).  *hmax == 0: the reference divides 0/0 at :60, the caller must raise. */
int ssg_hausdorff_symmetrize(double* G, int N, double* hmax, ssg_stream_t stream);
/* out[il, j] = (H[il, j] / *hmax) * one_minus_lambda + (vec[j] + vec[row0+il]) * lambda_value, each operation rounded on its own
 * (:60-62; one_minus_lambda = 1 - lambda computed by the host in float64).  H, out: rows [row0, row0+nrows); out may be H. */
int ssg_hausdorff_blend(const double* H, const double* hmax, const double* vec, int N, int row0, int nrows, double one_minus_lambda,
                        double lambda_value, double* out, ssg_stream_t stream);
/* out = D / max(D) in numpy's half arithmetic (:41) for the whole half matrix D [N, N]; rowmax [N] = its row maxima as half bits;
 * *gmax (one word of workspace) receives max(D) as half bits */
int ssg_half_div_max(const uint16_t* D, const uint32_t* rowmax, int N, uint16_t* out, uint32_t* gmax, ssg_stream_t stream);

/* ---- retrieval metrics of the evaluation step (reid/evaluators.py:88-129 evaluate_all ->
 * reid/evaluation_metrics/ranking.py:18-79 cmc, :82-115 mean_ap + sklearn average_precision_score) */
/* dist [m, ld] float32 query x gallery block; ids / cams int32.  first_rank[q] = number of valid gallery entries
 * (different id or different camera; separate_cams != 0: different camera only, ranking.py:49-51) ordered before
 * the first true match of query q in (distance, gallery index) order, -1 when q has no valid true match;
 * ap[q] = its average precision (step-wise over distinct match distances like sklearn; NaN likewise).
 * Distances are ordered values: -0.0 == 0.0, and denormals and +-inf are accepted and ordered like any other number.  A NaN is not:
 * a query with a valid true match and a NaN distance in any valid gallery entry gets first_rank[q] = -2 and ap[q] = NaN (a NaN in
 * an entry the id / camera filter removes is never read).
 * *overflow = number of queries that were not evaluated: those with more than 2048 true matches (first_rank -1) plus those marked
 * -2.  The caller must treat a non-zero word as an error. */
int ssg_rank_metrics(const float* dist, int m, int n, int64_t ld, const int32_t* qid, const int32_t* qcam, const int32_t* gid,
                     const int32_t* gcam, int separate_cams, int32_t* first_rank, double* ap, int32_t* overflow, ssg_stream_t stream);
/* the same plus the 'allshots' CMC bins (ranking.py:62-75 with first_match_break=False): nmatch[q] = valid true matches of query q,
 * nm_before[q, s] (row stride nm_cap, s < min(nmatch[q], nm_cap)) = valid non-matching gallery entries ordered before its s-th match */
int ssg_rank_metrics_all(const float* dist, int m, int n, int64_t ld, const int32_t* qid, const int32_t* qcam, const int32_t* gid,
                         const int32_t* gcam, int separate_cams, int32_t* first_rank, double* ap, int32_t* overflow, int32_t* nm_before,
                         int32_t* nmatch, int nm_cap, ssg_stream_t stream);
/* the single-gallery-shot protocol ('cuhk03': ranking.py:10-16,53-66, ten random one-entry-per-identity gallery subsets per query) for a
 * chunk of mq queries, in three stages over one workspace of ssg_cmc_sgs_workspace_bytes(mq, n, G) bytes (0: shape outside the limits
 * n <= 131072, G <= 16384).  gden [n] = dense gallery identity 0..G-1, qden [mq] = the dense identity of the query's id or -1; no
 * identity may have more than ssg_cmc_sgs_max_group() = 16384 gallery entries (the caller checks).
 * groups: per query the valid entries grouped by identity, each group ascending in (distance, gallery index), the groups in order of
 *         first appearance.
 * draws:  numpy's legacy randint on the supplied 32-bit MT19937 words [word_base, word_base + nwords) of the stream (a group of s > 1
 *         entries takes the first word w with w & (2^bit_length(s-1) - 1) <= s - 1), queries -> 10 repeats -> groups.  state [4]:
 *         [0] words consumed so far (carried from chunk to chunk), [1] / [2] query and draw to resume at, [3] set when the words ran
 *         out: launch again with words from state[0] on.  The caller zeroes state[1..3] before a chunk's first launch.
 * counts: k [mq, 10] = other identities whose drawn entry is ordered before the drawn true match; -1: no valid true match. */
size_t ssg_cmc_sgs_workspace_bytes(int mq, int n, int G);
int ssg_cmc_sgs_max_group(void);
int ssg_cmc_sgs_groups(const float* dist, int mq, int n, int64_t ld, const int32_t* qid, const int32_t* qcam, const int32_t* qden,
                       const int32_t* gid, const int32_t* gcam, const int32_t* gden, int G, int separate_cams, void* ws, size_t ws_bytes,
                       ssg_stream_t stream);
int ssg_cmc_sgs_draws(void* ws, size_t ws_bytes, int mq, int n, int G, const uint32_t* words, uint64_t word_base, uint64_t nwords,
                      uint64_t* state, ssg_stream_t stream);
int ssg_cmc_sgs_counts(const void* ws, size_t ws_bytes, int mq, int n, int G, int32_t* k, ssg_stream_t stream);

/* ---- KISSME metric learning (reid/metric_learning/kissme.py:33-55; csrc/kissme.hip).  The reference visits the pairs (a, b), a < b,
 * in the order of its masked meshgrid: b ascending, a ascending inside b.  den [n] = dense class id of every row, 0 .. G-1
 * (1 <= G <= n <= 2^24); ids outside that range are never dereferenced, the outputs are then unspecified.
 * index:       a stable counting sort -- cls_ptr [G+1], members [n] (each class's rows ascending), rank [n] (position of a row inside
 *              its class) -- and two int64 exclusive scans over b: m_scan [n+1] counts the matching pairs (a < b) of the rows below b,
 *              nm_scan [n+1] the non-matching ones (b - rank[b] per row); m_scan[n] and nm_scan[n] are the two totals.
 * match_pairs: ia, ib [P1], P1 = m_scan[n]: every matching pair in the reference's order; slot m_scan[b] + j holds
 *              (members[cls_ptr[den[b]] + j], b).
 * unrank:      ia[t], ib[t] = the non-matching pair at position pos[t] of that order (T positions, int64).  b by bisection of nm_scan,
 *              q = pos[t] - nm_scan[b], then with L the member list of b's class and j the smallest index with L[j] - j > q: a = q + j.
 *              A position outside [0, nm_scan[n]) gives (-1, -1).
 * All outputs are functions of the inputs alone (the one atomic counts class sizes). */
int ssg_kissme_index(const int32_t* den, int n, int G, int32_t* cls_ptr, int32_t* members, int32_t* rank, int64_t* m_scan,
                     int64_t* nm_scan, ssg_stream_t stream);
int ssg_kissme_match_pairs(const int32_t* den, const int32_t* rank, const int32_t* cls_ptr, const int32_t* members,
                           const int64_t* m_scan, int n, int G, int64_t P1, int32_t* ia, int32_t* ib, ssg_stream_t stream);
int ssg_kissme_unrank(const int64_t* pos, int64_t T, const int32_t* den, const int32_t* rank, const int32_t* cls_ptr,
                      const int32_t* members, const int64_t* nm_scan, int n, int G, int32_t* ia, int32_t* ib, ssg_stream_t stream);
/* C [d, d] float64 = (sum over the P pairs of s s^T) / divisor, s = (double) X[ia[p]] - (double) X[ib[p]]; X [n, ldx] float32,
 * 16-byte aligned, ldx >= d, ldx % 4 == 0; 16 <= d <= 16384, d % 16 == 0 (the caller zero-pads the columns); any P >= 1 (the last slice
 * of 16 pairs is masked); a pair with an index outside [0, n) contributes nothing.  v_mfma_f64_16x16x4_f64, one workgroup per
 * 128 x 128 tile on or above the diagonal walking all P pairs: no split of the pair axis, no workspace, no float atomics -- the same
 * call gives the same bits, and C[i][j] and C[j][i] are the same bits (one is a copy of the other). */
int ssg_pairdiff_cov_f64(const float* X, int n, int64_t ldx, const int32_t* ia, const int32_t* ib, int64_t P, int d, double divisor,
                         double* C, ssg_stream_t stream);

/* ---- float32 re-ranking variant "re_ranking_init" (reid/rerank.py:171-234 == reid/rerank_initial.py:40-99) */
/* out[i,j] = 2 - 2<x_i,y_j> (rerank.py:174-182); d % 32 == 0, n % 64 == 0; zeros = n floats of 0 */
int ssg_cosine_dist_f32(const float* x, const float* y, int m, int n, int d, const float* zeros, float* out, ssg_stream_t stream);
int ssg_affine_2m2x_f32(const float* in, float* out, int64_t n, ssg_stream_t stream); /* out = 2 - 2*in (rerank_initial.py:50) */
/* D [N,N] symmetric float32: row max, top-(k1+1) ranking, k-reciprocal encoding -> sparse V (rerank.py:183-204) */
int ssg_rerank_init_stage1(const float* D, int N, int k1, int k2, int capV, float* rowmax, int32_t* rank, int32_t* v_idx, float* v_val,
                           int32_t* v_nnz, ssg_stream_t stream);
/* query expansion V_qe (rerank.py:207-212); max_nnz = max(v_nnz), capQ >= k2*max_nnz */
int ssg_rerank_init_expand(const int32_t* v_idx, const float* v_val, const int32_t* v_nnz, const int32_t* rank, int N, int k1, int k2, int capV,
                           int capQ, int max_nnz, int32_t* q_idx, float* q_val, int32_t* q_nnz, ssg_stream_t stream);
/* inverted index + Jaccard + blend for the nq query rows -> out [nq, N-nq] (rerank.py:214-233) */
int ssg_rerank_init_jaccard(const float* D, const float* rowmax, const int32_t* q_idx, const float* q_val, const int32_t* q_nnz, int capQ, int N,
                            int nq, float lambda_value, int32_t* colcnt, int64_t* colptr, int32_t* inv_row, float* inv_val, float* out,
                            ssg_stream_t stream);

/* ---- input transform of the extraction loaders (selftraining.py:43-47 applied by reid/utils/data/preprocessor.py:22-30):
 * Resize((H,W)) [= PIL.Image.resize((W,H), BILINEAR) on 8-bit RGB] + ToTensor + Normalize for a batch of equally sized decoded
 * images.  src [B,h,w,3] uint8, tmp [B,h,W,3] uint8 scratch, out [B,3,H,W] float32.  (xmin, xcnt, xk[W,xksize]) and
 * (ymin, ycnt, yk[H,yksize]) are Pillow's per-output-pixel windows of 22-bit fixed-point triangle coefficients
 * (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc; ssg_amd/preprocessor.py computes them), device arrays;
 * mean3_host / std3_host are HOST pointers to 3 floats.  Bit-exact with Pillow 12.2. */
int ssg_preprocess_u8(const uint8_t* src, int B, int h, int w, int H, int W, const int32_t* xmin, const int32_t* xcnt, const int32_t* xk,
                      int xksize, const int32_t* ymin, const int32_t* ycnt, const int32_t* yk, int yksize, const float* mean3_host,
                      const float* std3_host, uint8_t* tmp, float* out, ssg_stream_t stream);
/* Decode half of reid/utils/data/preprocessor.py:22-30 (`Image.open(fpath).convert('RGB')` = Pillow -> libjpeg-turbo, default
 * parameters) for a batch of baseline / extended-sequential Huffman JPEG files, bit-exact: Huffman decode (one thread per restart
 * segment), dequantisation + islow integer inverse DCT, fancy chroma upsampling (h2v1 / h2v2), YCbCr -> RGB.  The host parses the
 * marker segments and builds the tables (ssg_amd/jpeg.py):
 *   ecs   entropy-coded bytes of all files back to back, >= 32 zero bytes of padding behind them
 *   segs  int64 [nseg][5] per restart segment: image, byte offset into ecs, byte length, first MCU, MCU count
 *   imgs  int64 [nimg][32] per image: W, H, components (1 | 3), luma sampling h, v, MCUs per row, MCU rows, byte offset into out, then
 *         8 words per component: first block in coef, blocks per row, block rows, byte offset into planes, plane pitch, quantisation
 *         table index, DC table index, AC table index
 *   look [ntab][256] uint16 ((length << 8) | symbol of every code of at most 8 bits, 0 otherwise), maxcode [ntab][18], valoff [ntab][17],
 *   vals [ntab][256]: jdhuff.c's derived tables; qts [nqt][64] uint16 in natural order
 *   coef  workspace int16 [total_blocks][64] (zeroed by the call), planes workspace uint8 (sum of 64 * blocks), max_blocks / max_pixels =
 *         largest component (in blocks) / image (in pixels) of the batch; out: RGB bytes, H * W * 3 per image at its offset.
 *   status int32 [nimg] (zeroed by the call; round 4): non-zero = damaged entropy-coded data (bit 0: a zero run past coefficient 63,
 *         bit 1: a segment ran out of data before its MCUs were decoded), or data on which builds of libjpeg differ (bit 2: a
 *         dequantised coefficient or a pass-1 IDCT output outside int16, or a pass-2 IDCT output outside [-512, 511] -- jidctint.c
 *         wraps there, libjpeg-turbo's SIMD IDCT works in 16 bits and saturates; no 8-bit encoder emits such values) -- the pixels of
 *         such a file are not libjpeg's, or not every libjpeg's; the caller hands it to the reference's decoder (Pillow), which
 *         warns / raises like the reference.  An unknown Huffman code is no flag by itself: it decodes to 0 after 17 bits like in
 *         jdhuff.c, and what follows decides. */
int ssg_jpeg_decode_batch(const uint8_t* ecs, const int64_t* segs, int nseg, const int64_t* imgs, int nimg, const uint16_t* look,
                          const int32_t* maxcode, const int32_t* valoff, const uint8_t* vals, const uint16_t* qts, int16_t* coef,
                          int64_t total_blocks, int max_blocks, uint8_t* planes, int max_pixels, uint8_t* out, int32_t* status,
                          ssg_stream_t stream);
/* Host side of the same path, native and threaded (csrc/jpeg_host.hip; no device work): the marker walk + table building that
 * ssg_amd/jpeg.py states in Python, for a batch of files in host memory -- what the reference's DataLoader workers do in libjpeg's
 * jdmarker.c before decoding.  ssg_jpeg_parse_open: pass over files[i] (lens[i] bytes each; must stay valid until _close) on
 * `nthreads` threads; counts10 = [images the GPU decodes, restart segments, bytes of entropy-coded data incl. 64 of padding, Huffman
 * tables, quantisation tables, coefficient blocks, largest component (blocks), plane bytes, output bytes, largest image (pixels)];
 * file_status[i] = 0 (decoded on the GPU, images are numbered in file order) or 1 (not baseline / malformed header: left to the
 * reference's decoder).  ssg_jpeg_parse_fill writes the arguments of ssg_jpeg_decode_batch into host buffers of those sizes. */
int ssg_jpeg_parse_open(const void* const* files, const int64_t* lens, int nfiles, int nthreads, void** handle, int64_t* counts10,
                        int32_t* file_status);
int ssg_jpeg_parse_fill(void* handle, int64_t* imgs, int64_t* segs, uint8_t* pool, uint16_t* look, int32_t* maxcode, int32_t* valoff,
                        uint8_t* vals, uint16_t* qts);
int ssg_jpeg_parse_close(void* handle);
/* ---- training transform of the fine-tune loader (ssg_amd/trainloader.py; the per-item transform of selftraining.py:177-183 and
 * reid/eug.py:64-71): for every image b of a batch of ANY mix of source sizes, in one launch,
 *   out[b] = Normalize(ToTensor(flip(PIL.Image.crop(box).resize((W, H), BILINEAR)))) with the erase rectangle set to float32(fill[c]),
 * bit-exact with Pillow 12.2 + the published float32 formulas.  desc: device int32 [B, SSG_TT_WORDS = 20], per image:
 *   0-1 source address (uint8 [h, w, 3] RGB, low / high word), 2 h, 3 w, 4-7 crop box x0, y0, cw, ch,
 *   8 x-window offset into coef, 9 its ksize, 10 y-window offset, 11 its ksize, 12 flip (0 / 1),
 *   13-16 erase rectangle: first row, first column, rows eh, columns ew (eh = 0: none), 17-19 unused.
 * coef: device int32, per axis block at its offset: first[n], count[n], k[n, ksize] (n = W for x, H for y, Pillow's windows of the crop
 * size -> n; first relative to the crop).  One workgroup per (image, band of band_rows output rows); lds_rows >= the crop rows any band's
 * vertical windows read (lds_rows * W * 3 <= 65536).  mean3 / std3 / fill3: HOST pointers to 3 floats.  out [B, 3, H, W] float32. */
int ssg_train_transform_u8(const int32_t* desc, int B, const int32_t* coef, int H, int W, int band_rows, int lds_rows, const float* mean3_host,
                           const float* std3_host, const float* fill3_host, float* out, ssg_stream_t stream);
/* x = sqrt(max(x, lo)) in place: with ssg_pairwise_sqdist_f32 the pairwise block of the fine-tune phase's TripletLoss
 * (reid/loss/triplet.py:28-31: dist = (|x|^2 + |x|^2' - 2 x x').clamp(min=1e-12).sqrt()) */
int ssg_clamp_sqrt_f32(float* x, int64_t n, float lo, ssg_stream_t stream);
/* Backward of that block (round 4: lets ssg_amd.triplet.pairwise_dist replace reid/loss/triplet.py:28-31 inside the training step):
 * grad_x = diag(rowsum(S)) x - S x,  S = W + W^T,  W[i,j] = sq[i,j] >= lo ? grad_dist[i,j] / dist[i,j] : 0 (sq = the distances squared
 * before the clamp).  _weights writes S with row pitch ld >= n (zero padded) and its row sums; S x is one fp32-MFMA GEMM
 * (ssg_conv2d_nhwc_f32 as a 1x1 convolution: in = S [n,1,1,ld], w = x^T [d_pad][ld]); _combine forms the gradient. */
int ssg_triplet_grad_weights(const float* grad_dist, const float* sq, const float* dist, int n, int ld, float lo, float* S, float* rowsum,
                             ssg_stream_t stream);
int ssg_triplet_grad_combine(const float* x, const float* rowsum, const float* Sx, int n, int d, int ldo, float* grad_x, ssg_stream_t stream);
/* The rest of that TripletLoss (reid/loss/triplet.py:32-77, csrc/triplet_loss.hip): mining, hinge, loss and prec with no host read.
 * in [n, ld]: is_sq = 1: the squared distances of ssg_pairwise_sqdist_f32 at its row pitch, dist = sqrtf(max(sq, lo)) on the fly
 * (bit-equal to ssg_clamp_sqrt_f32); is_sq = 0: a finished dist.  targets int64 [n] (labels); 1 <= n <= 4096; K = num_instances >= 1.
 * semi = 1 (use_semi): anchors a = i*K + j (i < n / K), pairs (a, i*K + p) for p > j by position, an = the anchor's hardest negative,
 * M = (n / K) * K * (K - 1) / 2; semi = 0: every row an anchor with its hardest positive (itself included) and negative, M = n.
 * weighted = 1: the `w is not None` branch, (1/M) sum_i mean_m hinge(an_i, ap_m) (M <= 65536).
 * rec_f: 2n + 4M floats, rec_i: 2n + 2M ints (layout in csrc/triplet_loss.hip; dist_ap = rec_f + 2n, dist_an = rec_f + 2n + M, in the
 * reference's append order); loss, prec: one float each.  An anchor without a negative (the reference raises) makes loss and prec NaN.
 * Up to 3 launches (mining, w-branch counts, one-workgroup fixed-order reduction). */
int ssg_triplet_mine_f32(const float* in, int ld, int is_sq, float lo, const int64_t* targets, int n, int K, int semi, int M, float margin,
                         int weighted, float* rec_f, int32_t* rec_i, float* loss, float* prec, ssg_stream_t stream);
/* Backward from that record, densely: gdist [n, n] = d objective / d dist.  gloss != NULL: the objective is the loss, gloss a device
 * pointer to its upstream gradient; else the objective is sum(gap * dist_ap) + sum(gan * dist_an) (gap / gan [M] device, may be NULL).
 * Ties of a min / max share evenly; hinge terms >= 0 pass the gradient.  The arguments are those of the forward call. */
int ssg_triplet_grad_dist_f32(const float* in, int ld, int is_sq, float lo, const int64_t* targets, int n, int K, int semi, int M,
                              int weighted, const float* rec_f, const int32_t* rec_i, const float* gloss, const float* gap, const float* gan,
                              float* gdist, ssg_stream_t stream);
/* Feature-gradient weights straight from the record (sq at pitch ldq, the forward's is_sq = 1 input): S [n, ldS] = W + W^T,
 * W[a,c] = sq[a,c] >= lo ? G[a,c] / dist[a,c] : 0 (diagonal 0), rowsum [n]; the same launch writes xt = x^T [dp, ldS] zero padded and
 * zeros [dp] for the S x GEMM (ssg_conv2d_nhwc_f32), after which ssg_triplet_grad_combine forms grad_x.  ldS % 32 == 0, dp % 64 == 0. */
int ssg_triplet_grad_weights_rec(const float* sq, int ldq, float lo, const int64_t* targets, int n, int K, int semi, int M, int weighted,
                                 const float* rec_f, const int32_t* rec_i, const float* gloss, const float* x, int d, int ldS, int dp,
                                 float* S, float* rowsum, float* xt, float* zeros, ssg_stream_t stream);

/* ---- SSG++ label estimation and selection (reid/eug.py:193-290; caller semitraining.py:228-244) ------------------------
 * ssg_eug_nn_f32: the rerank=False branch (eug.py:201-214).  For every u row: dist_j = np.linalg.norm(l - u, axis=1)[j] bit for bit
 * (float32 differences and squares, numpy's pairwise order in sequential chunks of 8192, correctly rounded sqrt) and its np.argmin
 * (first index on ties, first NaN wins).  u [nu,d], l [nl,d] float32 row-major, 0 < d <= 32768; nsplit = ssg_eug_nn_splits(nu, nl);
 * part_val / part_idx: workspace of nsplit * nu entries.  Outputs (each may be NULL): argmin [nu], minval [nu] = the min distance,
 * labels [nu] = l_label[argmin] (l_label int64 [nl], needed with labels), scores [nu] = (double)(-minval). */
int ssg_eug_nn_splits(int nu, int nl);
int ssg_eug_nn_f32(const float* u, int nu, const float* l, int nl, int d, const int64_t* l_label, int nsplit, float* part_val,
                   int32_t* part_idx, int32_t* argmin, float* minval, int64_t* labels, double* scores, ssg_stream_t stream);
/* The rerank=True branch (eug.py:228-244) on D [nu,nl] float32 (re_ranking_init's output): argmin per row (np.argmin), labels =
 * l_label[argmin], scores = (double)(-min), confidence = (double)(1 - min / colmax[argmin]) in float32 with colmax = np.max(D, axis=0)
 * (NaN propagates).  ws: 65 * nl floats.  argmin may be NULL. */
int ssg_eug_dist_label_f32(const float* D, int nu, int nl, const int64_t* l_label, float* ws, int32_t* argmin, int64_t* labels,
                           double* scores, double* confidence, ssg_stream_t stream);
/* select_top_data (eug.py:284-289): mask[i] = 1 for the k largest of scores [n] float64 (0 <= k <= n); np.argsort(-scores) order:
 * NaN last, -0 == +0; equal scores that straddle the cut are taken lowest index first.  labels (float64 [n] or NULL):
 * select_top_true_data (eug.py:277-282), a selected entry whose label is -1 is cleared. */
int ssg_eug_select_top(const double* scores, int n, int k, const double* labels, uint8_t* mask, ssg_stream_t stream);

/* ---- device self-tests used by the parity suite ----------------------------------------- */
int ssg_selftest_half_table(int which, uint16_t* out65536, ssg_stream_t stream);
int ssg_selftest_half_binop(int which, const uint16_t* a, const uint16_t* b, int n, uint16_t* out, ssg_stream_t stream);
int ssg_selftest_d2h(const double* a, int n, uint16_t* out, ssg_stream_t stream);

/* ---- collectives of the sharded path: RCCL over xGMI, one rank per process / GPU ------------------------
 * The reference spreads the extraction over GPUs with nn.DataParallel (selftraining.py:135) and has no multi-GPU N x N path.
 * Every exchange of the sharded pipeline is an all-gather of equally sized blocks (embeddings, rank lists, sparse V / V_qe,
 * source vector) or an int64 sum all-reduce (eps histogram).  The Python product issues them through torch.distributed
 * (backend "nccl" = RCCL on ROCm); a host language without torch binds these four calls instead.
 * ssg_comm_unique_id: 128 host bytes created by rank 0, passed by EVERY rank to ssg_comm_init (a collective; the communicator
 * binds to the caller's current HIP device).  ssg_allgather: recv[r * bytes_per_rank ...] = rank r's block. */
/* RCCL is bound at the first collective call, to the build that is already mapped into the process if there is one (torch's
 * torch/lib/librccl.so next to torch.distributed), else $SSG_RCCL_PATH / librccl.so.1: never two RCCL builds in one process.
 * ssg_comm_library() = path of the bound library ("" if none). */
const char* ssg_comm_library(void);
int ssg_comm_unique_id(void* id128_host);
int ssg_comm_init(void** comm, int world, int rank, const void* id128_host);
int ssg_allgather(void* comm, const void* send, void* recv, size_t bytes_per_rank, ssg_stream_t stream);
int ssg_allreduce_sum_i64(void* comm, int64_t* buf, size_t count, ssg_stream_t stream);
int ssg_comm_destroy(void* comm);

/* DEC cluster head of the fine-tune phase (--dce-loss; reid/models/dce.py:39-51, reid/trainers.py:268-292; csrc/dec.hip).  float32 in
 * and out, every D-long sum, column sum, row sum and the loss accumulated in float64 in a fixed order (no float atomics: the same
 * call gives the same bits), no host read.  1 <= B <= 4096 rows, 1 <= K <= 64 centres, any D >= 1.
 * Soft assignment: x [B, D] at row pitch ldx >= D (elements), c [K, D] -> q [B, K]:
 *   ns[i,j] = sum_d (x[i,d] - c[j,d])^2,  n = (1 / (1 + ns/alpha)) ^ -(alpha+1)/2,  q[i,j] = n[i,j] / sum_j n[i,j]
 * (alpha = 1: q ~ 1 + ns, the FARTHEST centre gets the largest weight -- what the reference trains with).  ns [B, K]: optional output
 * (NULL: not written), the input of ssg_dec_assign_grad_f32. */
int ssg_dec_assign_f32(const float* x, int64_t ldx, const float* c, int B, int K, int D, double alpha, float* q, float* ns,
                       ssg_stream_t stream);
/* Target distribution and loss: f[j] = sum_i q[i,j], w = q^2 / f, p[i,j] = w[i,j] / sum_j w[i,j] (p [B, K] optional output),
 * loss[0] = sum_ij p (log p - log q) / B  (nn.KLDivLoss(size_average=False)(q.log(), p) / B; p == 0 contributes 0).  One launch. */
int ssg_dec_kl_loss_f32(const float* q, int B, int K, float* p, float* loss, ssg_stream_t stream);
/* gq [B, K] = gloss[0] * d loss / d q with p NOT detached (the reference's graph): through log q and through p.  gloss: device
 * pointer to the upstream gradient of the loss.  One launch. */
int ssg_dec_kl_loss_grad_f32(const float* q, int B, int K, const float* gloss, float* gq, ssg_stream_t stream);
/* Backward of the assignment: gq [B, K] = d objective / d q, ns the forward's output -> gx [B, D] (dense), gc [K, D]:
 *   g = d objective / d ns (float64, written to the workspace gns [B, K] doubles),
 *   gx = 2 (rowsum(g) x - g c),  gc = 2 (colsum(g) c - g^T x)  -- no [B, K, D] temporary.  3 launches. */
int ssg_dec_assign_grad_f32(const float* x, int64_t ldx, const float* c, const float* ns, const float* gq, int B, int K, int D, double alpha,
                            double* gns, float* gx, float* gc, ssg_stream_t stream);

/* ---- train-mode batch normalisation with fused ReLU and residual add (fine-tune phase; csrc/batchnorm.hip) ----------------------
 * float32 tensors of N x C x HW values, every channel sum and the per-element arithmetic in float64, no float atomics (the same call
 * gives the same bits), no host read.  channels_last = 0: NCHW contiguous (C <= 65535 when HW > 1); 1: the channel is contiguous
 * ([N, HW, C]: torch's channels_last; BatchNorm1d's [B, C] is HW = 1 in either).  N * HW >= 2 values per channel, fewer than 2^31
 * elements.  Bad arguments are refused (-1) before any launch.
 * ssg_bn_num_partials(): workgroups (partial sums) per channel of the two reductions, a function of the shape alone (-1: bad shape);
 * ws: ssg_bn_workspace_bytes() bytes, 8-byte aligned, for those partials (0: bad shape). */
int ssg_bn_num_partials(int N, int C, int HW, int channels_last);
size_t ssg_bn_workspace_bytes(int N, int C, int HW, int channels_last);
/* Forward statistics.  stat [3, C] float64 = {mean, biased variance, invstd = 1 / sqrt(var + eps)}.  running_mean / running_var [C]
 * (NULL: left out) are updated in place: r = (1 - f) r + f v with v = mean, var * n / (n - 1); f = momentum, or 1 / num_batches_tracked[0]
 * (device int64 that already counts this batch) when momentum < 0.  2 launches. */
int ssg_bn_stats_f32(const float* x, int N, int C, int HW, int channels_last, double eps, double momentum, const int64_t* num_batches_tracked,
                     float* running_mean, float* running_var, double* stat, void* ws, size_t ws_bytes, ssg_stream_t stream);
/* y = (x - mean) * invstd * weight + bias  [+ residual, NULL: none]  [max(., 0) when relu != 0], rounded to float32 once.  1 launch. */
int ssg_bn_apply_f32(const float* x, const double* stat, const float* weight, const float* bias, const float* residual, int relu, int N, int C,
                     int HW, int channels_last, float* y, ssg_stream_t stream);
/* Backward sums.  g = dy, or with y != NULL (the saved output of a forward with relu) g = dy where y > 0 and 0 elsewhere.
 * dbias [C] = sum g, dweight [C] = sum g xh with xh = (x - mean) * invstd (either may be NULL); coef [2, C] float64 = {sum g / n,
 * sum g xh / n}, the input of ssg_bn_backward_apply_f32.  2 launches. */
int ssg_bn_backward_reduce_f32(const float* dy, const float* x, const float* y, const double* stat, int N, int C, int HW, int channels_last,
                               double* coef, float* dweight, float* dbias, void* ws, size_t ws_bytes, ssg_stream_t stream);
/* dx = (g - coef[0] - xh coef[1]) * invstd * weight; dresidual (NULL: none) = g.  1 launch. */
int ssg_bn_backward_apply_f32(const float* dy, const float* x, const float* y, const double* stat, const float* weight, const double* coef, int N,
                              int C, int HW, int channels_last, float* dx, float* dresidual, ssg_stream_t stream);

/* ---- verification metrics (reid/evaluation_metrics/eval_far_gar.py:61-202; csrc/verify.hip) ------------------------------
 * D [m, n] float32 SQUARED distances at row pitch ld >= n (elements; m * ld * 4 may exceed 2^32), qlab int32 [m], rlab int32 [n], all on
 * the device and only read.  Element (i, j) is intra when rlab[j] == qlab[i], else inter (no camera filter); every element is taken as
 * s = sqrtf(d <= 0 ? 0 : d), correctly rounded.  ws: ssg_verify_workspace_bytes(m, n) bytes (8-byte aligned), shared by the three
 * passes, which must not run concurrently on it.  Each pass streams the block once per launch noted below and writes nothing into it.
 * No float atomics: the same call gives the same bits.  Bad arguments are refused (-1) before any launch. */
size_t ssg_verify_workspace_bytes(int m, int n);
/* Pass A.  counts[2] = {intra, inter} int64; sums[4] = {sum s, sum s^2 of intra, sum s, sum s^2 of inter} float64 (s widened before
 * squaring; per-workgroup partials added in index order); minmax[4] = {intra min, intra max, inter min, inter max} float32;
 * status[0] = 1 when some query row has no intra or no inter element, status[1] = 1 when a NaN was seen.  2 launches. */
int ssg_verify_stats_f32(const float* D, int m, int n, size_t ld, const int32_t* qlab, const int32_t* rlab, void* ws, size_t ws_bytes,
                         int64_t* counts, double* sums, float* minmax, int32_t* status, ssg_stream_t stream);
/* Pass B.  ranks_host: nr (1 .. 64) zero-based ranks, a HOST array, each >= 0.  values[r] = np.sort(inter s)[ranks[r]] exactly (a
 * four-level radix select on the bit patterns, all ranks in the same 4 passes; a rank inside a run of equal values returns that value).
 * status[0] = 1 when a rank is >= the number of inter elements (every value is then NaN).  8 launches. */
int ssg_verify_select_f32(const float* D, int m, int n, size_t ld, const int32_t* qlab, const int32_t* rlab, const int64_t* ranks_host, int nr,
                          void* ws, size_t ws_bytes, float* values, int32_t* status, ssg_stream_t stream);
/* Pass C.  thr_host: nt (1 .. 64) float64 thresholds, a HOST array in any order, none NaN.  counts [3, nt] int64: row 0 = intra with
 * s >= t, row 1 = inter with s < t, row 2 = intra with s < t, compared in double.  totals[2] = {intra, inter} element counts.
 * is_sq = 1: s as above; is_sq = 0: the block is compared as stored, no clamp and no sqrt (CalClassificationError_MPI with dist=).
 * NaN elements count in totals only.  2 launches. */
int ssg_verify_count_f32(const float* D, int m, int n, size_t ld, const int32_t* qlab, const int32_t* rlab, int is_sq, const double* thr_host,
                         int nt, void* ws, size_t ws_bytes, int64_t* counts, int64_t* totals, ssg_stream_t stream);
/* s[i] = the value the three passes take for a stored d[i] (parity suite: equals numpy's float32 sqrt bit for bit). */
int ssg_selftest_verify_sqrt(const float* d, int n, float* s, ssg_stream_t stream);

/* ---- train-mode Conv2d (fine-tune phase; csrc/conv_train.hip) ----------------------------------------------------------------------
 * Class: groups 1, dilation 1, no bias, stride 1, 1x1 with pad 0 or 3x3 with pad 1, Cin % 64 == 0, Cout % 64 == 0; float32 NHWC.
 * Forward and data gradient are ssg_conv2d_nhwc_f32 (zero bias, no residual, no ReLU) on the two packings written here:
 *   y [B,H,W,Cout] = conv(x, w_fwd),  dX [B,H,W,Cin] = conv(dY, w_dgrad) with Cin and Cout exchanged, same pad.
 * ssg_conv_pack_train_f32: w is the [Cout,Cin,KH,KW] weight at element strides (s_co, s_ci, s_r, s_s), so a channels_last weight needs
 * no copy.  w_fwd [Cout][KH*KW*Cin], k = ((ci/32)*KH*KW + r*KW + s)*32 + ci%32;  w_dgrad [Cin][KH*KW*Cout],
 * k = ((co/32)*KH*KW + (KH-1-r)*KW + (KW-1-s))*32 + co%32.  Either output may be NULL (not both).  1 launch. */
int ssg_conv_pack_train_f32(const float* w, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, int Cout, int Cin, int KH, int KW,
                            float* w_fwd, float* w_dgrad, ssg_stream_t stream);
/* Weight gradient dW[co][ci][r][s] = sum over the M = B*H*W pixels of dY[m][co] * x[m shifted by the tap][ci] (zeros outside the image).
 * The pixels are cut into ssg_conv_wgrad_num_slices() contiguous slices, a function of the shape alone (-1: bad shape); stage 1 writes
 * one fp32 partial [Cout][KH*KW*Cin] per slice to ws (ssg_conv_wgrad_workspace_bytes() bytes; 0: bad shape), stage 2 adds the slices of
 * every element in float64 in ascending order, rounds once and stores dw at element strides (s_co, s_ci, s_r, s_s).  No float atomics:
 * the same call gives the same bits.  dy [B,H,W,Cout], x [B,H,W,Cin], 16-byte aligned.  stages: 3 = both (2 launches); 1 / 2 = stage 1 /
 * stage 2 alone (timing).  Bad arguments are refused (-1) before any launch. */
int ssg_conv_wgrad_num_slices(int M, int Cout, int KH, int KW, int Cin);
size_t ssg_conv_wgrad_workspace_bytes(int M, int Cout, int KH, int KW, int Cin);
int ssg_conv_wgrad_f32(const float* dy, const float* x, int B, int H, int W, int Cin, int Cout, int KH, int KW, float* dw, int64_t s_co,
                       int64_t s_ci, int64_t s_r, int64_t s_s, void* ws, size_t ws_bytes, int stages, ssg_stream_t stream);

/* ---- train-mode strided Conv2d, the 7x7 stem and MaxPool2d(3, 2, 1) (fine-tune phase; csrc/conv_strided.hip) ------------------------
 * Classes, all stride 2, groups 1, dilation 1, no bias, float32 NHWC:
 *   S     1x1 with pad 0 or 3x3 with pad 1, Cin % 64 == 0, Cout % 64 == 0
 *   stem  7x7 with pad 3, Cin = 3, Cout = 64; x is [B,H,W,4] RGB0 pixels (ssg_nchw_to_nhwc4), no data gradient
 * OH = (H + 2 pad - KH) / 2 + 1, OW likewise.  Forward: y [B,OH,OW,Cout] = ssg_conv2d_nhwc_f32(x, w_fwd, stride 2, zero bias, no
 * residual, no ReLU), with Cin = 4 for the stem.  No float atomics anywhere: the same call gives the same bits.
 * ssg_conv_pack_strided_f32: w is the [Cout,Cin,KH,KW] weight at element strides.  Class S: w_fwd [Cout][KH*KW*Cin] as
 * ssg_conv_pack_train_f32 writes it, w_dgrad [KH*KW][Cout][Cin]; either may be NULL (not both); one launch each.  Stem: w_fwd [64][224],
 * k = (r*7 + s)*4 + c, zero where c == 3 or k >= 196; w_dgrad must be NULL. */
int ssg_conv_pack_strided_f32(const float* w, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, int Cout, int Cin, int KH, int KW,
                              float* w_fwd, float* w_dgrad, ssg_stream_t stream);
/* Data gradient of class S: dX [B,H,W,Cin] from dY [B,OH,OW,Cout] and the w_dgrad above.  The input pixels are split into their four
 * (h mod 2, w mod 2) classes; each is a dense fp32-MFMA GEMM over K = (its 0, 1, 2 or 4 taps) x Cout, so no zero of a zero-stuffed dY
 * is multiplied.  Every element of dX is written exactly once, the zeros that no tap reaches included.  All pointers 16-byte aligned.
 * The stem is refused (-1).  1 launch. */
int ssg_conv_dgrad_strided_f32(const float* dy, const float* w_dgrad, float* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                               int stride, ssg_stream_t stream);
/* Weight gradient of class S and of the stem: ssg_conv_wgrad_f32's two stages with the x row of output pixel (b, oh, ow) and tap (r, s)
 * at (oh*stride + r - pad, ow*stride + s - pad), zero outside the image.  M = B*OH*OW output pixels are cut into
 * ssg_conv_wgrad_strided_num_slices() slices (-1: bad shape); ws holds one fp32 partial per slice
 * (ssg_conv_wgrad_strided_workspace_bytes(); 0: bad shape; the stem's partial rows are 13 K tiles of 16 taps x RGB0 = 832 floats).
 * dw [Cout,Cin,KH,KW] at element strides; the stem's padding channel is never stored.  dy [B,OH,OW,Cout], x [B,H,W,Cin] (stem:
 * [B,H,W,4]), 16-byte aligned.  stages as in ssg_conv_wgrad_f32. */
int ssg_conv_wgrad_strided_num_slices(int M, int Cout, int KH, int KW, int Cin, int stride);
size_t ssg_conv_wgrad_strided_workspace_bytes(int M, int Cout, int KH, int KW, int Cin, int stride);
int ssg_conv_wgrad_strided_f32(const float* dy, const float* x, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, float* dw,
                               int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, void* ws, size_t ws_bytes, int stages, ssg_stream_t stream);
/* MaxPool2d(3, stride 2, padding 1) on NHWC for training, C % 4 == 0, B*H*W < 2^31.  _idx: out [B,OH,OW,C] and idx [B,OH,OW,C] bytes,
 * the winner's tap r*3 + s by torch's CPU rule: the maximum starts at -inf on the window's first element inside the image and an
 * element replaces it when `val > max || isnan(val)`, in row-major window order (first maximum; a NaN wins).  _bwd: dX [B,H,W,C] as a
 * gather -- every input element adds, oh ascending then ow ascending, the dY of the at most 2 x 2 windows that hold it and whose
 * winner it is, and is written exactly once.  in / out / dy / dx 16-byte, idx 4-byte aligned.  1 launch each. */
int ssg_maxpool3x3s2_idx_nhwc(const float* in, float* out, uint8_t* idx, int B, int H, int W, int C, ssg_stream_t stream);
int ssg_maxpool3x3s2_bwd_nhwc(const float* dy, const uint8_t* idx, float* dx, int B, int H, int W, int C, ssg_stream_t stream);

/* ---- train-mode head: stripe pooling and Linear (fine-tune phase; reid/models/resnet.py:93-120; csrc/head_train.hip) -----------------
 * Pool forward: ssg_gap_stripes above on the NHWC map -- one launch, out [nsets,B,C] with nsets = S + 1 when S = num_split > 1, else 1;
 * set 0 the global average, set s = 1..S the average of rows [(s-1)*(H/S), s*(H/S)); with H % S != 0 the trailing rows are in no stripe.
 * Pool backward: dX[b,y,x,c] = g[0][b][c] / (H W) + g[stripe(y)][b][c] / ((H/S) W), each term a float32 division, added in that order;
 * g [nsets,B,C]; bit s of set_mask says that set s received a gradient -- an absent set counts as zero and its part of g is not read
 * (g may be NULL when set_mask == 0).  Every element of dX [B,H,W,C] is written exactly once; rows in no stripe get the global term
 * alone.  C % 4 == 0, 1 <= num_split <= min(H, 30), g and dx 16-byte aligned.  1 launch.  Bad arguments are refused (-1) before any
 * launch. */
int ssg_gap_stripes_bwd(const float* g, int set_mask, float* dx, int B, int H, int W, int C, int num_split, ssg_stream_t stream);
/* Linear: x [B,K], w [N,K] contiguous (nn.Linear's own weight, read where it lies: no pack launch, no transposed copy), bias [N] or
 * NULL; B >= 1, N >= 1, K % 32 == 0, B and N at most 65535 * 32; the ragged last tile in B and in N is masked, nothing is padded in
 * memory.  Three fp32-MFMA GEMMs (v_mfma_f32_32x32x2_f32, one 32 x 32 output tile per workgroup):
 *   ssg_linear_fwd_f32    y  [B,N] = x w^T (+ bias)                       reduction over K
 *   ssg_linear_dgrad_f32  dx [B,K] = dy w                                 reduction over N
 *   ssg_linear_wgrad_f32  dw [N,K] = dy^T x  and  db [N] = sum_b dy[b][n] reduction over B; dw or db may be NULL (not both; x may be
 *                         NULL with dw).  db is summed in float64 in ascending b and rounded once (a second launch).
 * No reduction is cut across workgroups, so there is no workspace: inside a workgroup wave w of 4 takes the reduction steps
 * [128 t + 32 w, 128 t + 32 w + 32) of every stage t, and the four fp32 partial tiles are added per element in float64 in wave order
 * (then the bias), rounded once.  The order is a function of the shape alone and there are no float atomics: the same call gives the
 * same bits.  Bad arguments are refused (-1) before any launch. */
int ssg_linear_fwd_f32(const float* x, const float* w, const float* bias, float* y, int B, int K, int N, ssg_stream_t stream);
int ssg_linear_dgrad_f32(const float* dy, const float* w, float* dx, int B, int K, int N, ssg_stream_t stream);
int ssg_linear_wgrad_f32(const float* dy, const float* x, float* dw, float* db, int B, int K, int N, ssg_stream_t stream);

/* ---- optimiser step of the fine-tune phase: torch.optim.SGD over many tensors (selftraining.py:152-161; csrc/sgd.hip) ---------------
 * One call updates `count` float32 tensors, each flat: tensor i has numel[i] elements at params[i], grads[i] and bufs[i] (its momentum
 * buffer; may be NULL when its group's momentum is 0), belongs to group group[i] of num_groups, and first[i] != 0 says that its buffer
 * holds nothing yet (it is written, not read).  Group k has lr[k], momentum[k], dampening[k], weight_decay[k] (doubles, each rounded to
 * float32 once; 1 - dampening is formed in double first) and nesterov[k], maximize[k] (ints).  Per element, in float32, torch's
 * _single_tensor_sgd with every add(., alpha=.) one fused multiply-add, as torch's CPU kernels round:
 *   g = maximize ? -g : g;   g = weight_decay != 0 ? fma(weight_decay, p, g) : g
 *   momentum != 0:   buf = first ? g : fma(1 - dampening, g, momentum * buf);   g = nesterov ? fma(momentum, buf, g) : buf
 *   p = fma(-lr, g, p)
 * The gradients are not written.  Tensors need 4-byte alignment only; where p, g and buf of a tensor are all 16-byte aligned the
 * kernel moves float4s, and the bits are the same either way.  The descriptors travel by value in the kernel arguments: a launch
 * serves up to ssg_sgd_max_tensors_per_launch() descriptors of one group and ssg_sgd_max_chunks_per_launch() chunks (workgroups) of
 * ssg_sgd_chunk_elems() elements (a power of two); a tensor that does not fit the chunks left in a launch continues in the next.
 * Nothing is copied to the device, nothing is kept between calls, there is no workspace, no host read and no synchronisation.
 * count == 0 returns 0 without a launch.  Refused (-1) before any launch: a NULL array with count > 0, num_groups < 1, a NULL
 * parameter or gradient, a NULL buffer in a group with momentum, numel <= 0, a group index out of range, nesterov with momentum 0 or
 * dampening != 0, and a negative or non-finite lr, momentum or weight_decay. */
int ssg_sgd_step_f32(float* const* params, const float* const* grads, float* const* bufs, const int64_t* numel, const int* group, const int* first,
                     int count, const double* lr, const double* momentum, const double* dampening, const double* weight_decay,
                     const int* nesterov, const int* maximize, int num_groups, ssg_stream_t stream);
int ssg_sgd_max_tensors_per_launch(void);
int ssg_sgd_chunk_elems(void);
int ssg_sgd_max_chunks_per_launch(void);

/* ---- classification losses of the fine-tune phase: softmax cross-entropy with a per-row factor, accuracy, the OIM table
 * (reid/loss/triplet.py:79-106 FocalLoss, reid/loss/weight_cross_entropy.py, reid/loss/oim.py, nn.CrossEntropyLoss of reid/eug.py:132,
 * reid/evaluation_metrics/classification.py; csrc/softmax_ce.hip) -----------------------------------------------------------------------
 * x [B,C] float32 logits with a row stride ldx >= C in elements; base and rows need 4-byte alignment only -- a row that is 16-byte
 * aligned moves as float4s, and the bits are the same either way.  target [B] int64.  B >= 1 and C >= 1, B up to the grid limit.
 * Forward, per row i with t = target[i], everything in float64:
 *   lse_i   = max_j x[i][j] + log(sum_j exp(x[i][j] - max))      a thread adds the quads q = tid, tid + 256, ... of the row in ascending
 *                                                                column order; the 256 partial sums by a fixed tree
 *   logpt_i = x[i][t] - lse_i
 *   s_i     = row_w[i] * class_w[t] * (1 - exp(logpt_i))^gamma   an absent weight (NULL) counts as 1; gamma == 0 gives the factor 1
 *   loss_i  = -s_i * logpt_i                                     row_loss [B] float32 (may be NULL)
 * A row is staged in LDS up to ssg_softmax_ce_row_capacity() floats; a longer row is read from memory a second time instead (the same
 * order, the same bits).  lse [B] and s [B] float64 are kept for the backward.  reduction: 0 none (loss is not written, r = 1),
 * 1 sum (r = 1), 2 mean over B (r = 1 / B), 3 weighted mean (r = 1 / W, W = sum of row_w[i] * class_w[t] over the rows that are not
 * ignored: torch's rule for `weight=` with reduction='mean').  The batch loss is the float64 sum of the row losses in ascending row order,
 * divided and rounded once to the float32 *loss, by a second launch of one workgroup that also writes *r (float64, kept on the device
 * for the backward).  A row with t == ignore_index has s = 0 and loss 0 and is in no denominator; all rows ignored gives NaN under 3.
 * A target outside [0, C) that is not ignore_index never indexes memory: s_i = NaN, so loss_i, the batch loss and that row of dx are
 * NaN, and it counts in W with class weight 1, so that every other row keeps its finite gradient.
 * Backward: dx[i][j] = (g[i * g_stride] * r * s_i) * (exp(x[i][j] - lse_i) - [j == t]) in float64, rounded once; g is read on the
 * device with g_stride 0 (a scalar upstream gradient) or 1 (one per row, reduction none).  Every element of dx [B,C] (row stride
 * lddx >= C) is written exactly once; an ignored row gets zeros.  The factor s is a constant of the backward (the reference detaches pt).
 * 1 launch, B * ceil(C / 1024) workgroups (at most 2^31 - 1).
 * No float atomics, no workspace, no host read.  Refused (-1) before any launch: B < 1, C < 1, a row stride below C, a reduction code
 * outside 0..3, a negative or non-finite gamma, g_stride outside {0, 1}, a NULL pointer other than row_w, class_w, row_loss (and loss
 * under reduction 0). */
int ssg_softmax_ce_row_capacity(void);
int ssg_softmax_ce_fwd_f32(const float* x, int64_t ldx, const int64_t* target, int64_t ignore_index, const float* row_w, const float* class_w,
                           double gamma, int reduction, int B, int C, double* lse, double* s, double* r, float* row_loss, float* loss,
                           ssg_stream_t stream);
int ssg_softmax_ce_bwd_f32(const float* x, int64_t ldx, const int64_t* target, int64_t ignore_index, const double* lse, const double* s,
                           const double* r, const float* g, int g_stride, float* dx, int64_t lddx, int B, int C, ssg_stream_t stream);
/* accuracy: rank[i] = #{j : x[i][j] > x[i][t] or (x[i][j] == x[i][t] and j < t)} -- a tie goes to the lower index; C for a target outside
 * [0, C), which is never correct and never an index -- then out[a] = float(#{i : rank[i] < ks[a]}) * (float)(1.0 / B), the float32
 * product of torch's correct_k.mul_(1. / batch_size).  ks is a host array of num_k values >= 1, 1 <= num_k <= ssg_topk_correct_max_k();
 * rank [B] int32 and out [num_k] float32 on the device.  Integer counts: 2 launches, no atomics on floats, no host read. */
int ssg_topk_correct_max_k(void);
int ssg_topk_correct_f32(const float* x, int64_t ldx, const int64_t* target, int B, int C, const int* ks, int num_k, int* rank, float* out,
                         ssg_stream_t stream);
/* OIM table update (oim.py:24-26): for the rows b of the batch in order, y = target[b]: v = momentum * lut[y] + (1 - momentum) * x[b],
 * lut[y] = v / |v|.  Each step reads the float32 table row, forms v, the norm (a fixed order) and the quotient in float64 and rounds
 * once to float32; a zero norm gives NaN as in the reference.  Rows with the same target are applied in batch order by the workgroup of
 * the first of them; a target outside [0, C) updates nothing.  x [B,F] with row stride ldx >= F, lut [C,F] with row stride ldl >= F.
 * 1 launch, no workspace.  Refused (-1) before any launch: B, C or F < 1, a row stride below F, a negative or non-finite momentum, a
 * NULL pointer. */
int ssg_oim_update_f32(const float* x, int64_t ldx, const int64_t* target, float* lut, int64_t ldl, int B, int C, int F, double momentum,
                       ssg_stream_t stream);

/* ---- embedder refresh: Conv2d + eval-mode BatchNorm folded, packed and split on the device (ssg_amd/resnet.py refresh; csrc/fold.hip) --
 * One launch writes, for one convolution, exactly the bits the host fold (`_fold` of ssg_amd/resnet.py) produces:
 *   float64, no contraction, correctly rounded sqrt and division: scale = gamma / sqrt(var + eps), w' = float32(w * scale),
 *   bias [Cout] = float32(beta - mean * scale).
 * w is the [Cout,Cin,KH,KW] weight at element strides (s_co, s_ci, s_r, s_s): contiguous or channels_last, no copy; a Linear weight
 * [N,K] is Cout = N, Cin = K, KH = KW = 1, strides (K, 1, 1, 1).  gamma / beta / mean / var are the BatchNorm's float32 weight, bias,
 * running_mean and running_var [Cout].  w_out [Cout][Kp] float32 containers, 16-byte aligned:
 *   Cin % 32 == 0: Kp = KH*KW*Cin, k = ((c/32)*KH*KW + r*KW + s)*32 + c%32;
 *   Cin == 3 (stem): Kp = 32 * ceil(KH*KW / 8), k = (r*KW + s)*4 + c, zero where c == 3 or k >= 4*KH*KW.
 * split == 0: w_out holds the packed float32 row; ch_scale is not touched (may be NULL).
 * split != 0: row scale 2^e, e = clamp(floor(log2(16384 / max|w'_row|)), -40, 40), e = 0 for an all-zero row (taken from the bits of
 *   the maximum, no log2); v = w' * 2^e, hi = half(v), lo = half(v - float(hi)), stored h8l8 (per 8 values [8 hi][8 lo]; the stem h4l4,
 *   per 4 values [4 hi][4 lo]); ch_scale [Cout] = 2^-e.
 * _dual: two 1x1 sources with their own BatchNorm over the same Cout (the [conv3 | downsample] GEMM of a downsample block): each is
 *   folded and packed on its own, Kp = Cin1 + Cin2 with the first source first, one row scale over the whole row,
 *   bias = float32(b1) + float32(b2) added in float32.
 * One workgroup per output row, no atomics, no workspace, no host read.  Refused (-1) before any launch, outputs untouched: Cout % 64
 * != 0 other than 32 (the InceptionNet stem layers), Cin % 32 != 0 other than the stem's 3 (never in _dual), a packed row longer than ssg_fold_max_k() floats, a _dual source that is
 * not 1x1, a NULL pointer, a negative stride, w_out not 16-byte aligned.  Non-finite parameters are not refused: they propagate by
 * IEEE rules into w' and bias, and a row whose maximum is Inf or NaN gets e = -40. */
int ssg_fold_max_k(void);
int ssg_fold_conv_bn_f32(const float* w, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s, int Cout, int Cin, int KH, int KW, const float* gamma,
                         const float* beta, const float* mean, const float* var, double eps, int split, float* w_out, float* bias, float* ch_scale,
                         ssg_stream_t stream);
int ssg_fold_conv_bn_dual_f32(const float* w1, int64_t s1_co, int64_t s1_ci, int64_t s1_r, int64_t s1_s, int Cin1, int KH1, int KW1, const float* gamma1,
                              const float* beta1, const float* mean1, const float* var1, const float* w2, int64_t s2_co, int64_t s2_ci, int64_t s2_r,
                              int64_t s2_s, int Cin2, int KH2, int KW2, const float* gamma2, const float* beta2, const float* mean2, const float* var2,
                              double eps, int Cout, int split, float* w_out, float* bias, float* ch_scale, ssg_stream_t stream);

/* ---- affinity propagation on a precomputed similarity matrix (ssg_amd.cluster.AffinityPropagation; csrc/affinity.hip) ----------------
 * sklearn 1.7.2's _affinity_propagation in float64 with numpy's bits: every damped update rounds twice (no contraction), the column
 * sums add the rows in ascending order with one running sum per column, argmax takes the first maximum.  S, A, R, noise are row-major
 * [N,N] float64 (indexed with size_t); N >= 1.  No float atomics, and no host read in any of these calls.
 * ssg_ap_median_f64: out[0] = np.median of the n values of X: the middle order statistic, or (a + b) / 2 of the two middle ones when
 *   n is even -- an exact radix select over order-preserving 64-bit keys (13-bit digits, 10 launches); ws of
 *   ssg_ap_median_workspace_bytes() bytes, 8-byte aligned.  X must hold no NaN.
 * ssg_ap_stats_f64: the device form of the input check and of _equal_similarities_and_preferences, on the matrix as the caller gave it.
 *   pref [pref_n] float64 on the device, pref_n = 1 or N.  stats [8] int64: [0] non-finite entries of S (diagonal included),
 *   [1] / [2] minimum / maximum of the finite off-diagonal entries as order-preserving keys (key = ~bits for a negative value, else
 *   bits | 2^63; ~0 / 0 when there is none), [3] / [4] the same of pref, [5] non-finite entries of pref, [6] the bits of S[0][N-1],
 *   [7] the bits of pref[0].
 * ssg_ap_prepare_f64: S.flat[::N+1] = pref, then S += (eps64 * S + tiny64 * 100) * noise with the three roundings in that order.
 * One iteration `it` (0-based) is: ssg_ap_row_f64(it, do_r = 1), ssg_ap_colsum_f64, the convergence check -- ssg_ap_iterate_f64 queues
 * `count` of them from it0 on.  A, R [N,N], cs [N] float64, window [N][convergence_iter] and E [N] uint8 and ctrl [8] int64 start as
 * zeros.  ctrl[0] = 1 once sklearn's stopping rule fired, ctrl[1] = its n_iter (it + 1), ctrl[2] = K of the last check.
 *   row: the A update of iteration it - 1 (A = A*d - (1-d)*T, T = clip(max(R,0) - cs, 0, inf) off the diagonal, R - cs on it; skipped
 *     for it = 0) and then, when do_r, the R update of iteration it (R = R*d + (1-d)*(S - Y), Y2 at the first argmax of A + S).  One
 *     workgroup per row, 16-byte accesses when N is even.
 *   colsum: cs[k] = sum over i ascending of max(R[i][k], 0), the diagonal taken from R itself.
 *   check: E[k] = (A'[k][k] + R[k][k] > 0) with A' the value the next row call stores, the window column it % convergence_iter, the rule.
 *   Once ctrl[0] is set, the row call with it == ctrl[1] applies that A update and nothing else; every other call leaves A, R, cs,
 *   window and E untouched.  After the last iteration `last` the caller queues ssg_ap_row_f64(it = last + 1, do_r = 0) in every case.
 * ssg_ap_finish_f64: I [N] int32 = flatnonzero(E) (K = ctrl[2] entries, the rest untouched), c = argmax_k S[:, I] with c[I] = arange(K),
 *   sums[j] = the sum of S[i][j] over the members i of j's cluster in ascending i, I[k] = the member with the largest sum (lowest index on
 *   ties), c again.  labels = I[c] is left to the host.  K = 0 writes nothing but ctrl[2]. */
size_t ssg_ap_median_workspace_bytes(void);
int ssg_ap_median_f64(const double* X, int64_t n, void* ws, size_t ws_bytes, double* out, ssg_stream_t stream);
int ssg_ap_stats_f64(const double* S, int N, const double* pref, int pref_n, int64_t* stats, ssg_stream_t stream);
int ssg_ap_prepare_f64(double* S, int N, const double* pref, int pref_n, const double* noise, ssg_stream_t stream);
int ssg_ap_row_f64(const double* S, double* A, double* R, const double* cs, int N, double damping, int it, int do_r, const int64_t* ctrl,
                   ssg_stream_t stream);
int ssg_ap_colsum_f64(const double* R, int N, double* cs, const int64_t* ctrl, ssg_stream_t stream);
/* the same with tile `cfg` of the column walk, 0 <= cfg < ssg_ap_colsum_configs() (-1: chosen by the number of workgroups, as above);
 * every tile gives the same bits -- for tools/time_affinity.py --sweep and the tests */
int ssg_ap_colsum_configs(void);
int ssg_ap_colsum_cfg_f64(const double* R, int N, double* cs, const int64_t* ctrl, int cfg, ssg_stream_t stream);
int ssg_ap_iterate_f64(const double* S, double* A, double* R, double* cs, uint8_t* window, uint8_t* E, int64_t* ctrl, int N, double damping,
                       int convergence_iter, int it0, int count, ssg_stream_t stream);
int ssg_ap_finish_f64(const double* S, const uint8_t* E, int N, int32_t* I, int32_t* c, double* sums, int64_t* ctrl, ssg_stream_t stream);

/* ---- InceptionNet embedder (reid/models/inception.py:50-119; ssg_amd/inception.py; csrc/inception.hip) ------------------------------
 * The layers the ResNet entry points above do not cover.  Tensors are NHWC, fp32 or h8l8 containers as above.  Every output may be a
 * CHANNEL SLICE of a wider tensor: out points at the first channel of the slice and out_ld is the number of floats (containers) between
 * two pixels of that tensor (out_ld = the layer's own channel count writes a dense tensor); out_ld and the slice offset are multiples of
 * 8 channels (pools on fp32: 4), nothing outside the slice is written -- the branches of a block land where torch.cat would put them.
 * No tensor may exceed 2 GiB (SSG_ERR_INVALID, as ssg_conv2d_nhwc_x).
 * ssg_inc_conv2d_nhwc_x: ssg_conv2d_nhwc_x without a residual for Cout % 32 == 0 (the 32-channel stem layers included): K x K = 1x1 or
 *   3x3, stride 1 or 2, pad 0 or 1; Cin % 32 == 0 with w [Cout][K*K*Cin], or Cin == 4 (3x3 only: RGB0 pixels of ssg_nchw_to_nhwc4 /
 *   _h4l4, w [Cout][64]) in ssg_conv2d_nhwc_x's reduction order.  flags: SSG_CONV_IN_SPLIT (in and w split halves, w rows pre-multiplied
 *   by powers of two that ch_scale undoes; ch_scale is then required), SSG_CONV_OUT_SPLIT (out h8l8; *overflow = 1 when a value does not
 *   fit).  out = [relu](acc * ch_scale + bias).  One wave per 64 pixels x 32 (Cout % 64: 64) channels, operands read straight from memory.
 * ssg_inc_maxpool_nhwc_x: MaxPool2d(k, stride, pad), k <= 3, stride <= 2, 2 * pad <= k: OH = (H + 2 pad - k) / stride + 1; padding never
 *   wins.  Exact (h8l8: the maximum of the decoded values, encoded again).  C % 4 == 0 (h8l8: 8).
 * ssg_inc_avgpool3_nhwc_x: AvgPool2d(3, 1, 1), count_include_pad: the float32 sum of the nine taps in row-major order (rows outer) from
 *   +0, taps outside the map add nothing, then one float32 division by 9 (h8l8: taps decoded, quotient encoded).
 * ssg_inc_head_finish: x, out [rows, C] (out may be x): mode 0 out = relu(x); mode 1 out = x / max(||x||_2, 1e-12) (F.normalize). */
int ssg_inc_conv2d_nhwc_x(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout, int K, int stride,
                          int pad, int relu, int flags, const float* ch_scale, int out_ld, int32_t* overflow, ssg_stream_t stream);
int ssg_inc_maxpool_nhwc_x(const void* in, void* out, int B, int H, int W, int C, int k, int stride, int pad, int split, int out_ld,
                           ssg_stream_t stream);
int ssg_inc_avgpool3_nhwc_x(const void* in, void* out, int B, int H, int W, int C, int split, int out_ld, ssg_stream_t stream);
int ssg_inc_head_finish(const float* x, float* out, int rows, int C, int mode, ssg_stream_t stream);

/* ---- OPTICS on a precomputed distance matrix (ssg_amd.optics.OPTICS; csrc/optics.hip) ------------------------------------------------
 * sklearn 1.7.2's compute_optics_graph(metric='precomputed') with its bits.  The matrix is a view as above -- mode 0 (M = J' half,
 * v, lambda_value), mode 1 (half) or mode 2 (float64) -- always the whole N x N matrix of one GPU, widened to float64 element by element.
 * around15(x) = rint(x * 1e15) / 1e15 with the three roundings apart (np.around(x, 15); +inf stays +inf).
 * ssg_optics_core_dist: core[i] = around15(c > max_eps ? +inf : c), c = the min_samples-th smallest entry of row i with the diagonal
 *   entry counted as it stands; exact for every min_samples in [2, N] (one wave per row, radix select over order-preserving keys).
 * ssg_optics_order: the ordering loop in ONE workgroup.  Step t: p = the unprocessed index of smallest reachability (ties and all-inf:
 *   the smallest index), ordering[t] = p; when core[p] is finite every unprocessed j with X[p,j] <= max_eps takes
 *   r = around15(max(X[p,j], core[p])) and predecessor[j] = p when r < reachability[j].  ordering, predecessor [N] int64 (predecessor
 *   starts at -1), reachability [N] float64 (starts at +inf).  state: where the loop keeps the reachabilities of the unprocessed points --
 *   1 = LDS (N <= ssg_optics_lds_max_n()), 2 = global memory (ws: N * 8 bytes, 8-byte aligned), 0 = LDS when it fits, else global.
 *   No synchronisation between workgroups, no spin loop, no atomic: every loop is bounded by N.
 * Refused with SSG_ERR_INVALID before any device call: a null pointer, N < 2, min_samples outside [2, N], mode 0 without v, a negative
 *   or NaN max_eps, a state outside 0..2, state 1 with N too large, the global state without its workspace. */
int ssg_optics_lds_max_n(void);
int ssg_optics_core_dist(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int min_samples, double max_eps, double* core,
                         ssg_stream_t stream);
int ssg_optics_order(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const double* core, double max_eps, int state,
                     void* ws, size_t ws_bytes, int64_t* ordering, double* reachability, int64_t* predecessor, ssg_stream_t stream);

/* ---- HDBSCAN on a precomputed distance matrix (ssg_amd.hdbscan.HDBSCAN; csrc/hdbscan.hip) ---------------------------------------------
 * The matrix stages of sklearn 1.7.2's HDBSCAN(metric='precomputed') with their bits.  The matrix is a view as above -- mode 0 (M = J'
 * half, v, lambda_value), mode 1 (half) or mode 2 (float64) -- always the whole N x N matrix of one GPU, widened to float64 element by
 * element; nothing N x N is written.
 * ssg_hdbscan_check: one pass over the matrix.  counts[0] = the entries that are NaN; counts[1] = the ordered pairs (i, j), the
 *   diagonal included, that fail np.isclose(X[i,j], X[j,i], rtol=1e-7, atol=1e-9): |x - y| <= 1e-9 + 1e-7 |y| with y finite, or x == y
 *   (two equal infinities are close, an infinity against a finite value is not).  counts: two int64 words, zeroed by the call.
 * ssg_hdbscan_core_dist: core[i] = c / alpha, c = the min_samples-th smallest entry of row i with the diagonal entry counted as it
 *   stands; exact for every min_samples in [1, N] (the radix select of ssg_optics_core_dist).
 * ssg_hdbscan_mst: Prim from node 0 in ONE workgroup, N - 1 steps.  m[j] starts at +inf.  Step t with current node c: every node j
 *   outside the tree takes m[j] = min(m[j], max(core[c], core[j], X[c,j] / alpha)); new = the node outside the tree of smallest m (ties
 *   and all-inf: the smallest index); current[t] = c (the node the step started from, NOT the node that gave `new` its minimum),
 *   next[t] = new, distance[t] = m[new]; then c = new.  current, next [N - 1] int64, distance [N - 1] float64, in Prim order.  The
 *   matrix must hold no NaN (ssg_hdbscan_check counts them).  state: where the loop keeps m -- 1 = LDS (N <= ssg_hdbscan_lds_max_n()),
 *   2 = global memory (ws: N * 8 bytes, 8-byte aligned), 0 = LDS when it fits, else global; every placement gives the same bits.
 *   No synchronisation between workgroups, no spin loop, no atomic: every loop is bounded by N.
 * Refused with SSG_ERR_INVALID before any device call: a null or misaligned pointer, N < 2, min_samples outside [1, N], mode 0 without v,
 *   an alpha that is not positive and finite, a state outside 0..2, state 1 with N too large, the global state without its workspace. */
int ssg_hdbscan_lds_max_n(void);
int ssg_hdbscan_check(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int64_t* counts, ssg_stream_t stream);
int ssg_hdbscan_core_dist(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int min_samples, double alpha, double* core,
                          ssg_stream_t stream);
int ssg_hdbscan_mst(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const double* core, double alpha, int state,
                    void* ws, size_t ws_bytes, int64_t* current, int64_t* next, double* distance, ssg_stream_t stream);

/* ---- Agglomerative clustering of a precomputed distance matrix (ssg_amd.agglomerative; csrc/agglomerative.hip) ------------------------
 * scipy 1.15.3's linkage(y, 'average' | 'complete' | 'single') on the condensed upper triangle -- what sklearn 1.7.2's
 * AgglomerativeClustering(metric='precomputed', connectivity=None) calls -- with its bits, before the sort of the merges.  The matrix is
 * a view as above -- mode 0 (M = J' half, v, lambda_value), mode 1 (half) or mode 2 (float64) -- always the whole N x N matrix of one
 * GPU, widened to float64 element by element; d(i,j) = X[min(i,j), max(i,j)]: the diagonal and the lower triangle take no part.
 * ssg_agglo_check: one pass over the WHOLE matrix.  counts[0] = the entries that are NaN, counts[1] = the entries that are +inf or -inf.
 *   counts: two int64 words, zeroed by the call.
 * ssg_agglo_expand: W[i * ld + j] = W[j * ld + i] = d(i,j) for i != j, W[i * ld + i] = 0: the float64 working square, the only N x N
 *   write (8 N ld bytes).  ld >= N doubles between two rows, ld % 4 == 0, W 32-byte aligned; the columns N .. ld - 1 are left alone.
 * ssg_agglo_nn_chain: the merge loop in ONE workgroup; it rewrites W.  It returns at once, writing nothing, when counts[0] or counts[1]
 *   (the words ssg_agglo_check wrote, read on the device) is not zero.
 *   method 0 (average), 1 (complete): scipy's nn_chain.  A scan from x = chain[-1] finds the live slot i != x of smallest W[x,i], the
 *   lowest index on ties, except that chain[-2] keeps every tie with the minimum; it ends the walk when it finds chain[-2], else it
 *   pushes.  A merge pops two slots, a < b: x[k] = a, y[k] = b, distance[k] = W[a,b], size[k] = size[a] + size[b]; slot a dies, and for
 *   every live i != b  W[i,b] = W[b,i] = max(W[i,a], W[i,b])  or  (na * W[i,a] + nb * W[i,b]) / (na + nb), two products, one sum and
 *   one quotient rounded once each, never fused.  At most 3 (N - 1) scans are made; the kernel counts them and stops there.
 *   method 2 (single): scipy's mst_single_linkage, Prim from node 0: m[j] = min(m[j], W[c,j]) over the unmerged j, next = the unmerged
 *   node of smallest m, the lowest index on ties; x[k] = c, y[k] = next, distance[k] = m[next]; size is not written (may be NULL).
 *   x, y, size [N - 1] int64, distance [N - 1] float64, in merge order.  flag: two int64 words, zeroed by the call: flag[0] = 0, or 1
 *   when the scan bound was reached, or 2 when a scan found no live slot (neither can happen on a finite matrix); flag[1] = the scans
 *   (single: the steps) made.  state: where the loop keeps size[] and chain[] (single: m[]) -- 1 = LDS (N <= ssg_agglo_lds_max_n()),
 *   2 = global memory (ws: 8 * ((N + 3) & ~3) bytes, 16-byte aligned), 0 = LDS when it fits, else global; every placement gives the
 *   same bits.  No synchronisation between workgroups, no spin loop, no atomic.
 * Refused with SSG_ERR_INVALID before any device call: a null or misaligned pointer, N < 2, a mode outside 0..2, mode 0 without v, an
 *   ld below N or not a multiple of 4, a method or state outside 0..2, state 1 with N too large, the global state without its workspace. */
int ssg_agglo_lds_max_n(void);
int ssg_agglo_check(const void* M, const uint16_t* v, int N, int mode, double lambda_value, int64_t* counts, ssg_stream_t stream);
int ssg_agglo_expand(const void* M, const uint16_t* v, int N, int mode, double lambda_value, double* W, int64_t ld, ssg_stream_t stream);
int ssg_agglo_nn_chain(double* W, int N, int64_t ld, int method, int state, const int64_t* counts, void* ws, size_t ws_bytes, int64_t* x, int64_t* y,
                       double* distance, int64_t* size, int64_t* flag, ssg_stream_t stream);

/* ---- Silhouette coefficient of labelings of a precomputed distance matrix (ssg_amd.silhouette; csrc/silhouette.hip) ---------------------
 * The N x N part of sklearn 1.7.2's silhouette_samples(X, labels, metric='precomputed') -- _silhouette_reduce -- with its bits, for K
 * labelings in ONE pass over the matrix.  The matrix is a view as above -- mode 0 (M = J' half, v, lambda_value), mode 1 (half) or mode 2
 * (float64) -- always the whole N x N matrix of one GPU, widened to float64 element by element and never modified.
 * The selection: sel [m] int32 on the device, the selected samples in the order in which their columns are added (a sub-matrix
 *   X[sel][:, sel]; sklearn's sample_size hands over a permuted order); NULL = the identity, m = N.  sel_host: a HOST copy of sel, or
 *   NULL; when given, every entry is range-checked before the launch.  On the device an entry outside [0, N) is not dereferenced (its
 *   value enters as NaN).
 * ssg_silhouette_sums: for labeling k and position a (row sel[a]):
 *     intra_sum[k * m + a] = s[a, own],   inter_min[k * m + a] = min over c != own of s[a, c] / double(freq[c]),
 *   s[a, c] = the float64 sum of X[sel[a], sel[b]] over the members b of cluster c: it starts at +0.0, walks the members in ASCENDING
 *   POSITION and rounds once per add -- np.bincount(labels, weights=row) -- and the quotient is the IEEE division.  Per labeling:
 *   labels [K, m] int32, the encoded label 0 .. C_k - 1 of every position, or a negative value: that position takes no part in
 *   labeling k -- it is in no member list and its two outputs are left as the caller set them.  This is how per-labeling noise sets
 *   are carried (the choice between a per-labeling sel and grouping equal noise sets): sel stays shared, every labeling drops its own
 *   positions and selects m_k = start[k, C_k] <= m of them, so K labelings with K different noise sets still cost one pass.
 *   members [K, m] int32: the positions grouped by cluster, ascending inside each cluster (a stable counting sort, built by the caller);
 *   start [K, Cmax + 1] int32: cluster c of labeling k owns members[k, start[k,c] .. start[k,c+1]); freq[c] is that length.  ncl [K]
 *   int32: C_k <= Cmax.  Every index read from these arrays is clamped before it is used.  diag: 0 = the entry of a position in its own
 *   row enters as stored, 1 = it enters as +0.0 (the matrix after np.fill_diagonal(X, 0), without writing it).
 *   negatives: one int64 word, zeroed by the call: the number of entries of X[sel][:, sel] (after diag) that are below zero, which
 *   sklearn's pairwise_distances refuses; -0.0 is not counted.  An integer atomic per wave, the only atomic of the kernel.
 *   A workgroup owns one selected row at a time: it decodes the m selected entries once into a float64 stage, then for each labeling
 *   thread t of T sums the clusters t, t + T, ... one member after the other, divides, and the workgroup folds the minimum (the caller
 *   refuses NaN and infinity beforehand -- ssg_agglo_check -- so the fold order does not matter).  No float atomic, no synchronisation
 *   between workgroups, no spin loop; every loop is bounded by m or by the number of clusters.  T = 256 threads, or 512 or 1024 when
 *   a CU's LDS holds fewer than four or two stages.  state: where the stage lives -- 1 = LDS
 *   (m <= ssg_silhouette_lds_max_m()), 2 = global memory (ws: one slice of 8 * ((m + 1) & ~1) bytes per workgroup, 16-byte aligned; as
 *   many workgroups run as ws_bytes holds slices, at most 1024), 0 = LDS when it fits, else global; every placement gives the same bits.
 * ssg_silhouette_diag: count[0] = the number of selected samples i with |X[i,i]| > atol, one read per sample; count: one int64 word,
 *   zeroed by the call.
 * The NaN / infinity counts over the whole matrix are ssg_agglo_check's.
 * Refused with SSG_ERR_INVALID before any device call: a null or misaligned pointer, a mode outside 0..2, mode 0 without v, m < 3
 *   (diag: m < 1), m > N, m != N without sel, a sel_host entry outside [0, N), K < 1, Cmax outside [1, m], diag outside 0..1, a negative
 *   or NaN atol, a state outside 0..2, state 1 with m too large, the global stage without its workspace. */
int ssg_silhouette_lds_max_m(void);
int ssg_silhouette_diag(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const int32_t* sel, const int32_t* sel_host, int m,
                        double atol, int64_t* count, ssg_stream_t stream);
int ssg_silhouette_sums(const void* M, const uint16_t* v, int N, int mode, double lambda_value, const int32_t* sel, const int32_t* sel_host, int m,
                        int K, int Cmax, const int32_t* labels, const int32_t* members, const int32_t* start, const int32_t* ncl, int diag, int state,
                        void* ws, size_t ws_bytes, double* intra_sum, double* inter_min, int64_t* negatives, ssg_stream_t stream);

/* ---- test-time extraction and multi-query pooling (reid/extract_feature.py; csrc/tta.hip) ----------------------------------------------
 * ssg_tencrop_u8: the script's test-time transform (:47-52) for a batch of equally sized decoded images, bit for bit:
 *   Resize((RH, RW)) [Pillow bilinear on 8-bit RGB: the arithmetic, tables and scratch of ssg_preprocess_u8] -> TenCrop((CH, CW)) ->
 *   ToTensor -> Normalize.  src [B,h,w,3] uint8, tmp [B,h,RW,3] uint8 scratch, out [B, ncrops, 3, CH, CW] float32, ncrops 5 or 10.
 *   crops_host: HOST int32 [5][2], (top, left) of the crops tl, tr, bl, br, centre in the resized image -- torchvision's five_crop; the
 *   centre is int(round((RH - CH) / 2.0)), int(round((RW - CW) / 2.0)) with Python's round-half-to-even, computed by the caller.
 *   Crops 5..9 (ncrops = 10) are the same five windows of the horizontally mirrored resized image.  Every resized pixel is filtered
 *   once and stored into each crop that holds it.  Refused: a non-positive size, CH > RH, CW > RW, ncrops outside {5, 10}, a window
 *   that leaves the resized image, a NULL pointer.
 * ssg_crop_mean_f32: out [B, D] = the mean of n feature rows per image = torch's CPU x.view(B, n, -1).mean(1): the ascending
 *   sequential float32 sum in table order (no fused multiply-add, no float64), divided by (float)n.  src0 [B, nc0, D] and, optionally,
 *   src1 [B, nc1, D] (nc 5 or 10); table_host: HOST int32 [n][2] = (block 0 | 1, crop), 1 <= n <= 15 (torch sums 16 rows and more
 *   in cascaded levels).  tail: torch's kernel sums the columns in blocks of SIMD vectors and hands the columns behind the last
 *   whole block (D % 32 of them in its x86 builds) to a scalar loop with another order: four partial sums p[k] = v[k] + v[4 + k] +
 *   ... over the whole fours of rows, the remaining rows onto p[0], then ((p[0] + p[1]) + p[2]) + p[3].  The last `tail` columns
 *   are summed that way; tail = 0 sums every column sequentially.
 * ssg_group_pool_f32: the multi-query descriptors (:146-153).  x [M, D] float32; order [M]: row indices grouped by key, each group in
 *   the order its rows were met; offs [G + 1]; qgroup [Q]: the group of every query.  Per row y = (float)((double)x / norm), norm =
 *   sqrt of the float64 sum of squares (lane l of a wave sums the columns l, l + 64, ... ascending, then a fixed butterfly), 0 counts
 *   as 1 (sklearn.preprocessing.normalize).  Per group: out_max = the running max of y in group order, NaN once a NaN is met (np.max);
 *   out_avg = the ascending sequential float32 sum of y in group order / (float)rows (np.mean(axis=0) of a C-contiguous float32
 *   block).  Each group is computed once, into the row of the first query that names it, and copied to its other queries; no atomics
 *   on floats, no workspace.  out_max, out_avg [Q, D]; ynorm [M, D] receives y, or NULL.  Any D. */
int ssg_tencrop_u8(const uint8_t* src, int B, int h, int w, int RH, int RW, int CH, int CW, int ncrops, const int32_t* crops_host,
                   const int32_t* xmin, const int32_t* xcnt, const int32_t* xk, int xksize, const int32_t* ymin, const int32_t* ycnt,
                   const int32_t* yk, int yksize, const float* mean3_host, const float* std3_host, uint8_t* tmp, float* out,
                   ssg_stream_t stream);
int ssg_crop_mean_f32(const float* src0, int nc0, const float* src1, int nc1, int B, int D, const int32_t* table_host, int n, int tail,
                      float* out, ssg_stream_t stream);
int ssg_group_pool_f32(const float* x, int M, int D, const int32_t* order, const int32_t* offs, int G, const int32_t* qgroup, int Q,
                       float* out_max, float* out_avg, float* ynorm, ssg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SSG_HIP_H */
