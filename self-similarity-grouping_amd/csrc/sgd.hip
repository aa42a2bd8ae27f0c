// sgd.hip -- the optimiser step of the fine-tune phase: torch.optim.SGD over many float32 tensors in one pass (gfx950 only).
//
// The reference builds torch.optim.SGD(param_groups, lr, momentum=0.9, weight_decay) over about 160 parameter tensors
// (selftraining.py:152-161, semitraining.py:162).  The update is element-wise -- per element three reads (p, g, buf) and two writes
// (p, buf) -- so one launch serves many tensors:
//
//   descriptors by value   a launch carries, in its kernel arguments, the pointers, lengths and `first` flags of up to SGD_T tensors
//                          and the prefix table of their chunks; there is no device-side table, no copy, no workspace, no host read
//   chunk                  SGD_CHUNK consecutive elements of one tensor: one workgroup.  A workgroup finds its tensor with one ballot
//                          over the prefix table (SGD_T = 64 = one entry per lane) and its chunk by a subtraction
//   one group per launch   the hyper-parameters are scalar kernel arguments, rounded from double to float32 once on the host
//   cuts                   a launch ends at SGD_T descriptors, at SGD_MAX_CHUNKS chunks or where the group changes; a tensor that does
//                          not fit the chunks left in a launch continues in the next one at a multiple of SGD_CHUNK elements, so the
//                          alignment of its pointers is the same in every piece
//
// Arithmetic: torch's _single_tensor_sgd element by element in float32, every add(., alpha=.) one fused multiply-add as in torch's
// CPU kernels (written as fmaf: the library is compiled without contraction), `momentum * buf` rounded on its own:
//   g = maximize ? -g : g;  g = wd != 0 ? fma(wd, p, g) : g
//   momentum != 0:  buf = first ? g : fma(1 - dampening, g, momentum * buf);  g = nesterov ? fma(momentum, buf, g) : buf
//   p = fma(-lr, g, p)
// A chunk whose three pointers are 16-byte aligned moves float4s and finishes with at most 3 single elements; any other chunk moves
// single elements.  Both run the same function per element, so the bits do not depend on the path.  The gradient is never written.
//
// (*) The descriptor arrays are read through scalar loads at an index the workgroup computes.  A scalar load drops the two low bits
// of its base register and of its offset register separately, so an address split as (argument base + t) + 7 t, which the compiler
// formed when a byte array `first[t]` shared its index arithmetic with the 8-byte pointer arrays, reads the wrong dwords: the `first`
// flags are therefore the bits of one 64-bit word, and no array of the argument block has elements narrower than 4 bytes.
#include "train_common.h"
#include <math.h>

#ifndef SSG_SGD_CHUNK
#define SSG_SGD_CHUNK 1024
#endif

namespace ssg {

constexpr int SGD_T = 64;                         // descriptors per launch: one prefix-table entry per lane of a wave
constexpr int SGD_CHUNK = SSG_SGD_CHUNK;          // elements per workgroup
constexpr int SGD_MAX_CHUNKS = (1 << 24) / SGD_CHUNK;   // workgroups per launch: 2^24 elements
constexpr int SGD_V = SGD_CHUNK / 1024;           // float4s per thread and array
static_assert(SGD_CHUNK >= 1024 && (SGD_CHUNK & (SGD_CHUNK - 1)) == 0, "a chunk is a power of two of at least 256 float4s");
static_assert((int64_t)SGD_CHUNK * SGD_MAX_CHUNKS < 0x7fffffffLL, "a descriptor's length is an int");
static_assert(SGD_T <= 64, "the prefix table is searched by one ballot and the first flags are the bits of one word");

enum { SGD_MOMENTUM = 1, SGD_NESTEROV = 2, SGD_MAXIMIZE = 4, SGD_DECAY = 8 };

struct SgdLaunch {                                // 2080 bytes of kernel arguments; every array element is 4 or 8 bytes wide (*)
  float* p[SGD_T];
  const float* g[SGD_T];
  float* buf[SGD_T];                              // NULL without momentum
  int n[SGD_T];                                   // elements of this piece, 1 .. SGD_CHUNK * SGD_MAX_CHUNKS
  int start[SGD_T];                               // first workgroup of descriptor t; start[0] = 0, strictly ascending
  uint64_t first;                                 // bit t: the buffer of descriptor t holds nothing yet
  int count;
  int flags;
  float neg_lr, momentum, one_minus_dampening, weight_decay;
};

struct SgdHyper {
  float neg_lr, momentum, omd, wd;
  bool has_momentum, nesterov, maximize, decay, first;
};

__device__ __forceinline__ void sgd_element(float& p, float g, float& b, const SgdHyper& h) {
  if (h.maximize) g = -g;
  if (h.decay) g = fmaf(h.wd, p, g);
  if (h.has_momentum) {
    b = h.first ? g : fmaf(h.omd, g, h.momentum * b);
    g = h.nesterov ? fmaf(h.momentum, b, g) : b;
  }
  p = fmaf(h.neg_lr, g, p);
}

__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdLaunch a) {
  const int tid = threadIdx.x, lane = tid & 63, wg = (int)blockIdx.x;
  // the descriptor of this workgroup: the last one whose first workgroup is not past wg
  const int s = lane < a.count ? a.start[lane] : 0x7fffffff;
  const int t = __popcll(__ballot(s <= wg)) - 1;
  const int off = (wg - a.start[t]) * SGD_CHUNK;
  const int left = a.n[t] - off, cnt = left < SGD_CHUNK ? left : SGD_CHUNK;
  float* __restrict__ p = a.p[t] + off;
  const float* __restrict__ g = a.g[t] + off;
  SgdHyper h;
  h.neg_lr = a.neg_lr; h.momentum = a.momentum; h.omd = a.one_minus_dampening; h.wd = a.weight_decay;
  h.has_momentum = a.flags & SGD_MOMENTUM; h.nesterov = a.flags & SGD_NESTEROV; h.maximize = a.flags & SGD_MAXIMIZE; h.decay = a.flags & SGD_DECAY;
  h.first = (a.first >> t) & 1;
  float* __restrict__ b = h.has_momentum ? a.buf[t] + off : nullptr;
  const bool read_b = h.has_momentum && !h.first;

  int done = 0;                                   // elements the float4 part has served
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0) {
    const int nv = cnt >> 2;
    float4 pv[SGD_V], gv[SGD_V], bv[SGD_V];
#pragma unroll
    for (int i = 0; i < SGD_V; i++) {
      const int j = i * 256 + tid;
      if (j < nv) {
        pv[i] = reinterpret_cast<const float4*>(p)[j];
        gv[i] = reinterpret_cast<const float4*>(g)[j];
        bv[i] = read_b ? reinterpret_cast<const float4*>(b)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int i = 0; i < SGD_V; i++) {
      const int j = i * 256 + tid;
      if (j < nv) {
        sgd_element(pv[i].x, gv[i].x, bv[i].x, h);
        sgd_element(pv[i].y, gv[i].y, bv[i].y, h);
        sgd_element(pv[i].z, gv[i].z, bv[i].z, h);
        sgd_element(pv[i].w, gv[i].w, bv[i].w, h);
        reinterpret_cast<float4*>(p)[j] = pv[i];
        if (h.has_momentum) reinterpret_cast<float4*>(b)[j] = bv[i];
      }
    }
    done = nv << 2;
  }
  for (int e = done + tid; e < cnt; e += 256) {
    float pe = p[e], be = read_b ? b[e] : 0.f;
    sgd_element(pe, g[e], be, h);
    p[e] = pe;
    if (h.has_momentum) b[e] = be;
  }
}

}  // namespace ssg

namespace {

using namespace ssg;

bool sgd_bad_scalar(double v) { return !(v >= 0.0) || !isfinite(v); }

int sgd_flush(SgdLaunch& L, int chunks, hipStream_t stream) {
  if (L.count == 0) return SSG_OK;
  hipLaunchKernelGGL(sgd_step_kernel, dim3(chunks), dim3(256), 0, stream, L);
  SSG_LAUNCH_CHECK("sgd_step_kernel");
  L.count = 0;
  L.first = 0;
  return SSG_OK;
}

}  // namespace

extern "C" int ssg_sgd_max_tensors_per_launch(void) { return SGD_T; }
extern "C" int ssg_sgd_chunk_elems(void) { return SGD_CHUNK; }
extern "C" int ssg_sgd_max_chunks_per_launch(void) { return SGD_MAX_CHUNKS; }

extern "C" int ssg_sgd_step_f32(float* const* params, const float* const* grads, float* const* bufs, const int64_t* numel, const int* group, const int* first,
                                int count, const double* lr, const double* momentum, const double* dampening, const double* weight_decay,
                                const int* nesterov, const int* maximize, int num_groups, hipStream_t stream) {
  const char* fn = "ssg_sgd_step_f32";
  if (count < 0) { ssg_set_error("%s: count must not be negative (count=%d)", fn, count); return SSG_ERR_INVALID; }
  if (count == 0) return SSG_OK;
  if (!params || !grads || !bufs || !numel || !group || !first || !lr || !momentum || !dampening || !weight_decay || !nesterov || !maximize) {
    ssg_set_error("%s: NULL array with count=%d (every per-tensor and per-group array is needed)", fn, count);
    return SSG_ERR_INVALID;
  }
  if (num_groups <= 0) { ssg_set_error("%s: num_groups must be at least 1 (num_groups=%d)", fn, num_groups); return SSG_ERR_INVALID; }
  for (int k = 0; k < num_groups; k++) {
    if (sgd_bad_scalar(lr[k]) || sgd_bad_scalar(momentum[k]) || sgd_bad_scalar(weight_decay[k])) {
      ssg_set_error("%s: lr, momentum and weight_decay must be finite and not negative (group %d: lr=%g momentum=%g weight_decay=%g)", fn, k, lr[k],
                    momentum[k], weight_decay[k]);
      return SSG_ERR_INVALID;
    }
    if (nesterov[k] && (momentum[k] == 0.0 || dampening[k] != 0.0)) {
      ssg_set_error("%s: nesterov requires a momentum and zero dampening (group %d: momentum=%g dampening=%g)", fn, k, momentum[k], dampening[k]);
      return SSG_ERR_INVALID;
    }
  }
  for (int i = 0; i < count; i++) {
    if (group[i] < 0 || group[i] >= num_groups) {
      ssg_set_error("%s: group index out of range (tensor %d: group=%d, num_groups=%d)", fn, i, group[i], num_groups);
      return SSG_ERR_INVALID;
    }
    if (!params[i] || !grads[i]) { ssg_set_error("%s: NULL parameter or gradient pointer (tensor %d)", fn, i); return SSG_ERR_INVALID; }
    if (momentum[group[i]] != 0.0 && !bufs[i]) {
      ssg_set_error("%s: NULL momentum buffer in a group with momentum (tensor %d, group %d)", fn, i, group[i]);
      return SSG_ERR_INVALID;
    }
    if (numel[i] <= 0) { ssg_set_error("%s: n must be at least 1 (tensor %d: n=%lld)", fn, i, (long long)numel[i]); return SSG_ERR_INVALID; }
  }

  SgdLaunch L = {};
  int chunks = 0, cur = -1;
  for (int i = 0; i < count; i++) {
    const int k = group[i];
    const bool mom = momentum[k] != 0.0;
    for (int64_t off = 0; off < numel[i];) {
      if (L.count == SGD_T || chunks == SGD_MAX_CHUNKS || (L.count && k != cur))
        if (int rc = sgd_flush(L, chunks, stream)) return rc;
      if (L.count == 0) {
        chunks = 0;
        cur = k;
        L.flags = (mom ? SGD_MOMENTUM : 0) | (nesterov[k] ? SGD_NESTEROV : 0) | (maximize[k] ? SGD_MAXIMIZE : 0) | (weight_decay[k] != 0.0 ? SGD_DECAY : 0);
        L.neg_lr = -(float)lr[k];
        L.momentum = (float)momentum[k];
        L.one_minus_dampening = (float)(1.0 - dampening[k]);
        L.weight_decay = (float)weight_decay[k];
      }
      const int64_t room = (int64_t)(SGD_MAX_CHUNKS - chunks) * SGD_CHUNK, rest = numel[i] - off;
      const int len = (int)(rest < room ? rest : room);
      const int t = L.count++;
      L.p[t] = params[i] + off;
      L.g[t] = grads[i] + off;
      L.buf[t] = mom ? bufs[i] + off : nullptr;
      L.n[t] = len;
      L.start[t] = chunks;
      if (first[i]) L.first |= 1ULL << t;
      chunks += (len + SGD_CHUNK - 1) / SGD_CHUNK;
      off += len;
    }
  }
  return sgd_flush(L, chunks, stream);
}
