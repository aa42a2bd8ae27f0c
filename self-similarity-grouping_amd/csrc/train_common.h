// train_common.h -- what the train-mode launchers (conv_train.hip, conv_strided.hip, head_train.hip) share: the MFMA accumulator type
// and the argument checks that come before a launch.  (Not in ssg_common.h: that file is part of the fingerprint of the embedding's
// kernels, which these launchers do not touch.)
#pragma once
#include "ssg_common.h"
#include <initializer_list>

namespace ssg {

typedef float f32x16 __attribute__((ext_vector_type(16)));  // accumulator of v_mfma_f32_32x32x2_f32

}  // namespace ssg

// argument checks: SSG_OK, or SSG_ERR_INVALID with the error set to "<fn>: ..."
inline int ssg_need_pointers(const char* fn, bool all_given) {
  if (!all_given) { ssg_set_error("%s: NULL pointer", fn); return SSG_ERR_INVALID; }
  return SSG_OK;
}
inline int ssg_need_aligned16(const char* fn, const char* names, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15) { ssg_set_error("%s: %s must be 16-byte aligned", fn, names); return SSG_ERR_INVALID; }
  return SSG_OK;
}
inline int ssg_need_weight_strides(const char* fn, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_s) {
  if (s_co < 0 || s_ci < 0 || s_r < 0 || s_s < 0) { ssg_set_error("%s: negative weight stride", fn); return SSG_ERR_INVALID; }
  return SSG_OK;
}
// grid of a grid-stride loop over `total` elements with 256 threads per block, at most `cap` blocks
inline int ssg_blocks256(int64_t total, int cap) { const int64_t b = (total + 255) / 256; return (int)(b < cap ? b : cap); }
