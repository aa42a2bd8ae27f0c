// ssg_common.h -- shared device helpers for the SSG grouping kernels (gfx950 only).
//
// Half arithmetic follows numpy's half loops exactly (the reference computes the whole
// re-rank in np.float16, reid/rerank.py:33-122): every binary op is an IEEE float32 op
// followed by one round-to-nearest-even to half; double -> half is a single direct RNE
// (npy_double_to_half), never via float.
#pragma once
// numpy rounds a*b and +c separately (e.g. rerank.py:122 final_dist, the float64 distance epilogues): no FMA contraction
// anywhere in this library, whatever flags it is built with.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SSG_OK 0
#define SSG_ERR_INVALID (-1)
#define SSG_ERR_HIP (-2)
#define SSG_ERR_OVERFLOW (-3)
#define SSG_ERR_NAN (-4)

namespace ssg {

typedef uint16_t hbits;  // IEEE binary16 bit pattern

__device__ __forceinline__ float h2f(hbits h) { return (float)__builtin_bit_cast(_Float16, h); }
// float -> half RNE (v_cvt_f16_f32; f16 denormals are kept in hipcc's default mode)
__device__ __forceinline__ hbits f2h(float f) { return __builtin_bit_cast(hbits, (_Float16)f); }

// double -> half, one rounding (bit-exact port of npy_double_to_half; gfx950 has no
// direct f64->f16 convert and f64->f32->f16 double-rounds).
__device__ __forceinline__ hbits d2h(double d) {
  const uint64_t b = (uint64_t)__double_as_longlong(d);
  const hbits sign = (hbits)((b >> 48) & 0x8000u);
  const int e = (int)((b >> 52) & 0x7ff);
  uint64_t m = b & 0xfffffffffffffULL;
  if (e == 0x7ff) return (hbits)(sign | 0x7c00u | (m ? 0x200u : 0u));
  if (e == 0) return sign;
  const int he = e - 1023 + 15;
  if (he >= 31) return (hbits)(sign | 0x7c00u);
  m |= 1ULL << 52;
  int shift = 42;
  if (he <= 0) { shift = 43 - he; if (shift > 63) return sign; }
  uint64_t q = m >> shift;
  const uint64_t rem = m & ((1ULL << shift) - 1), half = 1ULL << (shift - 1);
  if (rem > half || (rem == half && (q & 1))) q++;
  if (he <= 0) return (hbits)(sign | (hbits)q);
  uint32_t r = ((uint32_t)he << 10) + (uint32_t)(q - 0x400);
  if (r >= 0x7c00u) r = 0x7c00u;
  return (hbits)(sign | r);
}

__device__ __forceinline__ hbits h_add(hbits a, hbits b) { return f2h(h2f(a) + h2f(b)); }
__device__ __forceinline__ hbits h_sub(hbits a, hbits b) { return f2h(h2f(a) - h2f(b)); }
__device__ __forceinline__ hbits h_mul(hbits a, hbits b) { return f2h(h2f(a) * h2f(b)); }
// IEEE-correct float division (hipcc default: -fhip-fp32-correctly-rounded-divide-sqrt)
__device__ __forceinline__ hbits h_div(hbits a, hbits b) { return f2h(h2f(a) / h2f(b)); }
__device__ __forceinline__ bool h_isnan(hbits h) { return (h & 0x7fffu) > 0x7c00u; }
// correctly rounded half exp(-x): f64 exp (<=1 ulp) then one direct rounding
__device__ __forceinline__ hbits h_exp_neg(hbits x) { return d2h(exp(-(double)h2f(x))); }

constexpr hbits H_ONE = 0x3c00, H_TWO = 0x4000;

// final_dist[i,k] of reid/rerank.py:122 rebuilt from the compact representation:
//   f64(J'[i,k]) + f64(half(v_i + v_k)) * lambda      (J' = half(J * half(1-lambda)))
__device__ __forceinline__ double final_dist_value(hbits jp, hbits vi, hbits vk, double lambda_value) {
  return (double)h2f(jp) + (double)h2f(h_add(vk, vi)) * lambda_value;
}

// wave64 helpers
// value of lane (l ^ 1): a DPP quad permutation [1,0,3,2] on the way into the VALU -- __shfl_xor(v, 1) compiles to ds_bpermute_b32,
// an LDS-pipe round trip per dword (the split-half epilogues exchange four dwords per 16-byte store).  Every lane must be active.
__device__ __forceinline__ unsigned lane_xor1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false); }
// take ? (send of lane l ^ 1) : keep -- one half of the hi <-> lo exchange of a lane pair in the split-half epilogues.  The DPP move
// runs for every lane before the select (inside a divergent branch it would read disabled lanes); bound_ctrl gives the 0 of lane_xor1
// for an invalid source lane without a v_mov of the old value.  (A DPP bank mask covers four consecutive lanes, not a parity, so the
// move itself cannot be the select; v_cndmask_b32_dpp can, but only from inline assembly, past the compiler's DPP hazard handling.)
__device__ __forceinline__ unsigned lane_pair_merge(unsigned keep, unsigned send, bool take) {
  const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1, 0xF, 0xF, true);
  return take ? recv : keep;
}
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ULL << lane_id()) - 1ULL; }

// ---- split-half codec: an fp32 value v travels as  hi = half(v), lo = half(v - float(hi))  and is read back as float(hi) + float(lo)
// (conv.hip has the format and what it is for).  Four values of a lane = one dword pair of hi halves and one of lo halves.
// SSG_SPLIT_MIX selects the mixed-precision FMA forms (v_fma_mix*: a half operand converted on the way into an fp32 FMA).  They round
// the same values once each: float(half) is exact, so fma(float(hi), 1, float(lo)) = float(hi) + float(lo) and fma(float(hi), -1, v) =
// v - float(hi); that difference is exact in fp32 for |v| < 65520, so rounding it to half directly equals rounding it to fp32 first.
// (A host compilation of this header -- tools/hostexec -- always takes the plain-C++ forms.)
#ifndef SSG_SPLIT_MIX
#define SSG_SPLIT_MIX 1
#endif
#if SSG_SPLIT_MIX && defined(__HIP_DEVICE_COMPILE__)
#define SSG_SPLIT_MIX_ASM 1
#else
#define SSG_SPLIT_MIX_ASM 0
#endif
typedef _Float16 split_h2 __attribute__((ext_vector_type(2)));
typedef _Float16 split_h4 __attribute__((ext_vector_type(4)));
typedef float split_f2 __attribute__((ext_vector_type(2)));
typedef float split_f4 __attribute__((ext_vector_type(4)));

#if SSG_SPLIT_MIX_ASM
// the lo dword of two values: half(a - float(hp.lo)) | half(b - float(hp.hi)) << 16.  VALU only; the destination is written in two steps
__device__ __forceinline__ unsigned split_lo2_mix(unsigned hp, float a, float b) {
  unsigned d;
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(d) : "v"(hp), "v"(a), "v"(b));
  return d;
}
template <int HIGH> __device__ __forceinline__ float split_sum_mix(unsigned h, unsigned l) {
  float d;
  if (HIGH) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(h), "v"(l));
  else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(h), "v"(l));
  return d;
}
#endif
// 4 values -> (hi pair of dwords, lo pair of dwords)
__device__ __forceinline__ void split_encode4(const float4 v, uint2& hi, uint2& lo) {
#if SSG_SPLIT_MIX_ASM
  const split_f2 a = {v.x, v.y}, b = {v.z, v.w};
  hi = make_uint2(__builtin_bit_cast(unsigned, __builtin_convertvector(a, split_h2)), __builtin_bit_cast(unsigned, __builtin_convertvector(b, split_h2)));
  lo = make_uint2(split_lo2_mix(hi.x, v.x, v.y), split_lo2_mix(hi.y, v.z, v.w));
#else
  const split_f4 f = {v.x, v.y, v.z, v.w};
  const split_h4 h = __builtin_convertvector(f, split_h4);                    // v_cvt_pk_f16_f32 x 2
  const split_h4 l = __builtin_convertvector(f - __builtin_convertvector(h, split_f4), split_h4);
  hi = __builtin_bit_cast(uint2, h);
  lo = __builtin_bit_cast(uint2, l);
#endif
}
__device__ __forceinline__ float4 split_decode4(const uint2 hi, const uint2 lo) {
#if SSG_SPLIT_MIX_ASM
  return make_float4(split_sum_mix<0>(hi.x, lo.x), split_sum_mix<1>(hi.x, lo.x), split_sum_mix<0>(hi.y, lo.y), split_sum_mix<1>(hi.y, lo.y));
#else
  const split_f4 r = __builtin_convertvector(__builtin_bit_cast(split_h4, hi), split_f4) + __builtin_convertvector(__builtin_bit_cast(split_h4, lo), split_f4);
  return make_float4(r.x, r.y, r.z, r.w);
#endif
}
// bits 15 / 31 of the result are set when a hi half is infinite or NaN, i.e. the value did not fit the split-half format (exponent field
// all ones: + 0x0400 carries into the sign position, nothing smaller does); kernels OR it over their tiles and test once at the end
__device__ __forceinline__ unsigned split_hi_nonfinite_bits(const uint2 hi) {
  return ((hi.x & 0x7c007c00u) + 0x04000400u) | ((hi.y & 0x7c007c00u) + 0x04000400u);
}
__device__ __forceinline__ bool split_hi_nonfinite(const uint2 hi) { return (split_hi_nonfinite_bits(hi) & 0x80008000u) != 0; }
// The 16-byte piece a lane of the pair (2g, 2g + 1) stores or loads: the even lane's is [hi x 8] of channel group g, the odd lane's
// [lo x 8]; each lane computes channels 4 * odd .. 4 * odd + 3 of the group.  Every lane must be active.
__device__ __forceinline__ uint4 split_pair_pack(const uint2 hp, const uint2 lp, const bool odd) {
  return make_uint4(lane_pair_merge(hp.x, lp.x, odd), lane_pair_merge(hp.y, lp.y, odd), lane_pair_merge(lp.x, hp.x, !odd), lane_pair_merge(lp.y, hp.y, !odd));
}
__device__ __forceinline__ float4 split_pair_decode4(const unsigned a0, const unsigned a1, const unsigned a2, const unsigned a3, const bool odd) {
  return split_decode4(make_uint2(lane_pair_merge(a0, a2, odd), lane_pair_merge(a1, a3, odd)), make_uint2(lane_pair_merge(a2, a0, !odd), lane_pair_merge(a3, a1, !odd)));
}

}  // namespace ssg

// host-side error plumbing (ssg_api.cpp)
void ssg_set_error(const char* fmt, ...);
int ssg_check_hip(hipError_t e, const char* what);
#define SSG_HIP(call) do { int rc_ = ssg_check_hip((call), #call); if (rc_) return rc_; } while (0)
#define SSG_LAUNCH_CHECK(name) do { int rc_ = ssg_check_hip(hipGetLastError(), name); if (rc_) return rc_; } while (0)
