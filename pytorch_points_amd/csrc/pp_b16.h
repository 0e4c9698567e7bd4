// pp_b16.h -- the 16-bit feature types of gather_points, group_points and three_interpolate (DESIGN.md §4
// "16-bit features").  Plain C++ besides the __host__ __device__ marks: tests/test_features16_host.py compiles the two
// narrowing functions for the host and compares them with torch's conversion.
//   widen  : exact (every fp16 / bf16 value is an fp32 value)
//   narrow : round to nearest even, once; fp16 overflows to +-inf; NaN stays NaN (bf16: the quiet NaN 0x7fc0)
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif

namespace pp {

struct bf16 {
  uint16_t bits;
};
typedef _Float16 f16;

PP_HD uint32_t f32_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
PP_HD float bits_f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

PP_HD float widen(float v) { return v; }
PP_HD float widen(f16 v) { return (float)v; }
PP_HD float widen(bf16 v) { return bits_f32((uint32_t)v.bits << 16); }  // a shift

PP_HD uint16_t narrow_bf16_bits(float f) {
  const uint32_t u = f32_bits(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN (adding the rounding bias could carry it into inf)
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);  // ties to the even upper half; overflow carries into inf
}
PP_HD uint16_t narrow_f16_bits(float f) {
  const f16 h = (f16)f;  // v_cvt_f16_f32 on the device: round to nearest even, overflow to inf
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}

template <typename T>
PP_HD T narrow(float f);
template <>
PP_HD float narrow<float>(float f) {
  return f;
}
template <>
PP_HD f16 narrow<f16>(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  // keep the fp32 value: fused with the fma in front of it (v_fma_mixlo_f16) the conversion would round the exact
  // result once, and the contract is the fp32 operator's rounded result rounded again
  asm("" : "+v"(f));
#endif
  return (f16)f;
}
template <>
PP_HD bf16 narrow<bf16>(float f) {
  bf16 r;
  r.bits = narrow_bf16_bits(f);
  return r;
}

}  // namespace pp
