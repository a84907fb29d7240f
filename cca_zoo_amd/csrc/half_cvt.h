// The 2-byte input / output formats of the deep objectives: bfloat16 and IEEE binary16 as bit patterns, widened to and
// narrowed from float32 with integer arithmetic only -- the same code on the device and on the host (tests/half_cvt_host.cpp
// compiles this header with g++ and compares every bit pattern with torch's CPU conversions).
//
//   widen   exact for both types (they embed in float32, fp16 subnormals included); NaN stays NaN
//   narrow  round to nearest even; overflow gives +-inf; fp16 subnormals are rounded correctly; NaN -> the quiet NaN
//
// Half precision is a FORMAT here, not an arithmetic: a kernel widens on load, computes in float32 (fp64 on the D x D side)
// and narrows once on store.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CCZ_HD __host__ __device__
#else
#define CCZ_HD
#endif

namespace ccz {

struct bf16_t { uint16_t bits; };
struct f16_t { uint16_t bits; };

CCZ_HD inline float bits_to_f32(uint32_t u) {
  union { uint32_t u; float f; } x;
  x.u = u;
  return x.f;
}
CCZ_HD inline uint32_t f32_to_bits(float f) {
  union { uint32_t u; float f; } x;
  x.f = f;
  return x.u;
}

CCZ_HD inline float widen(bf16_t h) { return bits_to_f32(uint32_t(h.bits) << 16); }

CCZ_HD inline float widen(f16_t h) {
  uint32_t o = uint32_t(h.bits & 0x7fffu) << 13;            // exponent and mantissa where float32 keeps them
  const uint32_t e = o & 0x0f800000u;
  o += uint32_t(127 - 15) << 23;                           // the bias
  if (e == 0x0f800000u) {
    o += uint32_t(128 - 16) << 23;                         // inf / NaN: the exponent field becomes all ones
  } else if (e == 0) {
    // zero or subnormal, m 2^-24: 2^-14 (1 + m / 1024) - 2^-14 is exact (both are normal float32 numbers, and so is the result)
    o = f32_to_bits(bits_to_f32(o + (1u << 23)) - bits_to_f32(113u << 23));
  }
  return bits_to_f32(o | (uint32_t(h.bits & 0x8000u) << 16));
}

CCZ_HD inline float widen(float x) { return x; }

// an element of any input type as a double (kernels that accumulate in fp64 straight from the rows)
CCZ_HD inline double to_f64(double x) { return x; }
CCZ_HD inline double to_f64(float x) { return double(x); }
CCZ_HD inline double to_f64(bf16_t x) { return double(widen(x)); }
CCZ_HD inline double to_f64(f16_t x) { return double(widen(x)); }

CCZ_HD inline bf16_t narrow_bf16(float f) {
  const uint32_t x = f32_to_bits(f);
  bf16_t r;
  if ((x & 0x7fffffffu) > 0x7f800000u) r.bits = 0x7fc0u;                   // NaN
  else r.bits = uint16_t((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);          // nearest even; a carry out of the mantissa reaches inf by itself
  return r;
}

CCZ_HD inline f16_t narrow_f16(float f) {
  const uint32_t x = f32_to_bits(f);
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  f16_t r;
  if (a > 0x7f800000u) {
    r.bits = uint16_t(sign | 0x7e00u);                                     // NaN
  } else if (a >= 0x477ff000u) {
    r.bits = uint16_t(sign | 0x7c00u);                                     // 65520 (halfway between 65504 and 2^16) and above: inf
  } else if (a >= 0x38800000u) {                                           // 2^-14 and above: a normal binary16 number
    const uint32_t v = a - (uint32_t(127 - 15) << 23);
    r.bits = uint16_t(sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13));     // (a carry runs into the exponent: correct)
  } else if (a <= 0x33000000u) {
    r.bits = uint16_t(sign);                                               // at most 2^-25, half the smallest subnormal: the tie goes to (even) zero
  } else {
    // subnormal: q 2^-24 with q = round(m 2^(e - 126)), m the 24-bit significand, e = 102 .. 112
    const uint32_t s = 126u - (a >> 23), m = (a & 0x7fffffu) | 0x800000u;
    uint32_t q = m >> s;
    const uint32_t rem = m & ((1u << s) - 1u), half = 1u << (s - 1u);
    if (rem > half || (rem == half && (q & 1u))) ++q;                      // (q = 1024 is the smallest normal number)
    r.bits = uint16_t(sign | q);
  }
  return r;
}

template <typename T> CCZ_HD inline T narrow(float f);
template <> CCZ_HD inline bf16_t narrow<bf16_t>(float f) { return narrow_bf16(f); }
template <> CCZ_HD inline f16_t narrow<f16_t>(float f) { return narrow_f16(f); }
template <> CCZ_HD inline float narrow<float>(float f) { return f; }

}  // namespace ccz
