// Host side of tests/test_half_cvt_host.py: csrc/half_cvt.h compiled by g++ (no HIP header), as arrays in, arrays out.
#include <cstdint>

#include "../cca_zoo_amd/csrc/half_cvt.h"

extern "C" {

// kind 0: bfloat16, 1: binary16
void half_widen(int kind, const uint16_t* in, int64_t n, uint32_t* out_bits) {
  for (int64_t i = 0; i < n; ++i)
    out_bits[i] = ccz::f32_to_bits(kind == 0 ? ccz::widen(ccz::bf16_t{in[i]}) : ccz::widen(ccz::f16_t{in[i]}));
}

void half_narrow(int kind, const uint32_t* in_bits, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    const float f = ccz::bits_to_f32(in_bits[i]);
    out[i] = kind == 0 ? ccz::narrow<ccz::bf16_t>(f).bits : ccz::narrow<ccz::f16_t>(f).bits;
  }
}

}  // extern "C"
