// The split-bf16 primitives every matrix-core network kernel here is written in (net_dev.hpp, fused16_dev.hpp): a float32
// is the exact sum of three bf16 pieces, each the next 8 significant bits, made by truncation and subtraction
// (DESIGN.md section 5).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nz {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// x with everything below its upper 16 bits cleared: the float its first bf16 piece stands for (x - bf16_trunc(x) is exact)
__device__ __forceinline__ float bf16_trunc(float x) {
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, x) & 0xFFFF0000u);
}
// (x0, x1) -> the two upper halves in one register: bf16(x0) | bf16(x1) << 16 (truncating; one v_perm)
__device__ __forceinline__ uint32_t pack_hi16(float x0, float x1) {
  return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, x1), __builtin_bit_cast(uint32_t, x0), 0x07060302u);
}
// the two pieces of such a register as float32
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& w, const u32x4& x, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), c, 0, 0, 0);
}

// ---- plain-bf16 arithmetic (NZ_PREC_BF16): the rule is stated in fused16_dev.hpp; net_dev.hpp follows it too ----------
constexpr int PREC_F32 = 0, PREC_BF16 = 1;     // = NZ_PREC_FLOAT32, NZ_PREC_BF16 (include/nuzero_amd.h)
__host__ __device__ constexpr int prec_pieces(int prec) { return prec == PREC_BF16 ? 1 : 3; }
// (x0, x1) -> bf16(x0) | bf16(x1) << 16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_rne16(float x0, float x1) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
}

}  // namespace nz
