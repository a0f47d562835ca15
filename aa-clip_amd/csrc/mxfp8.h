// The MX fp8 storage format of config C5, defined once for every kernel that writes it: the
// row kernels and aaclip_quant_fp8_mx (rows.hip), the GEMM epilogues (gemm.hip) and the
// attention epilogue (attention.hip). The MX GEMM reads what they write, so they agree bit
// for bit.
//
//   * values: OCP e4m3 (largest finite 448), one byte per element, row-major;
//   * block: 64 consecutive columns of one row share one e8m0 scale byte e + 127;
//   * exponent rule: e = the smallest integer with amax * 2^-e <= 448, amax = max |x| over
//     the block, clamped to [-126, 127]; e = 0 for an all-zero block. A value is stored as
//     RNE_e4m3(x * 2^-e): the scaling is exact (a power of two), the conversion the only rounding;
//   * scale buffer: [cols / 128][ld][2] bytes, ld >= rows: the scales of the two blocks of a
//     128-column group lie side by side, rows contiguous (the MFMA's scale operand layout).
#pragma once
#include "common.h"

__device__ __forceinline__ int mx_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int x;
  (void)frexpf(amax, &x);  // amax = m * 2^x, m in [0.5, 1)
  int e = x - 9;           // amax * 2^-e in [256, 512)
  if (ldexpf(amax, -e) > 448.f) e += 1;
  return max(min(e, 127), -126);
}
// 2^e as a float, e in [-126, 127]
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }

// e4m3 bytes of a * inv, b * inv, c * inv, d * inv (RNE), a in the low byte
__device__ __forceinline__ uint32_t mx_pack4(float a, float b, float c, float d, float inv) {
  const uint32_t w = __builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(c * inv, d * inv, w, true);
}

// the scale byte of (row, 64-column block blk) in the buffer sc [cols / 128][ld][2]; holds e + 127
__device__ __forceinline__ uint8_t* mx_scale_ptr(uint8_t* sc, int64_t ld, size_t row, int blk) {
  return sc + ((size_t)(blk >> 1) * ld + row) * 2 + (blk & 1);
}

// 4x4 dword transpose across the lane groups fq = lane/16: on entry lane fq holds
// d[j] = its 4 fp8 columns of column tile j; on exit it holds tile j = fq's 16
// consecutive bytes (d[q] = the 4 columns of lane group q).
__device__ __forceinline__ void transpose_fq(uint32_t (&d)[4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    auto r = __builtin_amdgcn_permlane32_swap(d[j], d[j + 2], false, false);
    d[j] = r[0];
    d[j + 2] = r[1];
  }
#pragma unroll
  for (int k = 0; k < 4; k += 2) {
    auto r = __builtin_amdgcn_permlane16_swap(d[k], d[k + 1], false, false);
    d[k] = r[0];
    d[k + 1] = r[1];
  }
}

// cross-lane max over the 4 lanes {c, c+16, c+32, c+48} (one row of a C^T tile)
__device__ __forceinline__ float max_over_fq(float v) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// MX quantisation of one row's 64-column block of a C^T tile (lane (fr, fq) holds columns
// 16 j + 4 fq .. + 3 of tile j): row max over the 4 lane groups, power-of-two scale, RNE to
// e4m3, 4x4 lane-group transpose. On exit d = the row's bytes 16 fq .. 16 fq + 15; returns the
// block exponent. (The attention epilogue writes the same steps out with these helpers: it folds
// its 1 / l into the scale and takes the max in its own asm form.)
__device__ __forceinline__ int mx_quant_row(const float4_t (&v)[4], uint32_t (&d)[4]) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) amax = fmaxf(amax, fabsf(v[j][t]));
  const int e = mx_exp(max_over_fq(amax));
  const float inv = pow2i(-e);
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = mx_pack4(v[j][0], v[j][1], v[j][2], v[j][3], inv);
  transpose_fq(d);
  return e;
}
