// fp32 row arithmetic shared by the row kernels (rows.hip) and their backwards
// (text_bwd.hip, visual_bwd.hip): one definition of the row layout, of the LayerNorm
// statistics and of the LayerNorm backward, so the forward and the backward agree on eps,
// on which lane owns which element and on the order every sum is taken in.
//
// One wave (64 lanes) owns one row of width 256 * VEC (768 -> VEC 3, 1024 -> VEC 4); lane l
// holds elements 256 c + 4 l .. + 3, so every load / store instruction moves one contiguous
// 1 KiB segment of the row.
#pragma once
#include "common.h"

constexpr float kLnEps = 1e-5f;  // nn.LayerNorm default (transformer.py:37-43)

template <int VEC>
__device__ __forceinline__ void load_row(const float* p, float4_t (&v)[VEC], int lane) {
#pragma unroll
  for (int c = 0; c < VEC; ++c) v[c] = *(const float4_t*)(p + 256 * c + 4 * lane);
}
template <int VEC>
__device__ __forceinline__ void store_row(float* p, const float4_t (&v)[VEC], int lane) {
#pragma unroll
  for (int c = 0; c < VEC; ++c) *(float4_t*)(p + 256 * c + 4 * lane) = v[c];
}
// a . b over the row: lane-local in element order, then the wave reduction (|x|^2 = row_dot(x, x))
template <int VEC>
__device__ __forceinline__ float row_dot(const float4_t (&a)[VEC], const float4_t (&b)[VEC]) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < VEC; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += a[c][j] * b[c][j];
  return wave_sum(s);
}

// F.layer_norm's statistics of one row: mean and 1 / sqrt(biased variance + eps)
struct LnStats {
  float mean, rstd;
};
template <int VEC>
__device__ __forceinline__ LnStats ln_stats(const float4_t (&x)[VEC]) {
  constexpr float inv_d = 1.0f / (256 * VEC);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < VEC; ++c) s += (x[c][0] + x[c][1]) + (x[c][2] + x[c][3]);
  const float mean = wave_sum(s) * inv_d;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < VEC; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = x[c][j] - mean;
      q += d * d;
    }
  return LnStats{mean, 1.0f / sqrtf(wave_sum(q) * inv_d + kLnEps)};
}

// dx = d LN(x; w) / dx applied to dy:
// g = dy w, xh = (x - mean) rstd, dx = rstd (g - mean(g) - xh mean(g xh)).
template <int VEC>
__device__ __forceinline__ void layer_norm_bwd(const float4_t (&x)[VEC], const float4_t (&dy)[VEC], const float* w,
                                               float4_t (&dx)[VEC], int lane) {
  constexpr float inv_d = 1.0f / (256 * VEC);
  const auto [mean, rstd] = ln_stats<VEC>(x);
  float4_t g[VEC], xh[VEC];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int c = 0; c < VEC; ++c) {
    const float4_t wv = *(const float4_t*)(w + 256 * c + 4 * lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      g[c][j] = dy[c][j] * wv[j];
      xh[c][j] = (x[c][j] - mean) * rstd;
      s1 += g[c][j];
      s2 += g[c][j] * xh[c][j];
    }
  }
  s1 = wave_sum(s1) * inv_d;
  s2 = wave_sum(s2) * inv_d;
#pragma unroll
  for (int c = 0; c < VEC; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) dx[c][j] = rstd * (g[c][j] - s1 - xh[c][j] * s2);
}

// host side: instantiate a launch for the two row widths of the towers
#define DISPATCH_VEC(width, ...)                            \
  switch ((width)) {                                        \
    case 768: { constexpr int V = 3; __VA_ARGS__; break; }  \
    case 1024: { constexpr int V = 4; __VA_ARGS__; break; } \
    default: return AACLIP_ERR_ARG;                         \
  }
