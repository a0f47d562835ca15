// Row arithmetic shared by the row kernels (rows.hip), their backwards (text_bwd.hip,
// visual_bwd.hip) and the map and loss kernels (anomaly_map.hip, segloss.hip): one definition
// of the row layout for every storage type, of the LayerNorm statistics and of the LayerNorm
// backward, so the forward and the backward agree on eps, on which lane owns which element and
// on the order every sum is taken in.
//
// One wave (64 lanes) owns one row of width 256 * VEC (768 -> VEC 3, 1024 -> VEC 4); lane l
// holds elements 256 c + 4 l .. + 3, so every load / store instruction moves one contiguous
// 1 KiB (fp32) or 512 B (16-bit) segment of the row. Registers are fp32 whatever the storage.
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
// The row at p + off elements, its storage fixed at compile time: fp32, else bf16 (widened
// exactly). For the kernels that read several rows at once: no dtype branch between the loads.
template <bool F32, int VEC>
__device__ __forceinline__ void load_row_as(const void* p, size_t off, float4_t (&v)[VEC], int lane) {
  if constexpr (F32) {
    load_row<VEC>((const float*)p + off, v, lane);
  } else {
    const uint16_t* q = (const uint16_t*)p + off;
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const uint2 r = *(const uint2*)(q + 256 * c + 4 * lane);
      v[c] = float4_t{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u),
                      __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
    }
  }
}
// The row at p, its storage (AACLIP_F32 / _BF16 / _F16) read at run time
template <int VEC>
__device__ __forceinline__ void load_any(const void* p, int dtype, float4_t (&v)[VEC], int lane) {
  if (dtype == AACLIP_F32) {
    load_row_as<true, VEC>(p, 0, v, lane);
  } else if (dtype == AACLIP_F16) {
    const uint16_t* q = (const uint16_t*)p;
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      uint2 r = *(const uint2*)(q + 256 * c + 4 * lane);
      v[c][0] = f16_to_f32((uint16_t)(r.x & 0xffff));
      v[c][1] = f16_to_f32((uint16_t)(r.x >> 16));
      v[c][2] = f16_to_f32((uint16_t)(r.y & 0xffff));
      v[c][3] = f16_to_f32((uint16_t)(r.y >> 16));
    }
  } else {
    load_row_as<false, VEC>(p, 0, v, lane);
  }
}
template <int VEC>
__device__ __forceinline__ void store_any(void* p, int dtype, const float4_t (&v)[VEC], int lane) {
  if (dtype == AACLIP_F32) {
    store_row<VEC>((float*)p, v, lane);
  } else {
    const bool h = dtype == AACLIP_F16;
    uint16_t* q = (uint16_t*)p;
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      uint2 r;
      r.x = h ? pack_f16x2(v[c][0], v[c][1]) : pack_bf16x2(v[c][0], v[c][1]);
      r.y = h ? pack_f16x2(v[c][2], v[c][3]) : pack_bf16x2(v[c][2], v[c][3]);
      *(uint2*)(q + 256 * c + 4 * lane) = r;
    }
  }
}

// The lane's 12 channels of the interleaved text-anchor pair T [768][2] (C = 768 = 3 x 256):
// t0 / t1 = normal / abnormal.
__device__ __forceinline__ void load_anchors(const float* T, float4_t (&t0)[3], float4_t (&t1)[3], int lane) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* tp = T + 2 * (256 * c + 4 * lane);
    float4_t a = *(const float4_t*)tp, b = *(const float4_t*)(tp + 4);
    t0[c] = float4_t{a[0], a[2], b[0], b[2]};
    t1[c] = float4_t{a[1], a[3], b[1], b[3]};
  }
}

// Index of the EOT token of sequence s of tokens [n_seq][ctx]: the first argmax of its ctx token
// ids (EOT = 49407 is the largest id), ties to the lower index; every lane of the wave returns it.
__device__ __forceinline__ int eot_index(const int32_t* tokens, int s, int ctx, int lane) {
  int best_v = -2147483647 - 1, best_i = 0;
  for (int t = lane; t < ctx; t += 64) {
    const int v = tokens[(size_t)s * ctx + t];
    if (v > best_v) { best_v = v; best_i = t; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(best_v, o, 64);
    const int oi = __shfl_xor(best_i, o, 64);
    if (ov > best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
  }
  return best_i;
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
