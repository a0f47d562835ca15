// Stage-2 backward in bf16 mixed precision: the c_fc activation and its backward with 16-bit
// I/O, and the row cast between the fp32 gradient stream and the 16-bit GEMM inputs. The
// attention backward on bf16 MFMA is attention_bwd.hip; everything else of the bf16 step is
// aaclip_gemm in bf16 on the transposed weights and the fp32 row kernels of text_bwd.hip /
// visual_bwd.hip.
//
// Deterministic (no atomics, fixed reduction orders: two launches give the same bits) and
// image / row local, as visual_bwd.hip.
#include "common.h"

namespace {

// ------------------------------------------------------------------ activations, 16-bit I/O
// 8 elements per thread (two float4 in, one 16-B vector out); the last n % 8 by one thread.
__device__ __forceinline__ float2_t act16_pair(int mode, float2_t v) {
  if (mode == AACLIP_EPI_GELU) return gelu_fast2(v);
  if (mode == AACLIP_EPI_QGELU) return qgelu_fast2(v);
  return float2_t{leaky_relu(v[0]), leaky_relu(v[1])};
}

template <bool H16>
__global__ __launch_bounds__(256) void act_to16_kernel(int mode, const float* __restrict__ x,
                                                       uint16_t* __restrict__ y, size_t n) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= n) return;
  if (i + 8 <= n) {
    const float4_t a = *(const float4_t*)(x + i), b = *(const float4_t*)(x + i + 4);
    const float2_t r0 = act16_pair(mode, float2_t{a[0], a[1]}), r1 = act16_pair(mode, float2_t{a[2], a[3]});
    const float2_t r2 = act16_pair(mode, float2_t{b[0], b[1]}), r3 = act16_pair(mode, float2_t{b[2], b[3]});
    *(uint4*)(y + i) = uint4{pack_h16x2<H16>(r0[0], r0[1]), pack_h16x2<H16>(r1[0], r1[1]),
                             pack_h16x2<H16>(r2[0], r2[1]), pack_h16x2<H16>(r3[0], r3[1])};
  } else {
    for (size_t j = i; j < n; ++j) {
      const float2_t r = act16_pair(mode, float2_t{x[j], x[j]});
      y[j] = (uint16_t)(pack_h16x2<H16>(r[0], r[0]) & 0xffffu);
    }
  }
}

// The derivative is aaclip_act_bwd's (common.h act_slope: the exact erf / sigmoid forms). The
// forward's gelu_fast2 is within 2.6e-5 absolute of the erf form, an order below the bf16
// rounding of dx.
template <bool H16>
__global__ __launch_bounds__(256) void act_bwd16_kernel(int mode, const uint16_t* dy, const float* __restrict__ ref,
                                                        uint16_t* dx, size_t n) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= n) return;
  if (i + 8 <= n) {
    const uint4 d = *(const uint4*)(dy + i);
    const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
    const float4_t a = *(const float4_t*)(ref + i), b = *(const float4_t*)(ref + i + 4);
    const float rv[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    uint32_t o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float lo = h16_to_f32<H16>((uint16_t)(dw[p] & 0xffffu)) * act_slope(mode, rv[2 * p]);
      const float hi = h16_to_f32<H16>((uint16_t)(dw[p] >> 16)) * act_slope(mode, rv[2 * p + 1]);
      o[p] = pack_h16x2<H16>(lo, hi);
    }
    *(uint4*)(dx + i) = uint4{o[0], o[1], o[2], o[3]};
  } else {
    for (size_t j = i; j < n; ++j) {
      const float v = h16_to_f32<H16>(dy[j]) * act_slope(mode, ref[j]);
      dx[j] = (uint16_t)(pack_h16x2<H16>(v, v) & 0xffffu);
    }
  }
}

// ------------------------------------------------------------------ row cast
// y[r][c] = (out type) x[r][c], 8 columns per thread: fp32 -> 16-bit rounds to nearest even (the
// GEMM epilogue's conversion), 16-bit -> fp32 is exact.
template <bool H16>
__global__ __launch_bounds__(256) void cast_rows_down_kernel(const float* __restrict__ x, int64_t ldx,
                                                             uint16_t* __restrict__ y, int64_t ldy, int rows,
                                                             int cols8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * cols8) return;
  const size_t r = i / cols8, c = (i % cols8) * 8;
  const float4_t a = *(const float4_t*)(x + r * ldx + c), b = *(const float4_t*)(x + r * ldx + c + 4);
  *(uint4*)(y + r * ldy + c) = uint4{pack_h16x2<H16>(a[0], a[1]), pack_h16x2<H16>(a[2], a[3]),
                                     pack_h16x2<H16>(b[0], b[1]), pack_h16x2<H16>(b[2], b[3])};
}
template <bool H16>
__global__ __launch_bounds__(256) void cast_rows_up_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                           float* __restrict__ y, int64_t ldy, int rows,
                                                           int cols8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * cols8) return;
  const size_t r = i / cols8, c = (i % cols8) * 8;
  const uint4 d = *(const uint4*)(x + r * ldx + c);
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  float4_t o[2];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    o[p >> 1][2 * (p & 1)] = h16_to_f32<H16>((uint16_t)(w[p] & 0xffffu));
    o[p >> 1][2 * (p & 1) + 1] = h16_to_f32<H16>((uint16_t)(w[p] >> 16));
  }
  *(float4_t*)(y + r * ldy + c) = o[0];
  *(float4_t*)(y + r * ldy + c + 4) = o[1];
}

inline bool is16(int dtype) { return dtype == AACLIP_BF16 || dtype == AACLIP_F16; }
}  // namespace

extern "C" int aaclip_act_to16(int mode, const float* x, void* y, int out_dtype, int64_t n, void* stream) {
  AACLIP_REQUIRE(x && y && n >= 0 && act_mode_ok(mode) && is16(out_dtype));
  AACLIP_REQUIRE((const void*)x != y && aligned16(x) && aligned16(y));
  if (n == 0) return AACLIP_OK;
  const unsigned blocks = (unsigned)((n + 2047) / 2048);
  if (out_dtype == AACLIP_F16)
    act_to16_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, x, (uint16_t*)y, (size_t)n);
  else
    act_to16_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, x, (uint16_t*)y, (size_t)n);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_act_bwd16(int mode, const void* dy, const float* ref, void* dx, int dtype, int64_t n,
                                void* stream) {
  AACLIP_REQUIRE(dy && ref && dx && n >= 0 && act_mode_ok(mode) && is16(dtype));
  AACLIP_REQUIRE((const void*)ref != dx && aligned16(dy) && aligned16(ref) && aligned16(dx));
  if (n == 0) return AACLIP_OK;
  const unsigned blocks = (unsigned)((n + 2047) / 2048);
  if (dtype == AACLIP_F16)
    act_bwd16_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, (const uint16_t*)dy, ref, (uint16_t*)dx,
                                                                    (size_t)n);
  else
    act_bwd16_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, (const uint16_t*)dy, ref, (uint16_t*)dx,
                                                                     (size_t)n);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_cast_rows(int in_dtype, int out_dtype, const void* x, int64_t ldx, void* y, int64_t ldy,
                                int rows, int cols, void* stream) {
  AACLIP_REQUIRE(x && y && rows >= 0 && cols > 0 && cols % 8 == 0 && x != y);
  AACLIP_REQUIRE((in_dtype == AACLIP_F32 && is16(out_dtype)) || (is16(in_dtype) && out_dtype == AACLIP_F32));
  const bool down = in_dtype == AACLIP_F32;
  // 16-B vectors on both sides: fp32 rows a multiple of 4 elements apart, 16-bit rows of 8
  AACLIP_REQUIRE(ldx >= cols && ldy >= cols && ldx % (down ? 4 : 8) == 0 && ldy % (down ? 8 : 4) == 0);
  AACLIP_REQUIRE(aligned16(x) && aligned16(y));
  if (rows == 0) return AACLIP_OK;
  const int cols8 = cols / 8;
  const size_t total = (size_t)rows * cols8;
  AACLIP_REQUIRE(total < ((size_t)1 << 39));
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  const bool h16 = (down ? out_dtype : in_dtype) == AACLIP_F16;
  if (down) {
    if (h16) cast_rows_down_kernel<true><<<blocks, 256, 0, s>>>((const float*)x, ldx, (uint16_t*)y, ldy, rows, cols8);
    else cast_rows_down_kernel<false><<<blocks, 256, 0, s>>>((const float*)x, ldx, (uint16_t*)y, ldy, rows, cols8);
  } else {
    if (h16) cast_rows_up_kernel<true><<<blocks, 256, 0, s>>>((const uint16_t*)x, ldx, (float*)y, ldy, rows, cols8);
    else cast_rows_up_kernel<false><<<blocks, 256, 0, s>>>((const uint16_t*)x, ldx, (float*)y, ldy, rows, cols8);
  }
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
