// Shared device helpers for the AA-CLIP gfx950 kernels.
// Wave = 64 lanes (CDNA); every reduction below is written for 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/aaclip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(8))) short short8_t;
typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((ext_vector_type(4))) float float4_t;
typedef __attribute__((ext_vector_type(2))) float float2_t;

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// ---------------------------------------------------------------- bf16 <-> f32
__device__ __forceinline__ float bf16_to_f32(uint16_t h) {
  return __uint_as_float(((uint32_t)h) << 16);
}
// round-to-nearest-even; a plain cast lowers to v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(uint16_t, b);
}
// one v_cvt_pk_bf16_f32 (RNE) for the pair; the scalar form costs 2 cvt + shift + or
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2v_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){lo, hi}, bf16x2v_t));
}

// ---------------------------------------------------------------- fp16 <-> f32
// fp16 (IEEE binary16, 11 significant bits) is the parity-grade 16-bit storage:
// same MFMA rate as bf16 (v_mfma_f32_16x16x32_f16), 8x finer rounding. One
// v_cvt_pk_f16_f32 (RNE) per pair on gfx950.
__device__ __forceinline__ float f16_to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ uint16_t f32_to_f16(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2v_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){lo, hi}, f16x2v_t));
}

// 16-bit storage flavour chosen at compile time: H16 = false -> bf16, true -> fp16
template <bool H16>
__device__ __forceinline__ uint32_t pack_h16x2(float lo, float hi) {
  if constexpr (H16) return pack_f16x2(lo, hi);
  else return pack_bf16x2(lo, hi);
}
template <bool H16>
__device__ __forceinline__ float h16_to_f32(uint16_t h) {
  if constexpr (H16) return f16_to_f32(h);
  else return bf16_to_f32(h);
}
template <bool H16>
using h16x8_t = typename std::conditional<H16, f16x8_t, bf16x8_t>::type;
template <bool H16>
using h16_t = typename std::conditional<H16, _Float16, __bf16>::type;

// C^T-tile MFMA on 16-bit operands (bf16 or fp16 by overload; same cycles)
__device__ __forceinline__ float4_t mfma16(const bf16x8_t& a, const bf16x8_t& b, const float4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float4_t mfma16(const f16x8_t& a, const f16x8_t& b, const float4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------- wave reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------- bilinear taps / channel softmax
// ATen upsample_bilinear2d, align_corners=True, one axis: src = scale * dst in fp32
// (scale = (g - 1) / (S - 1), rounded once on the host), rounded before the lambdas:
// no FMA contraction. Shared by the forward (blur_band) and its backward
// (upsample_softmax_bwd_kernel), so both put every pixel on the same source cells
// with the same weights, bit for bit.
__device__ __forceinline__ void bilinear_tap(float scale, int dst, int g, int& i0, int& i1, float& w0, float& w1) {
#pragma clang fp contract(off)
  const float s = scale * (float)dst;
  i0 = (int)s;
  i1 = i0 + (i0 < g - 1 ? 1 : 0);
  w1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
  w0 = 1.0f - w1;
}
// torch.softmax over the C channels of pixel slot p, in place (max, exp, sum in channel
// order, one reciprocal).
template <int C, int N>
__device__ __forceinline__ void softmax_channels(float (&v)[C][N], int p) {
#pragma clang fp contract(off)
  float m = v[0][p];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, v[c][p]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    v[c][p] = expf(v[c][p] - m);
    sum += v[c][p];
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int c = 0; c < C; ++c) v[c][p] *= inv;
}

// ---------------------------------------------------------------- fp32 activations
// The exact forms the fp32 GEMM epilogue applies (gemm.hip epilogue_store1). Shared with the
// elementwise aaclip_act (text_bwd.hip), which the training forward runs on a stored c_fc
// pre-activation: the same function on the same value, so the training forward's bits are
// the eval path's.
__device__ __forceinline__ float gelu_erf(float v) {
  return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
}
// QuickGELU (reference transformer.py:46-49: x * sigmoid(1.702 x)). Exact form for the
// fp32 parity kernel: the same expf/division as torch.sigmoid's fp32 CPU path.
__device__ __forceinline__ float qgelu_exact(float v) { return v * (1.0f / (1.0f + expf(-1.702f * v))); }
// nn.LeakyReLU(0.01), written as the epilogue writes it
__device__ __forceinline__ float leaky_relu(float v) { return v >= 0.f ? v : 0.01f * v; }
// The derivative of the activation `mode` (its GEMM epilogue flag, AACLIP_EPI_GELU / _QGELU /
// _LEAKY) at the reference value v, for aaclip_act_bwd and aaclip_act_bwd16. GELU / QuickGELU:
// v = the pre-activation; gelu'(v) = Phi(v) + v phi(v), quick'(v) = s + 1.702 v s (1 - s),
// s = sigmoid(1.702 v). LeakyReLU: v = the OUTPUT (its sign is the input's); slope 1 above 0,
// 0.01 at and below 0 (torch's leaky_relu_backward).
__device__ __forceinline__ float act_slope(int mode, float v) {
  if (mode == AACLIP_EPI_GELU) {
    const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
    return cdf + v * (0.39894228040143267794f * expf(-0.5f * v * v));
  }
  if (mode == AACLIP_EPI_QGELU) {
    const float s = 1.0f / (1.0f + expf(-1.702f * v));
    return s + 1.702f * v * s * (1.0f - s);
  }
  return v > 0.f ? 1.0f : 0.01f;
}
// host side: the modes the elementwise activation entry points accept
inline bool act_mode_ok(int mode) {
  return mode == AACLIP_EPI_GELU || mode == AACLIP_EPI_QGELU || mode == AACLIP_EPI_LEAKY;
}

// ---------------------------------------------------------------- 16-bit activations
// The forms the 16-bit GEMM epilogues apply (gemm.hip wave_epilogue / wave_epilogue_lds). Shared
// with aaclip_act_to16 (visual_bwd16.hip), which the bf16 training forward runs on a stored fp32
// c_fc pre-activation: the same function on the same value, so its bits are the eval path's.
// GELU for the bf16-input kernel: v * sigmoid(v * P(v^2)), P quadratic, fitted
// (minimax on [-12, 12]) to the erf form: |error| <= 2.6e-5 absolute, an order
// below the bf16 rounding of the output for |y| >= 0.01. The clamp keeps the
// quintic in its monotone range (|v| > 8: sigmoid is 0/1 to 1e-12). 7 VALU + one
// v_exp + one v_rcp per element, vs 16 + 2 for an erfc-polynomial form; the c_fc
// epilogue is VALU-bound (all waves of the chip run it at once, no MFMA to hide
// behind). -log2(e) is folded into the coefficients so v_exp_f32 (2^x) applies
// directly. The fp32 parity kernel keeps the exact erff form (gelu_erf, common.h).
__device__ __forceinline__ float gelu_fast(float v) {
  const float vc = __builtin_amdgcn_fmed3f(v, -8.0f, 8.0f);
  const float s = vc * vc;
  const float w = vc * fmaf(s, fmaf(s, 0.0010142630f, -0.10677572f), -2.3011212f);
  return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(w));
}

// gelu_fast on a column pair in packed f32 arithmetic (v_pk_mul/v_pk_fma/v_pk_add: two
// elements per VALU issue; the epilogue runs with no MFMA beside it, so the packed
// forms are pure savings here): 2 v_med3 + 5 packed + 2 v_exp + 2 v_rcp per pair,
// the same roundings as gelu_fast element by element.
__device__ __forceinline__ float2_t gelu_fast2(float2_t v) {
  const float2_t vc = {__builtin_amdgcn_fmed3f(v[0], -8.0f, 8.0f), __builtin_amdgcn_fmed3f(v[1], -8.0f, 8.0f)};
  const float2_t s = vc * vc;
  const float2_t c2 = {0.0010142630f, 0.0010142630f}, c1 = {-0.10677572f, -0.10677572f},
                 c0 = {-2.3011212f, -2.3011212f}, one = {1.0f, 1.0f};
  const float2_t w = vc * __builtin_elementwise_fma(s, __builtin_elementwise_fma(s, c2, c1), c0);
  const float2_t d = float2_t{__builtin_amdgcn_exp2f(w[0]), __builtin_amdgcn_exp2f(w[1])} + one;
  return v * float2_t{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}

// 16-bit kernels, a column pair in packed f32: v * rcp(1 + 2^(-1.702 log2(e) v)); the
// argument is clamped to |.| <= 64 (exp2 stays finite, sigmoid is 0/1 to 1e-19 there).
// |error| vs qgelu_exact <= 2 ulp of v (1.2 measured), which is 2 ulp of the result for v >= 0;
// for v < 0 the rounding of the exponent's argument is amplified by its size, so in ulp of the
// (tiny) result it is 2.8 on [-2, 0), 4.8 at v = -6, 8.4 at v = -12 (tests/test_gemm_host.py):
// still far below the 16-bit rounding of the output.
__device__ __forceinline__ float2_t qgelu_fast2(float2_t v) {
  constexpr float c = -1.702f * 1.44269504088896340736f;
  const float2_t w = float2_t{__builtin_amdgcn_fmed3f(v[0] * c, -64.0f, 64.0f),
                              __builtin_amdgcn_fmed3f(v[1] * c, -64.0f, 64.0f)};
  const float2_t d = float2_t{__builtin_amdgcn_exp2f(w[0]), __builtin_amdgcn_exp2f(w[1])} + float2_t{1.0f, 1.0f};
  return v * float2_t{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}

// ---------------------------------------------------------------- launch checking
#define AACLIP_CHECK_LAUNCH()                                 \
  do {                                                        \
    hipError_t _e = hipGetLastError();                        \
    if (_e != hipSuccess) return AACLIP_ERR_LAUNCH + (int)_e; \
  } while (0)

#define AACLIP_REQUIRE(cond) \
  do {                       \
    if (!(cond)) return AACLIP_ERR_ARG; \
  } while (0)

// Dynamic-LDS opt-in for a kernel, once per device: the attribute lives in the
// current device's context, so a process driving several GPUs sets it on each.
// `done` is the call site's bitmask of devices already set (a race between host
// threads only repeats the idempotent attribute write).
inline bool lds_attr_once(const void* fn, int bytes, unsigned& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const unsigned bit = (dev >= 0 && dev < 32) ? 1u << dev : 0u;
  if (bit && (done & bit)) return true;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
  done |= bit;
  return true;
}

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// host-side argument checks: what a 16-B (float4) / 4-B access of the pointer needs
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// ---------------------------------------------------------------- step timeline (diagnostic)
// Built only with -DAACLIP_TRACE (`make trace` -> libaaclip_hip_trace.so; the product
// library compiles none of this): every wave of an instrumented kernel appends one
// record {t0, t1 (s_memrealtime, the chip-wide 100 MHz clock), tag, HW_ID, XCC_ID | the
// wave's shader-clock cycles (s_memtime delta) << 4, workgroup} to a caller-provided
// device buffer (aaclip_trace_buffer), so a tool can rebuild which CU ran what when over
// a whole concurrent step, and at what clock (tools/timeline.py).
// Records go to a per-CU slab (slot = XCC, SE, SH, CU: 2048 slots) through a per-slot
// counter 64 B apart: one counter for the whole chip serialised ~1.7 M same-address
// atomics per step and doubled the step time. Written with vector stores after the
// wave's own last memory op.
enum TraceTag : uint32_t {
  TR_GEMM_8PH = 1, TR_GEMM_TILE = 2, TR_GEMM_FP8MX = 3, TR_ATTN = 4, TR_LAYERNORM = 5, TR_BLOCK_TAIL = 6,
  TR_EMBED_LN = 7, TR_IM2COL = 8, TR_PARTIAL_SCORES = 9, TR_BLUR_SCORE = 10, TR_GEMM_F32 = 11, TR_ATTN_F32 = 12,
  TR_PATCH_SCORES = 13, TR_BLUR = 14, TR_DET = 15
};
constexpr int kTraceSlots = 2048;  // XCC (3 bits) x SE (3) x SH (1) x CU (4)
#ifdef AACLIP_TRACE
struct TraceState {
  uint32_t* rec;   // [kTraceSlots][cap][8] uint32
  uint32_t* count; // [kTraceSlots][16] uint32 (slot counters, one per 64 B)
  uint32_t cap;    // records per slot
};
static __device__ TraceState g_trace;
struct TraceScope {
  uint64_t t0, c0;
  uint32_t tag;
  __device__ __forceinline__ explicit TraceScope(uint32_t tag_) : tag(tag_) {
    t0 = __builtin_amdgcn_s_memrealtime();
    c0 = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ ~TraceScope() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    const uint64_t dc = __builtin_amdgcn_s_memtime() - c0;  // shader cycles over the same span
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if ((threadIdx.x & 63) == 0 && g_trace.rec) {
      const uint32_t slot = ((xcc & 7) << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
      const uint32_t i = atomicAdd(g_trace.count + slot * 16, 1u);
      if (i < g_trace.cap) {
        const uint32_t wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        uint4* r = (uint4*)(g_trace.rec + ((size_t)slot * g_trace.cap + i) * 8);
        r[0] = uint4{(uint32_t)t0, (uint32_t)(t0 >> 32), (uint32_t)t1, (uint32_t)(t1 >> 32)};
        r[1] = uint4{tag, hw, (xcc & 15) | ((uint32_t)min(dc, (uint64_t)0xFFFFFFF) << 4), wg};
      }
    }
  }
};
#define AACLIP_TRACE_SCOPE(tag) TraceScope _aaclip_trace_scope(tag)
// one per translation unit: points this TU's g_trace at the buffer (host side)
#define AACLIP_TRACE_SETTER(name)                                                          \
  int name(void* rec, void* count, unsigned cap) {                                        \
    TraceState t{(uint32_t*)rec, (uint32_t*)count, cap};                                  \
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &t, sizeof t) == hipSuccess ? 0 : -1;  \
  }
#else
#define AACLIP_TRACE_SCOPE(tag) ((void)0)
#define AACLIP_TRACE_SETTER(name)
#endif
