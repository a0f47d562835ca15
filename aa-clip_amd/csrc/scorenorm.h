// The class normalisation of the pixel maps (reference forward_utils.py:241-242 in numpy float32
// semantics) and the order-preserving score keys, shared by the device metrics (metrics.hip) and the
// region extraction (regions.hip): one formula, so a threshold that the metrics report means the
// same pixels to whoever applies it.
#pragma once
#include "common.h"

namespace {

constexpr int MT = 256;  // threads per block for the element-wise passes

__device__ __forceinline__ float block_min(float v, float* sh) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  v = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) v = fminf(v, sh[i]);
  return v;
}
__device__ __forceinline__ float block_max(float v, float* sh) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  v = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) v = fmaxf(v, sh[i]);
  return v;
}

// per-image min / max of the raw maps (one block per image)
__global__ __launch_bounds__(MT) void row_minmax_kernel(const float* __restrict__ p, int64_t pix,
                                                        float* __restrict__ rmin, float* __restrict__ rmax) {
  __shared__ float sh[MT / 64];
  const float* row = p + (size_t)blockIdx.x * pix;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = threadIdx.x; i < pix; i += MT) {
    const float v = row[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  lo = block_min(lo, sh);
  hi = block_max(hi, sh);
  if (threadIdx.x == 0) {
    rmin[blockIdx.x] = lo;
    rmax[blockIdx.x] = hi;
  }
}

// the class's min / max from the per-image ones (whole block; every thread gets both)
__device__ __forceinline__ void class_minmax(const float* __restrict__ rmin, const float* __restrict__ rmax,
                                             int n_img, float* sh, float& lo, float& hi) {
  lo = INFINITY;
  hi = -INFINITY;
  for (int i = threadIdx.x; i < n_img; i += MT) {
    lo = fminf(lo, rmin[i]);
    hi = fmaxf(hi, rmax[i]);
  }
  lo = block_min(lo, sh);
  hi = block_max(hi, sh);
}

struct Norm {  // numpy float32 semantics of forward_utils.py:241-248
  float pmin, pmax, imin, imax;
  int pnorm, inorm;
};

// a set of scores is min-max normalised unless its maximum is exactly 1
__device__ __forceinline__ bool norm_wanted(float hi) { return hi != 1.0f; }
__device__ __forceinline__ float norm_apply(float x, float lo, float hi) { return (x - lo) / (hi - lo); }
// the class-normalised value of a raw map pixel
__device__ __forceinline__ float pixel_score(float x, const Norm& z) {
  return z.pnorm ? norm_apply(x, z.pmin, z.pmax) : x;
}

// order-preserving uint32 image of a float (+0 and -0 map to the same key)
__device__ __forceinline__ uint32_t ord_bits(float v) {
  if (v == 0.0f) v = 0.0f;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the inverse of ord_bits
__device__ __forceinline__ float ord_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

}  // namespace
