// What the head_dim-64 attention kernels share (attention.hip, vv_attention.hip,
// attention_bwd.hip): the softmax scale constants and the swizzled 16-bit LDS tile image.
#pragma once
#include "common.h"

constexpr float kAttnLog2Scale = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
constexpr float kLn2 = 0.69314718055994530942f;

// ds_read_b64_tr_b16: row-major 16-bit tile in, column-major fragment out
__device__ __forceinline__ short4_t tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(p));
}

// byte offset of (row, 16-B chunk) in a swizzled [64][128 B] tile
__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
