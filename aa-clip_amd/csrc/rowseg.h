// One wave per 64-pixel row segment of a batch of images: the work layout of the component
// labelling (components.hip) and of the per-region statistics (regions.hip). A wave sees its
// segment's foreground as one __ballot word, so whatever is per run of adjacent pixels costs
// bit arithmetic, not memory traffic.
#pragma once
#include "common.h"

namespace {

constexpr int CT = 256;  // threads per block: four row-segment waves

struct Segment {  // the row segment of this wave
  bool valid;
  int img, y, x0, lane;
  size_t base;  // first pixel of the image
};

__device__ __forceinline__ Segment my_segment(int n, int H, int W) {
  const int segs = (W + 63) >> 6;
  const int64_t sid = (int64_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  const int64_t per_img = (int64_t)H * segs;
  Segment s;
  s.valid = sid < (int64_t)n * per_img;
  s.img = s.valid ? (int)(sid / per_img) : 0;
  const int64_t rem = s.valid ? sid % per_img : 0;
  s.y = (int)(rem / segs);
  s.x0 = (int)(rem % segs) << 6;
  s.lane = threadIdx.x & 63;
  s.base = (size_t)s.img * ((size_t)H * W);
  return s;
}

// first lane of the run of set bits of `row` that holds the set bit `lane`: one past the highest
// clear bit below the lane
__device__ __forceinline__ int run_start(uint64_t row, int lane) {
  const uint64_t gaps = ~row & ((1ull << lane) - 1ull);
  return gaps ? 64 - __clzll(gaps) : 0;
}

}  // namespace
