// Tiled high-resolution inference (no reference counterpart): a C x C canvas is cut into G x G
// overlapping S x S tiles, each tile goes through the tower at its native scale, and the tile
// maps are put back together on the canvas, optionally mixed with the map of a global view (the
// whole photo at S x S). The geometry, the blend weights and the outputs are stated once in
// include/aaclip.h; tests/tiled_ref.py is the same statement in numpy float64.
//
//   plan     aaclip_tile_plan (host only): per canvas coordinate of one axis the first covering
//            tile, its weight and the next tile's, and the global view's bilinear source cell and
//            its two weights; integer arithmetic, every weight computed in double and rounded
//            once to fp32. The canvas and the grid are square, so one table serves both axes.
//   gather   aaclip_tile_gather: a pure copy, canvas[b, :, oy:oy+S, ox:ox+S] -> tile row b G^2 + t.
//            One thread per four consecutive floats of the flat output: a 16-byte store whatever
//            S is (4 S is rarely a multiple of 16, so tile rows start at every alignment); the
//            source run is unaligned and is read float by float; the last 1-3 floats and a
//            misaligned output go out as floats.
//   stitch   aaclip_tile_stitch: one writer per canvas pixel, in gather form: the pixel reads
//            the one, two or four tile pixels that cover it and, with a global view, its four
//            bilinear cells. No atomics; the terms are added in one stated order, nothing is
//            contracted into an FMA. A wave owns one canvas row at a time, so the row's table
//            entry is wave-uniform and only the column's is per lane. A row is cut into the
//            16-byte groups of its own global address: the whole groups are 16-byte stores, the
//            row's head and tail (C is often odd, so a row starts at any of the four alignments)
//            go out as floats.
//   score    aaclip_tile_score: per image the maximum of its tiles' scores, mixed with the
//            global view's score.
// All three kernels are memory-bound: 256-thread blocks, at most 2048 of them, grid-stride.
#include <cmath>

#include "common.h"

namespace {

constexpr int TB = 256;          // threads per block
constexpr int MAX_BLOCKS = 2048; // 256 CUs x 8 blocks: the grid cap of a streaming kernel
constexpr int MAX_GRID = 8;      // tiles per axis

struct Geometry {
  int S, G, O, C, step;
};

bool geometry(int S, int G, int O, Geometry& g) {
  if (S < 1 || S > 16384 || G < 2 || G > MAX_GRID || O < 0 || 2 * O > S) return false;
  g = Geometry{S, G, O, G * S - (G - 1) * O, S - O};
  return true;
}

int grid_for(int64_t work_items) { return (int)std::min<int64_t>((work_items + TB - 1) / TB, MAX_BLOCKS); }

// the 1-D blend weight of tile i at local coordinate u, in double
double ramp(const Geometry& g, int i, int u) {
  if (i > 0 && u < g.O) return (u + 0.5) / g.O;
  if (i < g.G - 1 && u >= g.S - g.O) return (g.S - u - 0.5) / g.O;
  return 1.0;
}

__global__ __launch_bounds__(TB) void tile_gather_kernel(const float* __restrict__ canvas, int S, int G, int C,
                                                         int step, int tile0, int64_t n_out, int vec,
                                                         float* __restrict__ tiles) {
  const int64_t groups = (n_out + 3) / 4;
  for (int64_t grp = (int64_t)blockIdx.x * TB + threadIdx.x; grp < groups; grp += (int64_t)gridDim.x * TB) {
    const int64_t p0 = 4 * grp;
    const int cnt = (int)min((int64_t)4, n_out - p0);
    // flat output index -> (tile plane = local tile x 3 + channel, v, u)
    int plane = (int)(p0 / ((int64_t)S * S));
    int rem = (int)(p0 - (int64_t)plane * S * S);
    int v = rem / S, u = rem - v * S;
    float val[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      val[j] = 0.f;
      if (j < cnt) {
        const int tile = tile0 + plane / 3, ch = plane % 3;
        const int b = tile / (G * G), t = tile - b * G * G, ty = t / G, tx = t - ty * G;
        val[j] = canvas[((int64_t)(b * 3 + ch) * C + (ty * step + v)) * C + (tx * step + u)];
      }
      if (++u == S) {
        u = 0;
        if (++v == S) v = 0, ++plane;
      }
    }
    float* o = tiles + p0;
    if (vec && cnt == 4) {
      *(float4_t*)o = float4_t{val[0], val[1], val[2], val[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) o[j] = val[j];
    }
  }
}

// One axis of one canvas coordinate, as the kernel follows it: the table's indices are clamped
// to what exists, never followed outside (the tables come from the caller).
struct Axis {
  int u0;       // local coordinate in the first covering tile
  int f;        // that tile
  bool two;     // the next tile covers the coordinate too
  float w0, w1; // their weights
  int i0, i1;   // the global view's source cells
  float l0, l1; // and their weights
};

__device__ __forceinline__ Axis axis_entry(const int32_t* __restrict__ index, const float* __restrict__ weight,
                                           int c, int S, int G, int step) {
  Axis a;
  const float4_t w = *(const float4_t*)(weight + 4 * (int64_t)c);
  a.f = min(max(index[2 * c], 0), G - 1);
  a.u0 = min(max(c - a.f * step, 0), S - 1);
  a.w0 = w[0], a.w1 = w[1];
  a.two = w[1] != 0.f && a.f + 1 < G && a.u0 - step >= 0;
  a.i0 = min(max(index[2 * c + 1], 0), S - 1);
  a.i1 = min(a.i0 + 1, S - 1);
  a.l0 = w[2], a.l1 = w[3];
  return a;
}

// one canvas pixel: the covering tiles ty then tx, then the bilinear cells row then column, then
// the blend; every product and sum is one rounded fp32 operation
template <bool GLOBAL>
__device__ __forceinline__ float stitch_pixel(const float* __restrict__ timg, const float* __restrict__ gimg,
                                              const Axis& ay, const Axis& ax, int S, int G, int step, float keep,
                                              float alpha) {
#pragma clang fp contract(off)
  const int64_t plane = (int64_t)S * S;
  const float* r0 = timg + ((int64_t)ay.f * G + ax.f) * plane + (int64_t)ay.u0 * S + ax.u0;
  float acc = (ay.w0 * ax.w0) * r0[0];
  if (ax.two) acc += (ay.w0 * ax.w1) * r0[plane - step];
  if (ay.two) {
    const float* r1 = r0 + (int64_t)G * plane - (int64_t)step * S;
    acc += (ay.w1 * ax.w0) * r1[0];
    if (ax.two) acc += (ay.w1 * ax.w1) * r1[plane - step];
  }
  if constexpr (GLOBAL) {
    const float* g0 = gimg + (int64_t)ay.i0 * S;
    const float* g1 = gimg + (int64_t)ay.i1 * S;
    float bil = (ay.l0 * ax.l0) * g0[ax.i0];
    bil += (ay.l0 * ax.l1) * g0[ax.i1];
    bil += (ay.l1 * ax.l0) * g1[ax.i0];
    bil += (ay.l1 * ax.l1) * g1[ax.i1];
    return keep * acc + alpha * bil;
  }
  return acc;
}

template <bool GLOBAL>
__global__ __launch_bounds__(TB) void tile_stitch_kernel(const float* __restrict__ tile_maps,
                                                         const float* __restrict__ global_maps,
                                                         const int32_t* __restrict__ index,
                                                         const float* __restrict__ weight, int64_t rows, int S,
                                                         int G, int C, int step, float keep, float alpha,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (TB / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (TB / 64);
  // the alignment of the output in floats: a row's 16-byte groups are those of its address
  const int base = (int)(((uintptr_t)out >> 2) & 3);
  for (int64_t row = wave; row < rows; row += waves) {
    const int64_t b = row / C;
    const int y = (int)(row - b * C);
    const Axis ay = axis_entry(index, weight, y, S, G, step);  // wave-uniform
    const float* timg = tile_maps + b * G * G * (int64_t)S * S;
    const float* gimg = GLOBAL ? global_maps + b * (int64_t)S * S : nullptr;
    float* orow = out + row * C;
    // group k holds the row's columns [4 k - a, 4 k - a + 4), a = the row's offset into its group
    const int a = (int)((row * C + base) & 3);
    const int groups = (a + C + 3) / 4;
    for (int k = lane; k < groups; k += 64) {
      const int lo = max(4 * k - a, 0), hi = min(4 * k - a + 4, C);
      float val[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = 4 * k - a + j;
        val[j] = 0.f;
        if (x >= lo && x < hi)
          val[j] = stitch_pixel<GLOBAL>(timg, gimg, ay, axis_entry(index, weight, x, S, G, step), S, G, step, keep,
                                        alpha);
      }
      if (hi - lo == 4) {
        *(float4_t*)(orow + lo) = float4_t{val[0], val[1], val[2], val[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = 4 * k - a + j;
          if (x >= lo && x < hi) orow[x] = val[j];
        }
      }
    }
  }
}

__global__ __launch_bounds__(TB) void tile_score_kernel(const float* __restrict__ tile_scores,
                                                        const float* __restrict__ global_scores, int batch,
                                                        int tiles, float keep, float alpha,
                                                        float* __restrict__ out) {
#pragma clang fp contract(off)
  for (int b = blockIdx.x * TB + threadIdx.x; b < batch; b += gridDim.x * TB) {
    const float* s = tile_scores + (int64_t)b * tiles;
    float m = s[0];
    for (int t = 1; t < tiles; ++t) m = fmaxf(m, s[t]);
    out[b] = global_scores != nullptr ? keep * m + alpha * global_scores[b] : m;
  }
}

}  // namespace

extern "C" int aaclip_tile_plan(int S, int G, int O, int32_t* index, float* weight) {
  Geometry g;
  AACLIP_REQUIRE(index && weight && geometry(S, G, O, g));
  for (int c = 0; c < g.C; ++c) {
    const int first = c < S ? 0 : (c - S) / g.step + 1;
    const int u = c - first * g.step;
    const bool two = first + 1 < G && u >= g.step;
    index[2 * c] = first;
    weight[4 * c] = (float)ramp(g, first, u);
    weight[4 * c + 1] = two ? (float)ramp(g, first + 1, u - g.step) : 0.f;
    // half-pixel centres: source coordinate ((2 c + 1) S - C) / (2 C), clamped at 0
    const int64_t num = (int64_t)(2 * c + 1) * S - g.C, den = 2 * (int64_t)g.C;
    const int64_t i0 = num < 0 ? 0 : num / den, rem = num < 0 ? 0 : num - i0 * den;
    index[2 * c + 1] = (int32_t)i0;
    weight[4 * c + 2] = (float)((double)(den - rem) / (double)den);
    weight[4 * c + 3] = (float)((double)rem / (double)den);
  }
  return AACLIP_OK;
}

extern "C" int aaclip_tile_gather(const float* canvas, int n_images, int S, int G, int O, int64_t tile0,
                                  int64_t n_tiles, float* tiles, void* stream) {
  Geometry g;
  AACLIP_REQUIRE(canvas && tiles && n_images > 0 && geometry(S, G, O, g));
  const int64_t all_tiles = (int64_t)n_images * G * G;
  AACLIP_REQUIRE(all_tiles * 3 < (1LL << 31) && tile0 >= 0 && n_tiles > 0 && n_tiles <= all_tiles &&
                 tile0 <= all_tiles - n_tiles);
  AACLIP_REQUIRE(aligned4(canvas) && aligned4(tiles));
  const int64_t n_out = n_tiles * 3 * S * S;
  tile_gather_kernel<<<grid_for((n_out + 3) / 4), TB, 0, (hipStream_t)stream>>>(canvas, S, G, g.C, g.step, (int)tile0,
                                                                                n_out, aligned16(tiles) ? 1 : 0,
                                                                                tiles);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_tile_stitch(const float* tile_maps, const float* global_maps, const int32_t* index,
                                  const float* weight, int batch, int S, int G, int O, float global_weight,
                                  float* out, void* stream) {
  Geometry g;
  AACLIP_REQUIRE(tile_maps && index && weight && out && batch > 0 && geometry(S, G, O, g));
  AACLIP_REQUIRE(global_weight >= 0.f && global_weight < 1.f && (global_weight == 0.f || global_maps));
  AACLIP_REQUIRE(aligned4(tile_maps) && aligned4(global_maps) && aligned4(index) && aligned16(weight) &&
                 aligned4(out));
  const int64_t rows = (int64_t)batch * g.C;
  AACLIP_REQUIRE(rows < (1LL << 31));
  const int grid = grid_for(rows * 64);  // a wave per row
  const float keep = 1.0f - global_weight;
  hipStream_t s = (hipStream_t)stream;
  if (global_weight == 0.f)
    tile_stitch_kernel<false><<<grid, TB, 0, s>>>(tile_maps, nullptr, index, weight, rows, S, G, g.C, g.step, 1.0f,
                                                  0.f, out);
  else
    tile_stitch_kernel<true><<<grid, TB, 0, s>>>(tile_maps, global_maps, index, weight, rows, S, G, g.C, g.step,
                                                 keep, global_weight, out);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_tile_score(const float* tile_scores, const float* global_scores, int batch, int G,
                                 float global_weight, float* out, void* stream) {
  AACLIP_REQUIRE(tile_scores && out && batch > 0 && G >= 2 && G <= MAX_GRID);
  AACLIP_REQUIRE(global_weight >= 0.f && global_weight < 1.f && (global_weight == 0.f || global_scores));
  AACLIP_REQUIRE(aligned4(tile_scores) && aligned4(global_scores) && aligned4(out));
  tile_score_kernel<<<grid_for(batch), TB, 0, (hipStream_t)stream>>>(
      tile_scores, global_weight == 0.f ? nullptr : global_scores, batch, G * G, 1.0f - global_weight,
      global_weight, out);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
