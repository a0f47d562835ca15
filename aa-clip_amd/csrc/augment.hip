// Training-time augmentation on the device (replaces the per-item CPU transforms of the
// reference's train split, dataset/__init__.py:30-52, 89-94).
//
//   aaclip_color_jitter_u8   ColorJitter(brightness) -> (contrast) -> (saturation) on decoded
//                            uint8 RGB, i.e. Pillow's ImageEnhance.Brightness / .Contrast / .Color,
//                            each an Image.blend(degenerate, image, f): per channel
//                            t = d + f * (i - d) in fp32 (no contraction), truncated for
//                            0 <= f <= 1, clipped to [0, 255] and truncated otherwise.
//   aaclip_geom_augment      RandomRotation -> RandomAffine(translate) -> horizontal flip ->
//                            vertical flip of the fp32 image + mask planes, nearest with fill 0,
//                            as ONE gather through the composed index map.
//
// Both are memory bound. Per-image parameters are host arrays: they are validated before the
// first launch and travel as kernel arguments, CHUNK images per launch, so nothing is copied,
// allocated or synchronised and the calls can be captured into a graph.
//
// Bytes moved per image
//   jitter reduce (only images whose contrast factor != 1): reads 3 H W.
//   jitter apply: reads 3 H W, writes 3 H W (+ RED_BLOCKS * 8 B of partial sums).
//     -> 9 H W bytes with contrast, 6 H W without, 0 when all three factors are 1 (dst == src).
//   geometry: writes 4 C S^2, reads at most 4 C S^2 (less by the zero-filled share).
//
// The contrast mean is a whole-image integer reduction: the reduce kernel writes RED_BLOCKS
// 64-bit partial sums per image, every block of the apply kernel adds them up again (2 KB
// from L2). Integer sums are exact in any order, so the result is deterministic; a 64-bit
// sum of values <= 255 cannot overflow for any H * W below 2^56.
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 64;       // images per launch (their parameters are kernel arguments)
constexpr int RED_BLOCKS = NT;  // partial sums per image: each apply block adds them up, one per thread
constexpr int MAX_BLOCKS = 2048;

struct JitterArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t img_stride, pitch;
  int H, W, b0, vec;
  unsigned long long* partial;  // [batch][RED_BLOCKS]
  float f[CHUNK][3];            // brightness, contrast, saturation
};

// Pillow ImagingBlend(degenerate, image, f) for one channel
__device__ __forceinline__ int blend(int d, int i, float f) {
#pragma clang fp contract(off)
  const float t = (float)d + f * (float)(i - d);
  if (f >= 0.f && f <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// Pillow's RGB -> L
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// n (1..4) pixels at p into px[12]; vec: p is 4-byte aligned and n == 4 is read as three dwords
__device__ __forceinline__ void load_group(const uint8_t* p, int n, bool vec, uint8_t (&px)[12]) {
  if (vec && n == 4) {
    const uint32_t* q = (const uint32_t*)p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t w = q[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) px[4 * k + e] = (uint8_t)(w >> (8 * e));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < 3 * n) px[k] = p[k];
  }
}

__device__ __forceinline__ void store_group(uint8_t* p, int n, bool vec, const uint8_t (&px)[12]) {
  if (vec && n == 4) {
    uint32_t* q = (uint32_t*)p;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      q[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) |
             ((uint32_t)px[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < 3 * n) p[k] = px[k];
  }
}

// sum of L over the image after the brightness step -> partial[b][blockIdx.x].
// Bytes per image: reads 3 H W, writes RED_BLOCKS * 8; nothing for an image whose contrast factor is 1.
__global__ __launch_bounds__(NT) void jitter_reduce_kernel(JitterArgs a) {
  const int lb = blockIdx.y, b = a.b0 + lb;
  const float fb = a.f[lb][0], fc = a.f[lb][1];
  if (fc == 1.f) return;  // contrast not applied: nobody reads this image's partials
  const uint8_t* img = a.src + (size_t)b * a.img_stride;
  const int G = (a.W + 3) >> 2;
  const size_t items = (size_t)a.H * G;
  unsigned long long s = 0;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < items; it += (size_t)gridDim.x * NT) {
    const int y = (int)(it / G), g = (int)(it - (size_t)y * G);
    const int n = min(4, a.W - 4 * g);
    uint8_t px[12] = {};
    load_group(img + (size_t)y * a.pitch + 12 * (size_t)g, n, a.vec, px);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= n) break;
      int r = px[3 * k], gg = px[3 * k + 1], bl = px[3 * k + 2];
      if (fb != 1.f) {
        r = blend(0, r, fb);
        gg = blend(0, gg, fb);
        bl = blend(0, bl, fb);
      }
      s += (unsigned)luma(r, gg, bl);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ unsigned long long part[NT / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < NT / 64; ++w) t += part[w];
    a.partial[(size_t)b * RED_BLOCKS + blockIdx.x] = t;
  }
}

// brightness -> contrast -> saturation of every pixel. Bytes per image: reads 3 H W (+ the 2 KB of
// partial sums per block, from L2), writes 3 H W; nothing for an identity in place.
__global__ __launch_bounds__(NT) void jitter_apply_kernel(JitterArgs a) {
  const int lb = blockIdx.y, b = a.b0 + lb;
  const float fb = a.f[lb][0], fc = a.f[lb][1], fs = a.f[lb][2];
  if (fb == 1.f && fc == 1.f && fs == 1.f && a.dst == a.src) return;  // identity in place
  __shared__ unsigned long long part[NT / 64];
  __shared__ int mean_s;
  if (fc != 1.f) {  // uniform over the block
    unsigned long long s = a.partial[(size_t)b * RED_BLOCKS + threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < NT / 64; ++w) t += part[w];
      // ImageEnhance.Contrast: int(ImageStat.Stat(L).mean[0] + 0.5), the division in fp64
      mean_s = (int)((double)t / ((double)a.H * (double)a.W) + 0.5);
    }
    __syncthreads();
  }
  const int mean = fc != 1.f ? mean_s : 0;
  const uint8_t* img = a.src + (size_t)b * a.img_stride;
  uint8_t* out = a.dst + (size_t)b * a.img_stride;
  const int G = (a.W + 3) >> 2;
  const size_t items = (size_t)a.H * G;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < items; it += (size_t)gridDim.x * NT) {
    const int y = (int)(it / G), g = (int)(it - (size_t)y * G);
    const int n = min(4, a.W - 4 * g);
    const size_t off = (size_t)y * a.pitch + 12 * (size_t)g;
    uint8_t px[12] = {};
    load_group(img + off, n, a.vec, px);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= n) break;
      int c[3] = {px[3 * k], px[3 * k + 1], px[3 * k + 2]};
      if (fb != 1.f)
        for (int e = 0; e < 3; ++e) c[e] = blend(0, c[e], fb);
      if (fc != 1.f)
        for (int e = 0; e < 3; ++e) c[e] = blend(mean, c[e], fc);
      if (fs != 1.f) {
        const int l = luma(c[0], c[1], c[2]);
        for (int e = 0; e < 3; ++e) c[e] = blend(l, c[e], fs);
      }
      for (int e = 0; e < 3; ++e) px[3 * k + e] = (uint8_t)c[e];
    }
    store_group(out + off, n, a.vec, px);
  }
}

struct GeomArgs {
  const float* src;
  const float* src2;
  float* dst;
  float* dst2;
  int C, C2, S, b0;
  int tx[CHUNK], ty[CHUNK];
  float a[CHUNK], b[CHUNK];  // cos r / (0.5 S), sin r / (0.5 S)
  uint8_t flags[CHUNK];      // 1 rotate, 2 hflip, 4 vflip
};

// one thread per output pixel: the source index once, then every channel through it.
// Bytes per image: writes 4 (C + C2) S^2 (coalesced), reads at most as much (a gather: along rotated
// lines each wave takes a few bytes from many cache lines).
__global__ __launch_bounds__(NT) void geom_kernel(GeomArgs g) {
#pragma clang fp contract(off)
  const int lb = blockIdx.y, S = g.S;
  const size_t bimg = (size_t)(g.b0 + lb), plane = (size_t)S * S;
  const int fl = g.flags[lb], tx = g.tx[lb], ty = g.ty[lb];
  const float ca = g.a[lb], sb = g.b[lb], Sf = (float)S, half = 0.5f * Sf;
  for (size_t p = (size_t)blockIdx.x * NT + threadIdx.x; p < plane; p += (size_t)gridDim.x * NT) {
    const int i = (int)(p / S), j = (int)(p - (size_t)i * S);
    const int i1 = (fl & 4) ? S - 1 - i : i, j1 = (fl & 2) ? S - 1 - j : j;
    int si = i1 - ty, sj = j1 - tx;  // |tx|, |ty| <= S (clamped on the host): no overflow
    bool ok = si >= 0 && si < S && sj >= 0 && sj < S;
    if (ok && (fl & 1)) {
      // torchvision's tensor rotate: _gen_affine_grid, then grid_sample(nearest, zeros,
      // align_corners=False); halves round to even (nearbyint)
      const float xb = (float)sj + 0.5f - half, yb = (float)si + 0.5f - half;
      const float gx = xb * ca + yb * sb;
      const float gy = xb * (-sb) + yb * ca;
      const float x = rintf(((gx + 1.f) * Sf - 1.f) / 2.f), y = rintf(((gy + 1.f) * Sf - 1.f) / 2.f);
      ok = x >= 0.f && x < Sf && y >= 0.f && y < Sf;  // false for NaN
      sj = ok ? (int)x : 0;
      si = ok ? (int)y : 0;
    }
    const size_t sp = ok ? (size_t)si * S + sj : 0;  // in [0, plane)
    for (int c = 0; c < g.C; ++c) {
      const size_t base = (bimg * g.C + c) * plane;
      g.dst[base + p] = ok ? g.src[base + sp] : 0.f;
    }
    for (int c = 0; c < g.C2; ++c) {
      const size_t base = (bimg * g.C2 + c) * plane;
      g.dst2[base + p] = ok ? g.src2[base + sp] : 0.f;
    }
  }
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

}  // namespace

extern "C" int aaclip_color_jitter_workspace(int batch, size_t* bytes) {
  AACLIP_REQUIRE(batch > 0 && bytes);
  *bytes = (size_t)batch * RED_BLOCKS * sizeof(unsigned long long);
  return AACLIP_OK;
}

extern "C" int aaclip_color_jitter_u8(const uint8_t* src, int64_t img_stride, int64_t row_pitch, int batch, int h,
                                      int w, const float* factors, uint8_t* dst, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  AACLIP_REQUIRE(src && dst && factors && batch > 0 && batch <= 65535 && h > 0 && w > 0);
  AACLIP_REQUIRE(row_pitch >= (int64_t)w * 3 && (img_stride >= row_pitch * h || batch == 1));
  const size_t extent = (size_t)(batch - 1) * img_stride + (size_t)(h - 1) * row_pitch + (size_t)w * 3;
  AACLIP_REQUIRE(dst == src || !overlap(src, extent, dst, extent));  // in place or disjoint
  bool contrast = false;
  for (int i = 0; i < batch * 3; ++i) {
    AACLIP_REQUIRE(std::isfinite(factors[i]));
    if (i % 3 == 1 && factors[i] != 1.f) contrast = true;
  }
  if (contrast)
    AACLIP_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 &&
                   workspace_bytes >= (size_t)batch * RED_BLOCKS * sizeof(unsigned long long));
  JitterArgs a{};
  a.src = src;
  a.dst = dst;
  a.img_stride = img_stride;
  a.pitch = row_pitch;
  a.H = h;
  a.W = w;
  a.partial = (unsigned long long*)workspace;
  // dword path: every row of every image starts on a 4-byte boundary, in src and dst
  a.vec = (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)img_stride | (uintptr_t)row_pitch) & 3) == 0;
  const size_t items = (size_t)h * ((w + 3) / 4);
  const int blocks = (int)std::min<size_t>((items + NT - 1) / NT, MAX_BLOCKS);
  const hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < batch; b0 += CHUNK) {
    const int nb = std::min(CHUNK, batch - b0);
    a.b0 = b0;
    bool any_contrast = false;
    for (int i = 0; i < nb; ++i)
      for (int k = 0; k < 3; ++k) {
        a.f[i][k] = factors[(size_t)(b0 + i) * 3 + k];
        if (k == 1 && a.f[i][k] != 1.f) any_contrast = true;
      }
    if (any_contrast) {
      jitter_reduce_kernel<<<dim3(RED_BLOCKS, nb), NT, 0, st>>>(a);
      AACLIP_CHECK_LAUNCH();
    }
    jitter_apply_kernel<<<dim3(blocks, nb), NT, 0, st>>>(a);
    AACLIP_CHECK_LAUNCH();
  }
  return AACLIP_OK;
}

extern "C" int aaclip_geom_augment(const float* src, const float* src2, float* dst, float* dst2, int batch,
                                   int channels, int channels2, int size, const int32_t* params,
                                   const float* cos_sin, void* stream) {
  AACLIP_REQUIRE(src && dst && params && cos_sin && batch > 0 && batch <= 65535);
  AACLIP_REQUIRE(channels >= 1 && channels2 >= 0 && size > 0 && size <= 16384);  // coordinates exact in fp32
  AACLIP_REQUIRE(channels2 == 0 || (src2 && dst2));
  const size_t n1 = (size_t)batch * channels * size * size * sizeof(float);
  const size_t n2 = (size_t)batch * channels2 * size * size * sizeof(float);
  // a gather cannot run in place: no output may alias an input (or the other output)
  AACLIP_REQUIRE(!overlap(src, n1, dst, n1));
  if (channels2) {
    AACLIP_REQUIRE(!overlap(src2, n2, dst2, n2) && !overlap(src, n1, dst2, n2) && !overlap(src2, n2, dst, n1) &&
                   !overlap(dst, n1, dst2, n2));
  }
  for (int i = 0; i < batch; ++i) {
    const int32_t* p = params + (size_t)i * 5;  // rotate, tx, ty, hflip, vflip
    AACLIP_REQUIRE((p[0] | 1) == 1 && (p[3] | 1) == 1 && (p[4] | 1) == 1);
    AACLIP_REQUIRE(std::isfinite(cos_sin[2 * i]) && std::isfinite(cos_sin[2 * i + 1]));
  }
  GeomArgs g{};
  g.src = src;
  g.src2 = src2;
  g.dst = dst;
  g.dst2 = dst2;
  g.C = channels;
  g.C2 = channels2;
  g.S = size;
  const float half = 0.5f * (float)size;
  const size_t plane = (size_t)size * size;
  const int blocks = (int)std::min<size_t>((plane + NT - 1) / NT, MAX_BLOCKS);
  const hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < batch; b0 += CHUNK) {
    const int nb = std::min(CHUNK, batch - b0);
    g.b0 = b0;
    for (int i = 0; i < nb; ++i) {
      const int32_t* p = params + (size_t)(b0 + i) * 5;
      g.flags[i] = (uint8_t)(p[0] | (p[3] << 1) | (p[4] << 2));
      // a shift of S or more empties the image whatever its size: clamp, so i - ty cannot overflow
      g.tx[i] = std::max(-size, std::min(size, p[1]));
      g.ty[i] = std::max(-size, std::min(size, p[2]));
      g.a[i] = cos_sin[2 * (b0 + i)] / half;
      g.b[i] = cos_sin[2 * (b0 + i) + 1] / half;
    }
    geom_kernel<<<dim3(blocks, nb), NT, 0, st>>>(g);
    AACLIP_CHECK_LAUNCH();
  }
  return AACLIP_OK;
}
