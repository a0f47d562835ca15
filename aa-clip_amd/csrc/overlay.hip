// Anomaly overlays on the device (reference forward_utils.py:283-327, visualize() and
// apply_ad_scoremap(), which paint them with cv2 on the host): per test image three panels stacked
// top to bottom, the photo, the ground truth over the photo, the prediction over the photo.
// Everything is integer or fp32 arithmetic with one stated result (include/aaclip.h), so the
// bytes are the same on every launch and equal tests/visualize_ref.py.
//
//   resize   aaclip_resize_bilinear_u8 (replaces cv2.resize, :312): 8-bit fixed-point bilinear,
//            weights of 11 fraction bits from host tables (aaclip_bilinear_plan). One thread per
//            four consecutive output pixels of the flat [batch, S, S] pixel array: 12 bytes, three
//            dwords, whatever S is; the last 1-3 pixels and a misaligned output go out as bytes.
//   range    aaclip_overlay_range (:296-299): lo / hi of a class's maps, row_minmax_kernel and the
//            block reductions of scorenorm.h; min / max only, no atomics. The range is over all
//            pixels of the class, so the rows handed to row_minmax_kernel need not be images: each
//            image is cut into the largest number of equal parts up to 64 (a block per part).
//   panels   aaclip_overlay_panels (:296-303, :283-285, :321-326): quantise the class-normalised
//            score (pixel_score of scorenorm.h), the jet ramp in closed form, the integer blend
//            and the stack, one pass. A block owns 1024 consecutive pixels of one image; a pixel's
//            map value, label and photo are read once and its nine bytes go to LDS, each panel's
//            3072-byte run at the offset its global address has modulo 16. The run is then written
//            with 16-byte stores where it covers whole aligned 16-byte groups and byte by byte at
//            its head and tail (3 S^2 is odd for odd S, so the runs of an image's panels start at
//            different alignments).
#include <cfloat>
#include <cmath>

#include "common.h"
#include "scorenorm.h"

namespace {

constexpr int PT = 1024;            // pixels of one image per block (panels)
constexpr int ROW = 3 * PT + 16;    // LDS bytes per panel: the run plus its alignment offset
constexpr int MAX_PARTS = 64;       // equal parts an image's pixels are cut into for the range

// one output pixel of the resize: table rows are (s, a0, a1), a0 + a1 = 2048
__device__ __forceinline__ void resize_pixel(const uint8_t* __restrict__ img, int64_t pitch, int in_h, int in_w,
                                             const int32_t* __restrict__ xt, const int32_t* __restrict__ yt,
                                             int y, int x, uint32_t (&px)[3]) {
  // (the tables come from the caller: an index outside the image is clamped, never followed)
  const int sy = min(max(yt[3 * y], 0), in_h - 1), b0 = yt[3 * y + 1], b1 = yt[3 * y + 2];
  const int sx = min(max(xt[3 * x], 0), in_w - 1), a0 = xt[3 * x + 1], a1 = xt[3 * x + 2];
  const uint8_t* r0 = img + (int64_t)sy * pitch;
  const uint8_t* r1 = img + (int64_t)min(sy + 1, in_h - 1) * pitch;
  const int c0 = 3 * sx, c1 = 3 * min(sx + 1, in_w - 1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = r0[c0 + c] * a0 + r0[c1 + c] * a1;
    const int h1 = r1[c0 + c] * a0 + r1[c1 + c] * a1;
    px[c] = (uint32_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2) & 0xFFu;
  }
}

__global__ __launch_bounds__(MT) void resize_bilinear_kernel(const uint8_t* __restrict__ src, int64_t img_stride,
                                                             int64_t pitch, int in_h, int in_w,
                                                             const int32_t* __restrict__ xt,
                                                             const int32_t* __restrict__ yt, int S, int n_pix,
                                                             int vec, uint8_t* __restrict__ out) {
  const int plane = S * S;
  const int groups = (n_pix + 3) / 4;
  for (int g = blockIdx.x * MT + threadIdx.x; g < groups; g += gridDim.x * MT) {
    const int p0 = 4 * g, cnt = min(4, n_pix - p0);
    int b = p0 / plane, y = (p0 - b * plane) / S, x = p0 - b * plane - y * S;
    uint32_t v[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t px[3] = {0u, 0u, 0u};
      if (j < cnt) resize_pixel(src + (int64_t)b * img_stride, pitch, in_h, in_w, xt, yt, y, x, px);
      v[3 * j] = px[0], v[3 * j + 1] = px[1], v[3 * j + 2] = px[2];
      if (++x == S) {
        x = 0;
        if (++y == S) y = 0, ++b;
      }
    }
    uint8_t* o = out + (int64_t)p0 * 3;
    if (vec && cnt == 4) {
      uint32_t* w = (uint32_t*)o;
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * cnt) o[k] = (uint8_t)v[k];
    }
  }
}

__global__ __launch_bounds__(MT) void class_range_kernel(const float* __restrict__ rmin,
                                                         const float* __restrict__ rmax, int n_img,
                                                         float* __restrict__ range) {
  __shared__ float sh[MT / 64];
  float lo, hi;
  class_minmax(rmin, rmax, n_img, sh, lo, hi);
  if (threadIdx.x == 0) range[0] = lo, range[1] = hi;
}

// numpy's (v * 255).astype(uint8) on float32 for v in [0, 1]; a non-finite v is 0, and what lies
// outside (a class whose maximum is 1 is not normalised) is clamped
__device__ __forceinline__ int quantise(float v) {
  if (!(fabsf(v) <= FLT_MAX)) return 0;
  return (int)fminf(fmaxf(truncf(v * 255.0f), 0.0f), 255.0f);
}

// the jet ramp in RGB: JET(0) = (0, 0, 128), JET(255) = (128, 0, 0)
__device__ __forceinline__ int jet_channel(int u, int centre) { return min(max(383 - abs(4 * u - centre), 0), 255); }
__device__ __forceinline__ void jet(int u, int (&rgb)[3]) {
  rgb[0] = jet_channel(u, 765);
  rgb[1] = jet_channel(u, 510);
  rgb[2] = jet_channel(u, 255);
}

__global__ __launch_bounds__(MT) void overlay_panels_kernel(const float* __restrict__ maps,
                                                            const uint8_t* __restrict__ labels,
                                                            const uint8_t* __restrict__ thumbs,
                                                            const float* __restrict__ range, int S, int swap_rb,
                                                            uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t sh[3][ROW];
  const int plane = S * S, tile0 = blockIdx.x * PT, npix = min(PT, plane - tile0);
  Norm z{0.f, 0.f, 0.f, 0.f, 0, 0};
  if (range != nullptr) {
    z.pmin = range[0];
    z.pmax = range[1];
    z.pnorm = norm_wanted(z.pmax);
  }
  // this block's run of panel k starts at run[k]; in LDS it starts at its address modulo 16
  uint8_t* run[3];
  int phase[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    run[k] = out + ((int64_t)blockIdx.y * 3 + k) * 3 * plane + (int64_t)tile0 * 3;
    phase[k] = (int)((uintptr_t)run[k] & 15u);
  }
  const int64_t base = (int64_t)blockIdx.y * plane + tile0;
  for (int i = threadIdx.x; i < npix; i += MT) {
    const int q = quantise(pixel_score(maps[base + i], z));
    const int L = labels != nullptr && labels[base + i] != 0 ? 255 : 0;
    const uint8_t* t = thumbs + (base + i) * 3;
    const int P[3] = {swap_rb ? t[2] : t[0], t[1], swap_rb ? t[0] : t[2]};
    int jl[3], jq[3];
    jet(L, jl);
    jet(q, jq);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sh[0][phase[0] + 3 * i + c] = (uint8_t)P[c];
      sh[1][phase[1] + 3 * i + c] = (uint8_t)((P[c] + jl[c]) >> 1);
      sh[2][phase[2] + 3 * i + c] = (uint8_t)((P[c] + jq[c]) >> 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int lo = phase[k], hi = phase[k] + 3 * npix;  // LDS bytes [lo, hi) go to run[k] + (j - lo)
    for (int a = 16 * threadIdx.x; a < hi; a += 16 * MT) {
      if (a >= lo && a + 16 <= hi) {
        *(uint4*)(run[k] + (a - lo)) = *(const uint4*)(&sh[k][a]);
      } else {
        for (int j = max(a, lo); j < min(a + 16, hi); ++j) run[k][j - lo] = sh[k][j];
      }
    }
  }
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
size_t range_rows_bytes(int n_images) { return align_up(4 * (size_t)n_images * MAX_PARTS); }

}  // namespace

extern "C" int aaclip_bilinear_plan(int in_size, int out_size, int32_t* table) {
#pragma clang fp contract(off)
  AACLIP_REQUIRE(in_size > 0 && out_size > 0 && table);
  const double scale = (double)in_size / out_size;
  for (int d = 0; d < out_size; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) s = 0, f = 0.f;
    if (s >= in_size - 1) s = in_size - 1, f = 0.f;
    table[3 * d] = s;
    table[3 * d + 1] = (int32_t)rintf((1.f - f) * 2048.f);
    table[3 * d + 2] = (int32_t)rintf(f * 2048.f);
  }
  return AACLIP_OK;
}

extern "C" int aaclip_resize_bilinear_u8(const uint8_t* src, int64_t img_stride, int64_t row_pitch, int batch,
                                         int in_h, int in_w, const int32_t* x_table, const int32_t* y_table,
                                         int out_size, uint8_t* out, void* stream) {
  AACLIP_REQUIRE(src && x_table && y_table && out && batch > 0 && in_h > 0 && in_w > 0 && out_size > 0);
  AACLIP_REQUIRE(row_pitch >= (int64_t)in_w * 3 && (img_stride >= row_pitch * in_h || batch == 1));
  const int64_t n_pix = (int64_t)batch * out_size * out_size;
  AACLIP_REQUIRE(n_pix < (1LL << 31) - 4);
  const int groups = (int)((n_pix + 3) / 4);
  const int grid = std::min((groups + MT - 1) / MT, 1 << 16);
  resize_bilinear_kernel<<<grid, MT, 0, (hipStream_t)stream>>>(src, img_stride, row_pitch, in_h, in_w, x_table,
                                                               y_table, out_size, (int)n_pix, aligned4(out) ? 1 : 0,
                                                               out);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_overlay_workspace(int n_images, size_t* bytes) {
  AACLIP_REQUIRE(bytes && n_images > 0);
  *bytes = 2 * range_rows_bytes(n_images);
  return AACLIP_OK;
}

extern "C" int aaclip_overlay_range(const float* maps, int n_images, int64_t pix_per_image, void* workspace,
                                    size_t workspace_bytes, float* range, void* stream) {
  AACLIP_REQUIRE(maps && workspace && range && n_images > 0 && pix_per_image > 0);
  AACLIP_REQUIRE(n_images <= (1 << 24));
  AACLIP_REQUIRE(aligned4(workspace) && workspace_bytes >= 2 * range_rows_bytes(n_images));
  float* rmin = (float*)workspace;
  float* rmax = (float*)((char*)workspace + range_rows_bytes(n_images));
  int parts = MAX_PARTS;
  while (pix_per_image % parts) --parts;  // (1 divides everything)
  const int rows = n_images * parts;
  hipStream_t s = (hipStream_t)stream;
  row_minmax_kernel<<<rows, MT, 0, s>>>(maps, pix_per_image / parts, rmin, rmax);
  class_range_kernel<<<1, MT, 0, s>>>(rmin, rmax, rows, range);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_overlay_panels(const float* maps, const uint8_t* labels, const uint8_t* thumbs,
                                     const float* range, int batch, int size, int swap_rb, uint8_t* out,
                                     void* stream) {
  AACLIP_REQUIRE(maps && thumbs && out && batch > 0 && batch <= 65535 && size > 0 && size <= 16384);
  const int plane = size * size;
  overlay_panels_kernel<<<dim3((plane + PT - 1) / PT, batch), MT, 0, (hipStream_t)stream>>>(
      maps, labels, thumbs, range, size, swap_rb != 0, out);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
