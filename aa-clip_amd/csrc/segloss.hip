// Stage-1 segmentation loss head and its backward (reference train.py:86-100,
// forward_utils.py:21-126, :199-202, :211-215, :219-227): from the train-branch
// probabilities [B, 2, S, S] and the mask to the loss, and from the loss back to the
// anchors T and the patch features f.
//
//   seg_loss             FocalLoss() + BinaryDiceLoss() x 2: one pass over probs and mask,
//                        7 sums per (image, chunk of kChunk pixels), then one finalize
//                        block sums the chunks in index order in fp64.
//   seg_loss_bwd         elementwise dprobs from probs, mask and the per-image sums.
//   upsample_softmax_bwd softmax backward + the transpose of the align_corners bilinear
//                        upsample, written as a gather: one wave per source cell.
//   patch_logits_bwd     dT (per image or shared) and df; one wave per (image, chunk of
//                        kRows patch rows) owns the 768 columns, then a finalize pass.
//
// (The per-image logits forward, aaclip_patch_logits_per_image, lives in anomaly_map.hip:
// it is patch_logits_kernel itself with an anchor stride, so that a shared anchor set
// gives aaclip_patch_logits' bits by construction.)
//
// No atomics anywhere: every sum has a fixed order, an image's sums and gradient rows
// depend on that image alone, and nothing allocates, syncs or reads on the host.
#include <math.h>

#include "common.h"
#include "rowmath.h"  // the wave-row layout: load_row_as, load_anchors

namespace {

constexpr int kChunk = AACLIP_SEGLOSS_CHUNK;  // pixels per seg_loss workgroup (256 threads x 16)
constexpr int kRows = AACLIP_LOGITS_BWD_ROWS;  // patch rows per patch_logits_bwd wave
constexpr float kSmooth = 1e-5f;               // FocalLoss(smooth=1e-5), forward_utils.py:41
// clamp(one_hot, smooth / (num_class - 1), 1 - smooth) in fp32 (forward_utils.py:94-97)
constexpr float kOneHotLo = 1e-5f;
constexpr float kOneHotHi = (float)(1.0 - 1e-5);

// The focal pieces of one pixel: pt = o_0 p0 + o_1 p1 + smooth.
__device__ __forceinline__ float focal_pt(float p0, float p1, float m, float& o0, float& o1) {
#pragma clang fp contract(off)
  const int k = (int)m;
  o0 = k == 0 ? kOneHotHi : kOneHotLo;
  o1 = k == 1 ? kOneHotHi : kOneHotLo;
  return (o0 * p0 + o1 * p1) + kSmooth;
}

struct Sums7 {
  float v[7];  // term, p0*t0, p0, t0, p1*t1, p1, t1
};

__device__ __forceinline__ void pixel_sums(float p0, float p1, float m, Sums7& s) {
#pragma clang fp contract(off)
  float o0, o1;
  const float pt = focal_pt(p0, p1, m, o0, o1);
  const float q = 1.0f - pt;
  const float t0 = 1.0f - m;
  s.v[0] += -1.0f * (q * q) * logf(pt);
  s.v[1] += p0 * t0;
  s.v[2] += p0;
  s.v[3] += t0;
  s.v[4] += p1 * m;
  s.v[5] += p1;
  s.v[6] += m;
}

// One workgroup per (chunk of kChunk pixels, image). VEC: 16-byte loads (S*S % 4 == 0 and
// 16-byte aligned bases), else dwords. Per thread fp32 sums over its <= 16 pixels, the
// wave butterfly, then the 4 waves in index order in fp64: partial[b][chunk][8] doubles.
template <bool VEC>
__global__ __launch_bounds__(256) void seg_loss_kernel(const float* __restrict__ probs,
                                                       const float* __restrict__ mask, int npix, int nchunk,
                                                       double* __restrict__ partial) {
  __shared__ float red[4][8];
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
  const float* p0 = probs + (size_t)b * 2 * npix;
  const float* p1 = p0 + npix;
  const float* mk = mask + (size_t)b * npix;
  Sums7 s{};
  if constexpr (VEC) {
    const int nq = npix >> 2;
#pragma unroll
    for (int it = 0; it < kChunk / 1024; ++it) {
      const int q = ch * (kChunk / 4) + it * 256 + tid;
      if (q < nq) {
        const float4_t a = *(const float4_t*)(p0 + 4 * (size_t)q);
        const float4_t c = *(const float4_t*)(p1 + 4 * (size_t)q);
        const float4_t m = *(const float4_t*)(mk + 4 * (size_t)q);
#pragma unroll
        for (int j = 0; j < 4; ++j) pixel_sums(a[j], c[j], m[j], s);
      }
    }
  } else {
#pragma unroll 4
    for (int it = 0; it < kChunk / 256; ++it) {
      const int x = ch * kChunk + it * 256 + tid;
      if (x < npix) pixel_sums(p0[x], p1[x], mk[x], s);
    }
  }
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const float t = wave_sum(s.v[j]);
    if ((tid & 63) == 0) red[tid >> 6][j] = t;
  }
  __syncthreads();
  if (tid < 8) {
    double t = 0.0;
    if (tid < 7) t = (((double)red[0][tid] + (double)red[1][tid]) + (double)red[2][tid]) + (double)red[3][tid];
    partial[((size_t)b * nchunk + ch) * 8 + tid] = t;
  }
}

// One workgroup of 256: thread (image slot tid / 8, sum tid % 8) adds that sum's chunks in
// index order -> sums[b][8]; then wave 0 forms the loss, lane l taking images l, l + 64, ...
// in order and lane 0 adding the lanes in order (all fp64; the outputs are rounded once).
__global__ __launch_bounds__(256) void seg_loss_finalize_kernel(const double* __restrict__ partial, int batch,
                                                                int nchunk, int npix, double* __restrict__ sums,
                                                                float* __restrict__ loss) {
  __shared__ double acc[64][3];
  const int tid = threadIdx.x;
  for (int b = tid >> 3; b < batch; b += 32) {
    const double* pp = partial + (size_t)b * nchunk * 8 + (tid & 7);
    double t = 0.0;
    for (int c = 0; c < nchunk; ++c) t += pp[(size_t)c * 8];
    sums[(size_t)b * 8 + (tid & 7)] = t;
  }
  __threadfence_block();
  __syncthreads();
  double fo = 0.0, d0 = 0.0, d1 = 0.0;
  if (tid < 64) {
    for (int b = tid; b < batch; b += 64) {
      const double* s = sums + (size_t)b * 8;
      fo += s[0];
      d0 += (2.0 * s[1] + 1.0) / (s[2] + s[3] + 1.0);
      d1 += (2.0 * s[4] + 1.0) / (s[5] + s[6] + 1.0);
    }
    acc[tid][0] = fo;
    acc[tid][1] = d0;
    acc[tid][2] = d1;
  }
  __syncthreads();
  if (tid == 0) {
    fo = d0 = d1 = 0.0;
    const int n = batch < 64 ? batch : 64;
    for (int l = 0; l < n; ++l) {
      fo += acc[l][0];
      d0 += acc[l][1];
      d1 += acc[l][2];
    }
    const float focal = (float)(fo / ((double)batch * (double)npix));
    const float dice0 = (float)(1.0 - d0 / (double)batch);
    const float dice1 = (float)(1.0 - d1 / (double)batch);
    loss[0] = focal;
    loss[1] = dice0;
    loss[2] = dice1;
    loss[3] = (focal + dice0) + dice1;  // loss = focal; loss += dice; loss += dice (forward_utils.py:224-226)
  }
}

// dprobs[b, c, x] = dloss * (dfocal/dp_c + ddice_c/dp_c). Grid (chunks of 1024 pixels, image).
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ probs,
                                                           const float* __restrict__ mask,
                                                           const double* __restrict__ sums,
                                                           const float* __restrict__ dloss, int batch, int npix,
                                                           float* __restrict__ dprobs) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const double* s = sums + (size_t)b * 8;
  // ddice_c/dp_c = -(2 t_c D - Nn) / (B D^2) = nb_c - t_c * na_c
  const double D0 = s[2] + s[3] + 1.0, D1 = s[5] + s[6] + 1.0;
  const double N0 = 2.0 * s[1] + 1.0, N1 = 2.0 * s[4] + 1.0;
  const float na0 = (float)(2.0 / ((double)batch * D0)), nb0 = (float)(N0 / ((double)batch * D0 * D0));
  const float na1 = (float)(2.0 / ((double)batch * D1)), nb1 = (float)(N1 / ((double)batch * D1 * D1));
  const float inv_bn = (float)(1.0 / ((double)batch * (double)npix));
  const float dl = dloss[0];
  const float* p0 = probs + (size_t)b * 2 * npix;
  const float* p1 = p0 + npix;
  const float* mk = mask + (size_t)b * npix;
  float* g0 = dprobs + (size_t)b * 2 * npix;
  float* g1 = g0 + npix;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int x = blockIdx.x * 1024 + it * 256 + threadIdx.x;
    if (x < npix) {
      const float m = mk[x];
      float o0, o1;
      const float pt = focal_pt(p0[x], p1[x], m, o0, o1);
      const float q = 1.0f - pt;
      const float common = (2.0f * q * logf(pt) - (q * q) / pt) * inv_bn;
      const float t0 = 1.0f - m;
      g0[x] = dl * (o0 * common + (nb0 - t0 * na0));
      g1[x] = dl * (o1 * common + (nb1 - m * na1));
    }
  }
}

// One wave per source cell (j, i, image). The cell scans a conservative window of output
// pixels (every pixel whose taps can reach row i / column j, +-1 pixel: the fp32 rounding
// of scale * dst moves a boundary by far less) and accepts a pixel only where
// bilinear_tap -- the forward's own index computation -- lands on the cell, so membership
// and weights are the forward's at every rounding boundary. Lanes run along x (coalesced
// dprobs rows, one row per half-wave); the 3 x 3 neighbourhood of the cell is staged in LDS for the softmax
// recomputation (blur_band's expression order, no contraction).
__global__ __launch_bounds__(64) void upsample_softmax_bwd_kernel(const float* __restrict__ grid,
                                                                  const float* __restrict__ dprobs, int g, int S,
                                                                  float scale, float* __restrict__ dgrid) {
#pragma clang fp contract(off)
  __shared__ float nb[2][3][3];
  const int j = blockIdx.x, i = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  if (lane < 18) {
    const int c = lane / 9, r = (lane % 9) / 3, q = lane % 3;
    const int gy = min(max(i - 1 + r, 0), g - 1), gx = min(max(j - 1 + q, 0), g - 1);
    nb[c][r][q] = grid[(((size_t)b * 2 + c) * g + gy) * g + gx];
  }
  __builtin_amdgcn_wave_barrier();
  // pixels with floor(src) in {i - 1, i}: src in [i - 1, i + 1), dst = src * (S - 1) / (g - 1)
  const int y_lo = max(0, (max(i - 1, 0) * (S - 1)) / (g - 1) - 1);
  const int y_hi = min(S - 1, ((i + 1) * (S - 1) + g - 2) / (g - 1) + 1);
  const int x_lo = max(0, (max(j - 1, 0) * (S - 1)) / (g - 1) - 1);
  const int x_hi = min(S - 1, ((j + 1) * (S - 1) + g - 2) / (g - 1) + 1);
  const float* d0 = dprobs + (size_t)b * 2 * S * S;
  const float* d1 = d0 + (size_t)S * S;
  float a0 = 0.f, a1 = 0.f;
  // the two half-waves take alternate rows, 32 lanes along x: a window is about
  // 2 (S - 1) / (g - 1) pixels wide (28 at 518 px / g = 37), which would leave half of a
  // 64-wide row idle
  const int half = lane >> 5, l32 = lane & 31;
  for (int y = y_lo + half; y <= y_hi; y += 2) {
    int iy0, iy1;
    float hy0, hy1;
    bilinear_tap(scale, y, g, iy0, iy1, hy0, hy1);
    const float wy = (iy0 == i ? hy0 : 0.f) + (iy1 == i ? hy1 : 0.f);
    if (iy0 != i && iy1 != i) continue;  // uniform in the half-wave
    const int r0 = iy0 - (i - 1), r1 = iy1 - (i - 1);  // 0..2 for a member row
    for (int x = x_lo + l32; x <= x_hi; x += 32) {
      int ix0, ix1;
      float w0, w1;
      bilinear_tap(scale, x, g, ix0, ix1, w0, w1);
      if (ix0 != j && ix1 != j) continue;
      const float wx = (ix0 == j ? w0 : 0.f) + (ix1 == j ? w1 : 0.f);
      const int q0 = ix0 - (j - 1), q1 = ix1 - (j - 1);
      float v[2][1];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float H0 = w0 * nb[c][r0][q0] + w1 * nb[c][r0][q1];
        const float H1 = w0 * nb[c][r1][q0] + w1 * nb[c][r1][q1];
        v[c][0] = hy0 * H0 + hy1 * H1;
      }
      softmax_channels<2, 1>(v, 0);
      // dz_c = p_c (g_c - sum_k p_k g_k) written as p_c sum_k p_k (g_c - g_k): for two channels
      // dz_0 = p0 p1 (g_0 - g_1) = -dz_1. The first form leans on p0 + p1 == 1, which the
      // forward's reciprocal-normalised p's meet only to an ulp, and that ulp times g_c is
      // then measured against a small p_other (g_c - g_other); this form has no such term.
      const float gA = d0[(size_t)y * S + x], gB = d1[(size_t)y * S + x];
      const float dz = (v[0][0] * v[1][0]) * (gA - gB);
      const float w = wy * wx;
      a0 += w * dz;
      a1 += w * (-dz);
    }
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (lane == 0) {
    dgrid[(((size_t)b * 2 + 0) * g + i) * g + j] = a0;
    dgrid[(((size_t)b * 2 + 1) * g + i) * g + j] = a1;
  }
}

// One wave per (chunk of kRows patch rows, image); the lane owns columns
// 256 c + 4 lane + 0..3 (c = 0..2) as patch_logits_kernel does. Per row: the two dgrid
// values (wave-uniform), df row = 100 * (d0 * T[:, 0] + d1 * T[:, 1]) stored as it goes,
// and the dT partial f * d_a accumulated in fp32 over the chunk's rows in order ->
// partial[b][chunk][768][2]. f is read once.
template <bool F32IN>
__global__ __launch_bounds__(64) void patch_logits_bwd_kernel(const void* __restrict__ f, int64_t ld,
                                                              const float* __restrict__ T, int64_t t_stride,
                                                              const float* __restrict__ dgrid, int group,
                                                              int nchunk, float* __restrict__ partial,
                                                              float* __restrict__ df) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, ch = blockIdx.x, b = blockIdx.y;
  const float* Tb = T + (size_t)b * t_stride;
  float4_t t0[3], t1[3];
  if (df) load_anchors(Tb, t0, t1, lane);
  float4_t acc0[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, acc1[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  const float* dg = dgrid + (size_t)b * 2 * group;
  const int p_end = min((ch + 1) * kRows, group);
#pragma unroll 4
  for (int p = ch * kRows; p < p_end; ++p) {
    const size_t row = (size_t)b * group + p;
    const float d0 = dg[p], d1 = dg[group + p];
    if (partial) {
      float4_t v[3];
      load_row_as<F32IN, 3>(f, row * ld, v, lane);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        acc0[c] += v[c] * d0;
        acc1[c] += v[c] * d1;
      }
    }
    if (df) {
      float* o = df + row * 768;
#pragma unroll
      for (int c = 0; c < 3; ++c) *(float4_t*)(o + 256 * c + 4 * lane) = 100.0f * (t0[c] * d0 + t1[c] * d1);
    }
  }
  if (partial) {
    float* pp = partial + ((size_t)b * nchunk + ch) * 1536;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = pp + 2 * (256 * c + 4 * lane);
      *(float4_t*)o = float4_t{acc0[c][0], acc1[c][0], acc0[c][1], acc1[c][1]};
      *(float4_t*)(o + 4) = float4_t{acc0[c][2], acc1[c][2], acc0[c][3], acc1[c][3]};
    }
  }
}

// dT element e = 2 * column + anchor of image blockIdx.y (per image) or of all images
// (shared: images in index order), chunks in index order, summed in fp64, x 100.
__global__ __launch_bounds__(256) void patch_logits_bwd_finalize_kernel(const float* __restrict__ partial,
                                                                        int b_lo, int n_img, int nchunk,
                                                                        float* __restrict__ dT) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int b0 = b_lo + blockIdx.y;
  double t = 0.0;
  for (int b = b0; b < b0 + n_img; ++b) {
    const float* pp = partial + (size_t)b * nchunk * 1536 + e;
    for (int c0 = 0; c0 < nchunk; c0 += 8) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = c0 + k < nchunk ? pp[(size_t)(c0 + k) * 1536] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + k < nchunk) t += (double)v[k];
    }
  }
  dT[(size_t)blockIdx.y * 1536 + e] = (float)(100.0 * t);
}

// S * S and batch * 2 * S * S as ints the kernels index with size_t; the grid's y / z
// dimensions take the batch (<= 65535).
bool image_dims_ok(int batch, int out_size) {
  return batch > 0 && batch <= 65535 && out_size >= 2 && out_size <= 16384;
}

}  // namespace

extern "C" int aaclip_seg_loss(const float* probs, const float* mask, int batch, int out_size, double* partial,
                               size_t partial_bytes, double* sums, float* loss, void* stream) {
  AACLIP_REQUIRE(probs && mask && partial && sums && loss);
  AACLIP_REQUIRE(image_dims_ok(batch, out_size));
  AACLIP_REQUIRE(aligned4(probs) && aligned4(mask) && aligned4(loss));
  AACLIP_REQUIRE(((uintptr_t)partial & 7) == 0 && ((uintptr_t)sums & 7) == 0);
  const int npix = out_size * out_size;
  const int nchunk = ceil_div(npix, kChunk);
  AACLIP_REQUIRE(partial_bytes >= (size_t)batch * nchunk * 8 * sizeof(double));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grd(nchunk, batch);
  if (npix % 4 == 0 && aligned16(probs) && aligned16(mask))
    seg_loss_kernel<true><<<grd, 256, 0, s>>>(probs, mask, npix, nchunk, partial);
  else
    seg_loss_kernel<false><<<grd, 256, 0, s>>>(probs, mask, npix, nchunk, partial);
  AACLIP_CHECK_LAUNCH();
  seg_loss_finalize_kernel<<<1, 256, 0, s>>>(partial, batch, nchunk, npix, sums, loss);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_seg_loss_bwd(const float* probs, const float* mask, const double* sums, const float* dloss,
                                   int batch, int out_size, float* dprobs, void* stream) {
  AACLIP_REQUIRE(probs && mask && sums && dloss && dprobs);
  AACLIP_REQUIRE(image_dims_ok(batch, out_size));
  AACLIP_REQUIRE(aligned4(probs) && aligned4(mask) && aligned4(dloss) && aligned4(dprobs));
  AACLIP_REQUIRE(((uintptr_t)sums & 7) == 0 && dprobs != probs);
  const int npix = out_size * out_size;
  seg_loss_bwd_kernel<<<dim3(ceil_div(npix, 1024), batch), 256, 0, (hipStream_t)stream>>>(probs, mask, sums, dloss,
                                                                                         batch, npix, dprobs);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_upsample_softmax_bwd(const float* grid, const float* dprobs, int batch, int channels, int g,
                                           int out_size, float* dgrid, void* stream) {
  AACLIP_REQUIRE(grid && dprobs && dgrid && dgrid != grid);
  AACLIP_REQUIRE(channels == 2 && g >= 2 && g <= 64);
  AACLIP_REQUIRE(image_dims_ok(batch, out_size));
  AACLIP_REQUIRE(aligned4(grid) && aligned4(dprobs) && aligned4(dgrid));
  const float scale = (float)(g - 1) / (float)(out_size - 1);  // as aaclip_blur_upsample
  upsample_softmax_bwd_kernel<<<dim3(g, g, batch), 64, 0, (hipStream_t)stream>>>(grid, dprobs, g, out_size, scale,
                                                                                dgrid);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_patch_logits_bwd_workspace(int rows, int group, size_t* bytes) {
  AACLIP_REQUIRE(bytes && rows > 0 && group > 0 && rows % group == 0);
  *bytes = (size_t)(rows / group) * ceil_div(group, kRows) * 1536 * sizeof(float);
  return AACLIP_OK;
}

extern "C" int aaclip_patch_logits_bwd(int in_dtype, const void* f, int64_t ld, const float* T, int64_t t_stride,
                                       int n_anchor, const float* dgrid, int rows, int channels, int group,
                                       float* workspace, size_t workspace_bytes, float* dT, float* df,
                                       void* stream) {
  AACLIP_REQUIRE(in_dtype == AACLIP_F32 || in_dtype == AACLIP_BF16);
  AACLIP_REQUIRE(f && T && dgrid && (dT || df) && n_anchor == 2);
  AACLIP_REQUIRE(rows > 0 && channels == 768 && ld >= channels && ld % 4 == 0 && group > 0 && rows % group == 0);
  AACLIP_REQUIRE(rows / group <= 65535);
  AACLIP_REQUIRE(t_stride == 0 || t_stride >= 1536);
  AACLIP_REQUIRE(t_stride % 4 == 0 && aligned16(T) && aligned16(workspace) && aligned16(df) && aligned4(dgrid) &&
                 aligned4(dT));
  AACLIP_REQUIRE(in_dtype == AACLIP_F32 ? aligned16(f) : ((uintptr_t)f & 7) == 0);
  AACLIP_REQUIRE((const void*)df != f);
  const int batch = rows / group, nchunk = ceil_div(group, kRows);
  if (dT) AACLIP_REQUIRE(workspace && workspace_bytes >= (size_t)batch * nchunk * 1536 * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  float* part = dT ? workspace : nullptr;
  const dim3 grd(nchunk, batch);
  if (in_dtype == AACLIP_F32)
    patch_logits_bwd_kernel<true><<<grd, 64, 0, s>>>(f, ld, T, t_stride, dgrid, group, nchunk, part, df);
  else
    patch_logits_bwd_kernel<false><<<grd, 64, 0, s>>>(f, ld, T, t_stride, dgrid, group, nchunk, part, df);
  AACLIP_CHECK_LAUNCH();
  if (dT) {
    if (t_stride == 0)
      patch_logits_bwd_finalize_kernel<<<dim3(6, 1), 256, 0, s>>>(part, 0, batch, nchunk, dT);
    else
      patch_logits_bwd_finalize_kernel<<<dim3(6, batch), 256, 0, s>>>(part, 0, 1, nchunk, dT);
    AACLIP_CHECK_LAUNCH();
  }
  return AACLIP_OK;
}
