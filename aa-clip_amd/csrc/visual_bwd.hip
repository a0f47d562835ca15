// Backward of the adapted visual tower (stage 2: train.py:117-174 trains image_adapter only):
// the level tap + ln_post backward and the L2-normalise backward of the projection tail. The
// attention backward for long sequences is attention_bwd.hip; everything else of the stage-2
// backward reuses text_bwd.hip's entries and aaclip_gemm on transposed weights.
//
// All fp32, deterministic (no floating-point atomics, fixed reduction orders: two launches
// give the same bits) and image / row local.
#include "common.h"
#include "rowmath.h"  // the row layout, the LayerNorm statistics and layer_norm_bwd, shared with rows.hip

namespace {

// ------------------------------------------------------------------ level tap + ln_post backward
// Token row (b, t >= 1) of g += LN_bwd(dtap[b, t - 1]; x[b, t], w) (layer_norm_bwd, rowmath.h).
// CLS rows return before they touch memory. One wave per token row.
template <int VEC>
__global__ __launch_bounds__(256) void tap_ln_bwd_kernel(const float* __restrict__ dtap, const float* __restrict__ x,
                                                         const float* __restrict__ w, float* __restrict__ g, int rows,
                                                         int n_tok) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int tk = row % n_tok;
  if (tk == 0) return;
  constexpr int D = 256 * VEC;
  const size_t trow = (size_t)(row / n_tok) * (n_tok - 1) + (tk - 1);
  float4_t xv[VEC], dy[VEC], gv[VEC], o[VEC];
  load_row<VEC>(x + (size_t)row * D, xv, lane);
  load_row<VEC>(dtap + trow * D, dy, lane);
  load_row<VEC>(g + (size_t)row * D, gv, lane);
  layer_norm_bwd<VEC>(xv, dy, w, o, lane);
#pragma unroll
  for (int c = 0; c < VEC; ++c) o[c] = gv[c] + o[c];
  store_row<VEC>(g + (size_t)row * D, o, lane);
}

// ------------------------------------------------------------------ L2-normalise backward
// y = x / max(|x|, 1e-12) (l2norm_kernel; |x| = sqrt(row_dot(x, x)), its own call). With
// gy = scale * dy[row / group] (group 0: dy[row]):
//   |x| >  1e-12:  dx = (gy - y (y . gy)) / |x|
//   |x| <= 1e-12:  dx = gy / 1e-12                 (the clamp passes no gradient to the norm)
template <int VEC>
__global__ __launch_bounds__(256) void l2_normalize_bwd_kernel(const float* dy, int64_t lddy, int group, float scale,
                                                               const float* __restrict__ x, int64_t ldx, float* dx,
                                                               int64_t lddx, int rows) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4_t xv[VEC], gy[VEC];
  load_row<VEC>(x + (size_t)row * ldx, xv, lane);
  load_row<VEC>(dy + (size_t)(group > 0 ? row / group : row) * lddy, gy, lane);
#pragma unroll
  for (int c = 0; c < VEC; ++c) gy[c] = gy[c] * scale;
  const float n = sqrtf(row_dot<VEC>(xv, xv));
  float4_t o[VEC];
  if (n > 1e-12f) {  // wave-uniform
    const float inv = 1.0f / n;
#pragma unroll
    for (int c = 0; c < VEC; ++c) xv[c] = xv[c] * inv;
    const float a = row_dot<VEC>(xv, gy);
#pragma unroll
    for (int c = 0; c < VEC; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[c][j] = (gy[c][j] - xv[c][j] * a) * inv;
  } else {
#pragma unroll
    for (int c = 0; c < VEC; ++c) o[c] = gy[c] * 1e12f;
  }
  store_row<VEC>(dx + (size_t)row * lddx, o, lane);  // dx may be dy (group 0): read above, by the same lane
}

}  // namespace

extern "C" int aaclip_tap_ln_bwd(const float* dtap, const float* x, const float* w, float* g, int batch, int n_tok,
                                 int width, void* stream) {
  AACLIP_REQUIRE(dtap && x && w && g && batch > 0 && n_tok >= 2 && (width == 768 || width == 1024));
  AACLIP_REQUIRE((int64_t)batch * n_tok < (1ll << 31));
  AACLIP_REQUIRE(g != x && g != dtap);
  AACLIP_REQUIRE(aligned16(dtap) && aligned16(x) && aligned16(w) && aligned16(g));
  const int rows = batch * n_tok;
  DISPATCH_VEC(width,
               tap_ln_bwd_kernel<V><<<ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(dtap, x, w, g, rows, n_tok));
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_l2_normalize_bwd(const float* dy, int64_t lddy, int dy_group, float scale, const float* x,
                                       int64_t ldx, float* dx, int64_t lddx, int rows, int width, void* stream) {
  AACLIP_REQUIRE(dy && x && dx && rows >= 0 && dy_group >= 0 && (width == 768 || width == 1024));
  AACLIP_REQUIRE(lddy >= width && ldx >= width && lddx >= width && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0);
  AACLIP_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(dx));
  AACLIP_REQUIRE(dx != x && (dx != dy || (dy_group == 0 && lddx == lddy)));
  if (rows == 0) return AACLIP_OK;
  DISPATCH_VEC(width, l2_normalize_bwd_kernel<V><<<ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(
                          dy, lddy, dy_group, scale, x, ldx, dx, lddx, rows));
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
