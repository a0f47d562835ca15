// Backward of the adapted text tower (stage 1: train.py:38-114 trains text_adapter only):
// attention, LayerNorm, EOT gather + ln_final, activations, the adapter blend, the
// prompt-ensemble anchor and the weight gradient of a bias-free Linear, plus the
// elementwise activation the training forward applies to a stored pre-activation.
//
// All fp32, deterministic (no floating-point atomics, fixed reduction orders: two launches
// give the same bits) and row / sequence local. A few hundred token rows per call: the
// kernels are written for clarity and exactness, not for throughput; the input-gradient
// GEMMs around them are the existing aaclip_gemm on transposed weight copies.
#include "common.h"
#include "rowmath.h"  // the row layout, the LayerNorm statistics and layer_norm_bwd, shared with rows.hip

namespace {

// ------------------------------------------------------------------ attention backward
// One workgroup of 4 waves per (sequence, head). q, k, v, dout tiles [seq][64] (row pitch
// 65: lane j reading row j, or lane d reading column d, hits 64 different banks) and the
// probabilities P and score gradients dS [seq][seq | 1] live in LDS: 127.5 KB at seq 77,
// dynamic LDS above the 64 KB static limit, one workgroup per CU (160 KB).
// Phase 1, a wave per query i, a lane per key j (and j + 64): s = q_i . k_j / 8, softmax over
// the allowed keys, dP = dout_i . v_j, D = sum_j P dP, dS = P (dP - D).
// Phase 2, a wave per output row, a lane per head dim, sums in index order:
// dQ_i = sum_j dS_ij k_j / 8, dK_j = sum_i dS_ij q_i / 8, dV_j = sum_i P_ij dout_i.
constexpr int AB_MAX_SEQ = 77, AB_HD = 64, AB_LD = 65;
constexpr int AB_MAX_LDS = (4 * AB_MAX_SEQ * AB_LD + 2 * AB_MAX_SEQ * (AB_MAX_SEQ | 1)) * 4;

__global__ __launch_bounds__(256) void attention_bwd_kernel(const float* __restrict__ qkv,
                                                            const float* __restrict__ dout,
                                                            float* __restrict__ dqkv, int N, int H, int causal) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lds = N | 1;
  float* Qs = sm;
  float* Ks = Qs + N * AB_LD;
  float* Vs = Ks + N * AB_LD;
  float* Os = Vs + N * AB_LD;
  float* Ps = Os + N * AB_LD;
  float* Ds = Ps + N * lds;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int HDt = H * AB_HD;
  const size_t ld = 3 * (size_t)HDt;
  const float* base = qkv + (size_t)b * N * ld + h * AB_HD;
  const float* dob = dout + (size_t)b * N * HDt + h * AB_HD;
  for (int idx = t; idx < N * AB_HD; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    const float* src = base + (size_t)r * ld + c;
    Qs[r * AB_LD + c] = src[0];
    Ks[r * AB_LD + c] = src[HDt];
    Vs[r * AB_LD + c] = src[2 * HDt];
    Os[r * AB_LD + c] = dob[(size_t)r * HDt + c];
  }
  __syncthreads();
  for (int i = wid; i < N; i += 4) {
    const int lim = causal ? i + 1 : N;
    float s[2], dp[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = lane + 64 * jj;
      float a = 0.f, e = 0.f;
      if (j < lim) {
        for (int d = 0; d < AB_HD; ++d) {
          a += Qs[i * AB_LD + d] * Ks[j * AB_LD + d];
          e += Os[i * AB_LD + d] * Vs[j * AB_LD + d];
        }
      }
      s[jj] = j < lim ? a * 0.125f : -INFINITY;
      dp[jj] = e;
    }
    const float mx = wave_max(fmaxf(s[0], s[1]));  // key 0 is always allowed: finite
    float p[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) p[jj] = lane + 64 * jj < lim ? expf(s[jj] - mx) : 0.f;
    const float inv = 1.0f / wave_sum(p[0] + p[1]);
    p[0] *= inv;
    p[1] *= inv;
    const float D = wave_sum(p[0] * dp[0] + p[1] * dp[1]);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = lane + 64 * jj;
      if (j < N) {
        Ps[i * lds + j] = p[jj];
        Ds[i * lds + j] = p[jj] * (dp[jj] - D);
      }
    }
  }
  __syncthreads();
  float* ob = dqkv + (size_t)b * N * ld + h * AB_HD + lane;
  for (int task = wid; task < 3 * N; task += 4) {
    const int kind = task / N, r = task % N;
    float acc = 0.f;
    if (kind == 0) {
      const int lim = causal ? r + 1 : N;
      for (int j = 0; j < lim; ++j) acc += Ds[r * lds + j] * Ks[j * AB_LD + lane];
      acc *= 0.125f;
    } else if (kind == 1) {
      for (int i = causal ? r : 0; i < N; ++i) acc += Ds[i * lds + r] * Qs[i * AB_LD + lane];
      acc *= 0.125f;
    } else {
      for (int i = causal ? r : 0; i < N; ++i) acc += Ps[i * lds + r] * Os[i * AB_LD + lane];
    }
    ob[(size_t)r * ld + (size_t)kind * HDt] = acc;
  }
}

// ------------------------------------------------------------------ LayerNorm backward
template <int VEC>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* dy, int64_t lddy, const float* x,
                                                            int64_t ldx, const float* __restrict__ w,
                                                            const float* resid, int64_t ldr, float* dx,
                                                            int64_t lddx, int rows) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4_t xv[VEC], dv[VEC], o[VEC];
  load_row<VEC>(x + (size_t)row * ldx, xv, lane);
  load_row<VEC>(dy + (size_t)row * lddy, dv, lane);
  layer_norm_bwd<VEC>(xv, dv, w, o, lane);
  if (resid) {  // may be dx itself: each lane reads its own elements before it writes them
    float4_t r[VEC];
    load_row<VEC>(resid + (size_t)row * ldr, r, lane);
#pragma unroll
    for (int c = 0; c < VEC; ++c) o[c] = r[c] + o[c];
  }
  store_row<VEC>(dx + (size_t)row * lddx, o, lane);
}

// Backward of eot_ln_kernel: row (s, t) of g is LN_bwd(dy[s]; x[s, t]) at t = the first
// argmax of tokens[s] (eot_index, the forward's), zero elsewhere. One wave per row.
template <int VEC>
__global__ __launch_bounds__(256) void eot_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const int32_t* __restrict__ tokens,
                                                         const float* __restrict__ w, float* __restrict__ g,
                                                         int rows, int ctx) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  constexpr int D = 256 * VEC;
  const int s = row / ctx, t = row % ctx;
  const int best_i = eot_index(tokens, s, ctx, lane);
  float4_t o[VEC];
  if (t == best_i) {  // wave-uniform
    float4_t xv[VEC], dv[VEC];
    load_row<VEC>(x + (size_t)row * D, xv, lane);
    load_row<VEC>(dy + (size_t)s * D, dv, lane);
    layer_norm_bwd<VEC>(xv, dv, w, o, lane);
  } else {
#pragma unroll
    for (int c = 0; c < VEC; ++c) o[c] = float4_t{0.f, 0.f, 0.f, 0.f};
  }
  store_row<VEC>(g + (size_t)row * D, o, lane);
}

// ------------------------------------------------------------------ activations
// mode = the GEMM epilogue flag of the activation (AACLIP_EPI_GELU / _QGELU / _LEAKY)
__global__ __launch_bounds__(256) void act_kernel(int mode, const float* x, float* y, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  y[i] = mode == AACLIP_EPI_GELU ? gelu_erf(v) : mode == AACLIP_EPI_QGELU ? qgelu_exact(v) : leaky_relu(v);
}

// dx = dy * act_slope(ref) (common.h): ref = the pre-activation for GELU / QuickGELU, the
// OUTPUT for LeakyReLU.
__global__ __launch_bounds__(256) void act_bwd_kernel(int mode, const float* dy, const float* ref, float* dx,
                                                      size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float d = act_slope(mode, ref[i]);
  dx[i] = dy[i] * d;
}

// ------------------------------------------------------------------ adapter blend backward
// y = w u |x| / |u| + (1 - w) x (block_tail_kernel; adapter.py:131-136), a = sum dy u:
//   dx = (1 - w) dy + w (a / |u|) x / |x|         (the direct path and the path through |x|)
//   du = w (|x| / |u|) (dy - u a / |u|^2)
// Norms are sqrt(row_dot(x, x)), the forward's own call.
template <int VEC>
__global__ __launch_bounds__(256) void adapter_blend_bwd_kernel(const float* dy, const float* __restrict__ x,
                                                                const float* __restrict__ u, float aw, float* dx,
                                                                float* __restrict__ du, int rows) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  constexpr int D = 256 * VEC;
  float4_t gv[VEC], xv[VEC], uv[VEC];
  load_row<VEC>(dy + (size_t)row * D, gv, lane);
  load_row<VEC>(x + (size_t)row * D, xv, lane);
  load_row<VEC>(u + (size_t)row * D, uv, lane);
  const float xn = sqrtf(row_dot<VEC>(xv, xv));
  const float uq = row_dot<VEC>(uv, uv);
  const float un = sqrtf(uq);
  const float a = row_dot<VEC>(gv, uv);
  const float keep = 1.0f - aw;
  const float cx = aw * (a / un) / xn;
  const float cu = aw * (xn / un);
  const float au = a / uq;
  float4_t ox[VEC], ou[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ox[c][j] = keep * gv[c][j] + cx * xv[c][j];
      ou[c][j] = cu * (gv[c][j] - uv[c][j] * au);
    }
  store_row<VEC>(dx + (size_t)row * D, ox, lane);  // dx may be dy: read above, by the same lane
  store_row<VEC>(du + (size_t)row * D, ou, lane);
}

// ------------------------------------------------------------------ anchor backward
// T[:, col] = t = m / |m|, m = mean_s e_s / |e_s| (anchor_reduce_kernel). With g = dT[:, col]:
//   dm = (g - t (t . g)) / |m|;  de_s = (dm / n - eh_s (eh_s . dm / n)) / |e_s|, eh_s = e_s / |e_s|.
// One 256-thread block; thread j owns columns j, j + 256, ...; sums over s and over the
// columns run in index order.
__global__ __launch_bounds__(256) void anchor_reduce_bwd_kernel(const float* __restrict__ emb, int n, int dim,
                                                                const float* __restrict__ dT, int col, int ncols,
                                                                float* __restrict__ demb) {
  __shared__ float inv_norm[256];
  __shared__ float red[2][4];
  __shared__ float dm_s[1024];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int s = wid; s < n; s += 4) {
    float q = 0.f;
    for (int j = lane; j < dim; j += 64) {
      const float e = emb[(size_t)s * dim + j];
      q += e * e;
    }
    q = wave_sum(q);
    if (lane == 0) inv_norm[s] = 1.0f / sqrtf(q);
  }
  __syncthreads();
  float m_local[4], g_local[4];  // dim <= 1024
  float pm = 0.f, pg = 0.f;
  int cnt = 0;
  for (int j = threadIdx.x; j < dim; j += 256, ++cnt) {
    float acc = 0.f;
    for (int s = 0; s < n; ++s) acc += emb[(size_t)s * dim + j] * inv_norm[s];
    const float m = acc / (float)n;
    const float g = dT[(size_t)j * ncols + col];
    m_local[cnt] = m;
    g_local[cnt] = g;
    pm += m * m;
    pg += m * g;
  }
  pm = wave_sum(pm);
  pg = wave_sum(pg);
  if (lane == 0) {
    red[0][wid] = pm;
    red[1][wid] = pg;
  }
  __syncthreads();
  const float mm = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);  // |m|^2
  const float mg = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);  // m . g
  const float inv_m = 1.0f / sqrtf(mm);
  const float tg = mg * inv_m;  // t . g
  cnt = 0;
  for (int j = threadIdx.x; j < dim; j += 256, ++cnt)
    dm_s[j] = (g_local[cnt] - m_local[cnt] * inv_m * tg) * inv_m / (float)n;
  __syncthreads();
  for (int s = wid; s < n; s += 4) {
    const float in = inv_norm[s];
    float d = 0.f;
    for (int j = lane; j < dim; j += 64) d += emb[(size_t)s * dim + j] * in * dm_s[j];
    d = wave_sum(d);
    for (int j = lane; j < dim; j += 64) {
      const float eh = emb[(size_t)s * dim + j] * in;
      demb[(size_t)s * dim + j] = (dm_s[j] - eh * d) * in;
    }
  }
}

// ------------------------------------------------------------------ Linear weight gradient
// dW[n, k] = sum_m dY[m, n] X[m, k]. Rows are cut into chunks of kWgradRows (a function of M
// alone); workgroup (k tile, n tile, chunk) accumulates a 64 x 64 tile over its chunk's rows in
// index order with plain fp32 FMAs (16 x 16 threads, 4 x 4 outputs each, rows staged through
// LDS 16 at a time) into partial[chunk][N][K]; the finalize pass sums the chunks in index
// order in fp64, as patch_logits_bwd_finalize_kernel does.
constexpr int kWgradRows = AACLIP_WGRAD_ROWS;

__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float* __restrict__ dY, int64_t lddy,
                                                           const float* __restrict__ X, int64_t ldx, int M, int N,
                                                           int K, float* __restrict__ partial) {
  __shared__ float Ys[16][64];
  __shared__ float Xs[16][64];
  const int t = threadIdx.x, tn = t >> 4, tk = t & 15;
  const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64, ch = blockIdx.z;
  const int m_end = min((ch + 1) * kWgradRows, M);
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
  for (int m0 = ch * kWgradRows; m0 < m_end; m0 += 16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = t + 256 * j, r = f >> 6, c = f & 63;
      const bool ok = m0 + r < m_end;
      Ys[r][c] = ok ? dY[(size_t)(m0 + r) * lddy + n0 + c] : 0.f;
      Xs[r][c] = ok ? X[(size_t)(m0 + r) * ldx + k0 + c] : 0.f;
    }
    __syncthreads();
    const int nr = min(16, m_end - m0);
    for (int r = 0; r < nr; ++r) {
      float yv[4], xv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        yv[a] = Ys[r][tn + 16 * a];
        xv[a] = Xs[r][tk + 16 * a];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = fmaf(yv[a], xv[c], acc[a][c]);
    }
    __syncthreads();
  }
  float* pp = partial + (size_t)ch * N * K;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) pp[(size_t)(n0 + tn + 16 * a) * K + k0 + tk + 16 * c] = acc[a][c];
}

__global__ __launch_bounds__(256) void linear_wgrad_finalize_kernel(const float* __restrict__ partial, int nchunk,
                                                                    int N, int K, float* __restrict__ dW,
                                                                    int64_t lddw) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t nk = (size_t)N * K;
  if (e >= nk) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; ++c) s += (double)partial[(size_t)c * nk + e];
  dW[(e / K) * lddw + e % K] = (float)s;
}

}  // namespace

extern "C" int aaclip_attention_bwd(const float* qkv, const float* dout, float* dqkv, int batch, int seq, int heads,
                                    int head_dim, int flags, void* stream) {
  AACLIP_REQUIRE(qkv && dout && dqkv && dqkv != qkv);
  AACLIP_REQUIRE(head_dim == AB_HD && seq >= 1 && seq <= AB_MAX_SEQ && batch > 0 && heads > 0 && heads <= 1024);
  AACLIP_REQUIRE((flags & ~AACLIP_ATTN_CAUSAL) == 0);
  AACLIP_REQUIRE((int64_t)batch * heads < (1ll << 31));
  AACLIP_REQUIRE(aligned4(qkv) && aligned4(dout) && aligned4(dqkv));
  static unsigned done = 0;
  if (!lds_attr_once((const void*)attention_bwd_kernel, AB_MAX_LDS, done)) return AACLIP_ERR_LAUNCH;
  const int lds = (4 * seq * AB_LD + 2 * seq * (seq | 1)) * (int)sizeof(float);
  attention_bwd_kernel<<<(unsigned)(batch * heads), 256, lds, (hipStream_t)stream>>>(
      qkv, dout, dqkv, seq, heads, flags & AACLIP_ATTN_CAUSAL);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* w,
                                    const float* residual, int64_t ldr, float* dx, int64_t lddx, int rows,
                                    int width, void* stream) {
  AACLIP_REQUIRE(dy && x && w && dx && rows >= 0 && (width == 768 || width == 1024));
  AACLIP_REQUIRE(lddy >= width && ldx >= width && lddx >= width && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0);
  AACLIP_REQUIRE(!residual || (ldr >= width && ldr % 4 == 0 && aligned16(residual)));
  AACLIP_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(w) && aligned16(dx));
  AACLIP_REQUIRE(dx != x && (dx != dy || lddx == lddy) && (dx != residual || lddx == ldr));
  if (rows == 0) return AACLIP_OK;
  DISPATCH_VEC(width, layernorm_bwd_kernel<V><<<ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(
                          dy, lddy, x, ldx, w, residual, ldr, dx, lddx, rows));
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_eot_ln_bwd(const float* dy, const float* x, const int32_t* tokens, const float* w, float* g,
                                 int n_seq, int ctx, int width, void* stream) {
  AACLIP_REQUIRE(dy && x && tokens && w && g && n_seq > 0 && ctx > 0 && (width == 768 || width == 1024));
  AACLIP_REQUIRE((int64_t)n_seq * ctx < (1ll << 31) && g != x && g != dy);
  AACLIP_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(w) && aligned16(g) && aligned4(tokens));
  const int rows = n_seq * ctx;
  DISPATCH_VEC(width, eot_ln_bwd_kernel<V><<<ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(dy, x, tokens, w, g,
                                                                                              rows, ctx));
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_act(int mode, const float* x, float* y, int64_t n, void* stream) {
  AACLIP_REQUIRE(act_mode_ok(mode) && x && y && n >= 0 && n < (256ll << 31) && aligned4(x) && aligned4(y));
  if (n == 0) return AACLIP_OK;
  act_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(mode, x, y, (size_t)n);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_act_bwd(int mode, const float* dy, const float* ref, float* dx, int64_t n, void* stream) {
  AACLIP_REQUIRE(act_mode_ok(mode) && dy && ref && dx && n >= 0 && n < (256ll << 31));
  AACLIP_REQUIRE(aligned4(dy) && aligned4(ref) && aligned4(dx));
  if (n == 0) return AACLIP_OK;
  act_bwd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(mode, dy, ref, dx, (size_t)n);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_adapter_blend_bwd(const float* dy, const float* x, const float* u, float adapt_weight,
                                        float* dx, float* du, int rows, int width, void* stream) {
  AACLIP_REQUIRE(dy && x && u && dx && du && rows >= 0 && (width == 768 || width == 1024));
  AACLIP_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(u) && aligned16(dx) && aligned16(du));
  AACLIP_REQUIRE(dx != x && dx != u && du != x && du != u && du != dy && du != dx);
  if (rows == 0) return AACLIP_OK;
  DISPATCH_VEC(width, adapter_blend_bwd_kernel<V><<<ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(
                          dy, x, u, adapt_weight, dx, du, rows));
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_anchor_reduce_bwd(const float* emb, int n, int dim, const float* dT, int col, int ncols,
                                        float* demb, void* stream) {
  AACLIP_REQUIRE(emb && dT && demb && demb != emb);
  AACLIP_REQUIRE(n > 0 && n <= 256 && dim > 0 && dim <= 1024 && col >= 0 && col < ncols);
  AACLIP_REQUIRE(aligned4(emb) && aligned4(dT) && aligned4(demb));
  anchor_reduce_bwd_kernel<<<1, 256, 0, (hipStream_t)stream>>>(emb, n, dim, dT, col, ncols, demb);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_linear_wgrad_workspace(int M, int N, int K, size_t* bytes) {
  AACLIP_REQUIRE(bytes && M >= 1 && N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0);
  *bytes = (size_t)ceil_div(M, kWgradRows) * N * K * sizeof(float);
  return AACLIP_OK;
}

extern "C" int aaclip_linear_wgrad(const float* dY, int64_t lddy, const float* X, int64_t ldx, int M, int N, int K,
                                   float* workspace, size_t workspace_bytes, float* dW, int64_t lddw,
                                   void* stream) {
  AACLIP_REQUIRE(dY && X && workspace && dW && M >= 1 && N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0);
  AACLIP_REQUIRE(lddy >= N && ldx >= K && lddw >= K);
  AACLIP_REQUIRE(aligned4(dY) && aligned4(X) && aligned4(workspace) && aligned4(dW));
  const int nchunk = ceil_div(M, kWgradRows);
  AACLIP_REQUIRE(N / 64 <= 65535 && nchunk <= 65535);
  AACLIP_REQUIRE(workspace_bytes >= (size_t)nchunk * N * K * sizeof(float));
  const size_t nk = (size_t)N * K;
  AACLIP_REQUIRE((nk + 255) / 256 < (1ull << 31));
  AACLIP_REQUIRE((const void*)dW != (const void*)dY && (const void*)dW != (const void*)X && dW != workspace);
  hipStream_t s = (hipStream_t)stream;
  linear_wgrad_kernel<<<dim3(K / 64, N / 64, nchunk), 256, 0, s>>>(dY, lddy, X, ldx, M, N, K, workspace);
  AACLIP_CHECK_LAUNCH();
  linear_wgrad_finalize_kernel<<<(unsigned)((nk + 255) / 256), 256, 0, s>>>(workspace, nchunk, N, K, dW, lddw);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
