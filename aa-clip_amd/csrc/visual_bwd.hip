// Backward of the adapted visual tower (stage 2: train.py:117-174 trains image_adapter only):
// the attention backward for long sequences (577 / 1025 / 1370 tokens), the level tap + ln_post
// backward and the L2-normalise backward of the projection tail. Everything else of the
// stage-2 backward reuses text_bwd.hip's entries and aaclip_gemm on transposed weights.
//
// All fp32, deterministic (no floating-point atomics, fixed reduction orders: two launches
// give the same bits) and image / row local.
#include "common.h"
#include "rowmath.h"  // the row layout, the LayerNorm statistics and layer_norm_bwd, shared with rows.hip

namespace {

// ------------------------------------------------------------------ tiled attention backward
// fp32 on v_mfma_f32_16x16x4f32, non-causal, head_dim 64, any sequence length. With
// S = q k^T / 8, P = softmax(S), dP = dout v^T, D_i = dout_i . out_i, dS = P (dP - D):
//   dq = dS k / 8,  dk = dS^T q / 8,  dv = P^T dout.
// Two launches, 4 waves x 16 rows each, tiles of 64 rows staged through registers into
// row-padded LDS (68 floats per row: both fragment read patterns below hit 64 different
// banks), the next tile's global loads in flight while the current one is computed.
//
// Query-block kernel, one workgroup per (image, head, 64 queries). Same swapped layout as
// attn_f32_kernel: S^T = K . Q'^T (Q' = Q log2(e) / 8) puts the scores of query fr on the 4
// lanes {fr, fr+16, fr+32, fr+48}, 16 keys of a tile each. Pass 1 over the key tiles keeps a
// running (max, sum) per lane and merges the 4 lanes at the end: lse (log2 domain). D comes
// from the diagonal of an out . dout^T MFMA, i.e. with the operand roles and the summation
// order of dP, so that at seq == 1 (out == v) dP - D is exactly 0. Both go to the workspace.
// Pass 2 forms P = exp2(S' - lse), dP^T = V . dout^T and dS^T in registers, which are the B
// operand of dQ^T += K^T . dS^T. Keys past the end get P = 0 exactly.
//
// Key-block kernel, one workgroup per (image, head, 64 keys), walks the query tiles in index
// order with the stored lse and D: S = Q' . K^T and dP = dout . V^T put the 64 queries of a
// tile on the accumulator rows, P and dS are the B operands of dV^T += dout^T . P and
// dK^T += Q'^T . dS (times ln 2 = 1 / (8 log2(e) / 8) at the end). Queries past the end get
// P = dS = 0 exactly.
//
// Every output row is summed by one wave in a fixed order; rows past the end are loaded from
// the last valid row (finite values) and never stored.
constexpr int VT = 64, VLD = 68, VHD = 64;
constexpr float kQScale = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
constexpr float kLn2 = 0.69314718055994530942f;

__device__ __forceinline__ float4_t mfma4(float a, float b, const float4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// thread t moves float4 number t + 256 j (j < 4) of a [64][64] tile whose rows lie `ld` apart
__device__ __forceinline__ void tile_load(const float* src, int64_t ld, int row0, int N, int t, float4_t (&reg)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f = t + 256 * j, r = f >> 4, c4 = f & 15;
    reg[j] = *(const float4_t*)(src + (size_t)min(row0 + r, N - 1) * ld + 4 * c4);
  }
}
__device__ __forceinline__ void tile_store(float (*dst)[VLD], int t, const float4_t (&reg)[4], float scale) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f = t + 256 * j, r = f >> 4, c4 = f & 15;
    *(float4_t*)&dst[r][4 * c4] = reg[j] * scale;
  }
}

__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                         const float* __restrict__ dout, float* __restrict__ dqkv,
                                                         float* __restrict__ lse_ws, float* __restrict__ d_ws, int N,
                                                         int H) {
  __shared__ __attribute__((aligned(16))) float Ks[VT][VLD];
  __shared__ __attribute__((aligned(16))) float Vs[VT][VLD];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int HDt = H * VHD;
  const int64_t ld = 3 * (int64_t)HDt;
  const float* base = qkv + (size_t)b * N * ld + h * VHD;
  const int q = blockIdx.x * VT + wid * 16 + fr;  // this lane's query
  const int qc = min(q, N - 1);
  const size_t orow = ((size_t)b * N + qc) * HDt + h * VHD;

  float qv[16], dov[16];  // Q'[q][4 s + fq], dout[q][4 s + fq]
  float4_t dd = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    qv[s4] = base[(size_t)qc * ld + 4 * s4 + fq] * kQScale;
    dov[s4] = dout[orow + 4 * s4 + fq];
    dd = mfma4(out[orow + 4 * s4 + fq], dov[s4], dd);  // dd[e] = out[q0 + 4 fq + e] . dout[q0 + fr]
  }
  // the diagonal: query fr's own product sits in lane (fr, fq = fr / 4), element fr % 4
  const float sel = (fr & 3) == 0 ? dd[0] : (fr & 3) == 1 ? dd[1] : (fr & 3) == 2 ? dd[2] : dd[3];
  const float Dq = __shfl(sel, fr + 16 * (fr >> 2), 64);

  const int ntiles = (N + VT - 1) / VT;
  float4_t kreg[4], vreg[4];

  // ---- pass 1: row log-sum-exp (log2 domain)
  float m = -INFINITY, l = 0.f;
  tile_load(base + HDt, ld, 0, N, t, kreg);
  tile_store(Ks, t, kreg, 1.0f);
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) tile_load(base + HDt, ld, (tile + 1) * VT, N, t, kreg);
    float4_t st[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      st[kb] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) st[kb] = mfma4(Ks[kb * 16 + fr][4 * s4 + fq], qv[s4], st[kb]);
    }
    // st[kb][e] = score of key tile * 64 + 16 kb + 4 fq + e for query q
    const int lim = N - tile * VT - 4 * fq;  // valid: 16 kb + e < lim
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (16 * kb + e < lim) mx = fmaxf(mx, st[kb][e]);
    const float mn = fmaxf(m, mx);
    const float mu = mn == -INFINITY ? 0.f : mn;  // no valid key yet on this lane: l stays 0
    float ls = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 4; ++e) ls += (16 * kb + e < lim) ? __builtin_amdgcn_exp2f(st[kb][e] - mu) : 0.f;
    l = l * __builtin_amdgcn_exp2f(m - mu) + ls;
    m = mn;
    __syncthreads();
    if (tile + 1 < ntiles) {
      tile_store(Ks, t, kreg, 1.0f);
      __syncthreads();
    }
  }
  // merge the query's 4 lanes (key 0 is on lane group 0: the merged max is finite)
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
    const float mn = fmaxf(m, mo);
    const float mu = mn == -INFINITY ? 0.f : mn;
    l = l * __builtin_amdgcn_exp2f(m - mu) + lo * __builtin_amdgcn_exp2f(mo - mu);
    m = mn;
  }
  // one value per query for every lane and for the key-block kernel: lane group 0's
  const float lse = __shfl(m + log2f(l), fr, 64);
  if (fq == 0 && q < N) {
    lse_ws[(size_t)bh * N + q] = lse;
    d_ws[(size_t)bh * N + q] = Dq;
  }

  // ---- pass 2: dQ
  float4_t dq[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dq[db] = float4_t{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  tile_load(base + HDt, ld, 0, N, t, kreg);
  tile_load(base + 2 * HDt, ld, 0, N, t, vreg);
  tile_store(Ks, t, kreg, 1.0f);
  tile_store(Vs, t, vreg, 1.0f);
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) {
      tile_load(base + HDt, ld, (tile + 1) * VT, N, t, kreg);
      tile_load(base + 2 * HDt, ld, (tile + 1) * VT, N, t, vreg);
    }
    float4_t st[4], dp[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      st[kb] = float4_t{0.f, 0.f, 0.f, 0.f};
      dp[kb] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        st[kb] = mfma4(Ks[kb * 16 + fr][4 * s4 + fq], qv[s4], st[kb]);
        dp[kb] = mfma4(Vs[kb * 16 + fr][4 * s4 + fq], dov[s4], dp[kb]);
      }
    }
    const int lim = N - tile * VT - 4 * fq;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = (16 * kb + e < lim) ? __builtin_amdgcn_exp2f(st[kb][e] - lse) : 0.f;
        st[kb][e] = p * (dp[kb][e] - Dq);  // dS[q][key]
      }
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) dq[db] = mfma4(Ks[kb * 16 + 4 * fq + i][db * 16 + fr], st[kb][i], dq[db]);
    __syncthreads();
    if (tile + 1 < ntiles) {
      tile_store(Ks, t, kreg, 1.0f);
      tile_store(Vs, t, vreg, 1.0f);
      __syncthreads();
    }
  }
  if (q < N) {  // dq[db][e] = dQ[q][16 db + 4 fq + e]
    float* op = dqkv + ((size_t)b * N + q) * ld + h * VHD + 4 * fq;
#pragma unroll
    for (int db = 0; db < 4; ++db) *(float4_t*)(op + 16 * db) = dq[db] * 0.125f;
  }
}

__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float* __restrict__ qkv,
                                                          const float* __restrict__ dout, float* __restrict__ dqkv,
                                                          const float* __restrict__ lse_ws,
                                                          const float* __restrict__ d_ws, int N, int H) {
  __shared__ __attribute__((aligned(16))) float Qs[VT][VLD];
  __shared__ __attribute__((aligned(16))) float Os[VT][VLD];
  __shared__ __attribute__((aligned(16))) float Ls[VT];
  __shared__ __attribute__((aligned(16))) float Ds[VT];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int HDt = H * VHD;
  const int64_t ld = 3 * (int64_t)HDt;
  const float* base = qkv + (size_t)b * N * ld + h * VHD;
  const float* dob = dout + (size_t)b * N * HDt + h * VHD;
  const int k = blockIdx.x * VT + wid * 16 + fr;  // this lane's key
  const int kc = min(k, N - 1);

  float kv[16], vv[16];  // K[k][4 s + fq], V[k][4 s + fq]
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    kv[s4] = base[(size_t)kc * ld + HDt + 4 * s4 + fq];
    vv[s4] = base[(size_t)kc * ld + 2 * HDt + 4 * s4 + fq];
  }
  float4_t dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    dk[db] = float4_t{0.f, 0.f, 0.f, 0.f};
    dv[db] = float4_t{0.f, 0.f, 0.f, 0.f};
  }

  const int ntiles = (N + VT - 1) / VT;
  float4_t qreg[4], oreg[4];
  float lreg = 0.f, dreg = 0.f;
  auto load_tile = [&](int tile) {
    tile_load(base, ld, tile * VT, N, t, qreg);
    tile_load(dob, HDt, tile * VT, N, t, oreg);
    if (t < VT) {
      const size_t i = (size_t)bh * N + min(tile * VT + t, N - 1);
      lreg = lse_ws[i];
      dreg = d_ws[i];
    }
  };
  auto store_tile = [&]() {
    tile_store(Qs, t, qreg, kQScale);
    tile_store(Os, t, oreg, 1.0f);
    if (t < VT) {
      Ls[t] = lreg;
      Ds[t] = dreg;
    }
  };
  load_tile(0);
  store_tile();
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) load_tile(tile + 1);
    float4_t st[4], dp[4];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      st[qb] = float4_t{0.f, 0.f, 0.f, 0.f};
      dp[qb] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        st[qb] = mfma4(Qs[qb * 16 + fr][4 * s4 + fq], kv[s4], st[qb]);
        dp[qb] = mfma4(Os[qb * 16 + fr][4 * s4 + fq], vv[s4], dp[qb]);
      }
    }
    // st[qb][e] = score, dp[qb][e] = dP of query tile * 64 + 16 qb + 4 fq + e for key k
    const int lim = N - tile * VT - 4 * fq;  // valid: 16 qb + e < lim
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const float4_t l4 = *(const float4_t*)&Ls[qb * 16 + 4 * fq];
      const float4_t d4 = *(const float4_t*)&Ds[qb * 16 + 4 * fq];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = (16 * qb + e < lim) ? __builtin_amdgcn_exp2f(st[qb][e] - l4[e]) : 0.f;
        st[qb][e] = p;
        dp[qb][e] = p * (dp[qb][e] - d4[e]);
      }
    }
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int qb = 0; qb < 4; ++qb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dv[db] = mfma4(Os[qb * 16 + 4 * fq + i][db * 16 + fr], st[qb][i], dv[db]);
          dk[db] = mfma4(Qs[qb * 16 + 4 * fq + i][db * 16 + fr], dp[qb][i], dk[db]);
        }
    __syncthreads();
    if (tile + 1 < ntiles) {
      store_tile();
      __syncthreads();
    }
  }
  if (k < N) {  // d*[db][e] = d*[k][16 db + 4 fq + e]
    float* op = dqkv + ((size_t)b * N + k) * ld + HDt + h * VHD + 4 * fq;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      *(float4_t*)(op + 16 * db) = dk[db] * kLn2;
      *(float4_t*)(op + HDt + 16 * db) = dv[db];
    }
  }
}

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

extern "C" int aaclip_attention_bwd_tiled_workspace(int batch, int seq, int heads, size_t* bytes) {
  AACLIP_REQUIRE(bytes && batch > 0 && seq >= 1 && heads > 0);
  *bytes = 2 * (size_t)batch * heads * seq * sizeof(float);
  return AACLIP_OK;
}

extern "C" int aaclip_attention_bwd_tiled(const float* qkv, const float* out, const float* dout, float* dqkv,
                                          int batch, int seq, int heads, int head_dim, float* workspace,
                                          size_t workspace_bytes, void* stream) {
  AACLIP_REQUIRE(qkv && out && dout && dqkv && workspace);
  AACLIP_REQUIRE(head_dim == VHD && seq >= 1 && batch > 0 && heads > 0);
  AACLIP_REQUIRE((int64_t)batch * heads <= 65535 && (int64_t)batch * seq < (1ll << 31));
  AACLIP_REQUIRE(dqkv != qkv && dqkv != out && dqkv != dout);
  AACLIP_REQUIRE((const float*)workspace != qkv && (const float*)workspace != out &&
                 (const float*)workspace != dout && workspace != dqkv);
  AACLIP_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && aligned16(workspace));
  const size_t n = (size_t)batch * heads * seq;
  AACLIP_REQUIRE(workspace_bytes >= 2 * n * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ceil_div(seq, VT), batch * heads);
  float* lse = workspace;
  float* dsum = workspace + n;
  attn_bwd_q_kernel<<<grid, 256, 0, s>>>(qkv, out, dout, dqkv, lse, dsum, seq, heads);
  AACLIP_CHECK_LAUNCH();
  attn_bwd_kv_kernel<<<grid, 256, 0, s>>>(qkv, dout, dqkv, lse, dsum, seq, heads);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

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
