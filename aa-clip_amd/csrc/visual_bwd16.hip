// Stage-2 backward in bf16 mixed precision: the attention backward on bf16 MFMA, the c_fc
// activation and its backward with 16-bit I/O, and the row cast between the fp32 gradient
// stream and the 16-bit GEMM inputs. Everything else of the bf16 step is aaclip_gemm in bf16 on
// the transposed weights and the fp32 row kernels of text_bwd.hip / visual_bwd.hip.
//
// Deterministic (no atomics, fixed reduction orders: two launches give the same bits) and
// image / row local, as visual_bwd.hip.
#include "common.h"

namespace {

// ------------------------------------------------------------------ attention backward, bf16
// aaclip_attention_bwd_tiled's two launches on v_mfma_f32_16x16x32_bf16, non-causal, head_dim 64,
// any sequence length; fp32 softmax statistics, fp32 accumulation, bf16 operands. With
// S' = q' k^T (q' = q log2(e) / 8: folded into q by the caller under AACLIP_ATTN_Q_PRESCALED,
// else applied to the bf16 q at load and rounded to bf16 again), P = exp2(S' - lse),
// dP = dout v^T, D_i = dout_i . out_i and dS = P (dP - D):
//   dq' = ln2 dS k   (prescaled: the gradient of q';  else dq = dS k / 8),
//   dk  = ln2 dS^T q',   dv = P^T dout.
// P and dS enter their second product rounded to bf16; dS is formed from the fp32 P.
//
// 4 waves x 16 rows per workgroup, tiles of 64 rows staged through registers into an
// XOR-swizzled [64][128 B] LDS image (attention.hip's), the next tile's global loads in flight
// while the current one is computed. MFMA maps (c = lane & 15, g = lane >> 4): A[row c][8 g + j],
// B[8 g + j][col c], accumulator element i = D[row 4 g + i][col c].
//
// Every product is oriented so that the next one sums over its accumulator ROW index: P and
// dS then go back in as B operands straight from the registers. Two stacked 16 x 16
// accumulators (tile rows 32 s + 4 g + i and 32 s + 16 + 4 g + i) are the 8 values of k-step s,
// and the other operand is read with the same permutation of the summed index by the
// transposing LDS read ds_read_b64_tr_b16 (row-major tile in, column-major fragment out). No
// accumulator crosses LDS.
//
// Query-block kernel, one workgroup per (image, head, 64 queries), the query on the lane:
// S'^T = K . Q'^T and dP^T = V . dout^T have the key on the accumulator row. Pass 1 keeps a
// running (max, sum) per lane and merges the query's 4 lanes: lse (log2 domain). D is the
// diagonal of an out . dout^T MFMA with dP's operand roles and summation order, so that at
// seq == 1 (out == v) dP - D is exactly 0. Both go to the workspace. Pass 2 forms dS^T, the B
// operand of dQ^T += K^T . dS^T. Keys past the end get P = 0 exactly.
//
// Key-block kernel, one workgroup per (image, head, 64 keys), the key on the lane, walks the
// query tiles in index order with the stored lse and D: S' = Q' . K^T and dP = dout . V^T have
// the query on the accumulator row; P and dS are the B operands of dV^T += dout^T . P and
// dK^T += Q'^T . dS. Queries past the end get P = dS = 0 exactly.
//
// Rows past the end are loaded from the last valid row (finite values) and never stored.
constexpr int WT = 64, WHD = 64;
constexpr float kQScale16 = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
constexpr float kLn2_16 = 0.69314718055994530942f;

__device__ __forceinline__ short4_t tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(p));
}
// byte offset of (row, 16-B chunk) in a swizzled [64][128 B] tile
__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

__device__ __forceinline__ bf16x8_t scale8(const bf16x8_t& v, float s) {
  bf16x8_t r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (__bf16)((float)v[e] * s);
  return r;
}

// thread t moves 16-B chunk t + 256 j (j < 2) of a [64][64] bf16 tile whose rows lie `ld` elements apart
__device__ __forceinline__ void tile_load16(const uint16_t* src, int64_t ld, int row0, int N, int t,
                                            bf16x8_t (&reg)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = t + 256 * j, r = f >> 3, ch = f & 7;
    reg[j] = *(const bf16x8_t*)(src + (size_t)min(row0 + r, N - 1) * ld + 8 * ch);
  }
}
__device__ __forceinline__ void tile_store16(char* dst, int t, const bf16x8_t (&reg)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = t + 256 * j, r = f >> 3, ch = f & 7;
    *(bf16x8_t*)(dst + swz(r, ch)) = reg[j];
  }
}
// A operand, rows by rows: tile row 16 rb + c, columns 32 ks + 8 g .. + 7
__device__ __forceinline__ bf16x8_t row_frag(const char* tile, int rb, int ks, int c, int g) {
  return *(const bf16x8_t*)(tile + swz(rb * 16 + c, ks * 4 + g));
}
// A operand of a product that sums over the tile's rows: column 16 db + c of tile rows
// 32 ks + 4 g + {0..3} and 32 ks + 16 + 4 g + {0..3}, the order of pack_acc's B operand
__device__ __forceinline__ bf16x8_t col_frag(const char* tile, int db, int ks, int c, int g) {
  const int qq = c >> 2, pp = c & 3;
  const int chunk = db * 2 + (pp >> 1);
  const int r0 = ks * 32 + 4 * g + qq;
  const short4_t lo = tr_read(tile + swz(r0, chunk) + (pp & 1) * 8);
  const short4_t hi = tr_read(tile + swz(r0 + 16, chunk) + (pp & 1) * 8);
  return __builtin_bit_cast(bf16x8_t, short8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
}
// two stacked accumulators as the B operand of k-step s (RNE to bf16)
__device__ __forceinline__ bf16x8_t pack_acc(const float4_t& a, const float4_t& b) {
  bf16x8_t v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = (__bf16)a[i];
    v[4 + i] = (__bf16)b[i];
  }
  return v;
}
__device__ __forceinline__ void store4_bf16(uint16_t* p, const float4_t& v, float s) {
  *(uint2*)p = uint2{pack_bf16x2(v[0] * s, v[1] * s), pack_bf16x2(v[2] * s, v[3] * s)};
}

__global__ __launch_bounds__(256) void attn_bwd16_q_kernel(const uint16_t* __restrict__ qkv,
                                                           const uint16_t* __restrict__ out,
                                                           const uint16_t* __restrict__ dout,
                                                           uint16_t* __restrict__ dqkv, float* __restrict__ lse_ws,
                                                           float* __restrict__ d_ws, int N, int H, int prescaled) {
  __shared__ __attribute__((aligned(16))) char Ks[WT * 128];
  __shared__ __attribute__((aligned(16))) char Vs[WT * 128];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int HDt = H * WHD;
  const int64_t ld = 3 * (int64_t)HDt;
  const uint16_t* base = qkv + (size_t)b * N * ld + h * WHD;
  const int q = blockIdx.x * WT + wid * 16 + c;  // this lane's query
  const int qc = min(q, N - 1);
  const size_t orow = ((size_t)b * N + qc) * HDt + h * WHD;

  bf16x8_t qf[2], dof[2];  // Q'[q][32 ks + 8 g + j], dout[q][32 ks + 8 g + j]
  float4_t dd = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    qf[ks] = *(const bf16x8_t*)(base + (size_t)qc * ld + 32 * ks + 8 * g);
    if (!prescaled) qf[ks] = scale8(qf[ks], kQScale16);
    dof[ks] = *(const bf16x8_t*)(dout + orow + 32 * ks + 8 * g);
    // dd[i] = out[q0 + 4 g + i] . dout[q0 + c]: out rows as dP's V rows, dout as its B operand
    dd = mfma16(*(const bf16x8_t*)(out + orow + 32 * ks + 8 * g), dof[ks], dd);
  }
  // the diagonal: query c's own product sits in lane (c, g = c / 4), element c % 4
  const float sel = (c & 3) == 0 ? dd[0] : (c & 3) == 1 ? dd[1] : (c & 3) == 2 ? dd[2] : dd[3];
  const float Dq = __shfl(sel, c + 16 * (c >> 2), 64);

  const int ntiles = (N + WT - 1) / WT;
  bf16x8_t kreg[2], vreg[2];

  // ---- pass 1: row log-sum-exp (log2 domain)
  float m = -INFINITY, l = 0.f;
  tile_load16(base + HDt, ld, 0, N, t, kreg);
  tile_store16(Ks, t, kreg);
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) tile_load16(base + HDt, ld, (tile + 1) * WT, N, t, kreg);
    float4_t st[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      st[kb] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) st[kb] = mfma16(row_frag(Ks, kb, ks, c, g), qf[ks], st[kb]);
    }
    // st[kb][i] = score of key tile * 64 + 16 kb + 4 g + i for query q
    const int lim = N - tile * WT - 4 * g;  // valid: 16 kb + i < lim
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (16 * kb + i < lim) mx = fmaxf(mx, st[kb][i]);
    const float mn = fmaxf(m, mx);
    const float mu = mn == -INFINITY ? 0.f : mn;  // no valid key yet on this lane: l stays 0
    float ls = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) ls += (16 * kb + i < lim) ? __builtin_amdgcn_exp2f(st[kb][i] - mu) : 0.f;
    l = l * __builtin_amdgcn_exp2f(m - mu) + ls;
    m = mn;
    __syncthreads();
    if (tile + 1 < ntiles) {
      tile_store16(Ks, t, kreg);
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
  const float lse = __shfl(m + log2f(l), c, 64);
  if (g == 0 && q < N) {
    lse_ws[(size_t)bh * N + q] = lse;
    d_ws[(size_t)bh * N + q] = Dq;
  }

  // ---- pass 2: dQ
  float4_t dq[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dq[db] = float4_t{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  tile_load16(base + HDt, ld, 0, N, t, kreg);
  tile_load16(base + 2 * HDt, ld, 0, N, t, vreg);
  tile_store16(Ks, t, kreg);
  tile_store16(Vs, t, vreg);
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) {
      tile_load16(base + HDt, ld, (tile + 1) * WT, N, t, kreg);
      tile_load16(base + 2 * HDt, ld, (tile + 1) * WT, N, t, vreg);
    }
    float4_t st[4], dp[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      st[kb] = float4_t{0.f, 0.f, 0.f, 0.f};
      dp[kb] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        st[kb] = mfma16(row_frag(Ks, kb, ks, c, g), qf[ks], st[kb]);
        dp[kb] = mfma16(row_frag(Vs, kb, ks, c, g), dof[ks], dp[kb]);
      }
    }
    const int lim = N - tile * WT - 4 * g;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = (16 * kb + i < lim) ? __builtin_amdgcn_exp2f(st[kb][i] - lse) : 0.f;
        st[kb][i] = p * (dp[kb][i] - Dq);  // dS[q][key]
      }
    const bf16x8_t dsf[2] = {pack_acc(st[0], st[1]), pack_acc(st[2], st[3])};
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) dq[db] = mfma16(col_frag(Ks, db, ks, c, g), dsf[ks], dq[db]);
    __syncthreads();
    if (tile + 1 < ntiles) {
      tile_store16(Ks, t, kreg);
      tile_store16(Vs, t, vreg);
      __syncthreads();
    }
  }
  if (q < N) {  // dq[db][i] = dQ[q][16 db + 4 g + i]
    uint16_t* op = dqkv + ((size_t)b * N + q) * ld + h * WHD + 4 * g;
    const float s = prescaled ? kLn2_16 : 0.125f;
#pragma unroll
    for (int db = 0; db < 4; ++db) store4_bf16(op + 16 * db, dq[db], s);
  }
}

__global__ __launch_bounds__(256) void attn_bwd16_kv_kernel(const uint16_t* __restrict__ qkv,
                                                            const uint16_t* __restrict__ dout,
                                                            uint16_t* __restrict__ dqkv,
                                                            const float* __restrict__ lse_ws,
                                                            const float* __restrict__ d_ws, int N, int H,
                                                            int prescaled) {
  __shared__ __attribute__((aligned(16))) char Qs[WT * 128];
  __shared__ __attribute__((aligned(16))) char Os[WT * 128];
  __shared__ __attribute__((aligned(16))) float Ls[WT];
  __shared__ __attribute__((aligned(16))) float Ds[WT];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int HDt = H * WHD;
  const int64_t ld = 3 * (int64_t)HDt;
  const uint16_t* base = qkv + (size_t)b * N * ld + h * WHD;
  const uint16_t* dob = dout + (size_t)b * N * HDt + h * WHD;
  const int k = blockIdx.x * WT + wid * 16 + c;  // this lane's key
  const int kc = min(k, N - 1);

  bf16x8_t kf[2], vf[2];  // K[k][32 ks + 8 g + j], V[k][32 ks + 8 g + j]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    kf[ks] = *(const bf16x8_t*)(base + (size_t)kc * ld + HDt + 32 * ks + 8 * g);
    vf[ks] = *(const bf16x8_t*)(base + (size_t)kc * ld + 2 * HDt + 32 * ks + 8 * g);
  }
  float4_t dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    dk[db] = float4_t{0.f, 0.f, 0.f, 0.f};
    dv[db] = float4_t{0.f, 0.f, 0.f, 0.f};
  }

  const int ntiles = (N + WT - 1) / WT;
  bf16x8_t qreg[2], oreg[2];
  float lreg = 0.f, dreg = 0.f;
  auto load_tile = [&](int tile) {
    tile_load16(base, ld, tile * WT, N, t, qreg);
    tile_load16(dob, HDt, tile * WT, N, t, oreg);
    if (t < WT) {
      const size_t i = (size_t)bh * N + min(tile * WT + t, N - 1);
      lreg = lse_ws[i];
      dreg = d_ws[i];
    }
  };
  auto store_tile = [&]() {
    if (!prescaled) {  // the query-block kernel's Q': the same product, the same rounding
      qreg[0] = scale8(qreg[0], kQScale16);
      qreg[1] = scale8(qreg[1], kQScale16);
    }
    tile_store16(Qs, t, qreg);
    tile_store16(Os, t, oreg);
    if (t < WT) {
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
      for (int ks = 0; ks < 2; ++ks) {
        st[qb] = mfma16(row_frag(Qs, qb, ks, c, g), kf[ks], st[qb]);
        dp[qb] = mfma16(row_frag(Os, qb, ks, c, g), vf[ks], dp[qb]);
      }
    }
    // st[qb][i] = score, dp[qb][i] = dP of query tile * 64 + 16 qb + 4 g + i for key k
    const int lim = N - tile * WT - 4 * g;  // valid: 16 qb + i < lim
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const float4_t l4 = *(const float4_t*)&Ls[qb * 16 + 4 * g];
      const float4_t d4 = *(const float4_t*)&Ds[qb * 16 + 4 * g];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = (16 * qb + i < lim) ? __builtin_amdgcn_exp2f(st[qb][i] - l4[i]) : 0.f;
        st[qb][i] = p;
        dp[qb][i] = p * (dp[qb][i] - d4[i]);
      }
    }
    const bf16x8_t pf[2] = {pack_acc(st[0], st[1]), pack_acc(st[2], st[3])};
    const bf16x8_t dsf[2] = {pack_acc(dp[0], dp[1]), pack_acc(dp[2], dp[3])};
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        dv[db] = mfma16(col_frag(Os, db, ks, c, g), pf[ks], dv[db]);
        dk[db] = mfma16(col_frag(Qs, db, ks, c, g), dsf[ks], dk[db]);
      }
    __syncthreads();
    if (tile + 1 < ntiles) {
      store_tile();
      __syncthreads();
    }
  }
  if (k < N) {  // d*[db][i] = d*[k][16 db + 4 g + i]
    uint16_t* op = dqkv + ((size_t)b * N + k) * ld + HDt + h * WHD + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      store4_bf16(op + 16 * db, dk[db], kLn2_16);
      store4_bf16(op + HDt + 16 * db, dv[db], 1.0f);
    }
  }
}

// ------------------------------------------------------------------ activations, 16-bit I/O
// 8 elements per thread (two float4 in, one 16-B vector out); the last n % 8 by one thread.
__device__ __forceinline__ float2_t act16_pair(int mode, float2_t v) {
  if (mode == AACLIP_EPI_GELU) return gelu_fast2(v);
  if (mode == AACLIP_EPI_QGELU) return qgelu_fast2(v);
  return float2_t{leaky_relu(v[0]), leaky_relu(v[1])};
}

template <bool H16>
__global__ __launch_bounds__(256) void act_to16_kernel(int mode, const float* __restrict__ x,
                                                       uint16_t* __restrict__ y, size_t n) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= n) return;
  if (i + 8 <= n) {
    const float4_t a = *(const float4_t*)(x + i), b = *(const float4_t*)(x + i + 4);
    const float2_t r0 = act16_pair(mode, float2_t{a[0], a[1]}), r1 = act16_pair(mode, float2_t{a[2], a[3]});
    const float2_t r2 = act16_pair(mode, float2_t{b[0], b[1]}), r3 = act16_pair(mode, float2_t{b[2], b[3]});
    *(uint4*)(y + i) = uint4{pack_h16x2<H16>(r0[0], r0[1]), pack_h16x2<H16>(r1[0], r1[1]),
                             pack_h16x2<H16>(r2[0], r2[1]), pack_h16x2<H16>(r3[0], r3[1])};
  } else {
    for (size_t j = i; j < n; ++j) {
      const float2_t r = act16_pair(mode, float2_t{x[j], x[j]});
      y[j] = (uint16_t)(pack_h16x2<H16>(r[0], r[0]) & 0xffffu);
    }
  }
}

// aaclip_act_bwd's derivative (text_bwd.hip act_bwd_kernel) of the reference value v: the exact erf /
// sigmoid forms. The forward's gelu_fast2 is within 2.6e-5 absolute of the erf form, an order below
// the bf16 rounding of dx.
__device__ __forceinline__ float act_slope(int mode, float v) {
  if (mode == AACLIP_EPI_GELU) {
    const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
    return cdf + v * (0.39894228040143267794f * expf(-0.5f * v * v));
  }
  if (mode == AACLIP_EPI_QGELU) {
    const float s = 1.0f / (1.0f + expf(-1.702f * v));
    return s + 1.702f * v * s * (1.0f - s);
  }
  return v > 0.f ? 1.0f : 0.01f;
}

template <bool H16>
__global__ __launch_bounds__(256) void act_bwd16_kernel(int mode, const uint16_t* dy, const float* __restrict__ ref,
                                                        uint16_t* dx, size_t n) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= n) return;
  if (i + 8 <= n) {
    const uint4 d = *(const uint4*)(dy + i);
    const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
    const float4_t a = *(const float4_t*)(ref + i), b = *(const float4_t*)(ref + i + 4);
    const float rv[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    uint32_t o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float lo = h16_to_f32<H16>((uint16_t)(dw[p] & 0xffffu)) * act_slope(mode, rv[2 * p]);
      const float hi = h16_to_f32<H16>((uint16_t)(dw[p] >> 16)) * act_slope(mode, rv[2 * p + 1]);
      o[p] = pack_h16x2<H16>(lo, hi);
    }
    *(uint4*)(dx + i) = uint4{o[0], o[1], o[2], o[3]};
  } else {
    for (size_t j = i; j < n; ++j) {
      const float v = h16_to_f32<H16>(dy[j]) * act_slope(mode, ref[j]);
      dx[j] = (uint16_t)(pack_h16x2<H16>(v, v) & 0xffffu);
    }
  }
}

// ------------------------------------------------------------------ row cast
// y[r][c] = (out type) x[r][c], 8 columns per thread: fp32 -> 16-bit rounds to nearest even (the
// GEMM epilogue's conversion), 16-bit -> fp32 is exact.
template <bool H16>
__global__ __launch_bounds__(256) void cast_rows_down_kernel(const float* __restrict__ x, int64_t ldx,
                                                             uint16_t* __restrict__ y, int64_t ldy, int rows,
                                                             int cols8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * cols8) return;
  const size_t r = i / cols8, c = (i % cols8) * 8;
  const float4_t a = *(const float4_t*)(x + r * ldx + c), b = *(const float4_t*)(x + r * ldx + c + 4);
  *(uint4*)(y + r * ldy + c) = uint4{pack_h16x2<H16>(a[0], a[1]), pack_h16x2<H16>(a[2], a[3]),
                                     pack_h16x2<H16>(b[0], b[1]), pack_h16x2<H16>(b[2], b[3])};
}
template <bool H16>
__global__ __launch_bounds__(256) void cast_rows_up_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                           float* __restrict__ y, int64_t ldy, int rows,
                                                           int cols8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * cols8) return;
  const size_t r = i / cols8, c = (i % cols8) * 8;
  const uint4 d = *(const uint4*)(x + r * ldx + c);
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  float4_t o[2];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    o[p >> 1][2 * (p & 1)] = h16_to_f32<H16>((uint16_t)(w[p] & 0xffffu));
    o[p >> 1][2 * (p & 1) + 1] = h16_to_f32<H16>((uint16_t)(w[p] >> 16));
  }
  *(float4_t*)(y + r * ldy + c) = o[0];
  *(float4_t*)(y + r * ldy + c + 4) = o[1];
}

inline bool is16(int dtype) { return dtype == AACLIP_BF16 || dtype == AACLIP_F16; }
inline bool act_mode_ok(int mode) {
  return mode == AACLIP_EPI_GELU || mode == AACLIP_EPI_QGELU || mode == AACLIP_EPI_LEAKY;
}

}  // namespace

extern "C" int aaclip_attention_bwd16_workspace(int batch, int seq, int heads, size_t* bytes) {
  AACLIP_REQUIRE(bytes && batch > 0 && seq >= 1 && heads > 0);
  *bytes = 2 * (size_t)batch * heads * seq * sizeof(float);
  return AACLIP_OK;
}

extern "C" int aaclip_attention_bwd16(int dtype, const void* qkv, const void* out, const void* dout, void* dqkv,
                                      int batch, int seq, int heads, int head_dim, int flags, float* workspace,
                                      size_t workspace_bytes, void* stream) {
  AACLIP_REQUIRE(dtype == AACLIP_BF16);
  AACLIP_REQUIRE(qkv && out && dout && dqkv && workspace);
  AACLIP_REQUIRE(head_dim == WHD && seq >= 1 && batch > 0 && heads > 0);
  AACLIP_REQUIRE((flags & ~AACLIP_ATTN_Q_PRESCALED) == 0);
  AACLIP_REQUIRE((int64_t)batch * heads <= 65535 && (int64_t)batch * seq < (1ll << 31));
  AACLIP_REQUIRE(dqkv != qkv && dqkv != out && dqkv != dout);
  AACLIP_REQUIRE((const void*)workspace != qkv && (const void*)workspace != out &&
                 (const void*)workspace != dout && (void*)workspace != dqkv);
  AACLIP_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && aligned16(workspace));
  const size_t n = (size_t)batch * heads * seq;
  AACLIP_REQUIRE(workspace_bytes >= 2 * n * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ceil_div(seq, WT), batch * heads);
  float* lse = workspace;
  float* dsum = workspace + n;
  const int pre = (flags & AACLIP_ATTN_Q_PRESCALED) ? 1 : 0;
  attn_bwd16_q_kernel<<<grid, 256, 0, s>>>((const uint16_t*)qkv, (const uint16_t*)out, (const uint16_t*)dout,
                                           (uint16_t*)dqkv, lse, dsum, seq, heads, pre);
  AACLIP_CHECK_LAUNCH();
  attn_bwd16_kv_kernel<<<grid, 256, 0, s>>>((const uint16_t*)qkv, (const uint16_t*)dout, (uint16_t*)dqkv, lse, dsum,
                                            seq, heads, pre);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_act_to16(int mode, const float* x, void* y, int out_dtype, int64_t n, void* stream) {
  AACLIP_REQUIRE(x && y && n >= 0 && act_mode_ok(mode) && is16(out_dtype));
  AACLIP_REQUIRE((const void*)x != y && aligned16(x) && aligned16(y));
  if (n == 0) return AACLIP_OK;
  const unsigned blocks = (unsigned)((n + 2047) / 2048);
  if (out_dtype == AACLIP_F16)
    act_to16_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, x, (uint16_t*)y, (size_t)n);
  else
    act_to16_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, x, (uint16_t*)y, (size_t)n);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_act_bwd16(int mode, const void* dy, const float* ref, void* dx, int dtype, int64_t n,
                                void* stream) {
  AACLIP_REQUIRE(dy && ref && dx && n >= 0 && act_mode_ok(mode) && is16(dtype));
  AACLIP_REQUIRE((const void*)ref != dx && aligned16(dy) && aligned16(ref) && aligned16(dx));
  if (n == 0) return AACLIP_OK;
  const unsigned blocks = (unsigned)((n + 2047) / 2048);
  if (dtype == AACLIP_F16)
    act_bwd16_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, (const uint16_t*)dy, ref, (uint16_t*)dx,
                                                                    (size_t)n);
  else
    act_bwd16_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(mode, (const uint16_t*)dy, ref, (uint16_t*)dx,
                                                                     (size_t)n);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_cast_rows(int in_dtype, int out_dtype, const void* x, int64_t ldx, void* y, int64_t ldy,
                                int rows, int cols, void* stream) {
  AACLIP_REQUIRE(x && y && rows >= 0 && cols > 0 && cols % 8 == 0 && x != y);
  AACLIP_REQUIRE((in_dtype == AACLIP_F32 && is16(out_dtype)) || (is16(in_dtype) && out_dtype == AACLIP_F32));
  const bool down = in_dtype == AACLIP_F32;
  // 16-B vectors on both sides: fp32 rows a multiple of 4 elements apart, 16-bit rows of 8
  AACLIP_REQUIRE(ldx >= cols && ldy >= cols && ldx % (down ? 4 : 8) == 0 && ldy % (down ? 8 : 4) == 0);
  AACLIP_REQUIRE(aligned16(x) && aligned16(y));
  if (rows == 0) return AACLIP_OK;
  const int cols8 = cols / 8;
  const size_t total = (size_t)rows * cols8;
  AACLIP_REQUIRE(total < ((size_t)1 << 39));
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  const bool h16 = (down ? out_dtype : in_dtype) == AACLIP_F16;
  if (down) {
    if (h16) cast_rows_down_kernel<true><<<blocks, 256, 0, s>>>((const float*)x, ldx, (uint16_t*)y, ldy, rows, cols8);
    else cast_rows_down_kernel<false><<<blocks, 256, 0, s>>>((const float*)x, ldx, (uint16_t*)y, ldy, rows, cols8);
  } else {
    if (h16) cast_rows_up_kernel<true><<<blocks, 256, 0, s>>>((const uint16_t*)x, ldx, (float*)y, ldy, rows, cols8);
    else cast_rows_up_kernel<false><<<blocks, 256, 0, s>>>((const uint16_t*)x, ldx, (float*)y, ldy, rows, cols8);
  }
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
