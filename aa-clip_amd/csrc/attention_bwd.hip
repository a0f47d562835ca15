// Tiled attention backward of the visual tower (stage 2: 577 / 1025 / 1370 tokens): non-causal,
// head_dim 64, any sequence length. One pair of kernel bodies, instantiated for fp32 operands on
// v_mfma_f32_16x16x4f32 (aaclip_attention_bwd_tiled) and for bf16 operands on
// v_mfma_f32_16x16x32_bf16 (aaclip_attention_bwd16). Deterministic (no atomics, fixed reduction
// orders: two launches give the same bits) and image local.
//
// With S' = q' k^T (q' = q log2(e) / 8), P = exp2(S' - lse), dP = dout v^T, D_i = dout_i . out_i
// and dS = P (dP - D):
//   dq = dS k / 8,   dk = ln2 dS^T q',   dv = P^T dout.
// q' is formed at load; where the caller has folded the scale into q already
// (AACLIP_ATTN_Q_PRESCALED, bf16 only) q is taken as it is and the q columns of dqkv are the
// gradient of that q': dq' = ln2 dS k. Softmax statistics and accumulation are fp32.
//
// Two launches, 4 waves x 16 rows each, tiles of 64 rows staged through registers into LDS, the
// next tile's global loads in flight while the current one is computed. MFMA maps
// (c = lane & 15, g = lane >> 4): A[row c][k], B[k][col c], accumulator element
// i = D[row 4 g + i][col c]. Every product is oriented so that the next one sums over its
// accumulator ROW index: P and dS go back in as B operands straight from the registers, and no
// accumulator crosses LDS.
//
// Query-block kernel, one workgroup per (image, head, 64 queries), the query on the lane:
// S'^T = K . Q'^T and dP^T = V . dout^T have the key on the accumulator row, so the scores of
// query c are on the 4 lanes {c, c+16, c+32, c+48}, 16 keys of a tile each. Pass 1 over the key
// tiles keeps a running (max, sum) per lane and merges the 4 lanes at the end: lse (log2
// domain). D is the diagonal of an out . dout^T MFMA, i.e. with the operand roles and the
// summation order of dP, so that at seq == 1 (out == v) dP - D is exactly 0. Both go to the
// workspace. Pass 2 forms dS^T in registers, the B operand of dQ^T += K^T . dS^T. Keys past the
// end get P = 0 exactly.
//
// Key-block kernel, one workgroup per (image, head, 64 keys), the key on the lane, walks the
// query tiles in index order with the stored lse and D: S' = Q' . K^T and dP = dout . V^T have
// the query on the accumulator row; P and dS are the B operands of dV^T += dout^T . P and
// dK^T += Q'^T . dS. Queries past the end get P = dS = 0 exactly.
//
// Every output row is summed by one wave in a fixed order; rows past the end are loaded from
// the last valid row (finite values) and never stored.
//
// What the two operand policies differ in (OpsF32 / OpsBF16 below; nothing else does):
//   * k-steps per 64 summed values: 16 of 4 (one float per lane) / 2 of 32 (8 bf16 per lane).
//   * the LDS tile: [64][68] floats (row-padded: both fragment read patterns hit 64 different
//     banks) / attention.hip's XOR-swizzled [64][128 B] image.
//   * the A operand of a product that sums over the tile's rows (col_frag): scalar column reads /
//     the transposing LDS read ds_read_b64_tr_b16.
//   * its B operand (b_op): step (kb, i) is the bare accumulator element [kb][i] / two stacked
//     16 x 16 accumulators (tile rows 32 s + 4 g + i and 32 s + 16 + 4 g + i) are the 8 values of
//     k-step s, rounded to bf16 (dS is formed from the fp32 P), and col_frag reads the other
//     operand with the same permutation of the summed index.
//   * the Q scale: an fp32 product / applied to the bf16 q and rounded to bf16 again, in both
//     kernels alike (the same product, the same rounding), and skipped when prescaled.
//   * the output store: fp32 / rounded to bf16 (RNE).
#include "attn_lds.h"

namespace {

constexpr int AT = 64, AHD = 64;  // rows per tile, head dim

struct OpsF32 {
  using elem = float;   // storage element
  using frag = float;   // a lane's MFMA operand of one k-step
  using vec = float4_t;  // 16-B staging vector
  using tile = float[AT][68];
  // k-steps per 64 summed values; over a tile's rows they come as SB blocks of SI steps:
  // step (kb, i) is tile row 16 kb + 4 g + i, accumulator element [kb][i]
  static constexpr int SB = 4, SI = 4, KS = SB * SI;
  static constexpr bool kMayPrescale = false;
  static __device__ __forceinline__ float4_t mma(float a, float b, const float4_t& c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // row[4 ks + g], the lane's share of k-step ks of a global row: one address per row, ks in the offset field
  static __device__ __forceinline__ float load_frag(const float* row, int ks, int g) { return (row + g)[4 * ks]; }
  template <class V>
  static __device__ __forceinline__ V scale(const V& v, float s) {
    return v * s;
  }
  static __device__ __forceinline__ float4_t* chunk(tile& tl, int r, int ch) { return (float4_t*)&tl[r][4 * ch]; }
  static __device__ __forceinline__ float row_frag(const tile& tl, int rb, int ks, int c, int g) {
    return tl[rb * 16 + c][4 * ks + g];
  }
  static __device__ __forceinline__ float col_frag(const tile& tl, int db, int kb, int i, int c, int g) {
    return tl[kb * 16 + 4 * g + i][db * 16 + c];
  }
  static __device__ __forceinline__ float b_op(const float4_t (&acc)[4], int kb, int i) { return acc[kb][i]; }
  static __device__ __forceinline__ void store4(float* p, const float4_t& v, float s) { *(float4_t*)p = v * s; }
};

struct OpsBF16 {
  using elem = uint16_t;
  using frag = bf16x8_t;
  using vec = bf16x8_t;
  using tile = char[AT * 128];
  // step (s, 0) is tile rows 32 s + 4 g + {0..3} and 32 s + 16 + 4 g + {0..3}: accumulators 2 s and 2 s + 1
  static constexpr int SB = 2, SI = 1, KS = SB * SI;
  static constexpr bool kMayPrescale = true;
  static __device__ __forceinline__ float4_t mma(const bf16x8_t& a, const bf16x8_t& b, const float4_t& c) {
    return mfma16(a, b, c);
  }
  static __device__ __forceinline__ bf16x8_t load_frag(const uint16_t* row, int ks, int g) {
    return *(const bf16x8_t*)(row + 32 * ks + 8 * g);
  }
  static __device__ __forceinline__ bf16x8_t scale(const bf16x8_t& v, float s) {
    bf16x8_t r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (__bf16)((float)v[e] * s);
    return r;
  }
  static __device__ __forceinline__ bf16x8_t* chunk(tile& tl, int r, int ch) { return (bf16x8_t*)(tl + swz(r, ch)); }
  // tile row 16 rb + c, columns 32 ks + 8 g .. + 7
  static __device__ __forceinline__ bf16x8_t row_frag(const tile& tl, int rb, int ks, int c, int g) {
    return *(const bf16x8_t*)(tl + swz(rb * 16 + c, ks * 4 + g));
  }
  // column 16 db + c of step s's tile rows, in b_op's order
  static __device__ __forceinline__ bf16x8_t col_frag(const tile& tl, int db, int s, int, int c, int g) {
    const int qq = c >> 2, pp = c & 3;
    const int chunk = db * 2 + (pp >> 1);
    const int r0 = s * 32 + 4 * g + qq;
    const short4_t lo = tr_read(tl + swz(r0, chunk) + (pp & 1) * 8);
    const short4_t hi = tr_read(tl + swz(r0 + 16, chunk) + (pp & 1) * 8);
    return __builtin_bit_cast(bf16x8_t, short8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
  }
  static __device__ __forceinline__ bf16x8_t b_op(const float4_t (&acc)[4], int s, int) {
    bf16x8_t v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = (__bf16)acc[2 * s][i];
      v[4 + i] = (__bf16)acc[2 * s + 1][i];
    }
    return v;
  }
  static __device__ __forceinline__ void store4(uint16_t* p, const float4_t& v, float s) {
    *(uint2*)p = uint2{pack_bf16x2(v[0] * s, v[1] * s), pack_bf16x2(v[2] * s, v[3] * s)};
  }
};

// A [64][64] tile whose rows lie `ld` elements apart goes through registers to LDS in 16-B chunks
// of EPC elements, CPR to a row: thread t moves chunks t + 256 j (j < NV).
template <class P>
struct Stage {
  static constexpr int EPC = 16 / sizeof(typename P::elem);
  static constexpr int CPR = AHD / EPC;
  static constexpr int NV = AT * CPR / 256;
  using regs = typename P::vec[NV];
};
template <class P>
__device__ __forceinline__ void tile_load(const typename P::elem* src, int64_t ld, int row0, int N, int t,
                                          typename Stage<P>::regs& reg) {
  using S = Stage<P>;
#pragma unroll
  for (int j = 0; j < S::NV; ++j) {
    const int f = t + 256 * j, r = f / S::CPR, ch = f % S::CPR;
    reg[j] = *(const typename P::vec*)(src + (size_t)min(row0 + r, N - 1) * ld + S::EPC * ch);
  }
}
template <class P>
__device__ __forceinline__ void tile_store(typename P::tile& dst, int t, const typename Stage<P>::regs& reg) {
  using S = Stage<P>;
#pragma unroll
  for (int j = 0; j < S::NV; ++j) {
    const int f = t + 256 * j, r = f / S::CPR, ch = f % S::CPR;
    *P::chunk(dst, r, ch) = reg[j];
  }
}

constexpr float4_t kZero4 = {0.f, 0.f, 0.f, 0.f};

// One 16-row block of the first products (S and dP): s = rows 16 rb .. + 15 of tile ta times the
// lane's own row fa, d the same of tb times fb, interleaved. Element i is tile row 16 rb + 4 g + i.
template <class P>
__device__ __forceinline__ void first_products(const typename P::tile& ta, const typename P::frag (&fa)[P::KS],
                                               const typename P::tile& tb, const typename P::frag (&fb)[P::KS],
                                               int rb, float4_t& s, float4_t& d, int c, int g) {
  s = kZero4;
  d = kZero4;
#pragma unroll
  for (int ks = 0; ks < P::KS; ++ks) {
    s = P::mma(P::row_frag(ta, rb, ks, c, g), fa[ks], s);
    d = P::mma(P::row_frag(tb, rb, ks, c, g), fb[ks], d);
  }
}

template <class P>
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const typename P::elem* __restrict__ qkv,
                                                         const typename P::elem* __restrict__ out,
                                                         const typename P::elem* __restrict__ dout,
                                                         typename P::elem* __restrict__ dqkv,
                                                         float* __restrict__ lse_ws, float* __restrict__ d_ws, int N,
                                                         int H, int prescaled) {
  using E = typename P::elem;
  using F = typename P::frag;
  __shared__ __attribute__((aligned(16))) typename P::tile Ks;
  __shared__ __attribute__((aligned(16))) typename P::tile Vs;
  const bool pre = P::kMayPrescale && prescaled;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int HDt = H * AHD;
  const int64_t ld = 3 * (int64_t)HDt;
  const E* base = qkv + (size_t)b * N * ld + h * AHD;
  const int q = blockIdx.x * AT + wid * 16 + c;  // this lane's query
  const int qc = min(q, N - 1);
  const size_t orow = ((size_t)b * N + qc) * HDt + h * AHD;

  F qf[P::KS], dof[P::KS];  // the lane's k-step shares of Q'[q] and dout[q]
  float4_t dd = kZero4;
#pragma unroll
  for (int ks = 0; ks < P::KS; ++ks) {
    qf[ks] = P::load_frag(base + (size_t)qc * ld, ks, g);
    if (!pre) qf[ks] = P::scale(qf[ks], kAttnLog2Scale);
    dof[ks] = P::load_frag(dout + orow, ks, g);
    // dd[i] = out[q0 + 4 g + i] . dout[q0 + c]: out rows as dP's V rows, dout as its B operand
    dd = P::mma(P::load_frag(out + orow, ks, g), dof[ks], dd);
  }
  // the diagonal: query c's own product sits in lane (c, g = c / 4), element c % 4
  const float sel = (c & 3) == 0 ? dd[0] : (c & 3) == 1 ? dd[1] : (c & 3) == 2 ? dd[2] : dd[3];
  const float Dq = __shfl(sel, c + 16 * (c >> 2), 64);

  const int ntiles = (N + AT - 1) / AT;
  typename Stage<P>::regs kreg, vreg;

  // ---- pass 1: row log-sum-exp (log2 domain)
  float m = -INFINITY, l = 0.f;
  tile_load<P>(base + HDt, ld, 0, N, t, kreg);
  tile_store<P>(Ks, t, kreg);
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) tile_load<P>(base + HDt, ld, (tile + 1) * AT, N, t, kreg);
    float4_t st[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      st[kb] = kZero4;
#pragma unroll
      for (int ks = 0; ks < P::KS; ++ks) st[kb] = P::mma(P::row_frag(Ks, kb, ks, c, g), qf[ks], st[kb]);
    }
    // st[kb][i] = score of key tile * 64 + 16 kb + 4 g + i for query q
    const int lim = N - tile * AT - 4 * g;  // valid: 16 kb + i < lim
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
      tile_store<P>(Ks, t, kreg);
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
  for (int db = 0; db < 4; ++db) dq[db] = kZero4;
  __syncthreads();
  tile_load<P>(base + HDt, ld, 0, N, t, kreg);
  tile_load<P>(base + 2 * HDt, ld, 0, N, t, vreg);
  tile_store<P>(Ks, t, kreg);
  tile_store<P>(Vs, t, vreg);
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) {
      tile_load<P>(base + HDt, ld, (tile + 1) * AT, N, t, kreg);
      tile_load<P>(base + 2 * HDt, ld, (tile + 1) * AT, N, t, vreg);
    }
    float4_t st[4], dp[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) first_products<P>(Ks, qf, Vs, dof, rb, st[rb], dp[rb], c, g);
    const int lim = N - tile * AT - 4 * g;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = (16 * kb + i < lim) ? __builtin_amdgcn_exp2f(st[kb][i] - lse) : 0.f;
        st[kb][i] = p * (dp[kb][i] - Dq);  // dS[q][key]
      }
    F dsf[P::SB][P::SI];
#pragma unroll
    for (int kb = 0; kb < P::SB; ++kb)
#pragma unroll
      for (int i = 0; i < P::SI; ++i) dsf[kb][i] = P::b_op(st, kb, i);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int kb = 0; kb < P::SB; ++kb)
#pragma unroll
        for (int i = 0; i < P::SI; ++i) dq[db] = P::mma(P::col_frag(Ks, db, kb, i, c, g), dsf[kb][i], dq[db]);
    __syncthreads();
    if (tile + 1 < ntiles) {
      tile_store<P>(Ks, t, kreg);
      tile_store<P>(Vs, t, vreg);
      __syncthreads();
    }
  }
  if (q < N) {  // dq[db][i] = dQ[q][16 db + 4 g + i]
    E* op = dqkv + ((size_t)b * N + q) * ld + h * AHD + 4 * g;
    const float s = pre ? kLn2 : 0.125f;
#pragma unroll
    for (int db = 0; db < 4; ++db) P::store4(op + 16 * db, dq[db], s);
  }
}

template <class P>
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const typename P::elem* __restrict__ qkv,
                                                          const typename P::elem* __restrict__ dout,
                                                          typename P::elem* __restrict__ dqkv,
                                                          const float* __restrict__ lse_ws,
                                                          const float* __restrict__ d_ws, int N, int H,
                                                          int prescaled) {
  using E = typename P::elem;
  using F = typename P::frag;
  __shared__ __attribute__((aligned(16))) typename P::tile Qs;
  __shared__ __attribute__((aligned(16))) typename P::tile Os;
  __shared__ __attribute__((aligned(16))) float Ls[AT];
  __shared__ __attribute__((aligned(16))) float Ds[AT];
  const bool pre = P::kMayPrescale && prescaled;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int HDt = H * AHD;
  const int64_t ld = 3 * (int64_t)HDt;
  const E* base = qkv + (size_t)b * N * ld + h * AHD;
  const E* dob = dout + (size_t)b * N * HDt + h * AHD;
  const int k = blockIdx.x * AT + wid * 16 + c;  // this lane's key
  const int kc = min(k, N - 1);

  F kf[P::KS], vf[P::KS];  // the lane's k-step shares of K[k] and V[k]
#pragma unroll
  for (int ks = 0; ks < P::KS; ++ks) {
    kf[ks] = P::load_frag(base + (size_t)kc * ld + HDt, ks, g);
    vf[ks] = P::load_frag(base + (size_t)kc * ld + 2 * HDt, ks, g);
  }
  float4_t dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    dk[db] = kZero4;
    dv[db] = kZero4;
  }

  const int ntiles = (N + AT - 1) / AT;
  typename Stage<P>::regs qreg, oreg;
  float lreg = 0.f, dreg = 0.f;
  auto load_tile = [&](int tile) {
    tile_load<P>(base, ld, tile * AT, N, t, qreg);
    tile_load<P>(dob, HDt, tile * AT, N, t, oreg);
    if (t < AT) {
      const size_t i = (size_t)bh * N + min(tile * AT + t, N - 1);
      lreg = lse_ws[i];
      dreg = d_ws[i];
    }
  };
  auto store_tile = [&]() {
    if (!pre) {  // the query-block kernel's Q': the same product, the same rounding
#pragma unroll
      for (auto& v : qreg) v = P::scale(v, kAttnLog2Scale);
    }
    tile_store<P>(Qs, t, qreg);
    tile_store<P>(Os, t, oreg);
    if (t < AT) {
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
    for (int rb = 0; rb < 4; ++rb) first_products<P>(Qs, kf, Os, vf, rb, st[rb], dp[rb], c, g);
    // st[qb][i] = score, dp[qb][i] = dP of query tile * 64 + 16 qb + 4 g + i for key k
    const int lim = N - tile * AT - 4 * g;  // valid: 16 qb + i < lim
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
    F pf[P::SB][P::SI], dsf[P::SB][P::SI];
#pragma unroll
    for (int qb = 0; qb < P::SB; ++qb)
#pragma unroll
      for (int i = 0; i < P::SI; ++i) {
        pf[qb][i] = P::b_op(st, qb, i);
        dsf[qb][i] = P::b_op(dp, qb, i);
      }
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int qb = 0; qb < P::SB; ++qb)
#pragma unroll
        for (int i = 0; i < P::SI; ++i) {
          dv[db] = P::mma(P::col_frag(Os, db, qb, i, c, g), pf[qb][i], dv[db]);
          dk[db] = P::mma(P::col_frag(Qs, db, qb, i, c, g), dsf[qb][i], dk[db]);
        }
    __syncthreads();
    if (tile + 1 < ntiles) {
      store_tile();
      __syncthreads();
    }
  }
  if (k < N) {  // d*[db][i] = d*[k][16 db + 4 g + i]
    E* op = dqkv + ((size_t)b * N + k) * ld + HDt + h * AHD + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      P::store4(op + 16 * db, dk[db], kLn2);
      P::store4(op + HDt + 16 * db, dv[db], 1.0f);
    }
  }
}

int attention_bwd_workspace(int batch, int seq, int heads, size_t* bytes) {
  AACLIP_REQUIRE(bytes && batch > 0 && seq >= 1 && heads > 0);
  *bytes = 2 * (size_t)batch * heads * seq * sizeof(float);  // lse and D per (image, head, query)
  return AACLIP_OK;
}

template <class P>
int attention_bwd(const void* qkv, const void* out, const void* dout, void* dqkv, int batch, int seq, int heads,
                  int head_dim, int flags, float* workspace, size_t workspace_bytes, void* stream) {
  using E = typename P::elem;
  AACLIP_REQUIRE(qkv && out && dout && dqkv && workspace);
  AACLIP_REQUIRE(head_dim == AHD && seq >= 1 && batch > 0 && heads > 0);
  AACLIP_REQUIRE((flags & ~(P::kMayPrescale ? AACLIP_ATTN_Q_PRESCALED : 0)) == 0);
  AACLIP_REQUIRE((int64_t)batch * heads <= 65535 && (int64_t)batch * seq < (1ll << 31));
  AACLIP_REQUIRE(dqkv != qkv && dqkv != out && dqkv != dout);
  AACLIP_REQUIRE((const void*)workspace != qkv && (const void*)workspace != out &&
                 (const void*)workspace != dout && (void*)workspace != dqkv);
  AACLIP_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && aligned16(workspace));
  const size_t n = (size_t)batch * heads * seq;
  AACLIP_REQUIRE(workspace_bytes >= 2 * n * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ceil_div(seq, AT), batch * heads);
  float* lse = workspace;
  float* dsum = workspace + n;
  const int pre = (flags & AACLIP_ATTN_Q_PRESCALED) ? 1 : 0;
  attn_bwd_q_kernel<P><<<grid, 256, 0, s>>>((const E*)qkv, (const E*)out, (const E*)dout, (E*)dqkv, lse, dsum, seq,
                                            heads, pre);
  AACLIP_CHECK_LAUNCH();
  attn_bwd_kv_kernel<P><<<grid, 256, 0, s>>>((const E*)qkv, (const E*)dout, (E*)dqkv, lse, dsum, seq, heads, pre);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

}  // namespace

extern "C" int aaclip_attention_bwd_tiled_workspace(int batch, int seq, int heads, size_t* bytes) {
  return attention_bwd_workspace(batch, seq, heads, bytes);
}

extern "C" int aaclip_attention_bwd_tiled(const float* qkv, const float* out, const float* dout, float* dqkv,
                                          int batch, int seq, int heads, int head_dim, float* workspace,
                                          size_t workspace_bytes, void* stream) {
  return attention_bwd<OpsF32>(qkv, out, dout, dqkv, batch, seq, heads, head_dim, 0, workspace, workspace_bytes,
                               stream);
}

extern "C" int aaclip_attention_bwd16_workspace(int batch, int seq, int heads, size_t* bytes) {
  return attention_bwd_workspace(batch, seq, heads, bytes);
}

extern "C" int aaclip_attention_bwd16(int dtype, const void* qkv, const void* out, const void* dout, void* dqkv,
                                      int batch, int seq, int heads, int head_dim, int flags, float* workspace,
                                      size_t workspace_bytes, void* stream) {
  AACLIP_REQUIRE(dtype == AACLIP_BF16);
  return attention_bwd<OpsBF16>(qkv, out, dout, dqkv, batch, seq, heads, head_dim, flags, workspace, workspace_bytes,
                                stream);
}
