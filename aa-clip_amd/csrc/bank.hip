// Few-shot memory-bank scoring (reference test.py:39-50 get_support_features, utils.py:86-93
// cos_sim, which the reference carries but wires to nothing): every test patch is scored by its
// cosine distance to the nearest patch of a bank of normal support patches, per feature level.
//
//   search    aaclip_bank_nn: part[m][s] = max over the bank rows n of split s of Q[m,:] . R[n,:].
//             An MFMA GEMM (both operands K-contiguous, the "NT" form of gemm.hip) whose epilogue
//             keeps a running row maximum, so the [M, Nb] similarity matrix (43 808^2 per level at
//             the reference's defaults) is never written. 16-bit operands: 256 x 256 x 64 block
//             tiles (128 FLOP per byte staged: at 128 x 128 the search measured 0.53-0.71 PFLOP/s,
//             bound by the L2 -> LDS traffic), 8 waves of 128 x 64, global -> LDS by LDS-DMA (global_load_lds_dwordx4) into
//             lane-linear 128-byte rows with the XOR swizzle applied on the per-lane SOURCE
//             address and undone on the ds_read, two stages, one barrier per K-step -- the staging
//             idiom of gemm.hip's gemm_bf16_kernel. A block owns one row tile and one split of the
//             bank and walks the split's bank tiles in one flat (tile, K-step) pipeline: the first
//             K-step of the next bank tile is in flight under the last MFMAs of this one.
//             The MFMA takes the bank fragment first, so the tile comes out transposed: lane
//             (fr, fq) holds query row fr against bank columns 4 fq .. 4 fq + 3 of every 16-column
//             tile. The row maximum is then a per-lane fmaxf over the accumulators, folded into
//             8 running registers per lane after every bank tile, and crosses lanes (fq: lanes
//             fr, fr + 16, fr + 32, fr + 48) and the four wave columns (LDS) once, at the end.
//             Ragged edges clamp the SOURCE row: a clamped bank row is a duplicate of the last
//             row and cannot move a maximum, a clamped query row is not stored. Nothing is
//             zero-filled (a zero row would win wherever every true similarity is negative).
//             Every dot product accumulates K in the same order (K-steps ascending, the MFMA's
//             own order inside), wherever its row and column sit: the same bits for a query row
//             alone or in a batch, and under any permutation of the bank.
//             fp32 operands (the parity mode): v_mfma_f32_16x16x4_f32 on register-staged
//             256 x 256 x 16 tiles, the same tile walk, splits and reductions.
//             MX fp8 operands (aaclip_bank_nn_fp8mx, opt-in): the 16-bit kernel's staging and tile
//             walk at a K-step of 128 on the block-scaled fp8 MFMA, the result the exact cosine
//             between the stored rows (see bank_nn_mx_kernel).
//   combine   aaclip_bank_distance: grid[m] = (accumulate ? grid[m] : 0) + (1 - max_s part[m][s]).
//   fusion    aaclip_fewshot_fuse: class-normalised zero-shot + few-shot maps and scores, every
//             operation a rounded fp32 one (tests/fewshot_ref.py states it in numpy float32).
//   coreset   aaclip_bank_coreset: greedy k-centre subsampling of a bank ahead of the search, one
//             step kernel per pick (coreset_step_kernel; tests/coreset_ref.py states it in float64).
//
// Inputs are finite: the object is built with -fno-honor-nans (Makefile), which drops the
// canonicalising v_max hipcc otherwise puts in front of every fmaxf of an MFMA result.
#include <climits>
#include <cmath>

#include "common.h"
#include "scorenorm.h"

namespace {

constexpr int BM = AACLIP_BANK_TILE_M, BN = AACLIP_BANK_TILE_N;  // block tile: query rows x bank rows
constexpr int WM = 2, WN = 4, NWAVES = WM * WN;                  // 2 x 4 waves of 128 x 64
constexpr int TM = BM / WM, TN = BN / WN, RM = TM / 16, RN = TN / 16;
static_assert(BM == 256 && BN == 256, "the wave layout and the staging below are written for 256 x 256");

struct BankArgs {
  const void* Q;
  const void* R;
  float* part;
  int64_t ldq, ldr;  // elements
  int M, Nb, K;
  int n_splits, tiles_per_split, tiles_n;
};

// rmax[i] = max(rmax[i], the lane's 16 values of tile row i), then the tile starts over
__device__ __forceinline__ void fold_tile(float4_t (&acc)[RM][RN], float (&rmax)[RM]) {
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) rmax[i] = fmaxf(rmax[i], acc[i][j][e]);
      acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    }
}

// rows of the block tile: across the four lanes that share a row (fq), then across the WN
// wave columns through `red` (WN * BM floats of LDS nobody reads any more), then out; SCALED: times
// the row's positive factor row_scale[m] (it commutes with the maxima, rounding included)
template <bool SCALED = false>
__device__ __forceinline__ void store_rows(const BankArgs& a, const float (&rmax)[RM], float* red, int m0, int split,
                                           int wm, int wn, int lane, const float* row_scale = nullptr) {
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    float v = rmax[i];
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    if (fq == 0) red[wn * BM + wm * TM + i * 16 + fr] = v;
  }
  __syncthreads();
  const int r = threadIdx.x;
  if (r < BM && m0 + r < a.M) {
    float v = red[r];
#pragma unroll
    for (int w = 1; w < WN; ++w) v = fmaxf(v, red[w * BM + r]);
    if constexpr (SCALED) v *= row_scale[m0 + r];
    a.part[(size_t)(m0 + r) * a.n_splits + split] = v;
  }
}

// ============================================================== 16-bit operands
constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE_BYTES = A_BYTES + B_BYTES;
constexpr int A_LOADS = A_BYTES / (NWAVES * 1024), B_LOADS = B_BYTES / (NWAVES * 1024);  // glds per wave per stage
constexpr int kLds16 = 2 * STAGE_BYTES;
static_assert(A_LOADS * NWAVES * 1024 == A_BYTES && B_LOADS * NWAVES * 1024 == B_BYTES, "tile");
static_assert(WN * BM * (int)sizeof(float) <= STAGE_BYTES, "the row reduction reuses a stage");

// global -> LDS of one K-step of the query tile and a bank tile, 128 bytes per row (64 16-bit
// or 128 fp8 elements of ES bytes): per-lane DMA sources (row r = piece * 8 + lane / 8 of the
// tile, physical 16-B chunk p = lane % 8 holds logical chunk p ^ (r & 7)); rows past the end are
// the last row
template <int ES>
struct TileDma {
  const char* Rg;
  const char* q_src[A_LOADS];
  int b_row[B_LOADS], b_col[B_LOADS];
  __device__ __forceinline__ TileDma(const BankArgs& a, int m0, int wid, int lane) : Rg((const char*)a.R) {
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
      const int r = (i * NWAVES + wid) * 8 + (lane >> 3);
      q_src[i] = (const char*)a.Q + (size_t)min(m0 + r, a.M - 1) * a.ldq * ES + (((lane & 7) ^ (r & 7)) << 4);
    }
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
      b_row[i] = (i * NWAVES + wid) * 8 + (lane >> 3);
      b_col[i] = ((lane & 7) ^ (b_row[i] & 7)) << 4;
    }
  }
  // K-step kt of the query tile and of the bank tile at row n0 into the stage at base
  __device__ __forceinline__ void stage(const BankArgs& a, char* base, int n0, int kt, int wid) const {
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(q_src[i] + kt * 128), LDS_PTR(base + (i * NWAVES + wid) * 1024),
                                       16, 0, 0);
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
      const char* src = Rg + (size_t)min(n0 + b_row[i], a.Nb - 1) * a.ldr * ES + b_col[i] + kt * 128;
      __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(base + A_BYTES + (i * NWAVES + wid) * 1024), 16, 0,
                                       0);
    }
  }
};

template <bool H16>
__global__ __launch_bounds__(NWAVES * 64) void bank_nn16_kernel(BankArgs a) {
  using V8 = h16x8_t<H16>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int split = blockIdx.x % a.n_splits, m0 = (blockIdx.x / a.n_splits) * BM;
  const int t0 = split * a.tiles_per_split;
  const int nt = min(a.tiles_per_split, a.tiles_n - t0);  // >= 1: no split is empty (bank_plan)
  const int nk = a.K / 64;

  const TileDma<2> dma(a, m0, wid, lane);
  auto stage = [&](int t, int kt, int buf) { dma.stage(a, smem + buf * STAGE_BYTES, (t0 + t) * BN, kt, wid); };

  // fragment read offsets within a stage: 16-B chunk kk * 4 + fq of the row, swizzle undone
  const int fr = lane & 15, fq = lane >> 4;
  int a_off[RM][2], b_off[RN][2];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    const int r = wm * TM + i * 16 + fr;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) a_off[i][kk] = r * 128 + (((kk * 4 + fq) ^ (r & 7)) << 4);
  }
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int r = wn * TN + j * 16 + fr;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) b_off[j][kk] = A_BYTES + r * 128 + (((kk * 4 + fq) ^ (r & 7)) << 4);
  }

  float4_t acc[RM][RN];
  float rmax[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    rmax[i] = -INFINITY;
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
  }

  stage(0, 0, 0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk)
        stage(t, kt + 1, cur ^ 1);
      else if (t + 1 < nt)
        stage(t + 1, 0, cur ^ 1);
      const char* base = smem + cur * STAGE_BYTES;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        V8 bf[RN];
#pragma unroll
        for (int j = 0; j < RN; ++j) bf[j] = *(const V8*)(base + b_off[j][kk]);
#pragma unroll
        for (int i = 0; i < RM; ++i) {
          const V8 af = *(const V8*)(base + a_off[i][kk]);
#pragma unroll
          for (int j = 0; j < RN; ++j) acc[i][j] = mfma16(bf[j], af, acc[i][j]);  // C^T tile
        }
      }
      __syncthreads();
      cur ^= 1;
    }
    fold_tile(acc, rmax);
  }
  store_rows(a, rmax, (float*)smem, m0, split, wm, wn, lane);
}

// ============================================================== fp32 operands (parity mode)
__global__ __launch_bounds__(NWAVES * 64) void bank_nn32_kernel(BankArgs a) {
  constexpr int BK = 16, LDK = BK + 1;
  __shared__ float Qs[BM][LDK];
  __shared__ float Rs[BN][LDK];
  __shared__ float red[WN * BM];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int split = blockIdx.x % a.n_splits, m0 = (blockIdx.x / a.n_splits) * BM;
  const int t0 = split * a.tiles_per_split;
  const int nt = min(a.tiles_per_split, a.tiles_n - t0);
  const float* Qg = (const float*)a.Q;
  const float* Rg = (const float*)a.R;
  // a thread stages 4 consecutive K values of rows lr and lr + BM / 2 of either operand
  const int lr = threadIdx.x >> 2, lc = (threadIdx.x & 3) * 4;
  const float* q_src[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) q_src[h] = Qg + (size_t)min(m0 + lr + (BM / 2) * h, a.M - 1) * a.ldq + lc;
  const int fr = lane & 15, fk = lane >> 4;
  float4_t acc[RM][RN];
  float rmax[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    rmax[i] = -INFINITY;
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
  }
  for (int t = 0; t < nt; ++t) {
    const int n0 = (t0 + t) * BN;
    const float* r_src[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) r_src[h] = Rg + (size_t)min(n0 + lr + (BN / 2) * h, a.Nb - 1) * a.ldr + lc;
    for (int k0 = 0; k0 < a.K; k0 += BK) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4_t qv = *(const float4_t*)(q_src[h] + k0);
        const float4_t rv = *(const float4_t*)(r_src[h] + k0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          Qs[lr + (BM / 2) * h][lc + j] = qv[j];
          Rs[lr + (BN / 2) * h][lc + j] = rv[j];
        }
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < BK / 4; ++ks) {
        float qf[RM], rf[RN];
#pragma unroll
        for (int i = 0; i < RM; ++i) qf[i] = Qs[wm * TM + i * 16 + fr][ks * 4 + fk];
#pragma unroll
        for (int j = 0; j < RN; ++j) rf[j] = Rs[wn * TN + j * 16 + fr][ks * 4 + fk];
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j)  // bank fragment first: the C^T tile of the 16-bit kernel
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(rf[j], qf[i], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
    fold_tile(acc, rmax);
  }
  store_rows(a, rmax, red, m0, split, wm, wn, lane);
}

// ============================================================== MX fp8 operands (mxfp8.h)
// part[m][s] = max_n (Q^[m] . R^[n]) * r_rnorm[n] * q_rnorm[m]: the cosine between the fp8 MX
// representations, norms included. A 128-column K-step of e4m3 is the 128-byte row the 16-bit
// kernel stages, so the tile staging, the swizzle and the flat (tile, K-step) pipeline are its own;
// a lane's fragment is the row's chunks fq and 4 + fq (the two chunk offsets the 16-bit kernel
// reads one per half step), and v_mfma_scale_f32_16x16x128_f8f6f4 applies both operands' e8m0
// block scales: lane group fq supplies the scale of K 32 fq .. 32 fq + 31, which lies in the
// row's 64-block fq / 2. The scale pairs of a K-step's 256 + 256 rows (1 KiB) ride with the tile
// behind the two stages: one dword LDS-DMA per lane of waves 0-1 (query rows) and 2-3 (bank rows),
// contiguous in the [K / 128][ld][2] layout. At a ragged edge the dword's source is clamped into
// the buffer and the lane reads the scale of the row its clamped tile row duplicates, so a
// duplicate stays a duplicate. The bank row's reciprocal norm multiplies the accumulator ahead of
// the running maximum (it differs per column; waves 4-7 bring a tile's 256 of them into LDS with
// its first K-step), the query row's once at the end.
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

struct BankMxArgs {
  BankArgs b;  // Q, R: e4m3 bytes
  const uint8_t* q_sc;
  const uint8_t* r_sc;
  const float* q_rnorm;
  const float* r_rnorm;
  int64_t ld_qsc, ld_rsc;
};

constexpr int SC_BYTES = (BM + BN) * 2;  // per stage: the query rows' scale pairs, then the bank rows'
constexpr int RN_BYTES = BN * 4;         // per bank tile: its rows' reciprocal norms
// Three norm slots, tile t in slot t % 3. Tile t + 1's norms are issued no earlier than tile t's
// first K-step, and with a single K-step per tile (K = 128) tile t + 2's are issued during tile
// t + 1's, straight after the wave's own fold of tile t with no barrier in between: slot
// (t + 2) % 3 was last read by the fold of tile t - 1, which every wave has left behind at the
// barrier that closed tile t. Two slots would let a fast wave overwrite what a slow one still folds.
constexpr int RN_SLOTS = 3;
constexpr int kLdsMx = 2 * STAGE_BYTES + 2 * SC_BYTES + RN_SLOTS * RN_BYTES;
static_assert(BM * 2 == 2 * 64 * 4 && BN * 2 == 2 * 64 * 4 && RN_BYTES == 4 * 64 * 4,
              "a dword per lane: two waves move either operand's scale pairs, four the norms");

// rmax[i] = max(rmax[i], the lane's 16 values of tile row i, each times its bank row's rn:
// rn[j] = the reciprocal norms of bank columns 4 fq .. 4 fq + 3 of column tile j)
__device__ __forceinline__ void fold_tile_scaled(float4_t (&acc)[RM][RN], const float4_t* rn, float (&rmax)[RM]) {
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const float4_t f = rn[4 * j];  // 16 columns on
#pragma unroll
    for (int i = 0; i < RM; ++i) {
      const float4_t v = acc[i][j] * f;
#pragma unroll
      for (int e = 0; e < 4; ++e) rmax[i] = fmaxf(rmax[i], v[e]);
      acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    }
  }
}

__global__ __launch_bounds__(NWAVES * 64) void bank_nn_mx_kernel(BankMxArgs x) {
  const BankArgs& a = x.b;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int split = blockIdx.x % a.n_splits, m0 = (blockIdx.x / a.n_splits) * BM;
  const int t0 = split * a.tiles_per_split;
  const int nt = min(a.tiles_per_split, a.tiles_n - t0);
  const int nk = a.K / 128;

  const TileDma<1> dma(a, m0, wid, lane);
  // scale DMA (waves 0-1 the query rows', 2-3 the bank rows'): the lane's dword is the pairs of
  // tile rows sp and sp + 1; ld is even and at least the row count, so the clamped source stays
  // inside the buffer and every real row keeps its own. Waves 4-7 bring a bank tile's 256
  // reciprocal norms with its first K-step, a row past the end being the last row again.
  const int sp = ((wid & 1) * 64 + lane) * 2;
  const uint8_t* qs_src = x.q_sc + min((int64_t)m0 + sp, x.ld_qsc - 2) * 2;
  char* const sc_lds = smem + 2 * STAGE_BYTES;
  char* const rn_lds = sc_lds + 2 * SC_BYTES;
  auto stage = [&](int t, int kt, int buf, bool first) {
    const int n0 = (t0 + t) * BN;
    if (wid < 2) {
      __builtin_amdgcn_global_load_lds((const void*)(qs_src + (int64_t)kt * x.ld_qsc * 2),
                                       LDS_PTR(sc_lds + buf * SC_BYTES + wid * 256), 4, 0, 0);
    } else if (wid < 4) {
      const uint8_t* src = x.r_sc + ((int64_t)kt * x.ld_rsc + min((int64_t)n0 + sp, x.ld_rsc - 2)) * 2;
      __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(sc_lds + buf * SC_BYTES + BM * 2 + (wid - 2) * 256),
                                       4, 0, 0);
    } else if (first) {
      const float* src = x.r_rnorm + min(n0 + (wid - 4) * 64 + lane, a.Nb - 1);
      __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(rn_lds + (t % RN_SLOTS) * RN_BYTES + (wid - 4) * 256), 4, 0,
                                       0);
    }
    dma.stage(a, smem + buf * STAGE_BYTES, n0, kt, wid);
  };

  // fragment of tile row r0 + 16 i (r0 % 16 == fr): chunks fq and 4 + fq of the row, swizzle undone
  // (r & 7 == fr & 7 for every i, and the two chunk numbers differ in bit 2, so every offset is one
  // of two lane values plus a constant). The row's scale byte is the one of its block fq / 2; a
  // clamped query row is never stored, so it may read whatever scale its tile row has.
  const int fr = lane & 15, fq = lane >> 4;
  const int ch0 = (fq ^ (fr & 7)) << 4;
  const int a_off = (wm * TM + fr) * 128 + ch0, b_off = A_BYTES + (wn * TN + fr) * 128 + ch0;
  const int qs_off = (wm * TM + fr) * 2 + (fq >> 1);
  auto frag = [&](const char* p, int off) {  // off ^ 64: chunk 4 + fq (bit 6 of off is the chunk's bit 2)
    const i32x4_t lo = *(const i32x4_t*)(p + off), hi = *(const i32x4_t*)(p + (off ^ 64));
    return i32x8_t{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  };

  float4_t acc[RM][RN];
  float rmax[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    rmax[i] = -INFINITY;
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
  }

  stage(0, 0, 0, true);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    // where the scale pairs of the lane's bank rows lie: a tile row past the end duplicates the
    // last row, and takes its scales
    int bs_off[RN];
#pragma unroll
    for (int j = 0; j < RN; ++j)
      bs_off[j] = BM * 2 + min(wn * TN + j * 16 + fr, a.Nb - 1 - (t0 + t) * BN) * 2 + (fq >> 1);
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk)
        stage(t, kt + 1, cur ^ 1, false);
      else if (t + 1 < nt)
        stage(t + 1, 0, cur ^ 1, true);
      const char* base = smem + cur * STAGE_BYTES;
      const char* scb = sc_lds + cur * SC_BYTES;
      i32x8_t bf[RN];
      int sb[RN];
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        bf[j] = frag(base + j * 2048, b_off);
        sb[j] = *(const uint8_t*)(scb + bs_off[j]);
      }
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        const i32x8_t af = frag(base + i * 2048, a_off);
        const int sq = *(const uint8_t*)(scb + qs_off + i * 32);
#pragma unroll
        for (int j = 0; j < RN; ++j)  // formats 0/0 = e4m3/e4m3; bank block scale, query block scale; C^T tile
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af, acc[i][j], 0, 0, 0, sb[j], 0, sq);
      }
      __syncthreads();
      cur ^= 1;
    }
    fold_tile_scaled(acc, (const float4_t*)(rn_lds + (t % RN_SLOTS) * RN_BYTES) + (wn * TN) / 4 + fq, rmax);
  }
  store_rows<true>(a, rmax, (float*)smem, m0, split, wm, wn, lane, x.q_rnorm);
}

// ============================================================== combine, fusion
__global__ __launch_bounds__(MT) void bank_distance_kernel(const float* __restrict__ part, int M, int n_splits,
                                                           int accumulate, float* __restrict__ grid) {
  const int m = blockIdx.x * MT + threadIdx.x;
  if (m >= M) return;
  const float* p = part + (size_t)m * n_splits;
  float best = p[0];
  for (int s = 1; s < n_splits; ++s) best = fmaxf(best, p[s]);
  const float d = 1.0f - best;
  grid[m] = accumulate ? grid[m] + d : d;
}

// (x - lo) / (hi - lo), and 0 for a constant input
__device__ __forceinline__ float unit_range(float x, float lo, float hi) {
  return hi > lo ? (x - lo) / (hi - lo) : 0.0f;
}

// ranges: lo, hi of the zero-shot maps, the few-shot maps, the zero-shot scores, the few-shot scores
__global__ __launch_bounds__(MT) void fewshot_fuse_kernel(const float* __restrict__ zs_map,
                                                          const float* __restrict__ fs_map,
                                                          const float* __restrict__ zs_score,
                                                          const float* __restrict__ fs_score,
                                                          const float* __restrict__ ranges, int64_t total, int n_img,
                                                          float* __restrict__ fused_map,
                                                          float* __restrict__ fused_score) {
  const float zlo = ranges[0], zhi = ranges[1], flo = ranges[2], fhi = ranges[3];
  const int64_t i0 = (int64_t)blockIdx.x * MT + threadIdx.x;
  for (int64_t i = i0; i < total; i += (int64_t)gridDim.x * MT)
    fused_map[i] = unit_range(zs_map[i], zlo, zhi) + unit_range(fs_map[i], flo, fhi);
  if (i0 < n_img)
    fused_score[i0] = unit_range(zs_score[i0], ranges[4], ranges[5]) + unit_range(fs_score[i0], ranges[6], ranges[7]);
}

// ============================================================== greedy k-centre coreset
// aaclip_bank_coreset: farthest-point selection under 1 - cosine on unit rows (PatchCore's coreset
// subsampling), one launch of coreset_step_kernel per pick: the step boundary is the launch
// boundary, so there is no grid-wide wait, no atomic and no spin on memory.
//   centre    every block reduces the previous step's per-block candidates (value, index) to their
//             lexicographic minimum -- the same set in every block, and a minimum under a total
//             order does not depend on the reduction tree -- and block 0 stores sel[t], cover[t].
//   pass      the centre row goes to LDS as fp32; a block walks its slabs of CS_ROWS rows (slab
//             b, b + grid, ...: a function of N alone, the same in every step, so a row's bytes
//             keep coming from the same XCD's L2 and the Infinity Cache). Sixteen lanes share a
//             row, lane l taking its 16-byte chunks l, l + 16, ...; a wave has four such groups and
//             four passes of them in flight, so a lane holds four independent 16-byte loads per
//             chunk column against one LDS read of the centre.
//   order     a dot product is: per lane one fp32 accumulator from +0, fmaf over the lane's chunks
//             ascending and the elements of a chunk ascending; then across the sixteen lanes the
//             butterfly a += shfl_xor(a, 8), 4, 2, 1. A function of K and the dtype alone.
//   update    the group's lane 0 owns the row: maxsim = max(maxsim, dot) (step 0: = dot), the taken
//             byte (step 0 writes every row's, later steps only the centre's), and the running
//             (value, index) minimum over its rows that are not taken; wave shuffle and LDS bring
//             the block's candidate to thread 0, which stores it into the buffer of t's parity.
constexpr int CS_ROWS = AACLIP_CORESET_BLOCK_ROWS, CS_THREADS = 256, CS_WAVES = CS_THREADS / 64;
constexpr int CS_GROUP = 16, CS_PASSES = CS_ROWS / (CS_WAVES * (64 / CS_GROUP));
static_assert(CS_PASSES * CS_WAVES * (64 / CS_GROUP) == CS_ROWS, "a slab is whole passes of every wave");
typedef __attribute__((ext_vector_type(2))) int int2_t;
constexpr size_t kCoresetCandBytes = 2 * (size_t)AACLIP_CORESET_MAX_BLOCKS * sizeof(int2_t);

struct CoresetArgs {
  const void* R;
  int64_t ldr;  // elements
  int N, K, t, start;
  int32_t* sel;
  float* cover;
  float* maxsim;
  int2_t* cand;    // [2][AACLIP_CORESET_MAX_BLOCKS] (value bits, index)
  uint8_t* taken;  // [N]
};

// (v, i) < (bv, bi) in the order the pick minimises: the value, then the index
__device__ __forceinline__ void cand_min(float& bv, int& bi, float v, int i) {
  if (v < bv || (v == bv && i < bi)) bv = v, bi = i;
}

// the block's minimum of (v, i), in every thread; red: 2 * CS_WAVES words nobody else uses now
__device__ __forceinline__ void cand_block_min(float& v, int& i, float* red_v, int* red_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cand_min(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
  if ((threadIdx.x & 63) == 0) red_v[threadIdx.x >> 6] = v, red_i[threadIdx.x >> 6] = i;
  __syncthreads();
  v = red_v[0], i = red_i[0];
#pragma unroll
  for (int w = 1; w < CS_WAVES; ++w) cand_min(v, i, red_v[w], red_i[w]);
}

// DT: AACLIP_F32 (4 elements per 16-byte chunk), AACLIP_BF16 / AACLIP_F16 (8)
template <int DT>
__global__ __launch_bounds__(CS_THREADS) void coreset_step_kernel(CoresetArgs a) {
  constexpr int ES = DT == AACLIP_F32 ? 4 : 2, EPC = 16 / ES;
  __shared__ __attribute__((aligned(16))) float cs[AACLIP_CORESET_MAX_K];
  __shared__ float red_v[2][CS_WAVES];
  __shared__ int red_i[2][CS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nblocks = gridDim.x, nchunks = a.K / EPC;

  // ---- the centre
  int centre = a.start;
  float cov = -INFINITY;
  if (a.t > 0) {
    const int2_t* prev = a.cand + (size_t)((a.t - 1) & 1) * AACLIP_CORESET_MAX_BLOCKS;
    cov = INFINITY, centre = INT_MAX;
    for (int j = tid; j < nblocks; j += CS_THREADS) {
      const int2_t c = prev[j];
      cand_min(cov, centre, __int_as_float(c[0]), c[1]);
    }
    cand_block_min(cov, centre, red_v[0], red_i[0]);
    // t < N, so some row was not taken and the minimum is a row; non-finite inputs (outside the
    // contract) could leave INT_MAX here, and the centre is an address
    centre = min(centre, a.N - 1);
  }
  if (blockIdx.x == 0 && tid == 0) a.sel[a.t] = centre, a.cover[a.t] = cov;

  // ---- the centre row into LDS, fp32
  const char* Rg = (const char*)a.R;
  const size_t row_bytes = (size_t)a.ldr * ES;
  auto widen = [](const float4_t raw, float (&f)[EPC]) {
    if constexpr (DT == AACLIP_F32) {
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = raw[e];
    } else {
      const short8_t h = __builtin_bit_cast(short8_t, raw);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = h16_to_f32<DT == AACLIP_F16>((uint16_t)h[e]);
    }
  };
  for (int c = tid; c < nchunks; c += CS_THREADS) {
    float f[EPC];
    widen(*(const float4_t*)(Rg + (size_t)centre * row_bytes + (size_t)c * 16), f);
#pragma unroll
    for (int e = 0; e < EPC; ++e) cs[c * EPC + e] = f[e];
  }
  __syncthreads();

  // ---- the block's rows
  const int g = lane >> 4, l = lane & 15;
  const int slabs = ceil_div(a.N, CS_ROWS);
  float best_v = INFINITY;
  int best_i = INT_MAX;
  for (int slab = blockIdx.x; slab < slabs; slab += nblocks) {
    const int row0 = slab * CS_ROWS + wid * (CS_ROWS / CS_WAVES) + g;  // pass p: row0 + 4 p
    const char* src[CS_PASSES];
    float acc[CS_PASSES];
#pragma unroll
    for (int p = 0; p < CS_PASSES; ++p) {
      src[p] = Rg + (size_t)min(row0 + 4 * p, a.N - 1) * row_bytes;  // past the end: the last row, not stored
      acc[p] = 0.f;
    }
#pragma unroll 2
    for (int c = l; c < nchunks; c += CS_GROUP) {
      float4_t raw[CS_PASSES];
#pragma unroll
      for (int p = 0; p < CS_PASSES; ++p) raw[p] = *(const float4_t*)(src[p] + (size_t)c * 16);
      float cf[EPC];
#pragma unroll
      for (int e = 0; e < EPC; e += 4) {
        const float4_t v = *(const float4_t*)(cs + c * EPC + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) cf[e + j] = v[j];
      }
#pragma unroll
      for (int p = 0; p < CS_PASSES; ++p) {
        float rf[EPC];
        widen(raw[p], rf);
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[p] = fmaf(rf[e], cf[e], acc[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < CS_PASSES; ++p) {
      float d = acc[p];
#pragma unroll
      for (int o = CS_GROUP / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
      const int row = row0 + 4 * p;
      if (l == 0 && row < a.N) {
        const float ms = a.t == 0 ? d : fmaxf(a.maxsim[row], d);
        a.maxsim[row] = ms;
        bool tk = row == centre;
        if (a.t == 0 || tk)
          a.taken[row] = tk;
        else
          tk = a.taken[row] != 0;
        if (!tk) cand_min(best_v, best_i, ms, row);
      }
    }
  }
  cand_block_min(best_v, best_i, red_v[1], red_i[1]);
  if (tid == 0)
    a.cand[(size_t)(a.t & 1) * AACLIP_CORESET_MAX_BLOCKS + blockIdx.x] = int2_t{__float_as_int(best_v), best_i};
}

// blocks of a coreset launch: the slabs dealt evenly over the fewest grid-stride trips that keep
// the block count within AACLIP_CORESET_MAX_BLOCKS. A function of N alone.
int coreset_blocks(int N) {
  const int slabs = ceil_div(N, CS_ROWS);
  return ceil_div(slabs, ceil_div(slabs, AACLIP_CORESET_MAX_BLOCKS));
}

// the split of the bank tiles over blocks: of the even splits into at most AACLIP_BANK_MAX_SPLITS
// parts (never an empty one) the one whose blocks take the fewest rounds x tiles on a chip that
// holds AACLIP_BANK_RESIDENT_BLOCKS of them at once (one per CU: 128 KiB of LDS each), a block
// costing its tiles plus half a tile of start and end; ties go to the fewer splits. A function of
// M and Nb alone, so a launch's layout never depends on the machine.
void bank_plan(int M, int Nb, int& tiles_n, int& tiles_per_split, int& n_splits) {
  const int64_t tiles_m = ceil_div(M, BM);
  tiles_n = ceil_div(Nb, BN);
  int64_t best = INT64_MAX;
  for (int want = 1; want <= std::min(tiles_n, AACLIP_BANK_MAX_SPLITS); ++want) {
    const int tps = ceil_div(tiles_n, want), ns = ceil_div(tiles_n, tps);
    const int64_t rounds = (tiles_m * ns + AACLIP_BANK_RESIDENT_BLOCKS - 1) / AACLIP_BANK_RESIDENT_BLOCKS;
    const int64_t cost = rounds * (2 * tps + 1);
    if (cost < best) best = cost, tiles_per_split = tps, n_splits = ns;
  }
}

constexpr int kBankMaxRows = 1 << 30;
constexpr size_t kFuseHead = AACLIP_FEWSHOT_FUSE_HEAD;  // the four ranges, ahead of the range workspace

template <bool H16>
int launch16(const BankArgs& a, int blocks, hipStream_t s) {
  static unsigned attr_dev = 0;
  if (!lds_attr_once((const void*)bank_nn16_kernel<H16>, kLds16, attr_dev)) return AACLIP_ERR_LAUNCH;
  bank_nn16_kernel<H16><<<blocks, NWAVES * 64, kLds16, s>>>(a);
  return AACLIP_OK;
}

}  // namespace

extern "C" int aaclip_bank_nn_workspace(int M, int Nb, size_t* bytes, int* n_splits) {
  AACLIP_REQUIRE(bytes && n_splits && M > 0 && Nb > 0 && M <= kBankMaxRows && Nb <= kBankMaxRows);
  int tiles_n, tps, ns;
  bank_plan(M, Nb, tiles_n, tps, ns);
  *n_splits = ns;
  *bytes = (size_t)M * ns * sizeof(float);
  return AACLIP_OK;
}

extern "C" int aaclip_bank_nn(int dtype, int M, int Nb, int K, const void* Q, int64_t ldq, const void* R, int64_t ldr,
                              float* part, size_t part_bytes, void* stream) {
  AACLIP_REQUIRE(Q && R && part && M > 0 && Nb > 0 && K > 0 && M <= kBankMaxRows && Nb <= kBankMaxRows);
  AACLIP_REQUIRE(dtype == AACLIP_F32 || dtype == AACLIP_BF16 || dtype == AACLIP_F16);
  const int64_t es = dtype == AACLIP_F32 ? 4 : 2;
  AACLIP_REQUIRE(K % 64 == 0 && ldq >= K && ldr >= K && (ldq * es) % 16 == 0 && (ldr * es) % 16 == 0);
  AACLIP_REQUIRE(aligned16(Q) && aligned16(R) && aligned4(part));
  BankArgs a{Q, R, part, ldq, ldr, M, Nb, K, 0, 0, 0};
  bank_plan(M, Nb, a.tiles_n, a.tiles_per_split, a.n_splits);
  AACLIP_REQUIRE(part_bytes >= (size_t)M * a.n_splits * sizeof(float));
  const int64_t blocks = (int64_t)ceil_div(M, BM) * a.n_splits;
  AACLIP_REQUIRE(blocks < (1LL << 31));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AACLIP_F32) {
    bank_nn32_kernel<<<(int)blocks, NWAVES * 64, 0, s>>>(a);
  } else {
    const int rc = dtype == AACLIP_F16 ? launch16<true>(a, (int)blocks, s) : launch16<false>(a, (int)blocks, s);
    if (rc != AACLIP_OK) return rc;
  }
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_bank_nn_fp8mx(int M, int Nb, int K, const void* Q, int64_t ldq, const void* q_sc, int64_t ld_qsc,
                                    const float* q_rnorm, const void* R, int64_t ldr, const void* r_sc,
                                    int64_t ld_rsc, const float* r_rnorm, float* part, size_t part_bytes,
                                    void* stream) {
  AACLIP_REQUIRE(Q && q_sc && q_rnorm && R && r_sc && r_rnorm && part);
  AACLIP_REQUIRE(M > 0 && Nb > 0 && K > 0 && M <= kBankMaxRows && Nb <= kBankMaxRows && K % 128 == 0);
  AACLIP_REQUIRE(ldq >= K && ldr >= K && ldq % 16 == 0 && ldr % 16 == 0);
  AACLIP_REQUIRE(ld_qsc >= M && ld_rsc >= Nb && ld_qsc % 2 == 0 && ld_rsc % 2 == 0);
  AACLIP_REQUIRE(aligned16(Q) && aligned16(R) && aligned4(q_sc) && aligned4(r_sc));
  AACLIP_REQUIRE(aligned4(q_rnorm) && aligned4(r_rnorm) && aligned4(part));
  BankMxArgs x{{Q, R, part, ldq, ldr, M, Nb, K, 0, 0, 0}, (const uint8_t*)q_sc, (const uint8_t*)r_sc, q_rnorm, r_rnorm,
               ld_qsc, ld_rsc};
  bank_plan(M, Nb, x.b.tiles_n, x.b.tiles_per_split, x.b.n_splits);
  AACLIP_REQUIRE(part_bytes >= (size_t)M * x.b.n_splits * sizeof(float));
  const int64_t blocks = (int64_t)ceil_div(M, BM) * x.b.n_splits;
  AACLIP_REQUIRE(blocks < (1LL << 31));
  static unsigned attr_dev = 0;
  if (!lds_attr_once((const void*)bank_nn_mx_kernel, kLdsMx, attr_dev)) return AACLIP_ERR_LAUNCH;
  bank_nn_mx_kernel<<<(int)blocks, NWAVES * 64, kLdsMx, (hipStream_t)stream>>>(x);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_bank_distance(const float* part, int M, int n_splits, int accumulate, float* grid,
                                    void* stream) {
  AACLIP_REQUIRE(part && grid && M > 0 && n_splits > 0 && n_splits <= AACLIP_BANK_MAX_SPLITS);
  AACLIP_REQUIRE(aligned4(part) && aligned4(grid));
  bank_distance_kernel<<<ceil_div(M, MT), MT, 0, (hipStream_t)stream>>>(part, M, n_splits, accumulate != 0, grid);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_fewshot_fuse(const float* zs_map, const float* fs_map, const float* zs_score, int n_images,
                                   int64_t pix_per_image, void* workspace, size_t workspace_bytes, float* fused_map,
                                   float* fs_score, float* fused_score, void* stream) {
  AACLIP_REQUIRE(zs_map && fs_map && zs_score && workspace && fused_map && fs_score && fused_score);
  AACLIP_REQUIRE(n_images > 0 && n_images <= (1 << 24) && pix_per_image > 0);
  size_t rbytes = 0;
  AACLIP_REQUIRE(aaclip_overlay_workspace(n_images, &rbytes) == AACLIP_OK);
  AACLIP_REQUIRE(aligned16(workspace) && workspace_bytes >= kFuseHead + rbytes);
  float* ranges = (float*)workspace;
  void* rws = (char*)workspace + kFuseHead;
  hipStream_t s = (hipStream_t)stream;
  // fs_score = each image's maximum (the per-image minima go to the range workspace, which the
  // range calls below overwrite: all on one stream)
  row_minmax_kernel<<<n_images, MT, 0, s>>>(fs_map, pix_per_image, (float*)rws, fs_score);
  AACLIP_CHECK_LAUNCH();
  const float* src[4] = {zs_map, fs_map, zs_score, fs_score};
  for (int i = 0; i < 4; ++i) {
    const int rc = aaclip_overlay_range(src[i], n_images, i < 2 ? pix_per_image : 1, rws, rbytes, ranges + 2 * i, s);
    if (rc != AACLIP_OK) return rc;
  }
  const int64_t total = (int64_t)n_images * pix_per_image;
  const int64_t blocks = std::max<int64_t>(std::min<int64_t>((total + MT - 1) / MT, 1 << 16), ceil_div(n_images, MT));
  fewshot_fuse_kernel<<<(int)blocks, MT, 0, s>>>(zs_map, fs_map, zs_score, fs_score, ranges, total, n_images,
                                                fused_map, fused_score);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

extern "C" int aaclip_bank_coreset_workspace(int N, size_t* bytes) {
  AACLIP_REQUIRE(bytes && N > 0 && N <= kBankMaxRows);
  *bytes = kCoresetCandBytes + (((size_t)N + 15) & ~(size_t)15);  // the candidates, then the taken bytes
  return AACLIP_OK;
}

extern "C" int aaclip_bank_coreset(int dtype, int N, int K, const void* R, int64_t ldr, int m, int start,
                                   int32_t* sel, float* cover, float* maxsim, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  AACLIP_REQUIRE(R && sel && cover && maxsim && workspace && N > 0 && N <= kBankMaxRows && K > 0);
  AACLIP_REQUIRE(dtype == AACLIP_F32 || dtype == AACLIP_BF16 || dtype == AACLIP_F16);
  const int64_t es = dtype == AACLIP_F32 ? 4 : 2;
  AACLIP_REQUIRE(K % 64 == 0 && K <= AACLIP_CORESET_MAX_K && ldr >= K && (ldr * es) % 16 == 0);
  AACLIP_REQUIRE(m >= 1 && m <= N && start >= 0 && start < N);
  AACLIP_REQUIRE(aligned16(R) && aligned16(workspace) && aligned4(sel) && aligned4(cover) && aligned4(maxsim));
  size_t need = 0;
  AACLIP_REQUIRE(aaclip_bank_coreset_workspace(N, &need) == AACLIP_OK && workspace_bytes >= need);
  CoresetArgs a{R, ldr, N, K, 0, start, sel, cover, maxsim, (int2_t*)workspace,
                (uint8_t*)workspace + kCoresetCandBytes};
  const int blocks = coreset_blocks(N);
  hipStream_t s = (hipStream_t)stream;
  for (a.t = 0; a.t < m; ++a.t) {
    if (dtype == AACLIP_F32)
      coreset_step_kernel<AACLIP_F32><<<blocks, CS_THREADS, 0, s>>>(a);
    else if (dtype == AACLIP_F16)
      coreset_step_kernel<AACLIP_F16><<<blocks, CS_THREADS, 0, s>>>(a);
    else
      coreset_step_kernel<AACLIP_BF16><<<blocks, CS_THREADS, 0, s>>>(a);
    AACLIP_CHECK_LAUNCH();
  }
  return AACLIP_OK;
}
