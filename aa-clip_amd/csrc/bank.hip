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
//   combine   aaclip_bank_distance: grid[m] = (accumulate ? grid[m] : 0) + (1 - max_s part[m][s]).
//   fusion    aaclip_fewshot_fuse: class-normalised zero-shot + few-shot maps and scores, every
//             operation a rounded fp32 one (tests/fewshot_ref.py states it in numpy float32).
//
// Inputs are finite: the object is built with -fno-honor-nans (Makefile), which drops the
// canonicalising v_max hipcc otherwise puts in front of every fmaxf of an MFMA result.
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
// wave columns through `red` (WN * BM floats of LDS nobody reads any more), then out
__device__ __forceinline__ void store_rows(const BankArgs& a, const float (&rmax)[RM], float* red, int m0, int split,
                                           int wm, int wn, int lane) {
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
    a.part[(size_t)(m0 + r) * a.n_splits + split] = v;
  }
}

// ============================================================== 16-bit operands
constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE_BYTES = A_BYTES + B_BYTES;
constexpr int A_LOADS = A_BYTES / (NWAVES * 1024), B_LOADS = B_BYTES / (NWAVES * 1024);  // glds per wave per stage
constexpr int kLds16 = 2 * STAGE_BYTES;
static_assert(A_LOADS * NWAVES * 1024 == A_BYTES && B_LOADS * NWAVES * 1024 == B_BYTES, "tile");
static_assert(WN * BM * (int)sizeof(float) <= STAGE_BYTES, "the row reduction reuses a stage");

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

  // per-lane DMA sources (row r = piece * 8 + lane / 8 of the tile, physical 16-B chunk
  // p = lane % 8 holds logical chunk p ^ (r & 7)); rows past the end are the last row
  const char* __restrict__ Rg = (const char*)a.R;
  const char* q_src[A_LOADS];
  int b_row[B_LOADS], b_col[B_LOADS];
#pragma unroll
  for (int i = 0; i < A_LOADS; ++i) {
    const int r = (i * NWAVES + wid) * 8 + (lane >> 3);
    q_src[i] = (const char*)a.Q + (size_t)min(m0 + r, a.M - 1) * a.ldq * 2 + (((lane & 7) ^ (r & 7)) << 4);
  }
#pragma unroll
  for (int i = 0; i < B_LOADS; ++i) {
    b_row[i] = (i * NWAVES + wid) * 8 + (lane >> 3);
    b_col[i] = ((lane & 7) ^ (b_row[i] & 7)) << 4;
  }
  auto stage = [&](int t, int kt, int buf) {
    char* base = smem + buf * STAGE_BYTES;
    const int n0 = (t0 + t) * BN;
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(q_src[i] + kt * 128), LDS_PTR(base + (i * NWAVES + wid) * 1024),
                                       16, 0, 0);
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
      const char* src = Rg + (size_t)min(n0 + b_row[i], a.Nb - 1) * a.ldr * 2 + b_col[i] + kt * 128;
      __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(base + A_BYTES + (i * NWAVES + wid) * 1024), 16, 0,
                                       0);
    }
  };

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
