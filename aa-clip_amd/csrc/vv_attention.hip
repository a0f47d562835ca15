// v-v "surgery" attention of the frozen tower (include/aaclip.h aaclip_vv_attention;
// reference model/transformer.py:125-152 as DAPM_replace, :407-425, wires it in).
//
// The reference's Attention is handed the tower's [L, N, D] layout and unpacks it as
// [B, N, C], so its softmax runs ACROSS THE IMAGES of the batch, separately for every
// token position t and head h:
//   S[b,c] = v[b,t,h] . v[c,t,h] / 8,  P = softmax_c(S),  out[b,t,h] = sum_c P[b,c] v[c,t,h]
//
// Work split: one wave per (token, head), four heads per workgroup (1-D grid, the head
// groups of a token adjacent). The wave stages its
// batch x 64 tile as fp32 in LDS (row stride 68 floats: rows 4 banks apart, so the
// per-image 128-bit reads below do not collide). With BP = batch rounded up to a power of
// two, lane = q*BP + b owns image b and the BP head dims [q*BP, (q+1)*BP): a score is a
// BP-term partial dot per lane plus an xor butterfly over the 64/BP lanes of that image
// (fixed order, the same bits in every lane of the group). Two passes over the images:
// row maximum of the raw scores, then exp2((s - max) * log2(e)/8) / sum / P.V (scores
// recomputed: the same instructions, so the same bits; at batch 1 the result is v itself).
// All arithmetic fp32; the only rounding to the storage type is the final store. No atomics; every (token, head) is computed by one wave from its own tile, so a
// token's result does not depend on which other tokens the launch holds.
// Per layer the kernel reads and writes R x heads*64 elements once and does 6*B^2*64
// fp32 FLOP per (token, head) (the recomputed pass included): bandwidth-bound at B = 16.
#include "attn_lds.h"  // kAttnLog2Scale

namespace {

constexpr int HD_ = 64;
constexpr int VV_LDR = 68;    // LDS row stride in floats
constexpr int VV_WAVES = 4;   // heads per workgroup

template <int DT>
struct VvElem {  // 16-bit storage: 8 elements per 128-bit access
  using type = uint16_t;
  static constexpr int CH = 8;
};
template <>
struct VvElem<AACLIP_F32> {
  using type = float;
  static constexpr int CH = 4;
};

template <int DT>
__device__ __forceinline__ void vv_load_chunk(const typename VvElem<DT>::type* g, float* l) {
  if constexpr (DT == AACLIP_F32) {
    *(float4_t*)l = *(const float4_t*)g;
  } else {
    const short8_t raw = *(const short8_t*)g;
    float4_t lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo[j] = h16_to_f32<DT == AACLIP_F16>((uint16_t)raw[j]);
      hi[j] = h16_to_f32<DT == AACLIP_F16>((uint16_t)raw[4 + j]);
    }
    *(float4_t*)l = lo;
    *(float4_t*)(l + 4) = hi;
  }
}

template <int DT>
__device__ __forceinline__ void vv_store_chunk(const float* l, typename VvElem<DT>::type* g) {
  if constexpr (DT == AACLIP_F32) {
    *(float4_t*)g = *(const float4_t*)l;
  } else {
    const float4_t lo = *(const float4_t*)l, hi = *(const float4_t*)(l + 4);
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
    u32x4_t pk;
    pk[0] = pack_h16x2<DT == AACLIP_F16>(lo[0], lo[1]);
    pk[1] = pack_h16x2<DT == AACLIP_F16>(lo[2], lo[3]);
    pk[2] = pack_h16x2<DT == AACLIP_F16>(hi[0], hi[1]);
    pk[3] = pack_h16x2<DT == AACLIP_F16>(hi[2], hi[3]);
    *(u32x4_t*)g = pk;
  }
}

// the BP floats at p (16-byte aligned when BP >= 4)
template <int BP>
__device__ __forceinline__ void vv_read(const float* p, float (&r)[BP]) {
  if constexpr (BP >= 4) {
#pragma unroll
    for (int j = 0; j < BP; j += 4) {
      const float4_t x = *(const float4_t*)(p + j);
      r[j] = x[0], r[j + 1] = x[1], r[j + 2] = x[2], r[j + 3] = x[3];
    }
  } else {
#pragma unroll
    for (int j = 0; j < BP; ++j) r[j] = p[j];
  }
}

// raw score (v_b . v_c, unscaled) of this lane's image against the image whose tile row is vc
template <int BP>
__device__ __forceinline__ float vv_score(const float (&vb)[BP], const float (&vc)[BP]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < BP; ++j) s = fmaf(vb[j], vc[j], s);
#pragma unroll
  for (int o = BP; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  return s;
}

template <int DT, int BP>
__global__ __launch_bounds__(64 * VV_WAVES) void vv_attention_kernel(
    const typename VvElem<DT>::type* __restrict__ v, int64_t ld_v, typename VvElem<DT>::type* __restrict__ out,
    int64_t ld_out, int batch, int n_tok, int heads, int hgroups) {
  extern __shared__ __attribute__((aligned(16))) float vv_lds[];
  constexpr int CH = VvElem<DT>::CH;
  constexpr int LPR = HD_ / CH;  // lanes per tile row in the load / store phases
  constexpr int RPP = 64 / LPR;  // rows per pass
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // head groups fastest: neighbouring workgroups read neighbouring 512-byte pieces of a row
  const int t = blockIdx.x / hgroups, h = (blockIdx.x % hgroups) * VV_WAVES + wave;
  const bool live = h < heads;  // wave-uniform; idle waves still reach the barriers
  float* tile = vv_lds + (size_t)wave * batch * VV_LDR;
  const int lrow = lane / LPR, lcol = (lane % LPR) * CH;

  if (live) {
    for (int r0 = 0; r0 < batch; r0 += RPP) {
      const int r = r0 + lrow;
      if (r < batch)
        vv_load_chunk<DT>(v + ((int64_t)r * n_tok + t) * ld_v + h * HD_ + lcol, tile + r * VV_LDR + lcol);
    }
  }
  __syncthreads();

  const int b = lane % BP, q = lane / BP;
  float acc[BP];
  float inv = 0.f;
  if (live) {
    // lanes of the padding images (b >= batch) shadow the last image: same reads, no store
    const int bb = b < batch ? b : batch - 1;
    const float* col = tile + q * BP;
    float vb[BP], vc[BP];
    vv_read<BP>(col + bb * VV_LDR, vb);
    float m = -INFINITY;
    for (int c = 0; c < batch; ++c) {
      vv_read<BP>(col + c * VV_LDR, vc);
      m = fmaxf(m, vv_score<BP>(vb, vc));
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < BP; ++j) acc[j] = 0.f;
    for (int c = 0; c < batch; ++c) {
      vv_read<BP>(col + c * VV_LDR, vc);
      // the maximum is taken on the raw scores and the scale applied to the difference: the
      // maximum's own argument is an exact 0 (a scaled score minus a scaled maximum could be
      // contracted into one fma and leave the product's rounding error there instead)
      const float p = exp2f((vv_score<BP>(vb, vc) - m) * kAttnLog2Scale);
      l += p;
#pragma unroll
      for (int j = 0; j < BP; ++j) acc[j] = fmaf(p, vc[j], acc[j]);
    }
    inv = 1.0f / l;
  }
  __syncthreads();  // every read of the tile is done: results go back in place
  if (live && b < batch) {
    float* dst = tile + b * VV_LDR + q * BP;
#pragma unroll
    for (int j = 0; j < BP; ++j) dst[j] = acc[j] * inv;
  }
  __syncthreads();
  if (live) {
    for (int r0 = 0; r0 < batch; r0 += RPP) {
      const int r = r0 + lrow;
      if (r < batch)
        vv_store_chunk<DT>(tile + r * VV_LDR + lcol, out + ((int64_t)r * n_tok + t) * ld_out + h * HD_ + lcol);
    }
  }
}

template <int DT, int BP>
int vv_launch(const void* v, int64_t ld_v, void* out, int64_t ld_out, int batch, int n_tok, int heads,
              hipStream_t s) {
  using T = typename VvElem<DT>::type;
  static unsigned done = 0;
  const int lds = VV_WAVES * batch * VV_LDR * (int)sizeof(float);
  if (!lds_attr_once((const void*)vv_attention_kernel<DT, BP>, VV_WAVES * AACLIP_VV_MAX_BATCH * VV_LDR * 4, done))
    return AACLIP_ERR_LAUNCH;
  const int hgroups = ceil_div(heads, VV_WAVES);
  vv_attention_kernel<DT, BP><<<dim3(n_tok * hgroups), 64 * VV_WAVES, lds, s>>>((const T*)v, ld_v, (T*)out, ld_out,
                                                                             batch, n_tok, heads, hgroups);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

template <int DT>
int vv_dispatch(const void* v, int64_t ld_v, void* out, int64_t ld_out, int batch, int n_tok, int heads,
                hipStream_t s) {
  if (batch <= 1) return vv_launch<DT, 1>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  if (batch <= 2) return vv_launch<DT, 2>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  if (batch <= 4) return vv_launch<DT, 4>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  if (batch <= 8) return vv_launch<DT, 8>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  if (batch <= 16) return vv_launch<DT, 16>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  if (batch <= 32) return vv_launch<DT, 32>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  return vv_launch<DT, 64>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
}

}  // namespace

extern "C" int aaclip_vv_attention(int dtype, const void* v, int64_t ld_v, void* out, int64_t ld_out, int batch,
                                   int n_tok, int heads, int head_dim, void* stream) {
  AACLIP_REQUIRE(dtype == AACLIP_F32 || dtype == AACLIP_BF16 || dtype == AACLIP_F16);
  AACLIP_REQUIRE(v && out && v != out);
  AACLIP_REQUIRE(head_dim == HD_ && batch >= 1 && batch <= AACLIP_VV_MAX_BATCH && n_tok >= 1 && heads >= 1);
  AACLIP_REQUIRE((int64_t)n_tok * ceil_div(heads, VV_WAVES) < (1ll << 31));  // grid.x
  const int64_t width = (int64_t)heads * HD_;
  AACLIP_REQUIRE(ld_v >= width && ld_out >= width);
  // every access is one 128-bit vector: 8 elements in the 16-bit types, 4 in fp32
  const int esize = dtype == AACLIP_F32 ? 4 : 2;
  const int vec = 16 / esize;
  AACLIP_REQUIRE(ld_v % vec == 0 && ld_out % vec == 0);
  AACLIP_REQUIRE(((uintptr_t)v % 16) == 0 && ((uintptr_t)out % 16) == 0);
  // rows are indexed in 64 bits; the row count stays an int and the byte extent of either
  // operand below 2^46 (far above any device memory), so no offset product can wrap
  const int64_t rows = (int64_t)batch * n_tok;
  AACLIP_REQUIRE(rows < (1ll << 31));
  AACLIP_REQUIRE(ld_v < (1ll << 31) && ld_out < (1ll << 31));
  AACLIP_REQUIRE(rows * ld_v * esize < (1ll << 46) && rows * ld_out * esize < (1ll << 46));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AACLIP_F32) return vv_dispatch<AACLIP_F32>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  if (dtype == AACLIP_F16) return vv_dispatch<AACLIP_F16>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
  return vv_dispatch<AACLIP_BF16>(v, ld_v, out, ld_out, batch, n_tok, heads, s);
}
