/*
 * aaclip.h — C ABI of libaaclip_hip.so, the MI355X (gfx950) kernels behind
 * AA-CLIP's anomaly-map inference path.
 *
 * Conventions (every entry point):
 *   - extern "C", stateless, re-entrant; returns 0 (AACLIP_OK) or an error
 *     code (AACLIP_ERR_ARG for a rejected argument, AACLIP_ERR_LAUNCH + hipError_t
 *     when the launch itself failed).
 *   - All tensor arguments are caller-owned DEVICE pointers (the caller's
 *     allocator owns them; nothing here allocates, frees or synchronises, so every
 *     call can be captured into a hipGraph). Row-major, leading dimensions in
 *     ELEMENTS. `stream` is a hipStream_t passed as void*.
 *   - dtype enums: AACLIP_F32 = 0, AACLIP_BF16 = 1, AACLIP_FP8 = 2, AACLIP_F16 = 3.
 *     bf16 / fp16 are stored as uint16.
 *
 * The reference (wei-paul/AA-CLIP) has no native code: each entry point below
 * replaces the PyTorch/kornia call sites cited next to it
 * (paths relative to the reference root). The binding a maintainer adds on the
 * reference side is the ctypes stub shown in INTEGRATION.md.
 */
#ifndef AACLIP_H_
#define AACLIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AACLIP_OK 0
#define AACLIP_ERR_ARG 1
#define AACLIP_ERR_LAUNCH 1000

#define AACLIP_F32 0
#define AACLIP_BF16 1
#define AACLIP_FP8 2   /* OCP e4m3 + e8m0 block scales (fp8 MX activations, config C5) */
#define AACLIP_F16 3   /* IEEE fp16: the parity-grade 16-bit mode (fp16 MFMA, same rate as bf16) */

/* GEMM epilogue flags (applied in this order) */
#define AACLIP_EPI_BIAS 1      /* + bias[n] (fp32)                          */
#define AACLIP_EPI_GELU 2      /* exact erf GELU (nn.GELU)                  */
#define AACLIP_EPI_LEAKY 4     /* LeakyReLU(0.01) (nn.LeakyReLU)            */
#define AACLIP_EPI_RESID 8     /* + residual[row, n] (fp32; may alias C)    */
#define AACLIP_EPI_AUX_BF16 16 /* also store a 16-bit copy of the result: fp16 when
                                  in_dtype is AACLIP_F16, bf16 otherwise      */
#define AACLIP_EPI_QGELU 32    /* QuickGELU v * sigmoid(1.702 v), applied where GELU
                                  is (reference model/transformer.py:46-49; the
                                  towers built with quick_gelu=True, model.py:84,129);
                                  exclusive with AACLIP_EPI_GELU               */

/* ABI version (bumped on any signature change; 2 = MX fp8 LayerNorm outputs, 3 = fp16 dtype,
 * aaclip_patch_logits, any-size blur_upsample; 6 = round 5: the rejected A/B entry points
 * removed, aaclip_trace_buffer added; 8 = aaclip_vv_attention) and the target.
 * The stage-1 loss head (aaclip_patch_logits_per_image, aaclip_seg_loss, aaclip_seg_loss_bwd,
 * aaclip_upsample_softmax_bwd, aaclip_patch_logits_bwd, aaclip_patch_logits_bwd_workspace)
 * was added under version 8: additions only, no existing signature changed. A version-8
 * library built before them is still refused by the loader, which checks that every
 * symbol it binds is exported ("lacks ...: stale"). The later additions under version 9
 * (the device metrics' AUPRO and F1-max, aaclip_regions_workspace / aaclip_extract_regions, the
 * overlay entry points of csrc/overlay.hip) went in the same way. */
int aaclip_abi_version(void);
const char* aaclip_arch(void);

/*
 * Diagnostic step timeline (trace builds only: `make trace` -> libaaclip_hip_trace.so;
 * the product library returns AACLIP_ERR_ARG). Every wave of an instrumented kernel
 * appends one record of 8 uint32 {t0 lo, t0 hi, t1 lo, t1 hi, tag, HW_ID, word 6 = XCC_ID
 * (bits 0-3) | the wave's s_memtime shader-cycle delta capped at 2^28-1 (bits 4-31),
 * workgroup} to the slab of its CU: slot = XCC << 8 | SE << 5 | SH << 4 | CU (2048
 * slots), records [2048][capacity][8], counter [2048][16] uint32 (slot s counts at
 * counter[16 s]; zero it before a traced run); a slot's records past capacity are
 * dropped (its counter still counts them). t0 / t1 are s_memrealtime (100 MHz,
 * chip-wide). records = counter = NULL, capacity = 0 turns it off. Not a reference
 * interface: tools/timeline.py reads it to measure the gap share of a step.
 */
int aaclip_trace_buffer(void* records, void* counter, unsigned capacity);

/*
 * C[M,N] = epilogue(A[M,K] . W[N,K]^T)        (nn.Linear / conv-as-GEMM)
 * Replaces: every addmm/mm of the path — MHA in_proj / out_proj
 * (model/transformer.py:200 via torch F.multi_head_attention_forward), MLP
 * c_fc + GELU and c_proj (transformer.py:211-219, :256-257), conv1 as GEMM
 * (transformer.py:359-365), adapter Linear+LeakyReLU (model/adapter_modules.py:6-26,
 * model/adapter.py:93), seg_proj/det_proj (adapter.py:107-110), text projection
 * (adapter.py:140, model/model.py:200).
 * in_dtype: A and W (bf16 -> bf16 MFMA, f16 -> f16 MFMA, f32 -> f32 MFMA).
 * out_dtype: C, either f32 or the 16-bit in_dtype.
 * K % 64 == 0, N % 128 == 0 (bf16/f16) / K % 16 == 0, N % 64 == 0 (f32), checked for
 * M == 0 as well; lda, ldw multiples of 8. A 16-bit C and the 16-bit aux copy leave as
 * 16-byte stores, so ldc (16-bit C) and ldaux are multiples of 8 elements; an fp32 C and
 * the fp32 residual move as float4, so ldc (fp32 C) and ldr are multiples of 4.
 * Output row remap when row_group > 0:
 *   out_row = (m / row_group) * row_group_out + row_offset + (m % row_group)
 * (used to write patch embeddings after each image's CLS slot). The same
 * remapped row indexes `residual` and `aux`.
 */
int aaclip_gemm(int in_dtype, int out_dtype, int M, int N, int K,
                const void* A, int64_t lda, const void* W, int64_t ldw,
                void* C, int64_t ldc, int epilogue, const float* bias,
                const float* residual, int64_t ldr, void* aux, int64_t ldaux,
                int row_group, int row_group_out, int row_offset, void* stream);

/*
 * Level projection straight into anomaly-map partials (the predict path: the full
 * projected rows are never written):
 *   v = epilogue(A[M,K] . W[N,K]^T)   (epilogue 0 or AACLIP_EPI_LEAKY)
 *   part[m][g] = { sum ||v||^2, sum v.t0, sum v.t1, 0 } over columns 32g .. 32g+31
 * with t0/t1 = T[c % t_period][0/1] (T [t_period][2] fp32: normal, abnormal anchor),
 * as fp32 float4 per (row, 32-column group): part [M][ld_part >= N/8] floats.
 * Each group is summed in a fixed order that does not depend on the tile family, so
 * the partials of a row are the same whatever the batch. 16-bit in_dtype only;
 * K % 64 == 0, N % 256 == 0, t_period % 64 == 0.
 * Replaces: seg_proj / det_proj (adapter.py:107-110) + the row norms and anchor dots
 * of calculate_similarity_map (forward_utils.py:197-202) and of the image score
 * (test.py:83-84).
 */
int aaclip_gemm_scores(int in_dtype, int M, int N, int K, const void* A, int64_t lda,
                       const void* W, int64_t ldw, int epilogue, const float* T, int t_period,
                       float* part, int64_t ld_part, void* stream);

/*
 * fp8 GEMM (config C5: fp8 MFMA weights):
 *   C[M,N] = epilogue( a_scale[m] * w_scale[n] * (A8[M,K] . W8[N,K]^T) )
 * A8, W8: OCP e4m3 bytes (gfx950 FP8), per-row / per-output-channel fp32 scales
 * (dequantised value = byte * scale). The main loop runs the block-scaled
 * K=128 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales) at twice the
 * bf16 rate; the scales fold into the epilogue ahead of bias/activation/residual.
 * Same epilogue flags and row remap as aaclip_gemm. K % 128 == 0, N % 128 == 0,
 * lda/ldw multiples of 16 bytes, w_scale 16-B aligned.
 * Replaces: the same nn.Linear call sites as aaclip_gemm, at reduced precision.
 */
int aaclip_gemm_fp8(int out_dtype, int M, int N, int K, const void* A, int64_t lda,
                    const float* a_scale, const void* W, int64_t ldw, const float* w_scale,
                    void* C, int64_t ldc, int epilogue, const float* bias,
                    const float* residual, int64_t ldr, void* aux, int64_t ldaux,
                    int row_group, int row_group_out, int row_offset, void* stream);

/*
 * fp8 MX GEMM (config C5): C[M,N] = epilogue( w_scale[n] * sum_k A[m,k] 2^(a_mx[m,k/64]-127) W8[n,k] )
 * A: e4m3 with an e8m0 scale per (row, 64-K block), stored [K/128][ld_amx][2] bytes
 * (the two 64-blocks of one 128-K step adjacent); W8: e4m3 with fp32 per-output-
 * channel scales. The block scales are applied by the MFMA itself
 * (v_mfma_scale_f32_16x16x128_f8f6f4's per-lane B scale), staged through LDS.
 * out_dtype AACLIP_FP8 (only with bias+GELU, the c_fc -> c_proj hand-off): C is
 * written as e4m3 with its own e8m0 scale per (row, 64 columns) in c_mx
 * [N/128][ld_cmx][2], ready to be the A operand of the next MX GEMM.
 * K % 128 == 0, N % 256 == 0, ld_amx >= M and even (the scales move as dwords).
 */
int aaclip_gemm_fp8mx(int out_dtype, int M, int N, int K, const void* A, int64_t lda,
                      const void* a_mx, int64_t ld_amx, const void* W, int64_t ldw,
                      const float* w_scale, void* C, int64_t ldc, int epilogue,
                      const float* bias, const float* residual, int64_t ldr, void* aux,
                      int64_t ldaux, void* c_mx, int64_t ld_cmx, void* stream);

/*
 * MX fp8 quantisation: q[r,c] = e4m3(x[r,c] * 2^-e), e = the smallest exponent with
 * max|x[r, 64-block]| * 2^-e <= 448; sc[(c/128)*ld_sc + r][(c/64)%2] = e + 127.
 * x: fp32 or bf16 [rows, cols], cols % 128 == 0.
 */
int aaclip_quant_fp8_mx(int in_dtype, const void* x, int64_t ldx, void* q, int64_t ldq, void* sc,
                        int64_t ld_sc, int rows, int cols, void* stream);

/*
 * Per-row fp8 quantisation for aaclip_gemm_fp8's A operand:
 *   scale[r] = max_c |x[r,c]| / 448 (1 for an all-zero row); q[r,c] = e4m3(x[r,c] / scale[r])
 * (round-to-nearest-even, v_cvt_pk_fp8_f32). x: fp32 or bf16 [rows, cols], cols % 8 == 0.
 */
int aaclip_quant_fp8_rows(int in_dtype, const void* x, int64_t ldx, void* q, int64_t ldq,
                          float* scale, int rows, int cols, void* stream);

/*
 * Tuning hook: select the bf16 GEMM tile family for benchmarking. Bits 0-3:
 * 0 = default dispatch (N % 256 == 0: per shape, 256x256 8-phase ping-pong or
 * 320x256 LDS-DMA, whichever needs fewer tile rounds weighted by per-tile cost,
 * and 128x128 when that choice would fill under half the CUs; else 256x128),
 * 1 = 256x256 (N % 256 == 0), 2 = 256x128, 3 = 8-phase everywhere, 4 = 8-phase
 * for N >= 2048 only, 8 = 320x256 everywhere, 9 = 128x128 everywhere, 11 = 64x64
 * everywhere (N % 64 == 0; the default for single-image shapes); for the
 * fp8 MX GEMM: 0 = 8-phase ping-pong (default), 6 = the 256x256 LDS-DMA kernel; bits 4-7:
 * tile-order group height (0 = 4); bit 8: s_setprio around the MFMA cluster;
 * bit 9: diagnostic timing mode that skips the epilogue (outputs NOT written);
 * bit 10: diagnostic mode that runs the epilogue but skips its global stores;
 * bit 11: the 8-phase kernel writes 4 s_memtime stamps per wave (start, main loop
 * done, epilogue issued, stores complete) as uint64 to aaclip_gemm's aux pointer,
 * [tile][wave][4] (only for epilogues without AACLIP_EPI_AUX_BF16).
 * Process-global; not for production use.
 */
int aaclip_set_gemm_variant(int variant);

/*
 * Pin the tile family aaclip_gemm uses for one (in_dtype, M, N, K) (bf16 / f16):
 * 1 = 256x256, 2 = 256x128, 3 = 256x256 8-phase ping-pong, 8 = 320x256,
 * 9 = 128x128, 11 = 64x64, 0 = unpin (back to the
 * heuristic). Set by a measuring tuner at
 * engine setup (aaclip/ops.py tune_gemm); every family accumulates K in the same
 * order, so a pin changes speed, never bits. Process-global (mutex-guarded), host
 * only; unpinning removes the entry, so at most 256 shapes are pinned at once.
 */
int aaclip_gemm_pin(int in_dtype, int M, int N, int K, int family);

/*
 * Concurrent-chunk mode for the CALLING HOST THREAD (on = 1 / 0; *previous, if
 * non-null, receives the old state): while set, 16-bit GEMMs whose 256x256 tiles fill
 * at least one round of the CUs launch the 8-phase kernel (the other stream's chunk
 * fills the partial last round). Set by VisualEngine.predict around the enqueue of
 * concurrent image chunks (graph capture included: the choice is made at launch).
 * Pins and the variant hook take precedence. Same K order, so bits are unchanged.
 */
int aaclip_gemm_concurrent(int on, int* previous);

/* Name of the kernel aaclip_gemm launches for (in_dtype, M, N, K) with lda = ldw = K,
 * on the calling thread, under the current variant / pins / concurrent mode (the
 * dispatch's own decision). Host only, for reports. */
const char* aaclip_gemm_plan(int in_dtype, int M, int N, int K);

/*
 * Multi-head attention core, softmax(q k^T / sqrt(d)) v per head, flash-style
 * (scores never materialised). qkv: [batch*seq, 3*heads*head_dim] packed
 * [q|k|v] exactly as nn.MultiheadAttention's in_proj output; out:
 * [batch*seq, heads*head_dim] (heads merged, ready for out_proj).
 * flags: AACLIP_ATTN_CAUSAL adds the text tower's -inf upper triangle
 * (transformer.py:629-635); AACLIP_ATTN_Q_PRESCALED (bf16/fp8 only) says the q
 * columns already carry log2(e)/sqrt(head_dim) (folded into the Q projection
 * weights and bias, so the kernel's softmax runs in the log2 domain with no
 * per-score scaling); without it the kernel scales its Q fragments itself.
 * head_dim must be 64.
 * Replaces: torch F.multi_head_attention_forward's q-scale/bmm/softmax/bmm
 * (transformer.py:200, need_weights=True branch; the averaged weights are
 * discarded by the caller, model/adapter.py:91 — never computed here).
 */
#define AACLIP_ATTN_CAUSAL 1
#define AACLIP_ATTN_Q_PRESCALED 2
int aaclip_attention(int dtype, const void* qkv, void* out, int batch, int seq,
                     int heads, int head_dim, int flags, void* out_mx, int64_t ld_mx,
                     void* stream);
/* dtype AACLIP_FP8: bf16 qkv in, out written as MX e4m3 [batch*seq, heads*64] with one
 * e8m0 scale per (row, head) in out_mx [heads/2][ld_mx >= batch*seq][2] (the out-proj
 * A operand of aaclip_gemm_fp8mx, config C5); out_mx ignored otherwise. */

/*
 * v-v "surgery" attention of the frozen tower: the attention the reference's
 * Attention module (model/transformer.py:125-152) computes once
 * VisionTransformer.DAPM_replace (transformer.py:407-425) has put it into a block,
 * x = softmax(v v^T / sqrt(d)) v (the q.k path is computed and discarded there, never
 * here). That module receives the tower's [L, N, D] layout and unpacks it as [B, N, C],
 * so the softmax runs across the IMAGES of the batch, separately for every token
 * position t and head h: out[b,t,h] = sum_c softmax_c(v[b,t,h].v[c,t,h] / 8) v[c,t,h].
 * v: first V column of row 0; row b*n_tok + t holds heads*head_dim columns, row stride
 * ld_v elements (a [R, heads*64] buffer, or the V third of a packed [R, 3*heads*64]
 * qkv buffer). out: [R, heads*64], row stride ld_out; must not alias v. dtype F32,
 * BF16 or F16 (input and output alike); arithmetic is fp32, the 1/sqrt(64) scale is
 * applied inside. head_dim must be 64, batch 1..AACLIP_VV_MAX_BATCH (one lane per image),
 * ld_* >= heads*64 and a multiple of the 128-bit vector (8 elements in the 16-bit types,
 * 4 in fp32), pointers 16-byte aligned, batch*n_tok and n_tok*ceil(heads/4) (the grid)
 * < 2^31 and either operand's byte extent < 2^46. Fixed reduction order, no atomics: a token's result does not depend
 * on the other tokens of the launch, and two launches give the same bits.
 */
#define AACLIP_VV_MAX_BATCH 64
int aaclip_vv_attention(int dtype, const void* v, int64_t ld_v, void* out, int64_t ld_out,
                        int batch, int n_tok, int heads, int head_dim, void* stream);

/* Tuning hook for the 16-bit attention kernel: 0 = default (3), 1 = 4 waves x 32 queries per
 * workgroup, 2 = 2 waves x 64 queries, 3 = 1 with each full key tile phase-split so one
 * query block's softmax runs beside the other's MFMAs. Process-global; for benchmarking. */
int aaclip_set_attn_variant(int variant);

/*
 * Patchify for conv1-as-GEMM: img [batch, channels, S, S] fp32 ->
 * cols [batch*(S/patch)^2, k_padded], column k = c*patch*patch + kh*patch + kw
 * (conv weight flattening order), zero for k >= channels*patch^2.
 * Replaces: the im2col inside conv1 (model/adapter.py:68).
 */
int aaclip_im2col(int out_dtype, const float* img, void* cols, int batch, int channels,
                  int img_size, int patch, int k_padded, void* stream);

/*
 * Visual token assembly + ln_pre + block-0 ln_1, one row per token:
 *   e = (t == 0 ? cls : x[row]) + pos[t];  x[row] = LN_pre(e);  h[row] = LN_1(x[row])
 * x: [batch*n_tok, width] fp32, rows t>=1 already hold conv1 patch embeddings.
 * Replaces: model/adapter.py:72-85 + the first ln_1 (transformer.py:254).
 */
int aaclip_embed_ln(int out_dtype, float* x, const float* cls, const float* pos,
                    const float* ln_pre_w, const float* ln_pre_b, const float* ln1_w,
                    const float* ln1_b, void* h, int batch, int n_tok, int width,
                    void* h_mx, int64_t ld_mx, void* stream);

/*
 * Row epilogue after a residual block (all optional stages, one pass):
 *   if u:   x = w*(u*||x||/||u||) + (1-w)*x              (adapter blend)
 *   if h:   h = LN(x; ln_w, ln_b)                         (next block's ln_1)
 *   if tap: tap[b*(n_tok-1)+t-1] = LN(x; post_w, post_b)  for t >= 1 (level tap + ln_post)
 * x: [rows, width] fp32, rows = batch*n_tok.
 * Replaces: model/adapter.py:92-101 (image) / :129-136 (text), the ln_1 of
 * transformer.py:254, and ln_post of level taps (adapter.py:100-105).
 */
int aaclip_block_tail(int out_dtype, float* x, const float* u, float adapt_weight,
                      const float* ln_w, const float* ln_b, void* h, const float* post_w,
                      const float* post_b, void* tap, int rows, int n_tok, int width,
                      void* h_mx, int64_t ld_mx, void* stream);

/* y = LN(x) rows (F.layer_norm, eps 1e-5, biased variance; transformer.py:37-43). */
int aaclip_layernorm(int out_dtype, const float* x, int64_t ldx, const float* w,
                     const float* b, void* y, int64_t ldy, int rows, int width,
                     void* y_mx, int64_t ld_mx, void* stream);

/*
 * (embed_ln, block_tail, layernorm) out_dtype AACLIP_FP8: the LayerNorm row (h / y)
 * is written as MX fp8 — e4m3 bytes [rows, width] plus an e8m0 scale per (row, 64
 * columns) in h_mx / y_mx [width/128][ld_mx >= rows][2], the A-operand format of
 * aaclip_gemm_fp8mx (config C5); level taps stay bf16. h_mx / ld_mx are ignored for
 * the other dtypes (pass NULL, 0).
 */

/*
 * Text embedding: x[s*ctx+t] = tok_emb[tokens[s,t]] + pos[t]; h = LN_1(x).
 * Replaces: model/adapter.py:118-123 / model/model.py:192-194 + first ln_1.
 */
int aaclip_text_embed_ln(int out_dtype, const int32_t* tokens, const float* tok_emb,
                         const float* pos, const float* ln1_w, const float* ln1_b, float* x,
                         void* h, int n_seq, int ctx, int width, void* stream);

/*
 * EOT gather + ln_final: y[s] = LN(x[s*ctx + argmax_t tokens[s,t]]).
 * Replaces: model/adapter.py:138-140 / model/model.py:199-200.
 */
int aaclip_eot_ln(int out_dtype, const float* x, const int32_t* tokens, const float* w,
                  const float* b, void* y, int n_seq, int ctx, int width, void* stream);

/*
 * Prompt-ensemble anchor: T[:, col] = normalize(mean_s normalize(emb[s])).
 * T: [dim, ncols] fp32. Replaces: forward_utils.py:155-159.
 */
int aaclip_anchor_reduce(const float* emb, int n, int dim, float* T, int col, int ncols,
                         void* stream);

/* y = x / max(||x||, 1e-12) per row (F.normalize, model/adapter.py:109). */
int aaclip_l2_normalize(int in_dtype, int out_dtype, const void* x, int64_t ldx, void* y,
                        int64_t ldy, int rows, int width, void* stream);

/*
 * Patch x anchor similarity for n_levels feature tensors (levels: HOST array
 * of n_levels device pointers, each [rows, channels], row stride ld):
 *   f_hat = normalize ? f/max(||f||,1e-12) : f;  A_c = 100 * f_hat . T[:, c]
 *   mode 0 (test): out[row] = sum_l (A_1 + 1 - A_0) / 2
 *   mode 1 (train, n_levels == 1): out[b, c, p] = A_c with b = row / group,
 *          p = row % group (channel-major [B, 2, group], ready for blur_upsample)
 * T: [channels, 2] fp32. group = patches per image (mode 1 only). Replaces: forward_utils.py:199-207 (+ the level sum of
 * test.py:93, moved before the blur/upsample: both are linear).
 */
int aaclip_patch_scores(int in_dtype, const void* const* levels, int n_levels, int64_t ld,
                        const float* T, int rows, int channels, int normalize, int mode,
                        int group, float* out, void* stream);

/*
 * Train-branch logits for any number of anchors: out[b, a, p] = 100 * f[b*group+p] . T[:, a]
 * (no normalisation; channel-major [B, n_anchor, group], the grid blur_upsample takes).
 * f: [rows, channels] fp32/bf16 (channels == 768), T: [channels, n_anchor] fp32,
 * 1 <= n_anchor <= 64. Replaces: forward_utils.py:199-202 for C != 2.
 */
int aaclip_patch_logits(int in_dtype, const void* f, int64_t ld, const float* T, int n_anchor,
                        int rows, int channels, int group, float* out, void* stream);

/*
 * aaclip_patch_logits with per-image anchors: the anchors of image b = row / group are at
 * T + b * t_stride floats ([channels, n_anchor] each; t_stride == 0: one shared set, and
 * then the output is bit-identical to aaclip_patch_logits, the same kernel). 1 <= n_anchor
 * <= 8 (what aaclip_blur_upsample takes), t_stride == 0 or >= channels * n_anchor.
 * Replaces: forward_utils.py:199-202 on the [bs, 768, 2] anchors of train.py:69-72, :86-89.
 */
int aaclip_patch_logits_per_image(int in_dtype, const void* f, int64_t ld, const float* T, int64_t t_stride,
                                  int n_anchor, int rows, int channels, int group, float* out, void* stream);

/*
 * Gaussian blur (kornia 0.6.9 gaussian_blur2d, reflect border, separable;
 * skipped when ksize == 0) then bilinear upsample with align_corners=True
 * (F.interpolate) to any out_size, optional softmax over the channel dim
 * (train branch, any 1 <= channels <= 8; channels == 1 leaves the logits as they are).
 * grid: [batch, channels, g, g] fp32 (g <= 64) -> out [batch, channels, S, S] fp32.
 * Replaces: forward_utils.py:208-215.
 */
int aaclip_blur_upsample(const float* grid, float* out, int batch, int channels, int g,
                         int out_size, int ksize, float sigma, int softmax, void* stream);

/*
 * Stage-1 segmentation loss, forward: FocalLoss() + BinaryDiceLoss()(p0, 1 - mask) +
 * BinaryDiceLoss()(p1, mask) as forward_utils.py:219-227 constructs them (:21-126).
 * probs [batch, 2, S, S] fp32 (S = out_size >= 2), mask [batch, S, S] fp32 in [0, 1].
 * Per pixel k = (int)mask, o_k = 1 - 1e-5, o_other = 1e-5, pt = o_0 p0 + o_1 p1 + 1e-5,
 * term = -(1 - pt)^2 log(pt); t_0 = 1 - mask, t_1 = mask.
 * sums [batch][8] fp64 = {sum term, sum p0 t0, sum p0, sum t0, sum p1 t1, sum p1, sum t1, 0}
 * per image (each depends on that image alone); loss[4] fp32 = {focal, dice0, dice1,
 * (focal + dice0) + dice1}, focal = sum term / (batch S^2), dice_c = 1 - (1/batch) sum_n
 * (2 sum p_c t_c + 1) / (sum p_c + sum t_c + 1).
 * partial: caller-owned workspace of >= batch * ceil(S^2 / AACLIP_SEGLOSS_CHUNK) * 8 doubles
 * (partial_bytes is checked). fp32 per pixel, fixed-order sums (fp64 across waves and
 * chunks), no atomics: two launches give the same bits. Replaces: calculate_seg_loss in the
 * stage-1 step train.py:86-100 (:90).
 */
#define AACLIP_SEGLOSS_CHUNK 4096
int aaclip_seg_loss(const float* probs, const float* mask, int batch, int out_size, double* partial,
                    size_t partial_bytes, double* sums, float* loss, void* stream);

/*
 * Backward of aaclip_seg_loss: dprobs [batch, 2, S, S] = dloss * d loss[3] / d probs, from
 * probs, mask, the sums aaclip_seg_loss wrote and the DEVICE scalar dloss (autograd's
 * grad_output; no host read). d focal / d p_c = o_c (2 (1 - pt) log pt - (1 - pt)^2 / pt) /
 * (batch S^2); d dice_c / d p_c = -(2 t_c D - Nn) / (batch D^2) with the image's
 * Nn = 2 sum p_c t_c + 1, D = sum p_c + sum t_c + 1. The mask gets no gradient.
 * Replaces: the autograd of forward_utils.py:21-126, :219-227 under train.py:96.
 */
int aaclip_seg_loss_bwd(const float* probs, const float* mask, const double* sums, const float* dloss,
                        int batch, int out_size, float* dprobs, void* stream);

/*
 * Backward of aaclip_blur_upsample(ksize = 0, softmax = 1) for channels == 2: grid
 * [batch, 2, g, g] (the logits the forward consumed; 2 <= g <= 64) and dprobs
 * [batch, 2, S, S] -> dgrid [batch, 2, g, g]. Each pixel's two probabilities are
 * recomputed from grid with the forward's arithmetic (the same device functions), softmax
 * backward dz_c = p_c (g_c - sum_k p_k g_k) (evaluated as p_0 p_1 (g_c - g_other), which does
 * not lean on p_0 + p_1 == 1 in fp32), then the transpose of the align_corners
 * bilinear interpolation as a gather (one wave per source cell; a pixel belongs to a cell
 * iff the forward's index computation puts it there). No atomics, deterministic.
 * Replaces: the autograd of forward_utils.py:211-215 under train.py:96.
 */
int aaclip_upsample_softmax_bwd(const float* grid, const float* dprobs, int batch, int channels, int g,
                                int out_size, float* dgrid, void* stream);

/*
 * Backward of the train-branch logits out[b, a, p] = 100 f[b group + p] . T_b[:, a]
 * (n_anchor == 2; f [rows, channels == 768] fp32/bf16, T_b at T + b * t_stride as in
 * aaclip_patch_logits_per_image, dgrid [batch, 2, group]). Either output may be NULL:
 *   dT[b, c, a] = 100 sum_p f[b group + p, c] dgrid[b, a, p]   ([batch, 768, 2] fp32; with
 *                 t_stride == 0 summed over the images in index order into one [768, 2])
 *   df[row, c]  = 100 sum_a dgrid[b, a, p] T_b[c, a]           ([rows, 768] fp32, contiguous)
 * f is read once: one wave per (image, AACLIP_LOGITS_BWD_ROWS patch rows) writes a dT
 * partial into workspace (needed when dT != NULL; aaclip_patch_logits_bwd_workspace gives
 * its size in bytes), a finalize pass sums the chunks in index order in fp64.
 * Replaces: the autograd of forward_utils.py:199-202 under train.py:96.
 */
#define AACLIP_LOGITS_BWD_ROWS 16
int aaclip_patch_logits_bwd_workspace(int rows, int group, size_t* bytes);
int aaclip_patch_logits_bwd(int in_dtype, const void* f, int64_t ld, const float* T, int64_t t_stride,
                            int n_anchor, const float* dgrid, int rows, int channels, int group,
                            float* workspace, size_t workspace_bytes, float* dT, float* df, void* stream);

/*
 * ---- Backward of the adapted text tower (stage 1: train.py:38-114 trains text_adapter) ----
 * Added under ABI version 8 as the loss head was: additions only; the loader refuses a
 * library that lacks one. All fp32, deterministic (no floating-point atomics, fixed reduction
 * orders: two launches give the same bits); a row's / sequence's result depends on that row
 * / sequence alone; every argument is checked before the first launch; nothing allocates,
 * synchronises or reads on the host. The input-gradient GEMMs dX = dY . W between them are
 * aaclip_gemm on transposed weight copies. Only the four text_adapter weights get a
 * gradient: no dW / db of the frozen tower, no bias or LayerNorm-parameter gradients.
 */

/*
 * Backward of aaclip_attention (fp32): dqkv [batch*seq, 3*heads*64] (packed [dq|dk|dv], every
 * element written) from the packed qkv the forward consumed and dout [batch*seq, heads*64].
 * P = softmax(q k^T / 8) is recomputed from q, k (the forward's output is not needed: the
 * softmax term is D_i = sum_j P_ij dP_ij), dP = dout v^T, dS = P (dP - D), dq = dS k / 8,
 * dk = dS^T q / 8, dv = P^T dout. flags: AACLIP_ATTN_CAUSAL or 0. head_dim == 64, 1 <= seq <=
 * 77 (the text context; one (sequence, head) per workgroup, its tiles in LDS), else
 * AACLIP_ERR_ARG before any launch. dk / dv rows are summed over the queries in index order by
 * that workgroup alone. dqkv must not alias qkv.
 * Replaces: the autograd of F.multi_head_attention_forward's core (model/transformer.py:200,
 * attn_mask of transformer.py:629-635) under model/adapter.py:125-128, train.py:99.
 */
int aaclip_attention_bwd(const float* qkv, const float* dout, float* dqkv, int batch, int seq, int heads,
                         int head_dim, int flags, void* stream);

/*
 * dx = [residual +] d LN(x; w) / dx . dy per row: mean and rstd are recomputed from x (eps 1e-5,
 * biased variance, aaclip_layernorm's arithmetic), g = dy w, xh = (x - mean) rstd,
 * dx = rstd (g - mean(g) - xh mean(g xh)). No dw / db. residual (optional, NULL = none) is the
 * incoming residual-stream gradient and may be dx itself (with the same leading dimension), as
 * may dy. width 768 or 1024 (what aaclip_layernorm takes); ld* >= width, multiples of 4.
 * Replaces: the autograd of ln_1 / ln_2 (model/transformer.py:37-43, :254-257) under train.py:99.
 */
int aaclip_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* w,
                         const float* residual, int64_t ldr, float* dx, int64_t lddx, int rows, int width,
                         void* stream);

/*
 * Backward of aaclip_eot_ln: g [n_seq*ctx, width] (every row written) = the ln_final backward
 * of dy[s] at row s*ctx + argmax_t tokens[s,t] (first occurrence, as the forward), zero in
 * every other row. x is the [n_seq*ctx, width] residual stream the forward read.
 * Replaces: the autograd of model/adapter.py:138-140 under train.py:99.
 */
int aaclip_eot_ln_bwd(const float* dy, const float* x, const int32_t* tokens, const float* w, float* g,
                      int n_seq, int ctx, int width, void* stream);

/*
 * y = f(x) elementwise, f selected by the GEMM epilogue flag `mode` (AACLIP_EPI_GELU,
 * AACLIP_EPI_QGELU or AACLIP_EPI_LEAKY): the very device function the fp32 aaclip_gemm epilogue
 * applies, so aaclip_gemm(BIAS) followed by aaclip_act gives the bits of aaclip_gemm(BIAS | f).
 * The training forward stores the c_fc pre-activation this way (model/transformer.py:211-219).
 * y may be x.
 */
int aaclip_act(int mode, const float* x, float* y, int64_t n, void* stream);

/*
 * dx = dy * f'(.) elementwise (dx may be dy). GELU (exact erf, nn.GELU) and QuickGELU
 * (transformer.py:46-49) take ref = the PRE-activation: gelu'(v) = Phi(v) + v phi(v),
 * quick'(v) = s + 1.702 v s (1 - s) with s = sigmoid(1.702 v). LeakyReLU(0.01)
 * (model/adapter_modules.py:6-26) takes ref = the OUTPUT, whose sign is the input's: slope 1
 * above 0, 0.01 at and below 0 (as torch's leaky_relu backward).
 * Replaces: the autograd of those activations under train.py:99.
 */
int aaclip_act_bwd(int mode, const float* dy, const float* ref, float* dx, int64_t n, void* stream);

/*
 * Backward of aaclip_block_tail's adapter blend y = w u |x| / |u| + (1 - w) x
 * (model/adapter.py:130-136; the norms are differentiated, as autograd does): with a = dy . u,
 *   dx = (1 - w) dy + w (a / |u|) x / |x|        du = w (|x| / |u|) (dy - u a / |u|^2)
 * one pass per row, norms summed in the forward's order. x is the PRE-blend block output, u the
 * adapter output; dx is the gradient through x alone (the caller adds the adapter path du -> x).
 * dx may be dy. width 768 or 1024.
 */
int aaclip_adapter_blend_bwd(const float* dy, const float* x, const float* u, float adapt_weight, float* dx,
                             float* du, int rows, int width, void* stream);

/*
 * Backward of aaclip_anchor_reduce: demb [n, dim] from dT[:, col] (dT [dim, ncols] fp32)
 * through T[:, col] = normalize(mean_s normalize(emb[s])). n <= 256, dim <= 1024 (the
 * forward's limits). Replaces: the autograd of forward_utils.py:155-159 under train.py:99.
 */
int aaclip_anchor_reduce_bwd(const float* emb, int n, int dim, const float* dT, int col, int ncols,
                             float* demb, void* stream);

/*
 * Weight gradient of a bias-free Linear y = x W^T: dW[n, k] = sum_m dY[m, n] X[m, k]
 * (dY [M, N], X [M, K], dW [N, K]; leading dimensions in elements). Any M >= 1; N and K
 * multiples of 64. Rows are cut into chunks of AACLIP_WGRAD_ROWS (a function of M alone); each
 * chunk's partial [N, K] is accumulated over its rows in index order (fp32 FMA) into
 * workspace, and a finalize pass sums the chunks in index order in fp64. workspace:
 * aaclip_linear_wgrad_workspace bytes (ceil(M / AACLIP_WGRAD_ROWS) * N * K floats).
 * Replaces: the autograd of the SimpleAdapter / SimpleProj Linear (model/adapter_modules.py:6-47)
 * under train.py:99; the image adapters of stage 2 (1024 x 1024) take the same entry.
 */
#define AACLIP_WGRAD_ROWS 64
int aaclip_linear_wgrad_workspace(int M, int N, int K, size_t* bytes);
int aaclip_linear_wgrad(const float* dY, int64_t lddy, const float* X, int64_t ldx, int M, int N, int K,
                        float* workspace, size_t workspace_bytes, float* dW, int64_t lddw, void* stream);

/* ------------------------------------------------------------------ stage-2 backward
 * Backward of the adapted visual tower (attention_bwd.hip, visual_bwd.hip; train.py:117-174
 * trains image_adapter only). fp32, deterministic (no floating-point atomics, fixed reduction orders), image / row
 * local; arguments are checked before the first launch, nothing allocates, synchronises or
 * reads on the host. The rest of the stage-2 backward is aaclip_layernorm_bwd, aaclip_act /
 * aaclip_act_bwd, aaclip_adapter_blend_bwd, aaclip_linear_wgrad and aaclip_gemm on transposed
 * weight copies. Only the image_adapter weights get a gradient.
 */

/*
 * Backward of the fp32, non-causal aaclip_attention for any sequence length (the visual tower:
 * 577 tokens at 336 px, 1370 at 518 px; aaclip_attention_bwd holds a whole sequence in LDS and
 * stops at 77). qkv [batch*seq, 3*heads*64] is the packed input the forward consumed, out
 * [batch*seq, heads*64] the forward's output, dout its gradient; dqkv (packed [dq|dk|dv], every
 * element written) must not alias an input. head_dim == 64, seq >= 1, batch*heads <= 65535.
 * On v_mfma_f32_16x16x4_f32 with 64-row tiles in padded LDS, two launches:
 *   query blocks (image, head, 64 queries): pass 1 over the key tiles gives the row
 *     log-sum-exp, D_i = dout_i . out_i comes from the saved output (both stored in workspace,
 *     [batch, heads, seq] each); pass 2 forms P = exp(S - lse), dP = dout v^T,
 *     dS = P (dP - D), dq = dS k / 8;
 *   key blocks (image, head, 64 keys): walk the query tiles in index order with the stored lse
 *     and D: dv = P^T dout, dk = dS^T q / 8.
 * Each output row is summed by one wave in a fixed order; keys / queries past the end of a
 * ragged tile contribute exactly 0 and are never stored. At seq == 1: dq = dk = 0, dv = dout.
 * workspace: aaclip_attention_bwd_tiled_workspace bytes (2 * batch * heads * seq floats),
 * 16-byte aligned, as are the other operands.
 * Replaces: the autograd of F.multi_head_attention_forward's core (model/transformer.py:200)
 * under model/adapter.py:90-91, train.py:156.
 */
int aaclip_attention_bwd_tiled_workspace(int batch, int seq, int heads, size_t* bytes);
int aaclip_attention_bwd_tiled(const float* qkv, const float* out, const float* dout, float* dqkv, int batch,
                               int seq, int heads, int head_dim, float* workspace, size_t workspace_bytes,
                               void* stream);

/*
 * Backward of aaclip_block_tail's level tap (tap[b, t - 1] = ln_post(x[b, t]), t >= 1): token row
 * (b, t >= 1) of g [batch*n_tok, width] += LN_bwd(dtap[b*(n_tok-1) + t - 1]; x[b*n_tok + t], w)
 * with aaclip_layernorm_bwd's arithmetic and w = ln_post's weight; CLS rows (t == 0) of g are
 * not touched. x is the residual stream the tap read. g must not alias x or dtap. width 768 or
 * 1024, n_tok >= 2.
 * Replaces: the autograd of model/adapter.py:100-105 under train.py:156.
 */
int aaclip_tap_ln_bwd(const float* dtap, const float* x, const float* w, float* g, int batch, int n_tok, int width,
                      void* stream);

/*
 * Backward of aaclip_l2_normalize, y = x / max(|x|, 1e-12) (F.normalize), one wave per row, |x|
 * summed in the forward's order. The incoming gradient of row r is gy = scale * dy[r / dy_group]
 * (dy_group == 0: dy[r]), so det = mean_p normalize(d_p) is one launch with dy = ddet [B, width],
 * dy_group = P, scale = 1 / P. dx = (gy - y (y . gy)) / |x|; a row with |x| <= 1e-12 (the clamp
 * branch, e.g. all zeros) gets gy / 1e-12. dx may be dy when dy_group == 0 (same leading
 * dimension), never x. width 768 or 1024; ld* >= width, multiples of 4.
 * Replaces: the autograd of model/adapter.py:109 and :111 under train.py:156.
 */
int aaclip_l2_normalize_bwd(const float* dy, int64_t lddy, int dy_group, float scale, const float* x, int64_t ldx,
                            float* dx, int64_t lddx, int rows, int width, void* stream);

/* ------------------------------------------------------------------ stage-2 backward, bf16
 * The kernels of the bf16 mixed-precision stage-2 step (attention_bwd.hip's bf16
 * instantiation, visual_bwd16.hip). The residual and
 * gradient streams, the LayerNorm / blend / normalise backwards and the weight gradients stay
 * the fp32 entries above; every GEMM is aaclip_gemm in bf16 on the transposed packed weights.
 *
 * aaclip_attention_bwd16: aaclip_attention_bwd_tiled on bf16 operands (dtype must be
 * AACLIP_BF16) and v_mfma_f32_16x16x32_bf16: packed bf16 qkv, the forward's bf16 out and bf16
 * dout in, bf16 dqkv out; fp32 softmax statistics and accumulation. Same two launches, so
 * deterministic, atomics-free and image local; P and dS = P (dP - D) (from the fp32 P) are
 * rounded to bf16 before their second product. flags: 0 or AACLIP_ATTN_Q_PRESCALED (the q
 * columns carry log2(e) / sqrt(64), as aaclip_attention): the q columns of dqkv are then the
 * gradient of the PRESCALED q, what a GEMM on the prescaled in-projection weights expects;
 * without it q is scaled and rounded to bf16 at load, as aaclip_attention does. dk and dv
 * are the same either way. Non-causal, head_dim 64, any seq >= 1; at seq == 1 dq = dk = 0 and
 * dv = dout. dqkv must not alias an input; workspace: aaclip_attention_bwd16_workspace bytes
 * (2 * batch * heads * seq floats); all operands 16-byte aligned.
 * Replaces: the autograd of F.multi_head_attention_forward's core under train.py:156.
 */
int aaclip_attention_bwd16_workspace(int batch, int seq, int heads, size_t* bytes);
int aaclip_attention_bwd16(int dtype, const void* qkv, const void* out, const void* dout, void* dqkv, int batch,
                           int seq, int heads, int head_dim, int flags, float* workspace, size_t workspace_bytes,
                           void* stream);

/*
 * y = (out_dtype) f(x) on n fp32 values, f = the 16-bit GEMM epilogue's own activation of
 * mode AACLIP_EPI_GELU / _QGELU / _LEAKY and its own rounding: a bias-only GEMM with fp32
 * output followed by this launch gives the bits of the fused 16-bit epilogue and keeps the
 * pre-activation. out_dtype AACLIP_BF16 or AACLIP_F16; x and y 16-byte aligned, distinct.
 */
int aaclip_act_to16(int mode, const float* x, void* y, int out_dtype, int64_t n, void* stream);

/*
 * aaclip_act_bwd with 16-bit dy and dx (dtype AACLIP_BF16 or AACLIP_F16; dx may be dy) and
 * the fp32 reference value: dx = round(dy * f'(ref)), the derivative evaluated in fp32.
 */
int aaclip_act_bwd16(int mode, const void* dy, const float* ref, void* dx, int dtype, int64_t n, void* stream);

/*
 * y[r][c] = (out_dtype) x[r][c] for rows x cols elements: fp32 -> bf16 / fp16 (round to nearest
 * even, the GEMM epilogue's conversion) or bf16 / fp16 -> fp32 (exact). cols a multiple of 8;
 * ldx, ldy >= cols in elements with 16-byte aligned rows on both sides; x != y.
 */
int aaclip_cast_rows(int in_dtype, int out_dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int rows,
                     int cols, void* stream);

/*
 * Full test-branch anomaly map for one batch: patch_scores (mode 0) into the
 * caller's workspace grid_ws (>= batch*g*g fp32), then blur + upsample into
 * out [batch, S, S]. Replaces: test.py:86-93 + forward_utils.py:196-213.
 */
int aaclip_anomaly_map(int in_dtype, const void* const* levels, int n_levels, int64_t ld,
                       const float* T, int batch, int g, int channels, int normalize,
                       int out_size, int ksize, float sigma, float* grid_ws, float* out,
                       void* stream);

/*
 * The predict path's map + image score from aaclip_gemm_scores partials (the level
 * projections are never written as rows): part [batch*g*g][ld_part] fp32 holds, per
 * patch row, n_levels levels (+ the det projection when with_det) of 24 float4
 * partials {||v||^2, v.t0, v.t1, 0} (one per 32 columns of the 768). Stage 1 sums each
 * level's 24 partials in a fixed order, normalises and forms the level-summed test
 * score grid (as aaclip_patch_scores, normalize = 1) into grid_ws (>= batch*g*g) and,
 * with_det, normalize(d).t1 per row into det_ws (>= batch*g*g); stage 2 is
 * aaclip_blur_upsample (out [batch, S, S]) plus score[b] = (mean_p det_ws + 1) / 2.
 * Every argument is checked before the first launch.
 * Replaces: test.py:83-93 + forward_utils.py:196-213 after the projections.
 */
int aaclip_anomaly_map_partials(const float* part, int64_t ld_part, int n_levels, int with_det,
                                int batch, int g, int out_size, int ksize, float sigma,
                                float* grid_ws, float* det_ws, float* out, float* score,
                                void* stream);

/*
 * Image-level score: det[b] = mean_p normalize(det_raw[b*n_patch+p]) and
 * score[b] = (det[b] . T[:,1] + 1) / 2. partial: workspace
 * [batch, ceil(n_patch/16), channels] fp32 (fixed-order reduction, deterministic).
 * Replaces: model/adapter.py:110-111 + test.py:83-84.
 */
int aaclip_image_score(int in_dtype, const void* det_raw, int64_t ld, const float* T,
                       int batch, int n_patch, int channels, int normalize, float* partial,
                       float* det, float* score, void* stream);

/*
 * Device metrics_eval for one class (replaces forward_utils.py:233-280 + the
 * sklearn roc_auc_score / average_precision_score it calls): class-global
 * min-max normalisation of the maps (skipped when max == 1) and of the image
 * scores, image score fusion (0.5 * pixel max + 0.5 * score, or pixel max when
 * medical != 0), then exact tie-aware AUROC and AP for pixels and images.
 * pixel_preds [n_images, pix_per_image] fp32, pixel_label [same] uint8 (nonzero =
 * anomalous), image_preds [n_images] fp32, image_label [n_images] uint8.
 * out: device double[4] = pixel AUROC, pixel AP, image AUROC, image AP (unrounded;
 * the image pair is 0, 0 when all image labels are equal, as in the reference;
 * the pixel pair is NaN when all pixel labels are equal, where sklearn raises).
 * workspace: caller-owned device memory, 256-B aligned, of the size
 * aaclip_metrics_workspace reports (about 24 bytes per pixel). Deterministic.
 */
int aaclip_metrics_workspace(int64_t n_pixels, int n_images, size_t* bytes);
int aaclip_metrics_eval(const float* pixel_preds, const uint8_t* pixel_label, const float* image_preds,
                        const uint8_t* image_label, int n_images, int64_t pix_per_image, int medical,
                        void* workspace, size_t workspace_bytes, double* out, void* stream);

/*
 * 8-connected components of binary masks, per image (the regions of the per-region-overlap
 * metric below; the reference has no counterpart: MVTec AD's evaluation code labels them on
 * the host). mask [n_images, height, width] uint8, foreground = nonzero. labels [same] uint32:
 * 0 for background, 1 + the smallest linear index y * width + x of the pixel's component within
 * its image otherwise (canonical: independent of scheduling). areas [same] uint32: the pixel's
 * component's area, 0 for background. n_components [n_images] uint32. Pixels never connect
 * across the row end or between images. Union-find in global memory with atomicMin links; no
 * loop waits for another wave, and every data-dependent loop is capped at height * width trips
 * (a hit, which only a bug can cause, reports n_components = 0xFFFFFFFF for that image).
 * Allocates nothing, does not sync. Needs height * width < 2^31 and
 * n_images * height * width < 2^32 - 1. Deterministic.
 */
int aaclip_label_components(const uint8_t* mask, int n_images, int height, int width, uint32_t* labels,
                            uint32_t* areas, uint32_t* n_components, void* stream);

/*
 * aaclip_metrics_eval plus the pixel AUPRO (the localisation metric of MVTec AD / VisA).
 * out5[0..3]: what aaclip_metrics_eval gives on the same inputs, bit for bit (forward_utils.py:233-280;
 * same keys, kernels and reduction order). out5[4]: with the class-normalised fp32 scores s, the
 * 8-connected components r of pixel_label != 0 per image (R of them, areas |r|) and the N_ok pixels
 * of label 0 of every image,
 *   FPR(t) = #{ok pixels with s >= t} / N_ok,   PRO(t) = (1/R) sum_r #{p in r : s_p >= t} / |r|;
 * the curve runs from (0, 0) through one point per distinct score in descending order to (1, 1),
 * piecewise linear, and AUPRO = (1 / fpr_limit) * integral of PRO over FPR in [0, fpr_limit] (linear
 * interpolation at the limit), exact at every distinct threshold, ties included. NaN when R == 0 or
 * N_ok == 0. fpr_limit in (0, 1]; MVTec AD uses 0.3. pixel_preds / pixel_label [n_images, height,
 * width]. workspace: caller-owned device memory, 256-B aligned, of the size
 * aaclip_metrics_pro_workspace reports (about 32 bytes per pixel). No floating-point atomics or
 * scans: fixed-order fp64 sums, the same bits on every launch.
 */
int aaclip_metrics_pro_workspace(int64_t n_pixels, int n_images, size_t* bytes);
int aaclip_metrics_eval_pro(const float* pixel_preds, const uint8_t* pixel_label, const float* image_preds,
                            const uint8_t* image_label, int n_images, int height, int width, int medical,
                            double fpr_limit, void* workspace, size_t workspace_bytes, double* out5, void* stream);

/*
 * aaclip_metrics_eval plus F1-max and the score at which it is reached, for pixels and for images
 * (the column WinCLIP, APRIL-GAN / VAND and AdaCLIP report; the reference, forward_utils.py:233-280,
 * has no counterpart). out13[0..3]: what aaclip_metrics_eval gives on the same inputs, bit for bit.
 * out13[4]: the AUPRO of aaclip_metrics_eval_pro when with_pro != 0, else NaN (no component labelling
 * runs then, fpr_limit is ignored and only height * width matters). out13[5..8]: pixel F1-max, its
 * threshold, and the precision and recall there. out13[9..12]: the same four numbers for images.
 * With v the class-normalised fp32 map value that the sort keys are built from ((x - min) / (max - min)
 * when the class maximum is not 1, else x), y the label (!= 0), n the pixel count and P the positives,
 * every distinct score t has
 *   PP(t) = #{v >= t},   TP(t) = #{y = 1, v >= t},   F1(t) = (double)(2 TP) / (double)(PP + P):
 * two exact integers and one IEEE fp64 division. F1-max is the maximum over t; the threshold is the
 * LOWEST t whose F1 equals it (thresholds[argmax] on sklearn's ascending precision_recall_curve
 * thresholds, as the VAND code takes it), returned as the fp32 value widened to double; precision is
 * TP / PP and recall TP / P at that t, one fp64 division each. Images: the same over the fused fp32
 * image scores (the normalised row maximum when medical != 0, else 0.5 * that + 0.5 * the normalised
 * image score) and image_label. Thresholds are therefore in the normalised score domains, not in the
 * domain of the inputs. The pixel numbers are NaN when all pixel labels are equal (where out13[0] is
 * NaN); the image numbers are 0 when all image labels are equal (as out13[2..3]). One more pass over
 * the sorted positions and one O(n_images^2) kernel: no second sort, no atomics, fixed-order
 * reductions with ties to the lower score, the same bits on every launch. workspace: caller-owned
 * device memory, 256-B aligned, of the size aaclip_metrics_f1_workspace reports for the same with_pro.
 * Needs height * width < 2^31 and n_images * height * width < 2^32 - 1; fpr_limit in (0, 1] when
 * with_pro != 0.
 */
int aaclip_metrics_f1_workspace(int64_t n_pixels, int n_images, int with_pro, size_t* bytes);
int aaclip_metrics_eval_f1(const float* pixel_preds, const uint8_t* pixel_label, const float* image_preds,
                           const uint8_t* image_label, int n_images, int height, int width, int medical,
                           int with_pro, double fpr_limit, void* workspace, size_t workspace_bytes, double* out13,
                           void* stream);

/*
 * The defect regions of one class's anomaly maps: the 8-connected components of the pixels whose
 * score reaches a threshold, each with where it is, how large and how strong (what an inspection
 * user does with the F1-max threshold of aaclip_metrics_eval_f1; the reference has no counterpart:
 * its visualize() paints overlays with cv2).
 * pixel_preds [n_images, height, width] fp32; pixel_label [same] uint8 (nonzero = anomalous) or NULL.
 * Score v of a pixel: with normalise != 0 the class-normalised fp32 value of the metrics, bit for bit
 * (lo / hi the fp32 min / max over all n_images maps; v = (x - lo) / (hi - lo) when hi != 1, else x:
 * one shared formula, csrc/scorenorm.h), so that threshold may be out13[6] as it stands; with
 * normalise == 0 v = x (serving: a raw threshold on the maps of VisualEngine.predict).
 * A pixel is foreground when v >= threshold (the detection rule of the F1 kernels); a NaN v is
 * background, so a constant class, which normalises to 0 / 0, has no region. Regions are the
 * 8-connected components of the foreground per image, labelled by aaclip_label_components.
 * Regions of area < min_area (>= 1) are dropped. n_regions [n_images] uint32: the regions that are
 * left, which may exceed max_regions (>= 1); 0xFFFFFFFF where the labelling hit a cap (then the
 * image's slots are zero). Every other output is [n_images, max_regions] slots; the first
 * min(n_regions, max_regions) slots of an image hold its regions by area descending, ties by label
 * ascending, the rest are zero:
 *   labels        uint32  1 + the smallest linear index y * width + x of the region
 *   areas         uint32  pixels
 *   bboxes        uint32  [.., 4] = x0, y0, x1, y1, inclusive
 *   centroids     double  [.., 2] = (double)sum x / (double)area, (double)sum y / (double)area: exact
 *                         64-bit integer sums, one IEEE fp64 division each
 *   peaks         float   the maximum v (a zero peak is +0)
 *   peak_indices  uint32  the smallest linear index whose v is the peak
 *   gt_areas      uint32  the region's pixels with pixel_label != 0 (0 with a NULL pixel_label)
 * workspace: caller-owned device memory, 256-B aligned, of the size aaclip_regions_workspace reports
 * for n_pixels = n_images * height * width (about 49 bytes per pixel: the labelling arrays and, for
 * up to a component per two pixels, the per-region sums and sort buffers). Allocates nothing, does
 * not sync. Integer atomics (min / max / add on 32- and 64-bit words; the peak and its index are one
 * 64-bit max) and one radix sort: no floating-point atomics, the same bits on every launch. No loop
 * depends on data beyond those of aaclip_label_components, which are capped. Needs
 * height * width < 2^31, n_images * height * width < 2^32 - 1 and n_images * max_regions < 2^31.
 */
int aaclip_regions_workspace(int64_t n_pixels, int n_images, size_t* bytes);
int aaclip_extract_regions(const float* pixel_preds, const uint8_t* pixel_label, int n_images, int height, int width,
                           float threshold, int normalise, int min_area, int max_regions, void* workspace,
                           size_t workspace_bytes, uint32_t* n_regions, uint32_t* labels, uint32_t* areas,
                           uint32_t* bboxes, double* centroids, float* peaks, uint32_t* peak_indices,
                           uint32_t* gt_areas, void* stream);

/*
 * Anomaly overlays (csrc/overlay.hip; replaces forward_utils.py:283-327, visualize() and
 * apply_ad_scoremap(), which paint them with cv2 on the host). For one class: n maps fp32 [S, S],
 * n labels [S, S], n photos resized to [S, S, 3] -> n images uint8 [3 S, S, 3], three panels stacked
 * top to bottom: the photo, the ground truth over it, the prediction over it. Integer and fp32
 * arithmetic with one stated result, restated in numpy by tests/visualize_ref.py, which the device
 * equals byte for byte. cv2 itself is on no machine this was built on: the recipe is modelled on
 * OpenCV's, and equality with an OpenCV build's bytes is not claimed.
 *
 * aaclip_bilinear_plan (host only; the table of cv2.resize's INTER_LINEAR 8-bit path, :312): for
 * every output coordinate d of one axis table[3 d ..] = (s, a0, a1). With scale = in / out in double:
 *   f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s;
 *   s < 0: s = 0, f = 0;   s >= in - 1: s = in - 1, f = 0;
 *   a1 = rint(f * 2048), a0 = rint((1 - f) * 2048), both in fp32 (a0 + a1 = 2048).
 *
 * aaclip_resize_bilinear_u8: src batch uint8 RGB [in_h, in_w, 3] (row pitch / image stride in
 * bytes), x_table / y_table device copies of the plans of (in_w, S) / (in_h, S), out uint8
 * [batch, S, S, 3]. With the neighbour index min(s + 1, in - 1), per channel in int:
 *   r(row) = src[row][sx] * a0 + src[row][sx + 1] * a1                       (horizontal)
 *   dst = (((b0 * (r(sy) >> 4)) >> 16) + ((b1 * (r(sy + 1) >> 4)) >> 16) + 2) >> 2   (vertical)
 * in == out is the identity. A table index outside the source is clamped into it. Needs
 * batch * S * S < 2^31 - 4.
 *
 * aaclip_overlay_range (:296-299): range[0] = lo, range[1] = hi, the fp32 min / max over the
 * class's maps [n_images, pix_per_image] (NaNs are skipped, as fminf / fmaxf do), into a device
 * float[2]. workspace: caller-owned device memory of aaclip_overlay_workspace bytes (the partial
 * minima and maxima: an image is reduced in up to 64 equal parts). Min / max only and no atomics:
 * the same bits on every launch. Needs n_images <= 2^24.
 *
 * aaclip_overlay_panels (:296-303, :283-285, :321-326): maps fp32 [batch, S, S]; labels uint8
 * [batch, S, S] or NULL (all zero); thumbs uint8 [batch, S, S, 3] RGB (aaclip_resize_bilinear_u8);
 * range a device float[2] or NULL (no normalisation); out uint8 [batch, 3 S, S, 3].
 *   q  v = the class-normalised score of csrc/scorenorm.h: (x - lo) / (hi - lo) when hi != 1, else
 *      x (also with a NULL range); q = (uint8)trunc(v * 255.0f) in fp32, numpy's
 *      (pixel_preds * 255).astype(np.uint8). Defined here where the reference is not: a non-finite
 *      v (a constant class is 0 / 0) gives q = 0, and a finite v outside [0, 1] (hi == 1, where
 *      the reference hands floats to cv2) is clamped to 0..255 after the truncation.
 *   L  255 where the label != 0, else 0.
 *   JET(u), u in 0..255, RGB: r = clip(383 - |4 u - 765|, 0, 255), g the same around 510, b around
 *      255: JET(0) = (0, 0, 128), JET(255) = (128, 0, 0).
 *   P  the photo with red and blue exchanged when swap_rb != 0, else the photo. The reference
 *      blends an RGB photo with applyColorMap's BGR ramp and writes the sum as BGR, so on disk its
 *      photo has red and blue swapped and the ramp has its true colours: swap_rb = 1 is that.
 *   panel 0 = P, panel 1 = (P + JET(L)) >> 1, panel 2 = (P + JET(q)) >> 1 per channel in int,
 *   which is (0.5 * a + 0.5 * b).astype(uint8) exactly; out is in file (true RGB) channel order.
 * One pass, each input read once, 16-byte stores except at the ends of a block's runs.
 * Needs batch <= 65535 and S <= 16384.
 *
 * All of them allocate nothing, do not sync and return AACLIP_ERR_ARG for NULL or non-positive
 * arguments.
 */
int aaclip_bilinear_plan(int in_size, int out_size, int32_t* table);
int aaclip_resize_bilinear_u8(const uint8_t* src, int64_t img_stride, int64_t row_pitch, int batch, int in_h,
                              int in_w, const int32_t* x_table, const int32_t* y_table, int out_size, uint8_t* out,
                              void* stream);
int aaclip_overlay_workspace(int n_images, size_t* bytes);
int aaclip_overlay_range(const float* maps, int n_images, int64_t pix_per_image, void* workspace,
                         size_t workspace_bytes, float* range, void* stream);
int aaclip_overlay_panels(const float* maps, const uint8_t* labels, const uint8_t* thumbs, const float* range,
                          int batch, int size, int swap_rb, uint8_t* out, void* stream);

/*
 * Tiled high-resolution inference (csrc/tiles.hip); no reference counterpart: the reference has
 * one input shape, the whole photo resized to img_size squared. A C x C canvas is cut into G x G
 * overlapping S x S tiles, every tile goes through the tower at the native scale, the tile maps
 * are stitched back onto the canvas and may be mixed with the map of a global view (the whole
 * photo at S x S). tests/tiled_ref.py states all of it in numpy float64.
 *
 * Geometry: tile side S, G tiles per axis (2 <= G <= 8), overlap O pixels (0 <= O <= S / 2),
 * canvas side C = G S - (G - 1) O. Tile (ty, tx) has origin (ty (S - O), tx (S - O)) and index
 * t = ty G + tx; the tiles of image b are rows b G^2 + t, image-major. With O <= S / 2 at most two
 * tiles cover a canvas coordinate per axis. The 1-D blend weight of tile i at local coordinate u is
 * (u + 0.5) / O for u < O when i > 0, (S - u - 0.5) / O for u >= S - O when i < G - 1 and 1
 * elsewhere (the canvas borders get 1); in an overlap the two ramps sum to 1 in real arithmetic, so
 * nothing is divided by a weight sum. A pixel's weight is the product of its two 1-D weights.
 * The global view's map is upsampled to C x C bilinearly with half-pixel centres and a clamp at 0
 * (F.interpolate(mode="bilinear", align_corners=False)): per axis i0 = floor(((2 x + 1) S - C) /
 * (2 C)), clamped at 0, lambda = the remainder over 2 C (0 where clamped), i1 = min(i0 + 1, S - 1).
 *
 * aaclip_tile_plan (host only, no device work): the per-axis tables of one (S, G, O); the canvas and
 * the grid are square, so the same tables serve rows and columns. index int32 [C, 2] = (first
 * covering tile, i0); weight fp32 [C, 4] = (that tile's weight, the next tile's or 0 where one tile
 * covers, 1 - lambda, lambda). Everything comes from integer arithmetic, each weight computed in
 * double and rounded once to fp32.
 *
 * aaclip_tile_gather: tiles[k] = canvas[b, :, oy : oy + S, ox : ox + S] for the tile rows
 * tile0 + k = b G^2 + t, k in [0, n_tiles): a pure copy of fp32 values. canvas fp32
 * [n_images, 3, C, C], tiles fp32 [n_tiles, 3, S, S], both contiguous; any run of tile rows inside
 * [0, n_images G^2), so a caller can gather a chunk of images, or of tiles, at a time. Needs
 * 3 n_images G^2 < 2^31.
 *
 * aaclip_tile_stitch: with a = global_weight in [0, 1), both coefficients fp32 (1 - a rounded once),
 *   out[b, y, x] = (1 - a) * sum over the covering tiles, ty then tx, of
 *                      (wy * wx) * tile_maps[b G^2 + t, y - oy, x - ox]
 *                  + a * (((ly0 * lx0) * g[iy0, ix0] + (ly0 * lx1) * g[iy0, ix1])
 *                         + (ly1 * lx0) * g[iy1, ix0]) + (ly1 * lx1) * g[iy1, ix1]),  g = global_maps[b]
 * every product and sum one rounded fp32 operation in that order (no FMA contraction); a tile that
 * does not cover the pixel contributes no term. With a == 0 the result is the tile sum itself and
 * global_maps is not read (it may be NULL). tile_maps fp32 [batch G^2, S, S], global_maps fp32
 * [batch, S, S], index / weight device copies of the plan's tables (weight 16-byte aligned), out
 * fp32 [batch, C, C]. One writer per output pixel, no atomics: the same bits on every launch.
 * Offsets are 64-bit; needs batch C < 2^31. Table indices are clamped to what exists.
 *
 * aaclip_tile_score: out[b] = (1 - a) * max over t of tile_scores[b G^2 + t] + a * global_scores[b],
 * fp32; with a == 0 the maximum itself, global_scores not read (may be NULL).
 *
 * All of them return AACLIP_ERR_ARG, before any launch, for NULL pointers, non-positive sizes, G
 * outside [2, 8], O outside [0, S / 2], a tile range outside the canvas batch, a global weight
 * outside [0, 1) or misaligned operands; the device entries allocate nothing and do not sync.
 */
int aaclip_tile_plan(int S, int G, int O, int32_t* index, float* weight);
int aaclip_tile_gather(const float* canvas, int n_images, int S, int G, int O, int64_t tile0, int64_t n_tiles,
                       float* tiles, void* stream);
int aaclip_tile_stitch(const float* tile_maps, const float* global_maps, const int32_t* index, const float* weight,
                       int batch, int S, int G, int O, float global_weight, float* out, void* stream);
int aaclip_tile_score(const float* tile_scores, const float* global_scores, int batch, int G, float global_weight,
                      float* out, void* stream);

/*
 * Few-shot memory-bank scoring (csrc/bank.hip). Replaces what the reference carries for it and
 * wires to nothing: test.py:39-50 get_support_features (the bank: the level features of a few
 * normal support images, concatenated per level) and utils.py:86-93 cos_sim (the patch x bank
 * similarity matrix). A test patch's few-shot score at a level is 1 - its largest cosine with any
 * bank patch; the matrix itself is never written.
 *
 * aaclip_bank_nn: part[m][s] = max over the bank rows n of split s of Q[m,:] . R[n,:] in fp32.
 * Q [M, K] with row stride ldq, R [Nb, K] with row stride ldr (strides in elements), both of
 * `dtype`: AACLIP_F16 (v_mfma_f32_16x16x32_f16), AACLIP_BF16 (the same kernel on the bf16 MFMA) or
 * AACLIP_F32 (v_mfma_f32_16x16x4_f32). M >= 1 and Nb >= 1 are arbitrary, K % 64 == 0; Q and R 16-byte
 * aligned with 16-byte aligned row strides >= K. The bank's tiles of AACLIP_BANK_TILE_N rows are dealt
 * to n_splits splits, split s owning tiles [s * tps, (s + 1) * tps), tps = ceil(tiles / n_splits); a
 * block takes one tile of AACLIP_BANK_TILE_M query rows and one split. part: caller-owned device
 * fp32 [M][n_splits]; aaclip_bank_nn_workspace (host only, a function of M and Nb alone) gives its
 * bytes and n_splits: of the even splits into at most AACLIP_BANK_MAX_SPLITS parts, none empty, the
 * one whose row tiles x splits blocks take the fewest rounds x tiles at
 * AACLIP_BANK_RESIDENT_BLOCKS blocks on the chip at once (csrc/bank.hip, bank_plan). Ragged tiles read the last row again
 * instead of padding (a duplicate cannot move a maximum; a zero row could). Inputs must be finite.
 * Every dot product sums K in one order wherever its row and column sit in a tile or split, so a
 * query row's result has the same bits alone or in a batch, under any permutation of the bank rows
 * and on every launch. No atomics.
 *
 * aaclip_bank_distance: grid[m] = (accumulate ? grid[m] : 0) + (1 - max_s part[m][s]), the splits
 * read in order, fp32. Row m = b * P + p is element [b][0][p] of the [B, 1, g, g] grid that
 * aaclip_blur_upsample takes; called once per level, accumulate != 0 from the second on (the level
 * sum is taken ahead of the blur, as in the zero-shot path). No clamp: a self-match may give a
 * distance a hair below 0.
 *
 * aaclip_fewshot_fuse: one class's zero-shot and few-shot results into the pair the metrics take.
 * zs_map, fs_map fp32 [n_images, pix_per_image], zs_score fp32 [n_images]. With
 * N(x; lo, hi) = (x - lo) / (hi - lo), and 0 where hi == lo (a constant input contributes 0, not NaN):
 *   fs_score[b]    = max over the pixels of fs_map[b]
 *   fused_map[i]   = N(zs_map[i]; zs_map's range) + N(fs_map[i]; fs_map's range)
 *   fused_score[b] = N(zs_score[b]; zs_score's range) + N(fs_score[b]; fs_score's range)
 * each range the class's (lo, hi) from aaclip_overlay_range (for the scores with pix_per_image = 1),
 * every operation one rounded fp32 operation: numpy float32 gives the same bits
 * (tests/fewshot_ref.py). workspace: 16-byte aligned caller-owned device memory of
 * AACLIP_FEWSHOT_FUSE_HEAD + aaclip_overlay_workspace(n_images) bytes. Outputs must not overlap
 * inputs. Inputs must be finite. Needs n_images <= 2^24.
 *
 * All of them return AACLIP_ERR_ARG, before any launch, for NULL pointers, non-positive sizes, a
 * dtype outside the three, K % 64 != 0, a stride below K or not 16-byte aligned, misaligned
 * operands or a short workspace; they allocate nothing and do not sync.
 */
#define AACLIP_BANK_TILE_M 256
#define AACLIP_BANK_TILE_N 256
#define AACLIP_BANK_RESIDENT_BLOCKS 256
#define AACLIP_BANK_MAX_SPLITS 64
#define AACLIP_FEWSHOT_FUSE_HEAD 256
int aaclip_bank_nn_workspace(int M, int Nb, size_t* bytes, int* n_splits);
int aaclip_bank_nn(int dtype, int M, int Nb, int K, const void* Q, int64_t ldq, const void* R, int64_t ldr,
                   float* part, size_t part_bytes, void* stream);
int aaclip_bank_distance(const float* part, int M, int n_splits, int accumulate, float* grid, void* stream);

/*
 * The same search on MX fp8 operands (csrc/mxfp8.h: e4m3 bytes, one e8m0 scale byte e + 127 per
 * 64 columns of a row, scale buffer [cols / 128][ld][2]); opt-in, replacing the same reference
 * lines (test.py:39-50, utils.py:86-93). It returns the exact cosine between the two fp8
 * representations: quantised unit rows are no longer unit (norms about 1 +- 6e-3), so each side
 * carries the reciprocal norm of what it stored.
 *
 * aaclip_unit_rows_fp8mx: per row of x [rows, cols] (`in_dtype` AACLIP_F32 / _BF16 / _F16, row
 * stride ldx elements): y = x / max(|x|, 1e-12), |x| summed as aaclip_l2_normalize sums it; q =
 * y in MX e4m3 (RNE) with row stride ldq bytes, scales into sc [cols / 128][ld_sc][2], ld_sc >=
 * rows and even; rnorm[r] = 1 / sqrt(sum_c deq[r, c]^2) in fp32, deq = e4m3 * 2^e the values the
 * search reads (the squares are exact, the root and the reciprocal correctly rounded, so a
 * power-of-two norm gives that power of two), and 0 for a row that stores all zeros. cols is any
 * multiple of 128; x and q 16-byte aligned with 16-byte aligned row strides >= cols, sc and rnorm
 * 4-byte aligned. rows == 0 is a no-op.
 *
 * aaclip_bank_nn_fp8mx: part[m][s] = max over the bank rows n of split s of
 * (Q^[m] . R^[n]) * r_rnorm[n] * q_rnorm[m], Q^ / R^ the dequantised rows; the dot product on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with both block scales applied by the instruction, fp32
 * accumulation over K-steps of 128 ascending. Q [M, K], R [Nb, K] e4m3 bytes (strides in bytes),
 * q_sc / r_sc their scale buffers with row counts ld_qsc >= M, ld_rsc >= Nb, both even; q_rnorm
 * [M], r_rnorm [Nb] fp32 (aaclip_unit_rows_fp8mx writes all three). K % 128 == 0. The tiles, the
 * split plan (aaclip_bank_nn_workspace), `part`, the clamped ragged edges and the same-bits
 * properties are aaclip_bank_nn's; part holds cosines, so aaclip_bank_distance takes it as it
 * is. A bank row with r_rnorm 0 scores 0. Scales must not be 255 (NaN); values finite.
 * Q and R 16-byte aligned, the rest 4-byte; row strides multiples of 16.
 *
 * Both return AACLIP_ERR_ARG before any launch for NULL pointers, M or Nb < 1, a width that is
 * no multiple of 128, an odd or short ld_sc, short or misaligned strides or a short `part`.
 */
int aaclip_unit_rows_fp8mx(int in_dtype, const void* x, int64_t ldx, void* q, int64_t ldq, void* sc, int64_t ld_sc,
                           float* rnorm, int rows, int cols, void* stream);
int aaclip_bank_nn_fp8mx(int M, int Nb, int K, const void* Q, int64_t ldq, const void* q_sc, int64_t ld_qsc,
                         const float* q_rnorm, const void* R, int64_t ldr, const void* r_sc, int64_t ld_rsc,
                         const float* r_rnorm, float* part, size_t part_bytes, void* stream);
int aaclip_fewshot_fuse(const float* zs_map, const float* fs_map, const float* zs_score, int n_images,
                        int64_t pix_per_image, void* workspace, size_t workspace_bytes, float* fused_map,
                        float* fs_score, float* fused_score, void* stream);

/*
 * Greedy k-centre coreset of a memory bank (csrc/bank.hip): the subsampling that memory-bank
 * detectors of the PatchCore family apply to their bank; the reference has nothing of the kind.
 * Farthest-point selection under the distance 1 - cosine on rows taken as given (normalising
 * them is the caller's job, as for aaclip_bank_nn); tests/coreset_ref.py states it in float64:
 *
 *   maxsim = -inf everywhere; sel[0] = start; cover[0] = -inf
 *   for t in 0 .. m-1:
 *     c = sel[t]; c is taken
 *     maxsim[n] = max(maxsim[n], R[n,:] . R[c,:])        every row, taken ones included
 *     if t < m-1: sel[t+1] = the lowest index attaining the minimum of maxsim over the rows not
 *                 taken; cover[t+1] = that minimum
 *
 * aaclip_bank_coreset: R [N, K] of `dtype` AACLIP_F16, AACLIP_BF16 or AACLIP_F32 with row stride
 * ldr in elements; K % 64 == 0 and K <= AACLIP_CORESET_MAX_K (the centre row is staged in LDS as
 * fp32); R 16-byte aligned with a 16-byte aligned row stride >= K; 1 <= m <= N <= 2^30,
 * 0 <= start < N. Outputs: sel int32 [m], cover fp32 [m], maxsim fp32 [N] (after the last pick;
 * its minimum is the smallest cosine between any row and its nearest selected row), 4-byte
 * aligned. workspace: 16-byte aligned caller-owned device memory of aaclip_bank_coreset_workspace(N)
 * bytes (host only): two buffers of AACLIP_CORESET_MAX_BLOCKS (value, index) candidates, then a
 * taken byte per row; it needs no initialisation. Inputs must be finite.
 *
 * The call enqueues m launches of one step kernel on `stream`, nothing else: no host
 * synchronisation, no allocation, no atomics, no cooperative launch, no grid-wide wait. Step t:
 * every block reduces step t-1's per-block candidates to the (value, index) minimum, the lowest
 * index on ties (redundantly: blocks^2 x 8 bytes of L2 reads per step, which is what
 * AACLIP_CORESET_MAX_BLOCKS caps), block 0 stores sel[t] and cover[t]; the block stages the centre
 * row in LDS, streams its own rows once with 16-byte loads, updates maxsim, marks the centre as
 * taken and writes its own candidate into the buffer of t's parity (step t-1's is still being read
 * by other blocks). The rows are cut into slabs of AACLIP_CORESET_BLOCK_ROWS; the launch has
 * ceil(slabs / ceil(slabs / AACLIP_CORESET_MAX_BLOCKS)) blocks and block b owns slabs b, b + blocks,
 * ...: a function of N alone and the same in every step, so a row has one owner (no race on
 * maxsim or the taken bytes) and L2 and the Infinity Cache can serve its bytes again.
 *
 * Accumulation is fp32 and the summation order of a dot product is a function of K and the dtype
 * alone: the row's 16-byte chunks (8 16-bit or 4 fp32 elements) are dealt to 16 lanes, lane l
 * taking chunks l, l + 16, ...; a lane starts from +0 and adds product after product with one
 * fused multiply-add each, its chunks ascending and the elements of a chunk ascending; the 16
 * lane sums s are then combined as s += s[lane ^ 8], ^ 4, ^ 2, ^ 1. So a row's maxsim has the
 * same bits wherever the row sits, for any N, on any stream and on every launch, and sel is a
 * pure function of those values and the lowest-index tie rule.
 *
 * Both return AACLIP_ERR_ARG before any launch for NULL pointers, N outside [1, 2^30], m outside
 * [1, N], start outside [0, N), a dtype outside the three, K % 64 != 0 or K above
 * AACLIP_CORESET_MAX_K, a stride below K or not 16-byte aligned, misaligned operands or a short
 * workspace.
 */
#define AACLIP_CORESET_MAX_K 4096
#define AACLIP_CORESET_BLOCK_ROWS 64
#define AACLIP_CORESET_MAX_BLOCKS 512
int aaclip_bank_coreset_workspace(int N, size_t* bytes);
int aaclip_bank_coreset(int dtype, int N, int K, const void* R, int64_t ldr, int m, int start, int32_t* sel,
                        float* cover, float* maxsim, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Test-time preprocessing (replaces dataset/__init__.py:127-143
 * transform_x / transform_mask, i.e. Pillow's Image.resize as torchvision calls it,
 * then ToTensor + Normalize). Bit-exact with Pillow 8-bit resampling.
 *
 * Host-only plan builders (no device work): Pillow BICUBIC per-axis tables --
 * bounds [out_size, 2] int32 = (first source tap, tap count), coeffs
 * [out_size, ksize] int32 with 22 fraction bits; aaclip_bicubic_taps gives the
 * ksize to allocate. Nearest: index [out_size] int32 (Pillow's accumulated
 * in/out stepping).
 */
int aaclip_bicubic_taps(int in_size, int out_size, int* ksize);
int aaclip_bicubic_plan(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize);
int aaclip_nearest_plan(int in_size, int out_size, int32_t* index);

/*
 * src: batch uint8 RGB images [in_h, in_w, 3] (row pitch / image stride in
 * bytes); plans (device copies) from aaclip_bicubic_plan(in_w, S) and (in_h, S).
 * out: fp32 [batch, 3, S, S] = (bicubic(src) / 255 - mean) / std; mean_std:
 * host float[6] (mean rgb, std rgb) or NULL for the CLIP constants.
 */
int aaclip_preprocess_images(const uint8_t* src, int64_t img_stride, int64_t row_pitch, int batch,
                             int in_h, int in_w, const int32_t* x_bounds, const int32_t* x_coeffs,
                             int kx, const int32_t* y_bounds, const int32_t* y_coeffs, int ky,
                             int out_size, const float* mean_std, float* out, void* workspace,
                             size_t workspace_bytes, void* stream);
/* workspace (optional, caller-owned device memory of aaclip_preprocess_workspace
 * bytes): enables the two-pass path (horizontal pass into a uint8 intermediate,
 * then the vertical pass); NULL = one tiled kernel with no intermediate. Same
 * output bits either way. */
int aaclip_preprocess_workspace(int batch, int in_h, int in_w, int out_size, size_t* bytes);

/*
 * src: batch uint8 L masks [in_h, in_w]; out fp32 [batch, 1, S, S] =
 * (nearest-resized mask != 0). Index tables from aaclip_nearest_plan (device copies).
 */
int aaclip_resize_masks_nearest(const uint8_t* src, int64_t img_stride, int64_t row_pitch, int batch,
                                int in_h, int in_w, const int32_t* x_index, const int32_t* y_index,
                                int out_size, float* out, void* stream);

/*
 * Train-time augmentation on the device (csrc/augment.hip). Per-image parameters are HOST
 * arrays, validated before the first launch and passed to the kernels as arguments (64
 * images per launch): nothing is copied, allocated or synchronised. Deterministic.
 *
 * Colour jitter on decoded uint8 RGB (replaces dataset/__init__.py:44-52: three
 * RandomApply(ColorJitter(...)), which on a PIL image are ImageEnhance.Brightness, .Contrast,
 * .Color, each Image.blend(degenerate, image, f)). src / dst: batch images [h, w, 3] with the
 * image stride and row pitch (bytes, pitch may be padded) of aaclip_preprocess_images, the
 * same for both; dst == src (in place) or disjoint. factors: host float [batch, 3] =
 * brightness, contrast, saturation, applied in that order; exactly 1.0 = not applied. Per
 * channel t = d + f * (i - d) in fp32, truncated for 0 <= f <= 1, else clipped to [0, 255]
 * and truncated; degenerates: 0 / int(mean L + 0.5) of the image after the brightness step
 * (exact integer sum, fp64 division) / L of the pixel, L = (19595 R + 38470 G + 7471 B +
 * 0x8000) >> 16. Bit-exact with Pillow. workspace: 8-byte aligned device memory of
 * aaclip_color_jitter_workspace bytes (partial sums of the contrast mean); may be NULL when
 * every contrast factor is 1.
 */
int aaclip_color_jitter_workspace(int batch, size_t* bytes);
int aaclip_color_jitter_u8(const uint8_t* src, int64_t img_stride, int64_t row_pitch, int batch, int h, int w,
                           const float* factors, uint8_t* dst, void* workspace, size_t workspace_bytes,
                           void* stream);

/*
 * Geometric augmentation (replaces dataset/__init__.py:30-39, 89-94: RandomRotation(30 deg),
 * RandomAffine(translate), RandomHorizontalFlip, RandomVerticalFlip on the fp32 cat of image
 * and mask; nearest, fill 0) as one gather through the composed index map. src fp32
 * [batch, channels, size, size] -> dst of the same shape; optionally a second tensor src2
 * [batch, channels2, size, size] -> dst2 through the same map (the mask next to the image,
 * without a cat), channels2 = 0 and NULL otherwise. No output may overlap an input.
 * params: host int32 [batch, 5] = rotate flag, tx, ty, hflip flag, vflip flag (flags 0 / 1).
 * cos_sin: host float [batch, 2] = cos r, sin r, r = radians(-angle) (read only with the
 * rotate flag). For output pixel (i, j): i1 = vflip ? S-1-i : i, j1 = hflip ? S-1-j : j;
 * (i2, j2) = (i1 - ty, j1 - tx), outside [0, S) -> 0; without rotation the source is (i2, j2),
 * else, in fp32: xb = j2 + 0.5 - S/2, yb = i2 + 0.5 - S/2, gx = xb * (c / (0.5 S)) + yb *
 * (s / (0.5 S)), gy = xb * (-s / (0.5 S)) + yb * (c / (0.5 S)), x = ((gx + 1) * S - 1) / 2,
 * y likewise, source (nearbyint(y), nearbyint(x)) (halves to even), outside [0, S) -> 0.
 */
int aaclip_geom_augment(const float* src, const float* src2, float* dst, float* dst2, int batch, int channels,
                        int channels2, int size, const int32_t* params, const float* cos_sin, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AACLIP_H_ */
