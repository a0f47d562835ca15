"""Device-side execution of AA-CLIP's inference path on libaaclip_hip.so.

VisualEngine = AdaptedCLIP.forward (reference model/adapter.py:67-112) +
the anomaly map / image score of test.py:80-93; TextEngine =
AdaptedCLIP.encode_text / CLIP.encode_text (adapter.py:114-145,
model/model.py:190-201) + the prompt-ensemble anchors (forward_utils.py:138-162), and
TextEngine.encode_train, the same forward with a HIP backward into the text adapter
weights (stage 1, train.py:38-114); VisualEngine.forward_train, forward() with a HIP
backward into the image adapter weights (stage 2, train.py:117-174), in fp32 or, on a bf16 engine,
in bf16 mixed precision (fp32 residual / gradient streams and weights, bf16 GEMM inputs).

Data layout in HBM (token-major "NLD", one row per token):
  x      fp32 [B*(P+1), 1024]   residual stream (kept fp32 across all 24 blocks)
  h      cdt  [B*(P+1), 1024]   LayerNorm output feeding the next GEMM
  qkv    cdt  [B*(P+1), 3072]   packed [q|k|v] (nn.MultiheadAttention in_proj order)
  attn   cdt  [B*(P+1), 1024]   merged heads
  fc     cdt  [B*(P+1), 4096]   GELU(c_fc)
  xb     bf16 [B*(P+1), 1024]   bf16 copy of x written by the c_proj epilogue (adapter input)
  u      fp32 [B*(P+1), 1024]   LeakyReLU(adapter(x))
  tap_l  cdt  [B*P, 1024]       ln_post(x[:, 1:]) at each level
  seg    fp32 [B*P, (L+1)*768]  seg_proj of level l in cols l*768.., det_proj in cols L*768.. (forward())
  spart  fp32 [B*P, (L+1)*96]   predict(), 16-bit modes: per (row, level, 32 columns) {|v|^2, v.t0, v.t1, 0}
cdt = compute dtype: bf16 (MFMA bf16, perf path) or fp32 (fp32 MFMA, parity mode).
Weights are packed once: nn.Linear [N,K] layout kept (the GEMM is A.W^T);
conv1 flattened to [1024, 640] (K padded 588 -> 640 with zeros).
"""
from __future__ import annotations

import os

import torch

from . import ops

WIDTH = 1024
HEADS = 16
Q_LOG2_SCALE = 0.125 * 1.4426950408889634  # 1/sqrt(64) * log2(e)
WS_KEEP = 16  # resident per-chunk workspaces (per image size)
MAX_STREAMS = 8  # concurrent image chunks per predict (<= WS_KEEP / 2: two chunk sizes per stream)
LAYERS = 24
PATCH = 14
EMBED = 768
KPATCH = 640  # 3*14*14 = 588 padded to a multiple of 64
DOMAIN_BLUR = {"Industrial": (7, 1.0), "Medical": (9, 1.5)}
# measure + pin the GEMM tile family per block-GEMM shape at workspace creation
# (ops.tune_gemm) when AACLIP_GEMM_TUNE=1. Off by default: in the two-stream C2 pipeline the
# isolated ranking does not carry over (tools/pin_search.py: the heuristic ~= the best pins)
TUNE = os.environ.get("AACLIP_GEMM_TUNE", "0") == "1"


def _on_device(fn):
    """Run an engine entry point with its device current (ops launch on the current
    device's stream; an engine on cuda:1 must not launch on cuda:0's)."""
    import functools

    @functools.wraps(fn)
    def wrap(self, *a, **k):
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)
    return wrap


def _blur_for(domain: str):
    # forward_utils.py:205-206: Industrial k=7 sigma=1, anything else k=9 sigma=1.5
    return DOMAIN_BLUR["Industrial"] if domain == "Industrial" else DOMAIN_BLUR["Medical"]


def _proj_weight(ad: dict, prefix: str):
    if prefix + ".fc.0.weight" in ad:
        return ad[prefix + ".fc.0.weight"], True
    return ad[prefix + ".fc.weight"], False


FP8 = ops.FP8


def _quant_weight_fp8(w: torch.Tensor):
    """Per-output-channel e4m3 weights: scale[n] = max|W[n]|/448, W8 = RNE(W/scale)."""
    w = w.detach().float()
    s = (w.abs().amax(dim=1) / 448.0).clamp_min(1e-30)
    return (w / s[:, None]).to(FP8).contiguous(), s.contiguous()


# ---------------------------------------------------------------------- packing (all engines)
def _to(t: torch.Tensor, dev, dtype):
    return t.detach().to(dev, dtype).contiguous()


def _pack_block(params: dict, p: str, dev, dtype, **in_proj):
    """The block dict of `p` = "...resblocks.{i}.": LayerNorm pairs and biases fp32, GEMM weights
    in `dtype`, nn.Linear [N, K] layout kept. in_proj = the packed in-projection pair under the
    caller's key names (the Q fold and the surgery blocks' V-rows slice are the caller's)."""
    f32 = lambda k: _to(params[p + k], dev, torch.float32)  # noqa: E731
    cdt = lambda k: _to(params[p + k], dev, dtype)  # noqa: E731
    return dict(
        ln1=(f32("ln_1.weight"), f32("ln_1.bias")), ln2=(f32("ln_2.weight"), f32("ln_2.bias")), **in_proj,
        w_o=cdt("attn.out_proj.weight"), b_o=f32("attn.out_proj.bias"),
        w_fc=cdt("mlp.c_fc.weight"), b_fc=f32("mlp.c_fc.bias"),
        w_pr=cdt("mlp.c_proj.weight"), b_pr=f32("mlp.c_proj.bias"),
    )


def _pack_visual_stem(vparams: dict, dev, dtype):
    """(conv, cls, pos, ln_pre, ln_post) of a visual tower: conv1 flattened to [1024, 640] in
    `dtype` (K padded 588 -> 640 with zeros), the embeddings and LayerNorm pairs fp32."""
    f32 = lambda k: _to(vparams["visual." + k], dev, torch.float32)  # noqa: E731
    w = vparams["visual.conv1.weight"].detach().reshape(WIDTH, -1)
    conv = torch.zeros(WIDTH, KPATCH, device=dev, dtype=torch.float32)
    conv[:, : w.shape[1]] = w
    return (conv.to(dtype).contiguous(), f32("class_embedding"), f32("positional_embedding"),
            (f32("ln_pre.weight"), f32("ln_pre.bias")), (f32("ln_post.weight"), f32("ln_post.bias")))


def _check_image(x: torch.Tensor):
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] % PATCH:
        raise ValueError("input must be [B, 3, S, S] with S a multiple of 14")


def _check_pos(pos: torch.Tensor, n_tok: int):
    if pos.shape[0] != n_tok:
        raise ValueError(f"positional embedding has {pos.shape[0]} rows, image needs {n_tok} "
                         "(resize it at load time, reference model/model.py:395-426)")


# ---------------------------------------------------------------------- training (both towers)
def _check_adapter_weights(ws: list, shapes: list, device):
    """ws: the adapter weights of a training call, shapes: the shape each must have."""
    if len(ws) != len(shapes):
        raise ValueError(f"expected {len(shapes)} adapter weights, got {len(ws)}")
    for i, (w, want) in enumerate(zip(ws, shapes)):
        if w.device != device or w.dtype != torch.float32 or tuple(w.shape) != want or not w.is_contiguous():
            raise ValueError(f"adapter weight {i} must be a contiguous fp32 {list(want)} tensor on {device}")


def _lowest_trainable(need, adapt_until: int):
    """Index of the lowest layer adapter whose weight needs a gradient (None: none does)."""
    return next((i for i in range(adapt_until) if need[i]), None)


def _bwd_weights(blocks: list, upto: int):
    """W^T copies of the frozen weights of blocks 1..upto-1, in the dtype they are packed in: dX =
    dY . W is aaclip_gemm (C = A . W'^T) with W' = W^T. Packed once per engine, on the first
    training call; block 0 never needs a backward (no trainable weight lies below the adapter that
    follows it). A bf16 engine's w_qkv carries the folded Q scale, so its transpose takes the
    gradient of the prescaled q (aaclip_attention_bwd16 under AACLIP_ATTN_Q_PRESCALED)."""
    tr = lambda w: w.t().contiguous()  # noqa: E731
    return [None] + [dict(w_qkv=tr(b["w_qkv"]), w_o=tr(b["w_o"]), w_fc=tr(b["w_fc"]), w_pr=tr(b["w_pr"]))
                     for b in blocks[1:upto]]


def _train_block_fwd(blk: dict, X, H, scratch, attend, *, keep: bool, keep_blend: bool, keep_att: bool, act,
                     w_adapt, saved: dict, i: int, dtype=torch.float32):
    """Block i of a training forward in `dtype`, from the QKV GEMM through c_proj and the adapter
    GEMM (w_adapt, or None): the inference block's launches. X: the residual stream, H: ln_1(X)
    on entry; scratch = (qkv, att, fc, u), what a block without a backward writes;
    attend(qkv, att) launches the tower's attention. keep: the block has a backward, so it
    writes fresh buffers, filed under saved[i], with c_fc's pre-activation kept (aaclip_gemm
    bias-only + aaclip_act: the epilogue's own device function); keep_att: att among them (the
    attention backward reads the forward's output). keep_blend: so has the adapter after it.
    Returns (X, u) for the caller's block tail; u = LeakyReLU(adapter(X)), or None.
    dtype bfloat16 (mixed precision): X, u and the kept fc_pre stay fp32, H / qkv / att / fc are
    bf16 and scratch carries a fifth buffer xb, the bf16 copy of X that c_proj's epilogue writes
    for the adapter GEMM (the inference block's launches again); the kept pre-activation is
    activated by aaclip_act_to16, the 16-bit epilogue's own function and rounding."""
    R, W = X.shape
    e = lambda *s: torch.empty(*s, device=X.device, dtype=torch.float32)  # noqa: E731
    c = lambda *s: torch.empty(*s, device=X.device, dtype=dtype)  # noqa: E731
    low = dtype != torch.float32
    qkv, att, fc, u = scratch[:4]
    xb = scratch[4] if low and w_adapt is not None else None
    fc_pre = fc
    if keep:
        qkv = c(R, 3 * W)
        if keep_att:
            att = c(R, W)
        fc_pre = e(R, 4 * W)
    ops.gemm(H, blk["w_qkv"], qkv, bias=blk["b_qkv"])
    attend(qkv, att)
    x_in = X
    x_mid = e(R, W) if keep else X
    ops.gemm(att, blk["w_o"], x_mid, bias=blk["b_o"], residual=x_in)
    ops.layernorm(x_mid, blk["ln2"][0], blk["ln2"][1], H)
    if keep:
        ops.gemm(H, blk["w_fc"], fc_pre, bias=blk["b_fc"])
        if low:
            ops.act_to16(fc_pre, act, out=fc)
        else:
            ops.act(fc_pre, act, out=fc)
    else:
        ops.gemm(H, blk["w_fc"], fc, bias=blk["b_fc"], gelu=act)
    X = e(R, W) if (keep or keep_blend) else x_mid
    ops.gemm(fc, blk["w_pr"], X, bias=blk["b_pr"], residual=x_mid, aux=xb)
    if keep:
        saved[i] = dict(x_in=x_in, qkv=qkv, x_mid=x_mid, fc_pre=fc_pre)
        if keep_att:
            saved[i]["att"] = att
    if w_adapt is None:
        return X, None
    if keep_blend:
        u = e(R, W)
    ops.gemm(xb if low else X, w_adapt, u, leaky=True)
    if keep_blend:  # the blend is in place: keep the pre-blend x, blend a copy
        saved.setdefault(i, {}).update(x_pre=X, u=u)
        X = X.clone()
    return X, u


def _blend_bwd(i: int, lowest: int, g, du, sv: dict, ws: list, adapt_weight: float, need, grads: list, taps,
               du16=None):
    """g = dL/d(x after block i, blended) -> dL/d(block i's own output), in place; sv: the
    block's saved dict (no "u": no trainable adapter follows it and g passes through). Fills
    grads[i] where need[i] asks; at block `lowest` the walk ends and the adapter path's dx is
    not added. taps: the tap_blocks diagnostic's dict when it wants block i, else None.
    du16 (mixed precision): the 16-bit buffer du is copied to for the input-gradient GEMM on
    the adapter weight cast to its dtype; everything else here stays fp32."""
    if du16 is None:
        wt = lambda w: w.detach().t().contiguous()  # noqa: E731
        lo = lambda t: t  # noqa: E731
    else:
        wt = lambda w: w.detach().to(du16.dtype).t().contiguous()  # noqa: E731
        lo = lambda t: ops.cast_rows(t, du16)  # noqa: E731
    if "u" in sv:  # x <- w u |x| / |u| + (1 - w) x after block i, u = LeakyReLU(x Wa_i^T)
        ops.adapter_blend_bwd(g, sv["x_pre"], sv["u"], adapt_weight, dx=g, du=du)
        ops.act_bwd(du, sv["u"], "leaky", out=du)
        if need[i]:
            grads[i] = ops.linear_wgrad(du, sv["x_pre"])
        if i > lowest:
            ops.gemm(lo(du), wt(ws[i]), g, residual=g)
    if taps is not None:  # diagnostic: dL/d(block i's own output), the adapter path included
        taps[i] = g.clone() if i > lowest else ops.gemm(lo(du), wt(ws[i]), torch.empty_like(g), residual=g)


def _block_bwd(g, blk: dict, bt: dict, sv: dict, attend_bwd, act_mode: str, d_qkv, d_wide, d_w, lo=None):
    """g = dL/d(block output) -> dL/d(block input), in place, through the frozen block: the
    input-gradient GEMMs on the transposed weights bt (_bwd_weights), no weight gradient.
    attend_bwd(sv, d_att, d_qkv) launches the tower's attention backward; d_qkv / d_wide /
    d_w are [R, 3W] / [R, 4W] / [R, W] scratch.
    lo = (g16, d_att16), [R, W] 16-bit scratch: mixed precision. g, d_w and both LayerNorm
    backwards stay fp32; d_qkv / d_wide and bt are 16-bit, g is copied to g16 before steps 1 and 5
    (aaclip_cast_rows), steps 1 and 5 write 16-bit, steps 3 and 7 write fp32 into d_w."""
    if lo is None:
        g16 = lambda: g  # noqa: E731
        d_att, act_bwd = d_w, ops.act_bwd
    else:
        g16 = lambda: ops.cast_rows(g, lo[0])  # noqa: E731
        d_att, act_bwd = lo[1], ops.act_bwd16
    ops.gemm(g16(), bt["w_pr"], d_wide)                                    # 1. d_act = g . W_pr
    act_bwd(d_wide, sv["fc_pre"], act_mode, out=d_wide)                    # 2. d_pre = d_act gelu'(fc_pre)
    ops.gemm(d_wide, bt["w_fc"], d_w)                                      # 3. d_h2 = d_pre . W_fc
    ops.layernorm_bwd(d_w, sv["x_mid"], blk["ln2"][0], residual=g, out=g)  # 4. g_mid
    ops.gemm(g16(), bt["w_o"], d_att)                                      # 5. d_att = g_mid . W_o
    attend_bwd(sv, d_att, d_qkv)                                           # 6. d_qkv
    ops.gemm(d_qkv, bt["w_qkv"], d_w)                                      # 7. d_h1 = d_qkv . W_qkv
    ops.layernorm_bwd(d_w, sv["x_in"], blk["ln1"][0], residual=g, out=g)   # 8. g_in


class MemoryBank:
    """The few-shot memory bank of one class (VisualEngine.build_bank): levels, a list of L device
    tensors [rows, 768] of unit patch rows (dtype float8_e4m3fn: of ops.Fp8MxRows, the rows in
    MX fp8 with their block scales and reciprocal norms); img_size and dtype, which a
    predict_few_shot call must match; shots, the number of support images. source_rows: the
    shots * P rows per level the bank was built from. A coreset bank (build_bank(coreset=ratio))
    keeps ops.coreset_rows(source_rows, ratio) of them per level, in pick order, and carries per
    level coreset_index (int32 [rows], the kept source rows), cover (fp32 [rows], each pick's
    similarity to the picks before it) and coverage (0-d fp32, the smallest cosine between any
    source row and its nearest kept row); all three are None for a full bank."""

    def __init__(self, levels: list, img_size: int, dtype: torch.dtype, shots: int, *, source_rows=None,
                 coreset_index=None, cover=None, coverage=None):
        self.levels, self.img_size, self.dtype, self.shots = list(levels), int(img_size), dtype, int(shots)
        self.source_rows = int(source_rows) if source_rows is not None else self.rows
        self.coreset_index, self.cover, self.coverage = coreset_index, cover, coverage

    @property
    def rows(self):
        return self.levels[0].shape[0] if self.levels else 0

    def __repr__(self):
        return (f"MemoryBank(levels={len(self.levels)}, rows={self.rows}/{self.source_rows}, "
                f"img_size={self.img_size}, dtype={self.dtype}, shots={self.shots})")


class VisualEngine:
    def __init__(self, vparams: dict, adapter: dict, *, levels=(6, 12, 18, 24), image_adapt_until=6,
                 image_adapt_weight=0.1, dtype=torch.bfloat16, fold_q_scale=True, fp8_scope="mlp",
                 quick_gelu=False):
        """dtype: bfloat16 (perf path), float16 (parity-grade 16-bit path: fp16 MFMA at the
        bf16 rate with 8x finer operand rounding; the weights the OpenAI loader produces
        are fp16-exact, reference model/model.py:366), float32 (fp32-MFMA parity mode) or
        float8_e4m3fn (config C5:
        block GEMMs on e4m3 weights (per-output-channel scales) and MX e4m3 activations
        (e8m0 scale per 64 values, applied by the K=128 block-scaled MFMA), every input
        written in that format by its producer (LayerNorm / attention / c_fc epilogues).
        fp8_scope: "mlp" (default) = c_fc and c_proj in fp8, QKV / attention / out-proj in
        bf16 -- measured at C5: map rel-L2 0.9 % vs the fp32 mode at +24 % images/s over
        bf16; "all" = the four block GEMMs in fp8: +38 % but 8 % map rel-L2 (e4m3 q/k
        logits amplified by the softmax).
        quick_gelu: the MLP activation is QuickGELU (a tower built with quick_gelu=True,
        reference model/model.py:84) instead of nn.GELU; fused into the c_fc epilogue."""
        self.act = "quick" if quick_gelu else True
        if dtype not in (torch.bfloat16, torch.float16, torch.float32, FP8):
            raise ValueError("dtype must be bfloat16, float16, float32 or float8_e4m3fn")
        self.fp8 = dtype == FP8
        if fp8_scope not in ("all", "mlp"):
            raise ValueError("fp8_scope must be 'all' (QKV, out-proj, c_fc, c_proj) or 'mlp' (c_fc, c_proj)")
        self.fp8_mlp_only = self.fp8 and fp8_scope == "mlp"
        if self.fp8:
            dtype = torch.bfloat16
        self.dtype = dtype
        self.levels = list(levels)
        self.adapt_until = int(image_adapt_until)
        self.i_w = float(image_adapt_weight)
        if len(self.levels) > 8 or sorted(self.levels) != self.levels or self.levels[-1] > LAYERS:
            raise ValueError("levels must be sorted block indices in 1..24 (at most 8)")
        dev = vparams["visual.conv1.weight"].device
        if dev.type != "cuda":
            raise RuntimeError("VisualEngine needs device tensors (no CPU path)")
        self.device = dev
        self.conv, self.cls, self.pos, self.ln_pre, self.ln_post = _pack_visual_stem(vparams, dev, dtype)
        # bf16/fp8: the attention softmax runs in the log2 domain on q' = q * log2(e)/8;
        # the factor is folded into the Q rows of in_proj (weights and bias, in fp32
        # before the bf16/e4m3 rounding), so no per-score scaling remains in the kernel
        self.q_prescaled = dtype != torch.float32 and fold_q_scale  # False: the kernel scales Q at load (A/B)

        def qkv_param(t):
            t = t.detach().to(dev, torch.float32).clone()
            if self.q_prescaled:
                t[:WIDTH] *= Q_LOG2_SCALE
            return t.contiguous()

        self.blocks = []
        for i in range(LAYERS):
            p = f"visual.transformer.resblocks.{i}."
            self.blocks.append(_pack_block(vparams, p, dev, dtype,
                                           w_qkv=_to(qkv_param(vparams[p + "attn.in_proj_weight"]), dev, dtype),
                                           b_qkv=qkv_param(vparams[p + "attn.in_proj_bias"])))
        if self.fp8:  # e4m3 copies of the block GEMM weights (the bf16 copies are dropped)
            for blk in self.blocks:
                for k in (("w_fc", "w_pr") if self.fp8_mlp_only else ("w_qkv", "w_o", "w_fc", "w_pr")):
                    blk[k] = _quant_weight_fp8(blk[k])
        self._bwd = None  # transposed frozen block weights for the input-gradient GEMMs (forward_train)
        # tests / debugging: blocks whose output gradient [R, 1024] each backward appends to
        # tap_records as {"B", "n_tok", "taps": {block: tensor}} (empty: nothing is kept)
        self.tap_blocks, self.tap_records = (), []
        self.set_adapter(adapter)
        self._ws = {}
        self.poison = False  # tests: fill new workspaces with NaN (read-before-write screen)
        # predict(): projections straight into map partials (aaclip_gemm_scores +
        # aaclip_anomaly_map_partials) instead of segbuf rows + a stream over them;
        # AACLIP_MAP_PARTIALS=0 restores the row path (A/B). Captured graphs are keyed on it
        # (predict_cached).
        self.map_partials = os.environ.get("AACLIP_MAP_PARTIALS", "1") == "1"

    def set_adapter(self, adapter: dict):
        """(Re)bind the image_adapter weights forward() / predict() read: adapt_until layer
        adapters, one seg_proj per level and det_proj (packed behind the last level's rows, one
        GEMM). The frozen packing (block weights, their transposes, the embeddings) is
        untouched, so an optimizer step costs no repacking; fp32 device parameters are
        referenced, not copied. Captured predict graphs hold the previous weights and are
        dropped."""
        cdt = lambda t: t.detach().to(self.device, self.dtype).contiguous()  # noqa: E731
        self.w_adapt = [cdt(adapter[f"layer_adapters.{i}.fc.0.weight"]) for i in range(self.adapt_until)]
        w_seg, relus = [], []
        for i in range(len(self.levels)):
            wt, r = _proj_weight(adapter, f"seg_proj.{i}")
            w_seg.append(wt)
            relus.append(r)
        w_det, r_det = _proj_weight(adapter, "det_proj")
        if len(set(relus + [r_det])) != 1:
            raise ValueError("seg_proj/det_proj relu variants must agree")
        self.relu = r_det
        self.w_seg = [cdt(t) for t in w_seg[:-1]] + [cdt(torch.cat([w_seg[-1], w_det], 0))]
        self._graph_cache, self._last_key = {}, None

    # ------------------------------------------------------------------ training (stage 2)
    def forward_train(self, x: torch.Tensor, adapter_weights):
        """forward() with a grad_fn into the image adapter (stage 2, reference train.py:117-174).
        adapter_weights: the adapt_until layer-adapter weights [1024, 1024], one seg_proj weight
        per level and the det_proj weight [768, 1024] (contiguous fp32 tensors on this engine's
        device, normally the live nn.Parameters), read as they are at the call. The outputs are
        bit-identical to forward()'s on the same weights; backward fills .grad of the weights
        that require it, walks the tower down to the lowest layer adapter that does and computes
        nothing for the frozen weights. fp32 engines and, in mixed precision, bf16 engines (fp32
        residual and gradient streams, adapter weights, .grads and LayerNorm / blend / normalise
        backwards; bf16 GEMM inputs, the weights cast at each call); a single chunk only."""
        if self.dtype not in (torch.float32, torch.bfloat16) or self.fp8:
            raise RuntimeError("the visual tower trains in fp32 only, or in bf16 mixed precision (fp16 and "
                               "fp8 engines do not train: fp16 would need loss scaling)")
        ws = list(adapter_weights)
        L = len(self.levels)
        _check_adapter_weights(ws, [(WIDTH, WIDTH)] * self.adapt_until + [(EMBED, WIDTH)] * (L + 1), self.device)
        _check_image(x)
        if x.shape[0] > self.max_chunk(x.shape[-1]):
            raise ValueError(f"forward_train takes one chunk: at most {self.max_chunk(x.shape[-1])} images of "
                             f"{x.shape[-1]} px, got {x.shape[0]}")
        out = _VisualTrain.apply(self, x, *ws)
        return list(out[:L]), out[L]

    @_on_device
    def _train_forward(self, x, ws, lowest):
        """The launches of forward_raw() + forward() in the engine's dtype (_train_block_fwd per
        block), every block above `lowest` writing fresh buffers. lowest = index of the lowest
        layer adapter that needs a gradient (None: only seg_proj / det_proj train, nothing of the
        tower is kept beyond the level taps). A bf16 engine reads the fp32 weights ws through
        bf16 copies made here, as set_adapter makes them for forward()."""
        cdt = self.dtype
        low = cdt != torch.float32
        x = x.detach().to(self.device, torch.float32).contiguous()
        B, _, S, _ = x.shape
        g = S // PATCH
        P = g * g
        n_tok = P + 1
        _check_pos(self.pos, n_tok)
        R, W, dev = B * n_tok, WIDTH, self.device
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
        c = lambda *s: torch.empty(*s, device=dev, dtype=cdt)  # noqa: E731
        cols, X, H = c(B * P, KPATCH), e(R, W), c(R, W)
        ops.im2col(x, cols, PATCH)
        ops.gemm(cols, self.conv, X, row_group=P, row_group_out=n_tok, row_offset=1)
        ops.embed_ln(X, self.cls, self.pos, self.ln_pre, self.blocks[0]["ln1"], H, B, n_tok)
        lvl = {lv: j for j, lv in enumerate(self.levels)}
        last, L, au = self.levels[-1], len(self.levels), self.adapt_until
        # qkv, att, fc, u (+ xb, the 16-bit adapter input) of the blocks without a backward
        scratch = (c(R, 3 * W), c(R, W), c(R, 4 * W), e(R, W)) + ((c(R, W),) if low else ())
        taps = [c(B * P, W) for _ in range(L)]
        saved, x_tap = {}, {}
        wc = [w.to(cdt) for w in ws] if low else ws  # the GEMM operands of the live fp32 weights
        if low:
            attend = lambda qkv, att: ops.attention(qkv, att, B, n_tok, HEADS,  # noqa: E731
                                                    q_prescaled=self.q_prescaled)
        else:
            attend = lambda qkv, att: ops.attention(qkv, att, B, n_tok, HEADS)  # noqa: E731
        for i in range(last):
            keep = lowest is not None and i > lowest        # this block has a backward
            adapt = i < au
            keep_blend = lowest is not None and adapt and i >= lowest
            # attention_bwd_tiled reads the forward's output: att is kept
            X, u = _train_block_fwd(self.blocks[i], X, H, scratch, attend, keep=keep, keep_blend=keep_blend,
                                    keep_att=True, act=self.act, w_adapt=wc[i] if adapt else None, saved=saved, i=i,
                                    dtype=cdt)
            tap = taps[lvl[i + 1]] if (i + 1) in lvl else None
            nxt = self.blocks[i + 1]["ln1"] if i + 1 < last else None
            if u is not None or nxt is not None or tap is not None:
                ops.block_tail(X, n_tok, u=u, adapt_weight=self.i_w, ln=nxt, h=H if nxt else None,
                               post=self.ln_post, tap=tap)
            if tap is not None and lowest is not None and i >= lowest:
                x_tap[lvl[i + 1]] = X  # the stream the tap read: the blocks above write fresh buffers
        # projections: the level GEMMs of forward_raw (det_proj packed behind the last level)
        seg_raw = []
        for j in range(L - 1):
            seg_raw.append(ops.gemm(taps[j], wc[au + j], e(B * P, EMBED), leaky=self.relu))
        tail = ops.gemm(taps[L - 1], torch.cat([wc[au + L - 1], wc[au + L]], 0), e(B * P, 2 * EMBED), leaky=self.relu)
        seg_raw.append(tail[:, :EMBED])
        det_raw = tail[:, EMBED:]
        out = [ops.l2_normalize(s_, e(B * P, EMBED)).view(B, P, EMBED) for s_ in seg_raw]
        det = e(B, EMBED)
        ops.image_score(det_raw, B, P, e(B * ((P + 15) // 16) * EMBED), det=det)
        st = dict(B=B, P=P, n_tok=n_tok, lowest=lowest, blocks=saved, x_tap=x_tap, taps=taps, seg_raw=seg_raw,
                  det_raw=det_raw)
        return out, det, st

    @_on_device
    def _train_backward(self, st, ws, need, dseg, ddet):
        """Gradients of the adapter weights `need` marks, from dseg (one [B, P, 768] per level)
        and ddet [B, 768]."""
        B, P, n_tok, lowest = st["B"], st["P"], st["n_tok"], st["lowest"]
        R, W, dev = B * n_tok, WIDTH, self.device
        L, au, last = len(self.levels), self.adapt_until, self.levels[-1]
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
        cdt = self.dtype
        low = cdt != torch.float32
        c = lambda *s: torch.empty(*s, device=dev, dtype=cdt)  # noqa: E731
        wt = lambda w: w.detach().to(cdt).t().contiguous()  # noqa: E731
        grads = [None] * len(ws)
        # mixed precision: the projection gradients and the weight-gradient kernel stay fp32; a
        # bf16 tap is upcast exactly for it, d is copied to bf16 for the input-gradient GEMM
        tap32 = {}

        def tap_f32(lv):
            if not low:
                return st["taps"][lv]
            if lv not in tap32:
                tap32[lv] = ops.cast_rows(st["taps"][lv], dtype=torch.float32)
            return tap32[lv]
        d16 = c(B * P, EMBED) if low else None
        # a level's tap feeds the tower backward only if a trainable adapter lies at or below it
        flows = [lowest is not None and lv - 1 >= lowest for lv in self.levels]
        dtaps = [None] * L
        for j in range(L + 1):  # the L seg projections, then det (on the last level's tap)
            lv = min(j, L - 1)
            if not (need[au + j] or flows[lv]):
                continue
            if j < L:  # seg_j = normalize(act(tap_j W^T)) per patch row
                raw = st["seg_raw"][j]
                d = ops.l2_normalize_bwd(dseg[j].reshape(B * P, EMBED).contiguous(), raw)
            else:      # det = mean_p normalize(act(tap_last W^T))
                raw = st["det_raw"]
                d = ops.l2_normalize_bwd(ddet, raw, group=P, scale=1.0 / P)
            if self.relu:
                ops.act_bwd(d, raw.contiguous(), "leaky", out=d)
            if need[au + j]:
                grads[au + j] = ops.linear_wgrad(d, tap_f32(lv))
            if flows[lv]:
                dl = ops.cast_rows(d, d16) if low else d
                if dtaps[lv] is None:
                    dtaps[lv] = ops.gemm(dl, wt(ws[au + j]), e(B * P, W))
                else:
                    ops.gemm(dl, wt(ws[au + j]), dtaps[lv], residual=dtaps[lv])
        if lowest is None:
            return grads
        if self._bwd is None:
            self._bwd = _bwd_weights(self.blocks, last)
        lvl = {lv: j for j, lv in enumerate(self.levels)}
        g = torch.zeros(R, W, device=dev, dtype=torch.float32)
        d_qkv, d_wide, d_w, du = c(R, 3 * W), c(R, 4 * W), e(R, W), e(R, W)
        if low:
            lo, du16 = (c(R, W), c(R, W)), c(R, W)  # the 16-bit copy of g, d_att; the copy of du
            attn_ws = ops.attention_bwd16_workspace(B, n_tok, HEADS, dev)
            attend_bwd = lambda sv, d_att, dqkv: ops.attention_bwd16(  # noqa: E731
                sv["qkv"], sv["att"], d_att, B, n_tok, HEADS, q_prescaled=self.q_prescaled, dqkv=dqkv,
                workspace=attn_ws)
        else:
            lo = du16 = None
            attn_ws = ops.attention_bwd_tiled_workspace(B, n_tok, HEADS, dev)
            attend_bwd = lambda sv, d_att, dqkv: ops.attention_bwd_tiled(  # noqa: E731
                sv["qkv"], sv["att"], d_att, B, n_tok, HEADS, dqkv=dqkv, workspace=attn_ws)
        act_mode = "quick" if self.act == "quick" else "gelu"
        taps = {}
        for i in range(last - 1, lowest - 1, -1):
            j = lvl.get(i + 1)
            if j is not None and dtaps[j] is not None:  # the level tap read x after block i (blend included)
                ops.tap_ln_bwd(dtaps[j], st["x_tap"][j], self.ln_post[0], g, B, n_tok)
            sv = st["blocks"].get(i, {})
            _blend_bwd(i, lowest, g, du, sv, ws, self.i_w, need, grads, taps if i in self.tap_blocks else None,
                       du16=du16)
            if i == lowest:
                break
            _block_bwd(g, self.blocks[i], self._bwd[i], sv, attend_bwd, act_mode, d_qkv, d_wide, d_w, lo=lo)
        if self.tap_blocks:
            self.tap_records.append(dict(B=B, n_tok=n_tok, taps=taps))
        return grads

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B: int, S: int, slot: int = 0):
        key = (B, S, slot)
        if key in self._ws:
            self._ws[key] = self._ws.pop(key)  # most recently used last
            return self._ws[key]
        g = S // PATCH
        P = g * g
        n_tok = P + 1
        _check_pos(self.pos, n_tok)
        R = B * n_tok
        dev, cdt = self.device, self.dtype
        e = lambda *s, dt=cdt: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
        L = len(self.levels)
        ws = dict(
            g=g, P=P, n_tok=n_tok,
            cols=e(B * P, KPATCH), x=e(R, WIDTH, dt=torch.float32), h=e(R, WIDTH), qkv=e(R, 3 * WIDTH),
            attn=e(R, WIDTH), fc=e(R, 4 * WIDTH), u=e(R, WIDTH, dt=torch.float32),
            xb=e(R, WIDTH) if cdt != torch.float32 else None,  # 16-bit adapter input (bf16 / fp16)
            taps=[e(B * P, WIDTH) for _ in range(L)],
            # all level projections + det in one [B*P, (L+1)*768] fp32 buffer: level l at
            # columns l*768, det_proj at L*768 (one row stride for the map kernel).
            # fp32 even in bf16 mode: bf16 rounding of these final features moves a
            # patch cosine by ~1e-4 (x100 in the map) — the largest single bf16
            # term in the anomaly-map error budget, for ~15 us per batch of 32.
            segbuf=e(B * P, (L + 1) * EMBED, dt=torch.float32),
            # predict() in the 16-bit modes: the level / det projections leave as anomaly-map
            # partials (aaclip_gemm_scores: per row and 32 columns {||v||^2, v.t0, v.t1}),
            # 384 B per (row, level) instead of 3 KB rows; segbuf is then only forward()'s
            spart=e(B * P, (L + 1) * 4 * ops.SCORE_GROUPS, dt=torch.float32) if cdt != torch.float32 else None,
            detrow=e(B * P, dt=torch.float32),
            # fp8 mode (MX): e4m3 GEMM inputs with e8m0 scales per (row, 64 columns):
            # a8/asc for the 1024-wide inputs (quantised from bf16), f8/fsc for the
            # 4096-wide GELU output (written in fp8 by the c_fc epilogue itself)
            a8=e(R, WIDTH, dt=FP8) if self.fp8 else None,
            asc=ops.mx_scales(R, WIDTH, dev) if self.fp8 else None,
            f8=e(R, 4 * WIDTH, dt=FP8) if self.fp8 else None,
            fsc=ops.mx_scales(R, 4 * WIDTH, dev) if self.fp8 else None,
            grid=e(B * P, dt=torch.float32), partial=e(B * ((P + 15) // 16) * EMBED, dt=torch.float32),
            det=e(B, EMBED, dt=torch.float32), score=e(B, dt=torch.float32),
            map=e(B, S, S, dt=torch.float32),
        )
        # keep the workspaces of the current image size, at most WS_KEEP of them (least
        # recently used dropped first): uneven chunks (e.g. 16 + 17 images) use one per
        # chunk and must not evict each other. A captured graph keeps its own references
        # (graphed_predict), so dropping an entry here never frees memory a graph replays.
        def size_of(k):  # (B, S, slot) workspaces, ("out", B, S) chunked-output buffers
            return k[2] if k[0] == "out" else k[1]

        drop = [k for k in self._ws if size_of(k) != S]
        chunk_keys = [k for k in self._ws if k[0] != "out" and size_of(k) == S]
        drop += chunk_keys[:max(0, len(chunk_keys) - (WS_KEEP - 1))]
        if drop and not torch.cuda.is_current_stream_capturing():
            # a dropped workspace may have been written by another stream than the one it
            # was allocated on; let that work finish before its memory returns to the pool
            torch.cuda.synchronize(self.device)
        for k in drop:
            del self._ws[k]
        self._ws[key] = ws
        if self.poison:  # test hook: every buffer starts as NaN / 0xFF, so a read-before-write shows
            for t in list(ws.values()) + ws["taps"]:
                if isinstance(t, torch.Tensor):
                    if t.is_floating_point() and t.dtype != FP8:
                        t.fill_(float("nan"))
                    else:
                        t.view(torch.uint8).fill_(0xFF)
        if TUNE and cdt != torch.float32:
            self._tune(ws)
        return ws

    def _tune(self, ws):
        """Pin the fastest tile family for each 16-bit block-GEMM shape of this
        workspace (ops.tune_gemm: measured once per shape and process, on the
        workspace's own buffers and epilogues; bit-neutral). Runs when a workspace
        is first created, i.e. outside any graph capture (graphed_predict warms up
        eagerly first)."""
        blk, X, H = self.blocks[0], ws["x"], ws["h"]
        scratch = torch.empty_like(X)
        if not (self.fp8 and not self.fp8_mlp_only):
            ops.tune_gemm(H, blk["w_qkv"], ws["qkv"], bias=blk["b_qkv"])
            ops.tune_gemm(ws["attn"], blk["w_o"], scratch, bias=blk["b_o"], residual=scratch)
        if not self.fp8:
            ops.tune_gemm(H, blk["w_fc"], ws["fc"], bias=blk["b_fc"], gelu=self.act)
            ops.tune_gemm(ws["fc"], blk["w_pr"], scratch, bias=blk["b_pr"], residual=scratch, aux=ws["xb"])
        if self.adapt_until > 0:
            ops.tune_gemm(ws["xb"], self.w_adapt[0], ws["u"], leaky=True)
        del scratch

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    @_on_device
    def forward_raw(self, x: torch.Tensor, slot: int = 0, T: torch.Tensor | None = None):
        """Run the visual tower; returns (seg_raw list of [B*P, 768] views,
        det_raw [B*P, 768] view, workspace). Rows are unnormalised projections.
        With T (predict, 16-bit modes) the projections are written as anomaly-map
        partials against T into ws["spart"] instead, and (None, None, ws) is returned."""
        _check_image(x)
        x = x.to(self.device, torch.float32).contiguous()
        B, _, S, _ = x.shape
        ws = self._workspace(B, S, slot)
        P, n_tok = ws["P"], ws["n_tok"]
        X, H = ws["x"], ws["h"]
        ops.im2col(x, ws["cols"], PATCH)
        ops.gemm(ws["cols"], self.conv, X, row_group=P, row_group_out=n_tok, row_offset=1)
        lvl = {lv: j for j, lv in enumerate(self.levels)}
        last = self.levels[-1]
        a8, asc, f8, fsc = ws["a8"], ws["asc"], ws["f8"], ws["fsc"]  # None outside the fp8 modes

        def mlp_fp8(blk, aux):  # both fp8 scopes: ln_2 -> MX e4m3 -> c_fc (fp8, GELU, MX out) -> c_proj (fp8)
            ops.layernorm(X, blk["ln2"][0], blk["ln2"][1], a8, y_sc=asc)
            ops.gemm_fp8mx(a8, asc, blk["w_fc"][0], blk["w_fc"][1], f8, out_sc=fsc, bias=blk["b_fc"], gelu=self.act)
            ops.gemm_fp8mx(f8, fsc, blk["w_pr"][0], blk["w_pr"][1], X, bias=blk["b_pr"], residual=X, aux=aux)

        def mlp_16(blk, aux):  # 16-bit and fp32 modes
            ops.layernorm(X, blk["ln2"][0], blk["ln2"][1], H)
            ops.gemm(H, blk["w_fc"], ws["fc"], bias=blk["b_fc"], gelu=self.act)
            ops.gemm(ws["fc"], blk["w_pr"], X, bias=blk["b_pr"], residual=X, aux=aux)

        mlp = mlp_fp8 if self.fp8 else mlp_16
        if self.fp8 and not self.fp8_mlp_only:
            # every GEMM input is MX e4m3, written directly by its producer: the LayerNorm
            # kernels, the attention epilogue and the c_fc epilogue (no quantisation pass)
            Hq, Hsc = a8, asc
            ops.embed_ln(X, self.cls, self.pos, self.ln_pre, self.blocks[0]["ln1"], a8, B, n_tok, h_sc=asc)

            def qkv(blk):
                ops.gemm_fp8mx(a8, asc, blk["w_qkv"][0], blk["w_qkv"][1], ws["qkv"], bias=blk["b_qkv"])

            def attend():  # attention epilogue writes the out-proj input as MX e4m3
                ops.attention(ws["qkv"], a8, B, n_tok, HEADS, out_sc=asc, q_prescaled=self.q_prescaled)

            def out_proj(blk):
                ops.gemm_fp8mx(a8, asc, blk["w_o"][0], blk["w_o"][1], X, bias=blk["b_o"], residual=X)
        else:
            Hq, Hsc = H, None
            ops.embed_ln(X, self.cls, self.pos, self.ln_pre, self.blocks[0]["ln1"], H, B, n_tok)

            def qkv(blk):
                ops.gemm(H, blk["w_qkv"], ws["qkv"], bias=blk["b_qkv"])

            def attend():
                ops.attention(ws["qkv"], ws["attn"], B, n_tok, HEADS, q_prescaled=self.q_prescaled)

            def out_proj(blk):
                ops.gemm(ws["attn"], blk["w_o"], X, bias=blk["b_o"], residual=X)
        for i in range(last):
            blk = self.blocks[i]
            qkv(blk)
            attend()
            out_proj(blk)
            adapt = i < self.adapt_until
            mlp(blk, ws["xb"] if (adapt and ws["xb"] is not None) else None)
            tap = ws["taps"][lvl[i + 1]] if (i + 1) in lvl else None
            nxt = self.blocks[i + 1]["ln1"] if i + 1 < last else None
            u = None
            if adapt:
                ops.gemm(ws["xb"] if ws["xb"] is not None else X, self.w_adapt[i], ws["u"], leaky=True)
                u = ws["u"]
            if u is not None or nxt is not None or tap is not None:
                ops.block_tail(X, n_tok, u=u, adapt_weight=self.i_w, ln=nxt, h=Hq if nxt else None,
                               post=self.ln_post, tap=tap, h_sc=Hsc)
        L = len(self.levels)
        if T is not None and ws["spart"] is not None:
            sp = ws["spart"]
            G = 4 * ops.SCORE_GROUPS
            for j in range(L):
                ncol = self.w_seg[j].shape[0]
                ops.gemm_scores(ws["taps"][j], self.w_seg[j], T, sp[:, j * G:j * G + ncol // 8], leaky=self.relu)
            return None, None, ws
        sb = ws["segbuf"]
        for j in range(L):
            ncol = self.w_seg[j].shape[0]
            ops.gemm(ws["taps"][j], self.w_seg[j], sb[:, j * EMBED:j * EMBED + ncol], leaky=self.relu)
        seg = [sb[:, j * EMBED:(j + 1) * EMBED] for j in range(L)]
        det = sb[:, L * EMBED:]
        return seg, det, ws

    @staticmethod
    def max_chunk(img_size: int) -> int:
        """Most images one forward_raw may take: the attention kernel addresses a
        chunk's packed qkv through one buffer descriptor (< 2^31 bytes), i.e.
        B * n_tok * 3 * 1024 * 2 B (606 images at 336 px, 254 at 518). Larger
        batches are split into chunks of at most this many images."""
        n_tok = (img_size // PATCH) ** 2 + 1
        return max(1, ((1 << 31) - 1) // (n_tok * 3 * WIDTH * 2))

    @torch.no_grad()
    @_on_device
    def forward(self, x: torch.Tensor):
        """AdaptedCLIP.forward contract: (list[L] of [B,P,768] unit rows, det [B,768]) fp32
        (fresh tensors; batches above max_chunk run as consecutive chunks)."""
        B, S = x.shape[0], x.shape[-1]
        mc = self.max_chunk(S)
        out, det = None, None
        for b0 in range(0, B, mc):
            b1 = min(B, b0 + mc)
            seg_raw, det_raw, ws = self.forward_raw(x[b0:b1])
            P = ws["P"]
            if out is None:
                out = [torch.empty(B * P, EMBED, device=self.device, dtype=torch.float32) for _ in seg_raw]
                det = torch.empty(B, EMBED, device=self.device, dtype=torch.float32)
            for s_, y in zip(seg_raw, out):
                ops.l2_normalize(s_, y[b0 * P:b1 * P])
            ops.image_score(det_raw, b1 - b0, P, ws["partial"], det=det[b0:b1])
        P = out[0].shape[0] // B
        return [y.view(B, P, EMBED) for y in out], det

    def _tail(self, seg_raw, det_raw, ws, T, out_map, out_score, k, s):
        """Anomaly map + image score of one chunk from its projections: from the GEMM-emitted
        partials (predict, 16-bit modes), else two passes over segbuf (the level features,
        then the det rows). One-pass and one-launch forms measured slower (round 3) and were
        removed in round 5."""
        if seg_raw is None:  # projections as partials (forward_raw with T)
            ops.anomaly_map_partials(ws["spart"], len(self.levels), out_map, ws["grid"], g=ws["g"], ksize=k, sigma=s,
                                     det_ws=ws["detrow"], score=out_score)
            return
        ops.anomaly_map(seg_raw, T, out_map, ws["grid"], g=ws["g"], ksize=k, sigma=s)
        ops.image_score(det_raw, out_map.shape[0], ws["P"], ws["partial"], det=ws["det"], T=T, score=out_score)

    def _chunk_streams(self, n: int):
        if len(getattr(self, "_streams", [])) < n:
            self._streams = [torch.cuda.Stream(device=self.device) for _ in range(n)]
        return self._streams[:n]

    @torch.no_grad()
    @_on_device
    def predict(self, x: torch.Tensor, T: torch.Tensor, domain: str = "Industrial", streams: int = 1,
                _slot0: int = 0):
        """Fused test path: (anomaly map [B,S,S] fp32, image score [B] fp32),
        = test.py:80-93 with the level sum ahead of blur+upsample.

        streams > 1 splits the batch into that many image chunks, each run on its
        own HIP stream with its own workspace: the GEMM tails of one chunk
        (tile counts that leave CUs idle in the last wave) are filled by another
        chunk's tiles. A tuple gives the chunk sizes explicitly (summing to B).
        Batches above max_chunk(S) are cut into more chunks, round-robin over the
        streams (chunks sharing a stream share its workspace, in stream order).
        The outputs are ENGINE-OWNED buffers, overwritten by the next predict of the
        same (B, S): clone them to keep them (test.py does)."""
        B, S = x.shape[0], x.shape[-1]
        T = T.to(self.device, torch.float32).contiguous()
        k, s = _blur_for(domain)
        mc = self.max_chunk(S)
        if isinstance(streams, (tuple, list)):
            sizes = [int(v) for v in streams if int(v) > 0]
            if sum(sizes) != B:
                raise ValueError(f"chunk sizes {tuple(streams)} do not sum to the batch {B}")
            if max(sizes) > mc:
                raise ValueError(f"chunk of {max(sizes)} images exceeds max_chunk({S}) = {mc}")
            if len(sizes) > MAX_STREAMS:
                raise ValueError(f"at most {MAX_STREAMS} explicit chunks")
            nstreams = len(sizes)
        else:
            nstreams = max(1, min(int(streams), B, MAX_STREAMS))
            nchunks = max(nstreams, -(-B // mc))
            sizes = [(B * (i + 1)) // nchunks - (B * i) // nchunks for i in range(nchunks)]
        bounds = [0]
        for v in sizes:
            bounds.append(bounds[-1] + v)
        if len(sizes) == 1:
            seg_raw, det_raw, ws = self.forward_raw(x, slot=_slot0, T=T if self.map_partials else None)
            self._tail(seg_raw, det_raw, ws, T, ws["map"], ws["score"], k, s)
            return ws["map"], ws["score"]
        key = ("out", B, S, _slot0)
        if key not in self._ws:
            self._ws[key] = (torch.empty(B, S, S, device=self.device), torch.empty(B, device=self.device))
        out_map, out_score = self._ws[key]
        x = x.to(self.device, torch.float32).contiguous()
        main = torch.cuda.current_stream(self.device)
        if len(getattr(self, "_events", [])) < nstreams + 1:
            self._events = [torch.cuda.Event() for _ in range(nstreams + 1)]
        ready, done = self._events[0], self._events[1:nstreams + 1]
        ready.record(main)
        sts = self._chunk_streams(nstreams)
        for st in sts:
            st.wait_event(ready)
        # every chunk's workspace exists (and, with AACLIP_GEMM_TUNE, is tuned) before any
        # chunk is enqueued: tuning never runs beside the other streams' kernels. Each is
        # allocated on the stream that uses it: the caching allocator orders a block's
        # reuse only on its allocation stream (allocated on the main stream and written
        # by a chunk stream, a workspace came back NaN after a long GPU test session:
        # tests/test_fp16_gpu.py::test_concurrent_chunk_pins in the full suite)
        for i in range(len(sizes)):
            with torch.cuda.stream(sts[i % nstreams]):
                self._workspace(sizes[i], S, _slot0 + i % nstreams)
        # concurrent chunks share the CUs: one chunk's partial last round of GEMM tiles is
        # filled by the other's work, so the 8-phase 256x256 tile (faster per FLOP) wins
        # even where its tile count rounds up worse than the 320-row tile's (c_fc at 16
        # images per chunk): whole two-stream C2 step 2240 -> 2295 images/s bf16 (2164 ->
        # 2220 fp16); a single stream keeps the heuristic (1895 vs 2050). Thread-local
        # (aaclip_gemm_concurrent), chosen at launch, so graph capture keeps it.
        # (holding chunk 1 back by a few block sub-ops, or its stream at a lower priority,
        # measured 0.3-3.5 % slower: the free-running chunks drift into a good pairing,
        # profiles/r04/chunk_stagger_ab.txt, stream_priority_ab.txt)
        with ops.concurrent_gemms(nstreams > 1 and self.dtype in (torch.bfloat16, torch.float16)):
            for i in range(len(sizes)):
                b0, b1 = bounds[i], bounds[i + 1]
                st = sts[i % nstreams]
                with torch.cuda.stream(st):
                    seg_raw, det_raw, ws = self.forward_raw(x[b0:b1], slot=_slot0 + i % nstreams,
                                                            T=T if self.map_partials else None)
                    self._tail(seg_raw, det_raw, ws, T, out_map[b0:b1], out_score[b0:b1], k, s)
        for st, ev in zip(sts, done):
            ev.record(st)
            main.wait_event(ev)
        return out_map, out_score

    # ------------------------------------------------------------------ few-shot memory bank
    @property
    def search_dtype(self):
        """Operand dtype of the nearest-patch search: fp16 in every 16-bit and fp8 mode (unit rows fit
        its range, three more mantissa bits than bf16 at the same MFMA rate), fp32 in the fp32 mode."""
        return torch.float32 if self.dtype == torch.float32 else torch.float16

    def _unit_rows(self, seg_raw):
        out = []
        for s_ in seg_raw:
            y = torch.empty(s_.shape[0], EMBED, device=self.device, dtype=self.search_dtype)
            out.append(ops.l2_normalize(s_, y))
        return out

    @torch.no_grad()
    @_on_device
    def bank_rows(self, x: torch.Tensor):
        """The level features of x as unit rows: list[L] of [B*P, 768] in search_dtype (fresh tensors).
        forward_raw without T, then aaclip_l2_normalize straight into that dtype."""
        B, S = x.shape[0], x.shape[-1]
        mc = self.max_chunk(S)
        parts = [self._unit_rows(self.forward_raw(x[b0:min(B, b0 + mc)])[0]) for b0 in range(0, B, mc)]
        return parts[0] if len(parts) == 1 else [torch.cat(lv) for lv in zip(*parts)]

    @torch.no_grad()
    @_on_device
    def bank_rows_fp8mx(self, x: torch.Tensor):
        """The level features of x as unit rows in MX fp8: list[L] of ops.Fp8MxRows [B*P, 768]. The
        chunks' raw rows are joined ahead of the quantisation, so a level has one scale buffer."""
        B, S = x.shape[0], x.shape[-1]
        mc = self.max_chunk(S)
        if B <= mc:
            return [ops.unit_rows_fp8mx(s_) for s_ in self.forward_raw(x)[0]]
        parts = [[s_.clone() for s_ in self.forward_raw(x[b0:min(B, b0 + mc)])[0]] for b0 in range(0, B, mc)]
        return [ops.unit_rows_fp8mx(torch.cat(lv)) for lv in zip(*parts)]

    def build_bank(self, support_images: torch.Tensor, search_dtype=None, coreset=None) -> "MemoryBank":
        """The memory bank of k normal support images [k, 3, S, S] (reference test.py:39-50,
        get_support_features): per level the k*P unit patch rows, in search_dtype. search_dtype
        torch.float8_e4m3fn (any engine mode) keeps them in MX fp8 instead, half the bytes, for the
        block-scaled fp8 search; None is the engine's own. coreset: None or 1.0 keeps every row; a
        ratio in (0, 1) keeps per level the greedy k-centre coreset of ops.coreset_rows(k*P, ratio)
        rows (ops.bank_coreset from row 0, on the unit rows in this engine's search_dtype whatever
        the bank's dtype), in pick order."""
        _check_image(support_images)
        if support_images.shape[0] < 1:
            raise ValueError("build_bank needs at least one support image")
        if search_dtype is not None and search_dtype not in (self.search_dtype, torch.float8_e4m3fn):
            raise ValueError(f"build_bank: search_dtype must be None, {self.search_dtype} (this engine's) or "
                             f"torch.float8_e4m3fn, got {search_dtype}")
        if coreset is not None and not 0.0 < float(coreset) <= 1.0:
            raise ValueError(f"build_bank: coreset must be None or a ratio in (0, 1], got {coreset}")
        if coreset is not None and float(coreset) != 1.0:
            return self._build_coreset_bank(support_images, search_dtype == torch.float8_e4m3fn, float(coreset))
        if search_dtype == torch.float8_e4m3fn:
            return MemoryBank(self.bank_rows_fp8mx(support_images), int(support_images.shape[-1]),
                              torch.float8_e4m3fn, int(support_images.shape[0]))
        return MemoryBank(self.bank_rows(support_images), int(support_images.shape[-1]), self.search_dtype,
                          int(support_images.shape[0]))

    @torch.no_grad()
    @_on_device
    def _build_coreset_bank(self, x: torch.Tensor, fp8: bool, ratio: float) -> "MemoryBank":
        """build_bank with a coreset: the selection runs per level on the search_dtype unit rows; an
        fp8 bank then quantises only the selected raw rows (so its rows are the ones a full fp8
        bank holds at those indices)."""
        B, S = x.shape[0], x.shape[-1]
        if fp8:  # the raw rows outlive the next forward_raw only as copies
            mc = self.max_chunk(S)
            if B <= mc:
                raw = list(self.forward_raw(x)[0])
            else:
                parts = [[s_.clone() for s_ in self.forward_raw(x[b0:min(B, b0 + mc)])[0]] for b0 in range(0, B, mc)]
                raw = [torch.cat(lv) for lv in zip(*parts)]
            unit = self._unit_rows(raw)
        else:
            unit = self.bank_rows(x)
        n = int(unit[0].shape[0])
        m = ops.coreset_rows(n, ratio)
        levels, index, cover, coverage = [], [], [], []
        for j, u in enumerate(unit):
            sel, cov, maxsim = ops.bank_coreset(u, m, 0)
            at = sel.long()
            levels.append(ops.unit_rows_fp8mx(raw[j].index_select(0, at)) if fp8 else u.index_select(0, at))
            index.append(sel)
            cover.append(cov)
            coverage.append(maxsim.min())
        return MemoryBank(levels, int(S), torch.float8_e4m3fn if fp8 else self.search_dtype, int(B), source_rows=n,
                          coreset_index=index, cover=cover, coverage=coverage)

    @torch.no_grad()
    @_on_device
    def predict_few_shot(self, x: torch.Tensor, T: torch.Tensor, bank: "MemoryBank", domain: str = "Industrial"):
        """Zero-shot and few-shot results of one batch: (zs_map [B,S,S], zs_score [B], fs_map [B,S,S]),
        fp32, fresh tensors. zs_map / zs_score are predict()'s quantities from the projected rows (the
        row path of _tail: the few-shot search needs the rows, so not the partials form). fs_map: per
        level each patch's 1 - max cosine against the bank's rows of that level (ops.bank_nn +
        ops.bank_distance), summed over the levels, then the domain's blur + upsample. A
        float8_e4m3fn bank (build_bank(..., torch.float8_e4m3fn)) is searched in MX fp8: the level
        rows go through ops.unit_rows_fp8mx and ops.bank_nn_fp8mx. Eager, on the current stream."""
        _check_image(x)
        B, S = x.shape[0], x.shape[-1]
        if not isinstance(bank, MemoryBank) or len(bank.levels) != len(self.levels):
            raise ValueError(f"bank must be a MemoryBank of {len(self.levels)} levels (build_bank)")
        fp8 = bank.dtype == torch.float8_e4m3fn
        if bank.img_size != S or not (fp8 or bank.dtype == self.search_dtype):
            raise ValueError(f"the bank was built at {bank.img_size} px in {bank.dtype}; this call is at {S} px in "
                             f"{self.search_dtype}: rebuild it (build_bank)")
        if any(isinstance(lv, ops.Fp8MxRows) != fp8 for lv in bank.levels):
            raise ValueError(f"the bank's levels do not hold its dtype {bank.dtype}: rebuild it (build_bank)")
        T = T.to(self.device, torch.float32).contiguous()
        k, s = _blur_for(domain)
        zs_map = torch.empty(B, S, S, device=self.device, dtype=torch.float32)
        zs_score = torch.empty(B, device=self.device, dtype=torch.float32)
        fs_map = torch.empty(B, S, S, device=self.device, dtype=torch.float32)
        mc = self.max_chunk(S)
        for b0 in range(0, B, mc):
            b1 = min(B, b0 + mc)
            seg_raw, det_raw, ws = self.forward_raw(x[b0:b1])
            self._tail(seg_raw, det_raw, ws, T, zs_map[b0:b1], zs_score[b0:b1], k, s)
            g = ws["g"]
            grid = torch.empty(b1 - b0, 1, g, g, device=self.device, dtype=torch.float32)
            part = None
            if fp8:
                for j, (s_, r) in enumerate(zip(seg_raw, bank.levels)):
                    part = ops.bank_nn_fp8mx(ops.unit_rows_fp8mx(s_), r, part)
                    ops.bank_distance(part, grid, accumulate=j > 0)
            else:
                for j, (q, r) in enumerate(zip(self._unit_rows(seg_raw), bank.levels)):
                    part = ops.bank_nn(q, r, part)
                    ops.bank_distance(part, grid, accumulate=j > 0)
            ops.blur_upsample(grid, fs_map[b0:b1].view(b1 - b0, 1, S, S), ksize=k, sigma=s)
        return zs_map, zs_score, fs_map

    GRAPH_CACHE = 4  # captured steps kept per engine (predict_cached), least recently used dropped

    def predict_cached(self, x: torch.Tensor, T: torch.Tensor, domain: str = "Industrial", streams=1):
        """predict() through a captured hipGraph once a (batch, size, domain, streams) shape
        repeats BACK TO BACK (the harness's full batches within a class, or one-batch
        classes of equal size): a shape runs eagerly until it follows a call of the same
        shape, then that call captures and later ones replay (inputs copied into the
        graph's static buffers). A class's tail batch is followed by another shape, so it
        never triggers a capture (no warm-up + capture + device sync for a shape that is
        not coming back) and never evicts a full-batch graph; eviction is least recently
        used. Same kernels, same bits (tests/test_e2e_gpu.py); the outputs are
        graph-owned buffers, overwritten by the next replay of that shape."""
        # every engine setting that changes what a capture records is part of the key
        key = (x.shape[0], x.shape[-1], domain, tuple(streams) if isinstance(streams, (tuple, list)) else streams,
               bool(self.map_partials))
        if not hasattr(self, "_graph_cache"):
            self._graph_cache, self._last_key = {}, None
        run = self._graph_cache.get(key)
        repeat, self._last_key = key == self._last_key, key
        if run is None:
            if not repeat or not x.is_cuda:
                return self.predict(x, T, domain, streams=streams)
            if len(self._graph_cache) >= self.GRAPH_CACHE:
                self._graph_cache.pop(next(iter(self._graph_cache)))  # the least recently used
            run = self.graphed_predict(x.shape[0], x.shape[-1], domain, streams=streams)
        self._graph_cache.pop(key, None)
        self._graph_cache[key] = run  # most recently used last
        return run(x, T.to(self.device, torch.float32))

    # ------------------------------------------------------------------ tiled inference
    @torch.no_grad()
    @_on_device
    def predict_tiled(self, canvas: torch.Tensor, T: torch.Tensor, grid: int, overlap: int,
                      domain: str = "Industrial", global_view: torch.Tensor | None = None,
                      global_weight: float = 0.5, streams=1, tile_batch: int = 32):
        """Sliding-window inference at the native scale (no reference counterpart): canvas fp32
        [B, 3, C, C] is cut into grid x grid tiles of side S = (C + (grid - 1) overlap) / grid
        overlapping by `overlap` pixels (include/aaclip.h, tiled inference), every tile goes through
        predict at S, and the tile maps are stitched onto the canvas. Returns (map [B, C, C], score
        [B]) fp32, fresh tensors:
          map   = (1 - a) * blend-weighted sum of the covering tile maps + a * the global view's map
                  upsampled bilinearly to C x C
          score = (1 - a) * max over the image's tiles + a * the global view's score
        with a = global_weight in [0, 1) and global_view [B, 3, S, S] the whole photo at the tile
        size; a = 0 runs no global forward and reads no global_view. The tiles are gathered and run
        tile_batch at a time through predict_cached (so a repeated tile-batch shape replays its
        captured graph in the same workspaces; the last chunk may be ragged), each chunk's
        engine-owned outputs copied into a per-(B, S, grid) buffer before the next call; the global
        view goes through the same path. An image's result does not depend on B, tile_batch or
        streams. ValueError when S is no integer or not the size of the tower's positional
        embedding, or when a > 0 and global_view is missing or of another shape."""
        if canvas.dim() != 4 or canvas.shape[1] != 3 or canvas.shape[2] != canvas.shape[3] or canvas.shape[0] < 1:
            raise ValueError(f"canvas must be a non-empty [B, 3, C, C], got {tuple(canvas.shape)}")
        B, C, G, O = canvas.shape[0], canvas.shape[-1], int(grid), int(overlap)
        S = ops.tile_side(C, G, O)
        if S % PATCH:
            raise ValueError(f"a canvas of {C} px in {G} x {G} tiles overlapping by {O} gives tiles of {S} px, "
                             f"no multiple of {PATCH}")
        _check_pos(self.pos, (S // PATCH) ** 2 + 1)
        a = float(global_weight)
        if not 0.0 <= a < 1.0:
            raise ValueError(f"global_weight must lie in [0, 1), got {global_weight}")
        if a > 0.0 and (global_view is None or tuple(global_view.shape) != (B, 3, S, S)):
            raise ValueError(f"global_weight {a} needs global_view {(B, 3, S, S)}, got "
                             f"{None if global_view is None else tuple(global_view.shape)}")
        tile_batch = int(tile_batch)
        if tile_batch < 1:
            raise ValueError(f"tile_batch must be at least 1, got {tile_batch}")
        canvas = canvas.to(self.device, torch.float32).contiguous()
        n = B * G * G
        step = min(tile_batch, n, self.max_chunk(S))
        if not hasattr(self, "_tiled"):
            self._tiled = {}
        key = (B, S, G)
        if key not in self._tiled:
            for k in [k for k in self._tiled if k[1] != S]:  # as _workspace: one image size resident
                del self._tiled[k]
            self._tiled[key] = (torch.empty(n, S, S, device=self.device), torch.empty(n, device=self.device))
        tile_maps, tile_scores = self._tiled[key]
        stage = self._tiled.get(("stage", S, step))
        if stage is None:
            stage = self._tiled[("stage", S, step)] = torch.empty(step, 3, S, S, device=self.device)
        for t0 in range(0, n, step):
            t1 = min(n, t0 + step)
            tiles = ops.tile_gather(canvas, G, O, tiles=(t0, t1), out=stage[:t1 - t0])
            m, s = self.predict_cached(tiles, T, domain, streams=streams)
            tile_maps[t0:t1].copy_(m)
            tile_scores[t0:t1].copy_(s)
        gmap = gscore = None
        if a > 0.0:  # last: its engine-owned outputs are read by the stitch before any other predict
            gmap, gscore = self.predict_cached(global_view, T, domain, streams=streams)
        out_map = ops.tile_stitch(tile_maps, G, O, global_maps=gmap, global_weight=a)
        out_score = ops.tile_score(tile_scores, G, global_scores=gscore, global_weight=a)
        return out_map, out_score

    @torch.no_grad()
    @_on_device
    def graphed_predict(self, batch: int, img_size: int, domain: str = "Industrial", streams: int = 1):
        """Capture predict() for a fixed (batch, size, domain, streams) into one hipGraph
        (torch.cuda.CUDAGraph records the C-ABI launches on the capturing stream and the
        chunk streams' fork/join). Returns fn(x, T) -> (map, score) that copies the
        inputs into static device buffers and replays the graph: no per-kernel host
        launch cost (matters at small batch, e.g. config C1's bs=1). The graph runs in
        workspaces of its own (a private slot range), so eager predict() calls of the
        same shape never write into the buffers it replays into or returns."""
        self._graphs = getattr(self, "_graphs", 0) + 1
        slot0 = 1000 * self._graphs
        x_s = torch.zeros(batch, 3, img_size, img_size, device=self.device)
        T_s = torch.zeros(EMBED, 2, device=self.device)
        T_s[0, 0] = 1.0
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        before = set(self._ws)
        with torch.cuda.stream(side):  # warm-up: allocate workspaces, set kernel attributes
            self.predict(x_s, T_s, domain, streams=streams, _slot0=slot0)
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        mine = {k: v for k, v in self._ws.items() if k not in before}  # the graph's own workspaces
        graph = torch.cuda.CUDAGraph()
        # thread_local: only this thread's calls are checked against the capture. The harness
        # captures while its DataLoader's pin-memory thread keeps allocating pinned host
        # buffers and querying events; "global" mode would fail the capture (or that
        # thread) for calls that never touch the captured streams
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out_map, out_score = self.predict(x_s, T_s, domain, streams=streams, _slot0=slot0)
        held = list(mine.values())  # kept alive by the graph even if the LRU drops their keys
        dev = self.device

        def run(x: torch.Tensor, T: torch.Tensor):
            with torch.cuda.device(dev):
                x_s.copy_(x, non_blocking=True)
                T_s.copy_(T, non_blocking=True)
                graph.replay()
            return out_map, out_score

        run.graph = graph
        run.workspaces = held
        run.slot0 = slot0  # the private workspace slots (tools / bench diagnostics re-capture on them)
        return run


class _VisualTrain(torch.autograd.Function):
    """VisualEngine.forward with a backward into the image adapter weights (stage 2)."""

    @staticmethod
    def forward(ctx, engine, x, *ws):
        lowest = _lowest_trainable(ctx.needs_input_grad[2:], engine.adapt_until)
        out, det, st = engine._train_forward(x, [w.detach() for w in ws], lowest)
        ctx.engine, ctx.st = engine, st
        ctx.save_for_backward(*ws)
        return (*out, det)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *douts):
        ws = ctx.saved_tensors
        need = list(ctx.needs_input_grad[2:])
        eng = ctx.engine
        d = [t.to(eng.device, torch.float32).contiguous() for t in douts]
        grads = eng._train_backward(ctx.st, [w.detach() for w in ws], need, d[:-1], d[-1])
        ctx.st = None
        return (None, None, *grads)


class TextEngine:
    """12-block causal text tower; adapted (text_adapter) or plain CLIP projection."""

    def __init__(self, params: dict, text_adapter: dict | None, *, text_adapt_until=3, text_adapt_weight=0.1,
                 dtype=torch.float32, quick_gelu=False):
        self.act = "quick" if quick_gelu else True  # MLP activation (reference model.py:129)
        dev = params["token_embedding.weight"].device
        if dev.type != "cuda":
            raise RuntimeError("TextEngine needs device tensors (no CPU path)")
        self.device, self.dtype = dev, dtype
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()  # noqa: E731
        cdt = lambda t: t.detach().to(dev, dtype).contiguous()  # noqa: E731
        self.width = params["ln_final.weight"].shape[0]
        self.heads = self.width // 64
        self.tok_emb = f32(params["token_embedding.weight"])
        self.pos = f32(params["positional_embedding"])
        self.ln_final = (f32(params["ln_final.weight"]), f32(params["ln_final.bias"]))
        nl = len({k.split(".")[2] for k in params if k.startswith("transformer.resblocks.")})
        self.blocks = []
        for i in range(nl):
            p = f"transformer.resblocks.{i}."
            self.blocks.append(_pack_block(params, p, dev, dtype, w_qkv=cdt(params[p + "attn.in_proj_weight"]),
                                           b_qkv=f32(params[p + "attn.in_proj_bias"])))
        self.adapted = text_adapter is not None
        self.t_w = float(text_adapt_weight)
        self._bwd = None  # transposed frozen weights for the input-gradient GEMMs (encode_train)
        # tests / debugging: blocks whose output gradient [R, width] each backward appends to
        # tap_records as {"n", "ctx", "taps": {block: tensor}} (empty: nothing is kept)
        self.tap_blocks, self.tap_records = (), []
        if self.adapted:
            self.adapt_until = int(text_adapt_until)
            self.set_adapter(text_adapter)
        else:
            self.adapt_until = 0
            self.w_out = cdt(params["text_projection"].t())  # x @ P == x . (P^T)^T

    def set_adapter(self, text_adapter: dict):
        """(Re)bind the adapter weights encode() reads: adapt_until SimpleAdapters + the output
        SimpleProj (Linear + LeakyReLU). The frozen packing (block weights, their transposes,
        the token embedding) is untouched, so an optimizer step costs no repacking; fp32
        device parameters are referenced, not copied."""
        if not self.adapted:
            raise RuntimeError("this TextEngine was built without a text adapter")
        cdt = lambda t: t.detach().to(self.device, self.dtype).contiguous()  # noqa: E731
        self.w_adapt = [cdt(text_adapter[f"{i}.fc.0.weight"]) for i in range(self.adapt_until)]
        self.w_out = cdt(text_adapter[f"{self.adapt_until}.fc.0.weight"])  # Linear + LeakyReLU

    @torch.no_grad()
    @_on_device
    def encode(self, tokens: torch.Tensor, truncate: bool = True) -> torch.Tensor:
        """[n, 77] token ids -> [n, embed] (adapted: LeakyReLU(x_eot W^T), else x_eot @ proj).
        truncate: the tower is causal, so the EOT row (argmax token id, model.py:198)
        depends only on the tokens up to it; the columns after the longest prompt's EOT
        are dropped (prompts here are <= 39 of 77 tokens: ~half the text FLOPs). Rows are
        independent in every kernel, so the result is bit-identical to the full 77."""
        n, ctx = tokens.shape
        if ctx != self.pos.shape[0]:
            raise ValueError("token context length mismatch")
        if truncate and n > 0:
            ctx = int(tokens.argmax(-1).max()) + 1
            tokens = tokens[:, :ctx]
        tokens = tokens.to(self.device, torch.int32).contiguous()
        R, W = n * ctx, self.width
        dev, cdt = self.device, self.dtype
        e = lambda *s, dt=cdt: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
        X, H = e(R, W, dt=torch.float32), e(R, W)
        qkv, att, fc, u = e(R, 3 * W), e(R, W), e(R, 4 * W), e(R, W, dt=torch.float32)
        xb = e(R, W) if cdt != torch.float32 else None
        ops.text_embed_ln(tokens, self.tok_emb, self.pos, self.blocks[0]["ln1"], X, H)
        nb = len(self.blocks)
        for i, blk in enumerate(self.blocks):
            ops.gemm(H, blk["w_qkv"], qkv, bias=blk["b_qkv"])
            ops.attention(qkv, att, n, ctx, self.heads, causal=True)
            ops.gemm(att, blk["w_o"], X, bias=blk["b_o"], residual=X)
            ops.layernorm(X, blk["ln2"][0], blk["ln2"][1], H)
            ops.gemm(H, blk["w_fc"], fc, bias=blk["b_fc"], gelu=self.act)
            adapt = i < self.adapt_until
            ops.gemm(fc, blk["w_pr"], X, bias=blk["b_pr"], residual=X, aux=xb if (adapt and xb is not None) else None)
            nxt = self.blocks[i + 1]["ln1"] if i + 1 < nb else None
            if adapt:
                ops.gemm(xb if xb is not None else X, self.w_adapt[i], u, leaky=True)
                ops.block_tail(X, ctx, u=u, adapt_weight=self.t_w, ln=nxt, h=H if nxt else None)
            elif nxt is not None:
                ops.layernorm(X, nxt[0], nxt[1], H)
        eot = e(n, W)
        ops.eot_ln(X, tokens, self.ln_final, eot)
        out = torch.empty(n, self.w_out.shape[0], device=dev, dtype=torch.float32)
        ops.gemm(eot, self.w_out, out, leaky=self.adapted)
        return out

    @torch.no_grad()
    @_on_device
    def class_anchor(self, tok_normal: torch.Tensor, tok_abnormal: torch.Tensor) -> torch.Tensor:
        """forward_utils.py:146-161 -> T [768, 2] (normal, abnormal)."""
        T = torch.empty(self.w_out.shape[0], 2, device=self.device, dtype=torch.float32)
        for col, tok in enumerate((tok_normal, tok_abnormal)):
            ops.anchor_reduce(self.encode(tok), T, col)
        return T

    # ------------------------------------------------------------------ training (stage 1)
    def encode_train(self, tokens: torch.Tensor, adapter_weights, truncate: bool = True) -> torch.Tensor:
        """encode() with a grad_fn into the text adapter: adapter_weights are the adapt_until
        SimpleAdapter weights followed by the output SimpleProj weight ([width, width] ...,
        [embed, width]; fp32 tensors on this engine's device, normally the live nn.Parameters),
        read as they are at the call. The embeddings are bit-identical to encode()'s on the
        same weights; backward fills .grad of the weights that require it and computes nothing
        for the frozen tower."""
        if not self.adapted:
            raise RuntimeError("encode_train needs an engine built with a text adapter")
        if self.dtype != torch.float32:
            raise RuntimeError("the text tower trains in fp32 only")
        ws = list(adapter_weights)
        W = self.width
        _check_adapter_weights(ws, [(W, W)] * self.adapt_until + [(self.w_out.shape[0], W)], self.device)
        if tokens.dim() != 2 or tokens.shape[1] != self.pos.shape[0]:
            raise ValueError("token context length mismatch")
        return _TextTrain.apply(self, tokens, bool(truncate), *ws)

    @_on_device
    def _train_forward(self, tokens, truncate, ws, lowest):
        """The launches of encode() (_train_block_fwd per block), every block from `lowest` + 1
        up writing fresh buffers. lowest = index of the lowest adapter that needs a gradient
        (None: only the output projection trains, nothing below the EOT rows is kept)."""
        n, ctx = tokens.shape
        if truncate and n > 0:
            ctx = int(tokens.argmax(-1).max()) + 1
            tokens = tokens[:, :ctx]
        tokens = tokens.to(self.device, torch.int32).contiguous()
        R, W = n * ctx, self.width
        dev = self.device
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
        X, H = e(R, W), e(R, W)
        scratch = (e(R, 3 * W), e(R, W), e(R, 4 * W), e(R, W))  # qkv, att, fc, u of the blocks without a backward
        ops.text_embed_ln(tokens, self.tok_emb, self.pos, self.blocks[0]["ln1"], X, H)
        nb = len(self.blocks)
        saved = {}
        attend = lambda qkv, att: ops.attention(qkv, att, n, ctx, self.heads, causal=True)  # noqa: E731
        for i, blk in enumerate(self.blocks):
            keep = lowest is not None and i > lowest        # this block has a backward
            adapt = i < self.adapt_until
            keep_blend = lowest is not None and adapt and i >= lowest
            # attention_bwd takes qkv and dout only: att is not kept
            X, u = _train_block_fwd(blk, X, H, scratch, attend, keep=keep, keep_blend=keep_blend, keep_att=False,
                                    act=self.act, w_adapt=ws[i] if adapt else None, saved=saved, i=i)
            nxt = self.blocks[i + 1]["ln1"] if i + 1 < nb else None
            if adapt:
                ops.block_tail(X, ctx, u=u, adapt_weight=self.t_w, ln=nxt, h=H if nxt else None)
            elif nxt is not None:
                ops.layernorm(X, nxt[0], nxt[1], H)
        eot = e(n, W)
        ops.eot_ln(X, tokens, self.ln_final, eot)
        out = e(n, ws[-1].shape[0])
        ops.gemm(eot, ws[-1], out, leaky=True)
        return out, dict(tokens=tokens, n=n, ctx=ctx, blocks=saved, x_final=X if lowest is not None else None,
                         eot=eot, lowest=lowest)

    @_on_device
    def _train_backward(self, st, ws, need, demb):
        """Gradients of the adapter weights `need` marks, from demb = dL/d(embeddings)."""
        n, ctx, tokens, lowest = st["n"], st["ctx"], st["tokens"], st["lowest"]
        R, W = n * ctx, self.width
        dev = self.device
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
        grads = [None] * len(ws)
        # out = LeakyReLU(eot W_out^T)
        d_o = ops.act_bwd(demb, st["out"], "leaky")
        if need[-1]:
            grads[-1] = ops.linear_wgrad(d_o, st["eot"])
        if lowest is None:
            return grads
        if self._bwd is None:
            self._bwd = _bwd_weights(self.blocks, len(self.blocks))
        d_eot = ops.gemm(d_o, ws[-1].detach().t().contiguous(), e(n, W))
        g = ops.eot_ln_bwd(d_eot, st["x_final"], tokens, self.ln_final[0])
        d_qkv, d_wide, d_w, du = e(R, 3 * W), e(R, 4 * W), e(R, W), e(R, W)
        attend_bwd = lambda sv, d_att, dqkv: ops.attention_bwd(  # noqa: E731
            sv["qkv"], d_att, n, ctx, self.heads, causal=True, dqkv=dqkv)
        act_mode = "quick" if self.act == "quick" else "gelu"
        taps = {}
        for i in range(len(self.blocks) - 1, lowest - 1, -1):
            sv = st["blocks"].get(i, {})
            _blend_bwd(i, lowest, g, du, sv, ws, self.t_w, need, grads, taps if i in self.tap_blocks else None)
            if i == lowest:
                break
            _block_bwd(g, self.blocks[i], self._bwd[i], sv, attend_bwd, act_mode, d_qkv, d_wide, d_w)
        if self.tap_blocks:
            self.tap_records.append(dict(n=n, ctx=ctx, taps=taps))
        return grads


class _TextTrain(torch.autograd.Function):
    """TextEngine.encode with a backward into the text adapter weights (stage 1)."""

    @staticmethod
    def forward(ctx, engine, tokens, truncate, *ws):
        lowest = _lowest_trainable(ctx.needs_input_grad[3:], engine.adapt_until)
        out, st = engine._train_forward(tokens, truncate, [w.detach() for w in ws], lowest)
        ctx.engine, ctx.st = engine, st
        ctx.save_for_backward(*ws, out)  # the output (LeakyReLU's backward reads it) goes through autograd
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, demb):
        *ws, out = ctx.saved_tensors
        need = list(ctx.needs_input_grad[3:])
        eng = ctx.engine
        demb = demb.to(eng.device, torch.float32).contiguous()
        grads = eng._train_backward(dict(ctx.st, out=out), [w.detach() for w in ws], need, demb)
        ctx.st = None
        return (None, None, None, *grads)


class FrozenVisualEngine:
    """The frozen, forward-only CLIP image tower: CLIP.encode_image (reference
    model/model.py:185-188 -> VisionTransformer.forward, model/transformer.py:490-551),
    plain or after VisionTransformer.DAPM_replace (transformer.py:407-425).

    Same packing, fp32 residual stream, embed_ln / block_tail row kernels and GEMM
    epilogues as VisualEngine; no adapters. surgery_from = s (0..23) runs blocks s..23 as
    the reference's post-surgery blocks: ln_1, a V-only projection (rows [2048:3072] of
    in_proj: the q / k thirds are computed and discarded by the reference, never here),
    ops.vv_attention, out-proj + residual, ln_2 + MLP. That attention mixes the IMAGES of
    a batch (per token position and head; see aaclip_vv_attention), so a surgery batch is
    never cut into chunks or spread over streams, and holds at most ops.VV_MAX_BATCH
    images. Without surgery every image is independent and batches above max_chunk run
    as consecutive chunks."""

    def __init__(self, vparams: dict, *, dtype=torch.float16, surgery_from: int | None = None, quick_gelu=False):
        if dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError("FrozenVisualEngine dtype must be bfloat16, float16 or float32 (no fp8 mode)")
        if surgery_from is not None and not 0 <= int(surgery_from) < LAYERS:
            raise ValueError(f"surgery_from must be a block index in 0..{LAYERS - 1} or None")
        self.act = "quick" if quick_gelu else True
        self.dtype = dtype
        self.surgery_from = LAYERS if surgery_from is None else int(surgery_from)
        dev = vparams["visual.conv1.weight"].device
        if dev.type != "cuda":
            raise RuntimeError("FrozenVisualEngine needs device tensors (no CPU path)")
        self.device = dev
        self.conv, self.cls, self.pos, self.ln_pre, self.ln_post = _pack_visual_stem(vparams, dev, dtype)
        self.w_proj = _to(vparams["visual.proj"].t(), dev, dtype)  # x @ proj == x . (proj^T)^T
        self.q_prescaled = dtype != torch.float32  # log2(e)/8 folded into the Q rows (as VisualEngine)
        self.blocks = []
        for i in range(LAYERS):
            p = f"visual.transformer.resblocks.{i}."
            w_in = vparams[p + "attn.in_proj_weight"].detach().to(dev, torch.float32)
            b_in = vparams[p + "attn.in_proj_bias"].detach().to(dev, torch.float32)
            if i >= self.surgery_from:  # V rows only; the Q fold touches rows [:1024], so V is as loaded
                w_in, b_in = w_in[2 * WIDTH:], b_in[2 * WIDTH:]
            elif self.q_prescaled:
                w_in, b_in = w_in.clone(), b_in.clone()
                w_in[:WIDTH] *= Q_LOG2_SCALE
                b_in[:WIDTH] *= Q_LOG2_SCALE
            self.blocks.append(_pack_block(vparams, p, dev, dtype, w_in=_to(w_in, dev, dtype), b_in=b_in.contiguous()))
        self._ws = {}
        self._patch = None
        self.poison = False  # tests: fill new workspaces with NaN (read-before-write screen)

    @property
    def surgery(self) -> bool:
        return self.surgery_from < LAYERS

    max_chunk = staticmethod(VisualEngine.max_chunk)

    def _workspace(self, B: int, S: int):
        key = (B, S)
        if key in self._ws:
            return self._ws[key]
        g = S // PATCH
        P = g * g
        n_tok = P + 1
        _check_pos(self.pos, n_tok)
        R = B * n_tok
        dev, cdt = self.device, self.dtype
        e = lambda *s, dt=cdt: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
        ws = dict(
            P=P, n_tok=n_tok, cols=e(B * P, KPATCH), x=e(R, WIDTH, dt=torch.float32), h=e(R, WIDTH),
            qkv=e(R, 3 * WIDTH) if self.surgery_from > 0 else None,  # the standard blocks' packed [q|k|v]
            v=e(R, WIDTH) if self.surgery else None,                 # the surgery blocks' V projection
            attn=e(R, WIDTH), fc=e(R, 4 * WIDTH),
            tap=e(B * P, WIDTH),  # ln_post of the patch rows after block 24 (patch_features)
            cls_h=e(B, WIDTH),    # ln_post of the CLS rows
        )
        if self._ws and not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(self.device)
        self._ws.clear()  # one resident shape: the frozen paths run one batch shape per stage
        self._ws[key] = ws
        if self.poison:
            for t in ws.values():
                if isinstance(t, torch.Tensor):
                    t.fill_(float("nan"))
        return ws

    def _encode_chunk(self, x: torch.Tensor, out_layers, want_patch: bool):
        B, _, S, _ = x.shape
        ws = self._workspace(B, S)
        P, n_tok = ws["P"], ws["n_tok"]
        X, H = ws["x"], ws["h"]
        ops.im2col(x, ws["cols"], PATCH)
        ops.gemm(ws["cols"], self.conv, X, row_group=P, row_group_out=n_tok, row_offset=1)
        ops.embed_ln(X, self.cls, self.pos, self.ln_pre, self.blocks[0]["ln1"], H, B, n_tok)
        tokens = []
        for i, blk in enumerate(self.blocks):
            if i >= self.surgery_from:
                ops.gemm(H, blk["w_in"], ws["v"], bias=blk["b_in"])
                ops.vv_attention(ws["v"], ws["attn"], B, n_tok, HEADS)
            else:
                ops.gemm(H, blk["w_in"], ws["qkv"], bias=blk["b_in"])
                ops.attention(ws["qkv"], ws["attn"], B, n_tok, HEADS, q_prescaled=self.q_prescaled)
            ops.gemm(ws["attn"], blk["w_o"], X, bias=blk["b_o"], residual=X)
            ops.layernorm(X, blk["ln2"][0], blk["ln2"][1], H)
            ops.gemm(H, blk["w_fc"], ws["fc"], bias=blk["b_fc"], gelu=self.act)
            ops.gemm(ws["fc"], blk["w_pr"], X, bias=blk["b_pr"], residual=X)
            if i + 1 in out_layers:
                tokens.append(X.view(B, n_tok, WIDTH).clone())
            if i + 1 < LAYERS:
                ops.block_tail(X, n_tok, ln=self.blocks[i + 1]["ln1"], h=H)
            elif want_patch:
                ops.block_tail(X, n_tok, post=self.ln_post, tap=ws["tap"])
        # pooled = ln_post(x[:, 0]) @ proj: the CLS rows are read in place (row stride n_tok * width)
        ops.layernorm(X.view(B, n_tok * WIDTH)[:, :WIDTH], self.ln_post[0], self.ln_post[1], ws["cls_h"])
        pooled = torch.empty(B, EMBED, device=self.device, dtype=torch.float32)
        ops.gemm(ws["cls_h"], self.w_proj, pooled)
        patch = None
        if want_patch:
            patch = torch.empty(B * P, EMBED, device=self.device, dtype=torch.float32)
            ops.gemm(ws["tap"], self.w_proj, patch)
            patch = patch.view(B, P, EMBED)
        return pooled, tokens, patch

    @staticmethod
    def chunk_bounds(B: int, max_chunk: int) -> list:
        """[b0, b1) image ranges a plain (per-image) batch of B runs as."""
        return [(b0, min(B, b0 + max_chunk)) for b0 in range(0, B, max_chunk)]

    @torch.no_grad()
    @_on_device
    def encode(self, x: torch.Tensor, out_layers=(), patch_features: bool = False):
        """VisionTransformer.forward: (pooled [B, 768] fp32, [x after block i as a fresh
        [B, n_tok, 1024] fp32 tensor for each i in 1..24 that is in out_layers, ascending]).
        All 24 blocks always run. patch_features=True also keeps ln_post(patch rows after
        block 24) @ proj for patch_features() (AdaptedCLIP.forward_original)."""
        _check_image(x)
        out_layers = set(int(i) for i in out_layers)
        x = x.to(self.device, torch.float32).contiguous()
        B, S = x.shape[0], x.shape[-1]
        if self.surgery:
            if B > ops.VV_MAX_BATCH:
                raise ValueError(f"a surgery tower couples the images of a batch and takes at most "
                                 f"{ops.VV_MAX_BATCH} images at once, got {B}")
            bounds = [(0, B)]
        else:
            bounds = self.chunk_bounds(B, self.max_chunk(S))
        parts = [self._encode_chunk(x[b0:b1], out_layers, patch_features) for b0, b1 in bounds]
        if len(parts) == 1:
            pooled, tokens, patch = parts[0]
        else:
            pooled = torch.cat([p[0] for p in parts])
            tokens = [torch.cat(level) for level in zip(*(p[1] for p in parts))]
            patch = torch.cat([p[2] for p in parts]) if patch_features else None
        self._patch = patch
        return pooled, tokens

    def patch_features(self) -> torch.Tensor:
        """[B, P, 768] fp32: ln_post(patch tokens after block 24) @ proj of the last
        encode(..., patch_features=True) (reference model/adapter.py:57-62)."""
        if self._patch is None:
            raise RuntimeError("patch_features() follows encode(x, out_layers, patch_features=True)")
        return self._patch
