"""AdaptedCLIP — drop-in for reference model/adapter.py:6-145.

Same constructor, attributes (`clipmodel`, `image_encoder`, `image_adapter`
ModuleDict{layer_adapters, seg_proj, det_proj}, `text_adapter` ModuleList,
`t_w`, `i_w`, `levels`, ...) and state-dict keys. `forward` / `encode_text`
run on the MI355X engines (aaclip.engine) built from the module's current
parameters; the packed device copies are rebuilt whenever a parameter changes
(load_state_dict, in-place edits: tracked by tensor version counters; a changed adapter is
re-bound without repacking the frozen tower). `encode_text` under grad mode with a trainable
`text_adapter` is differentiable into it (stage 1), and so is `forward` into a trainable
`image_adapter` in the fp32 mode (stage 2), or in bf16 mixed precision when the model is built with
`compute_dtype=train_dtype=torch.bfloat16`.

Compute dtype of the visual tower: fp16 MFMA by default — the mode that meets the
north_star map contract (1e-3 abs + 1e-2 rel, argmax labels beyond rounding ties)
at the bf16 MFMA rate; `compute_dtype=torch.bfloat16` selects bf16 (config C2's
throughput mode), `torch.float32` the fp32-MFMA parity mode, `torch.float8_e4m3fn`
the config-C5 fp8 MX mode; env AACLIP_DTYPE=bf16 / fp16 / fp32 / fp8 too.
The text tower always runs fp32 (once per dataset, <1% of the work).
"""
from __future__ import annotations

import os

import torch
from torch import nn

from .adapter_modules import SimpleAdapter, SimpleProj


def param_signature(module: nn.Module, prefix_excl: str | None = None):
    return tuple((n, p.data_ptr(), p._version) for n, p in module.state_dict(keep_vars=True).items()
                 if prefix_excl is None or not n.startswith(prefix_excl))


def check_train_dtype(train_dtype):
    """train_dtype: None (stage 2 trains in the fp32 mode only) or torch.bfloat16 (it also trains
    in bf16 mixed precision when compute_dtype is bfloat16). fp16 would need loss scaling."""
    if train_dtype is not None and train_dtype != torch.bfloat16:
        raise ValueError(f"train_dtype must be None or torch.bfloat16, got {train_dtype!r}")
    return train_dtype


def _default_dtype():
    v = os.environ.get("AACLIP_DTYPE", "fp16").lower()
    if v in ("fp8", "float8", "e4m3"):  # config C5: fp8 MX block GEMMs
        return torch.float8_e4m3fn
    if v in ("fp16", "float16", "f16", "half"):  # parity-grade 16-bit mode (fp16 MFMA)
        return torch.float16
    if v in ("fp32", "float32", "f32"):
        return torch.float32
    if v in ("bf16", "bfloat16"):
        return torch.bfloat16
    raise ValueError(f"AACLIP_DTYPE={v!r}: expected bf16, fp16, fp32 or fp8")


class AdaptedCLIP(nn.Module):
    def __init__(self, clip_model, text_adapt_weight: float = 0.1, image_adapt_weight: float = 0.1,
                 text_adapt_until: int = 3, image_adapt_until: int = 6, levels: list = [6, 12, 18, 24],
                 relu: bool = True, compute_dtype: torch.dtype | None = None,
                 train_dtype: torch.dtype | None = None, **kwargs):
        super().__init__()
        self.clipmodel = clip_model
        self.image_encoder = clip_model.visual
        self.text_adapt_until = text_adapt_until
        self.image_adapt_until = image_adapt_until
        self.t_w = text_adapt_weight
        self.i_w = image_adapt_weight
        self.levels = list(levels)
        self.compute_dtype = compute_dtype or _default_dtype()
        self.train_dtype = check_train_dtype(train_dtype)
        width = clip_model.visual.conv1.weight.shape[0]
        embed = clip_model.visual.output_dim
        twidth = clip_model.transformer.width
        layer_adapters = nn.ModuleList([SimpleAdapter(width, width) for _ in range(image_adapt_until)])
        seg_proj = nn.ModuleList([SimpleProj(width, embed, relu) for _ in range(len(levels))])
        det_proj = SimpleProj(width, embed, relu)
        self.image_adapter = nn.ModuleDict({"layer_adapters": layer_adapters, "seg_proj": seg_proj,
                                            "det_proj": det_proj})
        self.text_adapter = nn.ModuleList([SimpleAdapter(twidth, twidth) for _ in range(text_adapt_until)]
                                          + [SimpleProj(twidth, embed, relu=True)])
        self._init_weights_()
        self._vis = None
        self._vis_sig = None
        self._vis_asig = None

    def _init_weights_(self):
        for p in self.image_adapter.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for p in self.text_adapter.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    # ------------------------------------------------------------------ engines
    def visual_engine(self):
        from aaclip.engine import VisualEngine
        # the frozen tower's packing (~1.2 GB in fp32, plus its transposes once training has
        # begun) is keyed on image_encoder alone; a changed image_adapter (load_state_dict, an
        # optimizer step) only re-binds the adapter weights (VisualEngine.set_adapter)
        sig = (param_signature(self.image_encoder), tuple(self.levels), self.image_adapt_until, self.i_w,
               self.compute_dtype)
        asig = param_signature(self.image_adapter)
        if self._vis is None or self._vis_sig != sig:
            vp = {"visual." + k: v for k, v in self.image_encoder.state_dict().items()}
            self._vis = VisualEngine(vp, self.image_adapter.state_dict(), levels=self.levels,
                                     image_adapt_until=self.image_adapt_until, image_adapt_weight=self.i_w,
                                     dtype=self.compute_dtype,
                                     quick_gelu=self.image_encoder.transformer.quick_gelu)
            self._vis_sig, self._vis_asig = sig, asig
        elif self._vis_asig != asig:
            self._vis.set_adapter(self.image_adapter.state_dict())
            self._vis_asig = asig
        return self._vis

    # ------------------------------------------------------------------ API
    def forward_original(self, x, modality="visual"):
        """([patch features [B, P, 768]], cls [B, 768]) of the un-adapted CLIP tower, fp32."""
        if modality != "visual":
            raise ValueError("modality must be visual")
        # reference model/adapter.py:55-63: encode_image(x, [24]), then ln_post and proj of the
        # patch tokens; the frozen engine (following a DAPM_replace made on clipmodel.visual)
        # taps and projects them itself, in self.compute_dtype
        eng = self.clipmodel.visual.frozen_engine(self.compute_dtype)
        cls_features, _ = eng.encode(x, [], patch_features=True)
        return [eng.patch_features()], cls_features

    def _adapter_weights(self):
        ad = self.image_adapter
        return ([m.fc[0].weight for m in ad["layer_adapters"]] + [m.weight for m in ad["seg_proj"]]
                + [ad["det_proj"].weight])

    def forward(self, x):
        """(list[len(levels)] of [B, P, 768] unit-norm patch features, det [B, 768]).

        Stage 2 (reference train.py:117-174): with grad mode on, compute_dtype float32 and at
        least one image_adapter weight requiring grad, the same tensors come back with a grad_fn
        into the image adapter weights, read live (VisualEngine.forward_train: the same launches
        and bits, activations kept for the HIP backward; one chunk). So they do in bf16 mixed
        precision, for a model built with compute_dtype == train_dtype == bfloat16. Every other
        call -- no_grad, a frozen image adapter, the 16-bit and fp8 modes without train_dtype even
        under grad -- is the forward-only path, unchanged."""
        eng = self.visual_engine()
        trains = self.compute_dtype == torch.float32 or (
            self.train_dtype == torch.bfloat16 and self.compute_dtype == torch.bfloat16)
        if torch.is_grad_enabled() and trains:
            weights = self._adapter_weights()
            if any(w.requires_grad for w in weights):
                return eng.forward_train(x, weights)
        return eng.forward(x)

    def predict(self, x, text_features, domain="Industrial", streams=1):
        """Fused test path (test.py:80-93): (anomaly map [B,S,S], image score [B]), fp32.
        streams > 1 (or a tuple of chunk sizes) runs image chunks on that many HIP
        streams (VisualEngine.predict); per-image results do not depend on it. A shape seen
        before replays a captured hipGraph of the step (VisualEngine.predict_cached).
        The outputs are engine-owned buffers: clone them to keep them (test.py does)."""
        return self.visual_engine().predict_cached(x, text_features, domain, streams=streams)

    def predict_tiled(self, canvas, text_features, grid, overlap, domain="Industrial", global_view=None,
                      global_weight=0.5, streams=1, tile_batch=32):
        """Sliding-window test path at the native scale (no reference counterpart): canvas
        [B, 3, C, C] is cut into grid x grid tiles of the tower's image size S overlapping by
        `overlap` pixels (C = grid S - (grid - 1) overlap), each tile runs through predict, and the
        tile maps are stitched on the device with linear ramps across the overlaps. Returns
        (anomaly map [B, C, C], image score [B]), fp32, fresh tensors: the map mixed with the
        bilinearly upsampled map of global_view [B, 3, S, S] (the whole photo at S) by
        global_weight in [0, 1), the score the tiles' maximum mixed with the global view's score
        the same way; global_weight 0 runs no global forward. tile_batch tiles run per predict
        call; results do not depend on it, on B or on streams (VisualEngine.predict_tiled)."""
        return self.visual_engine().predict_tiled(canvas, text_features, grid, overlap, domain, global_view,
                                                  global_weight, streams, tile_batch)

    def build_memory_bank(self, images, search_dtype=None, coreset=None):
        """The few-shot memory bank of a class from its normal support images [k, 3, S, S]
        (reference test.py:39-50, get_support_features): VisualEngine.build_bank. search_dtype
        torch.float8_e4m3fn keeps the bank in MX fp8 for the block-scaled fp8 search; coreset, a
        ratio in (0, 1), keeps per level only that share of the rows, a greedy k-centre coreset."""
        return self.visual_engine().build_bank(images, search_dtype, coreset)

    def predict_few_shot(self, x, text_features, bank, domain="Industrial"):
        """(zero-shot map [B,S,S], zero-shot score [B], few-shot map [B,S,S]), fp32, fresh tensors:
        predict()'s map and score, and each patch's distance to its nearest bank patch summed over the
        levels, blurred and upsampled (VisualEngine.predict_few_shot). A bank built at another
        image size or search dtype raises ValueError."""
        return self.visual_engine().predict_few_shot(x, text_features, bank, domain)

    def encode_text(self, text, adapt_text=True):
        if not adapt_text:
            return self.clipmodel.encode_text(text)
        eng = self.clipmodel.text_engine(self.text_adapter.state_dict(), self.text_adapt_until, self.t_w)
        # stage 1 (reference train.py:38-114): with grad enabled and a trainable text adapter the
        # result has a grad_fn into the adapter weights, read live (TextEngine.encode_train: the
        # same launches and bits, activations kept for the HIP backward). Every other call is
        # the forward-only path.
        weights = [m.fc[0].weight for m in self.text_adapter]
        if torch.is_grad_enabled() and any(w.requires_grad for w in weights):
            return eng.encode_train(text, weights)
        return eng.encode(text)
