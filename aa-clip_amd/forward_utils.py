"""Drop-in for the reference forward_utils.py entry points of the eval path.

  get_adapted_single_class_text_embedding / get_adapted_text_embedding
      forward_utils.py:138-162, :185-192 — prompt ensemble -> T [768, 2]; the
      encoder runs on the HIP text engine, the normalise/mean/normalise
      reduction in the aaclip_anchor_reduce kernel.
  calculate_similarity_map   forward_utils.py:196-216 — aaclip_patch_scores +
      aaclip_blur_upsample (test: (A1+1-A0)/2 -> Gaussian -> bilinear;
      train: bilinear -> softmax over the two anchors). The train branch also takes
      the per-image [B, 768, Cn] anchors of train.py:69-72 and, for two anchors,
      carries a backward to the anchors and the patch features
      (aaclip_upsample_softmax_bwd -> aaclip_patch_logits_bwd).
  calculate_seg_loss         forward_utils.py:219-227 — FocalLoss() + the two
      BinaryDiceLoss() terms in aaclip_seg_loss, backward in aaclip_seg_loss_bwd.
      With the map above this is train.py:86-100 from the anchors / features down
      to loss.backward(). With grad enabled and a trainable text_adapter,
      get_adapted_single_class_text_embedding's anchors carry a grad_fn through
      aaclip_anchor_reduce_bwd and the text tower's backward (TextEngine.encode_train)
      into the four text_adapter weights: train.py:62-72, :87-100 runs as written.
      Stage 2's backward into the image adapter is AdaptedCLIP.forward under grad.
  anomaly_map_multilevel     the fused form of test.py:86-93 (all levels in one
      stream kernel, level sum before blur+upsample).
  metrics_eval               forward_utils.py:233-280 — on device (aaclip_metrics_eval:
      min-max normalisation, score fusion, radix-sorted exact tie-aware AUROC / AP,
      identical to sklearn after the reference's 4-decimal rounding). numpy inputs
      are copied to the device; there is no CPU path (without a GPU it raises).
      pro=True adds the pixel AUPRO (aaclip_metrics_eval_pro), which the reference lacks;
      f1=True adds pixel and image F1-max and their thresholds (aaclip_metrics_eval_f1).
  anomaly_regions            a threshold applied to a class's maps, as data (aaclip_extract_regions):
      per image the 8-connected regions at or above it with area, bbox, centroid, peak and
      ground-truth overlap.
  visualize                  forward_utils.py:283-327 without cv2 — the three-panel overlays (photo, ground
      truth over photo, prediction over photo) rendered on the device: aaclip_resize_bilinear_u8
      (8-bit fixed-point bilinear), aaclip_overlay_range, aaclip_overlay_panels (quantise, jet
      ramp, integer blend, stack), encoded with Pillow on a small thread pool. The recipe is this
      build's own statement of what the reference asks of cv2 (include/aaclip.h,
      tests/visualize_ref.py); equality with an OpenCV build's bytes is not claimed.
FocalLoss / BinaryDiceLoss as classes with non-default arguments are out of scope.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from aaclip import ops
from aaclip.engine import _blur_for
from dataset.constants import CLASS_NAMES, DATA_PATH, PROMPTS, REAL_NAMES
from model.tokenizer import tokenize

prompt = PROMPTS
prompt_normal = prompt["prompt_normal"]
prompt_abnormal = prompt["prompt_abnormal"]
prompt_state = [prompt_normal, prompt_abnormal]
prompt_templates = prompt["prompt_templates"]


def _sentences(real_name):
    out = []
    for states in prompt_state:
        out.append([tpl.format(s.format(real_name)) for s in states for tpl in prompt_templates])
    return out


def get_adapted_single_class_text_embedding(model, dataset_name, class_name, device):
    if class_name == "object":
        real_name = class_name
    else:
        assert class_name in CLASS_NAMES[dataset_name], (
            f"class_name {class_name} not found; available class_names: {CLASS_NAMES[dataset_name]}")
        real_name = REAL_NAMES[dataset_name][class_name]
    device = torch.device(device)
    T = None
    cols = []
    for col, sentences in enumerate(_sentences(real_name)):
        emb = model.encode_text(tokenize(sentences).to(device))
        if torch.is_grad_enabled() and emb.requires_grad:
            # stage 1 (train.py:62-72): the same anchor kernel per column, with a backward to
            # the embeddings (aaclip_anchor_reduce_bwd) and on into the text adapter
            cols.append(ops.anchor_column(emb))
            continue
        emb = emb.to(torch.float32).contiguous()
        if T is None:
            T = torch.empty(emb.shape[1], 2, device=emb.device, dtype=torch.float32)
        ops.anchor_reduce(emb, T, col)
    if cols:
        T = torch.stack(cols, dim=1)
    return T.to(device)


def get_adapted_text_embedding(model, dataset_name, device):
    """forward_utils.py:185-192. Same result as one
    get_adapted_single_class_text_embedding per class, but every prompt of every
    class goes through the text tower in ONE encode call (MVTec: 240 sequences =
    18480 token rows, instead of 30 calls of 6-10 sequences that leave the GEMMs
    a few hundred rows): prompts are independent sequences and each one's
    encoding is bit-identical whatever batch it is in
    (tests/test_e2e_gpu.py::test_text_encode_sequence_invariance), so the
    anchors are unchanged."""
    device = torch.device(device)
    sentences, spans = [], []
    for c in CLASS_NAMES[dataset_name]:
        real_name = c if c == "object" else REAL_NAMES[dataset_name][c]
        for col, sents in enumerate(_sentences(real_name)):
            spans.append((c, col, len(sentences), len(sentences) + len(sents)))
            sentences.extend(sents)
    emb = model.encode_text(tokenize(sentences).to(device)).to(torch.float32).contiguous()
    out = {}
    for c, col, a, b in spans:
        if c not in out:
            out[c] = torch.empty(emb.shape[1], 2, device=emb.device, dtype=torch.float32)
        ops.anchor_reduce(emb[a:b], out[c], col)
    return {c: T.to(device) for c, T in out.items()}


class _TrainMap(torch.autograd.Function):
    """Two-anchor train-branch map with a backward: grads flow to the patch features and /
    or the anchors, whichever need them (aaclip_upsample_softmax_bwd -> aaclip_patch_logits_bwd)."""

    @staticmethod
    def forward(ctx, patch_features, epoch_text_feature, f, T, B, L, img_size):
        H = int(np.sqrt(L))
        grid = torch.empty(B, 2, H, H, device=f.device, dtype=torch.float32)
        _train_logits(f, T, grid, L)
        out = torch.empty(B, 2, img_size, img_size, device=f.device, dtype=torch.float32)
        ops.blur_upsample(grid, out, ksize=0, sigma=0.0, softmax=True)
        ctx.save_for_backward(f, T, grid)
        ctx.L = L
        ctx.f_meta = (patch_features.shape, patch_features.dtype)
        ctx.t_meta = (epoch_text_feature.shape, epoch_text_feature.dtype, epoch_text_feature.device)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        f, T, grid = ctx.saved_tensors
        need_df, need_dT = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        with torch.cuda.device(f.device):
            dgrid = ops.upsample_softmax_bwd(grid, dout.to(torch.float32).contiguous())
            dT, df = ops.patch_logits_bwd(f, T, dgrid, group=ctx.L, need_dT=need_dT, need_df=need_df)
        if df is not None:
            df = df.reshape(ctx.f_meta[0]).to(ctx.f_meta[1])
        if dT is not None:
            dT = dT.reshape(ctx.t_meta[0]).to(device=ctx.t_meta[2], dtype=ctx.t_meta[1])
        return df, dT, None, None, None, None, None


def _train_logits(f, T, grid, L):
    """The train-branch logits launch: a shared anchor pair goes through patch_scores (mode 1),
    any other shared count through patch_logits, per-image anchors through
    patch_logits_per_image."""
    if T.dim() == 3:
        ops.patch_logits_per_image(f, T, grid, group=L)
    elif T.shape[1] == 2:
        ops.patch_scores([f], T, grid, normalize=False, mode=1, group=L)
    else:  # any anchor count (reference forward_utils.py:199-215 handles every C)
        ops.patch_logits(f, T, grid, group=L)


def calculate_similarity_map(patch_features, epoch_text_feature, img_size, test=False, domain="Medical"):
    """[B, L, C] features x [C, 2] anchors -> [B, 1, S, S] (test) / [B, 2, S, S] (train).
    The train branch also takes per-image anchors [B, C, Cn] (train.py:69-72); with two
    anchors and a grad-requiring input its result has a backward."""
    B, L, C = patch_features.shape
    H = int(np.sqrt(L))
    if H * H != L:
        raise ValueError("patch count must be a square")
    if epoch_text_feature.dim() not in (2, 3) or (test and epoch_text_feature.dim() != 2):
        raise ValueError("anchors must be [C, Cn]" + ("" if test else " or per image [B, C, Cn]"))
    if epoch_text_feature.dim() == 3 and epoch_text_feature.shape[0] != B:
        raise ValueError(f"per-image anchors need one set per image: got {epoch_text_feature.shape[0]} for {B}")
    Cn = epoch_text_feature.shape[-1]
    if test:
        assert Cn == 2
    elif not 1 <= Cn <= 8:  # checked before any launch: the train-branch upsample holds <= 8 channels per pixel
        raise ValueError(f"train-branch similarity map supports 1..8 anchors, got {Cn}")
    wants_grad = not test and torch.is_grad_enabled() and (patch_features.requires_grad
                                                           or epoch_text_feature.requires_grad)
    if wants_grad and Cn != 2:
        raise NotImplementedError(f"the train-branch backward is written for 2 anchors, got {Cn}")
    f = patch_features.detach().reshape(B * L, C)
    if f.dtype not in (torch.float32, torch.bfloat16):
        f = f.float()
    f = f.contiguous()
    T = epoch_text_feature.detach().to(f.device, torch.float32).contiguous()
    dev = f.device
    if test:
        grid = torch.empty(B, 1, H, H, device=dev, dtype=torch.float32)
        ops.patch_scores([f], T, grid, normalize=False, mode=0)
        k, s = _blur_for(domain)
        out = torch.empty(B, 1, img_size, img_size, device=dev, dtype=torch.float32)
        return ops.blur_upsample(grid, out, ksize=k, sigma=s)
    if wants_grad:
        return _TrainMap.apply(patch_features, epoch_text_feature, f, T, B, L, img_size)
    grid = torch.empty(B, Cn, H, H, device=dev, dtype=torch.float32)
    _train_logits(f, T, grid, L)
    out = torch.empty(B, Cn, img_size, img_size, device=dev, dtype=torch.float32)
    return ops.blur_upsample(grid, out, ksize=0, sigma=0.0, softmax=Cn > 1)


class _SegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, patch_preds, probs, mask):
        sums, loss = ops.seg_loss(probs, mask)
        ctx.save_for_backward(probs, mask, sums)
        ctx.meta = (patch_preds.shape, patch_preds.dtype)
        return loss[3].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        probs, mask, sums = ctx.saved_tensors
        with torch.cuda.device(probs.device):
            dloss = dloss.to(probs.device, torch.float32).reshape(1).contiguous()
            dprobs = ops.seg_loss_bwd(probs, mask, sums, dloss)
        return dprobs.reshape(ctx.meta[0]).to(ctx.meta[1]), None, None


def calculate_seg_loss(patch_preds, mask):
    """forward_utils.py:219-227: FocalLoss()(patch_preds, mask) + BinaryDiceLoss()(patch_preds[:, 0],
    1 - mask) + BinaryDiceLoss()(patch_preds[:, 1], mask) as one device pass (aaclip_seg_loss), with
    a backward to patch_preds (aaclip_seg_loss_bwd). patch_preds [B, 2, S, S]; mask [B, 1, S, S] or
    [B, S, S], any float dtype, values in [0, 1] (outside that the reference's scatter_ raises; here
    it is undefined). Returns a 0-dim fp32 device tensor."""
    if patch_preds.dim() != 4 or patch_preds.shape[1] != 2 or patch_preds.shape[2] != patch_preds.shape[3]:
        raise ValueError("patch_preds must be [B, 2, S, S]")
    if not patch_preds.is_cuda:
        raise RuntimeError("calculate_seg_loss runs on the MI355X kernels (aaclip_seg_loss); it needs device "
                           "tensors and there is no CPU path")
    B, _, S, _ = patch_preds.shape
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if tuple(mask.shape) != (B, S, S) or not mask.is_floating_point():
        raise ValueError(f"mask must be a float [B, 1, S, S] or [B, S, S] matching patch_preds, got {tuple(mask.shape)}")
    mask = mask.detach().to(patch_preds.device, torch.float32).contiguous()
    probs = patch_preds.detach().to(torch.float32).contiguous()
    with torch.cuda.device(patch_preds.device):
        if torch.is_grad_enabled() and patch_preds.requires_grad:
            return _SegLoss.apply(patch_preds, probs, mask)
        return ops.seg_loss(probs, mask)[1][3].clone()


def anomaly_map_multilevel(patch_features, epoch_text_feature, img_size, domain="Industrial", normalize=False):
    """sum_l calculate_similarity_map(f_l, T, S, test=True, domain) -> [B, S, S] in one pass."""
    B, L, C = patch_features[0].shape
    g = int(np.sqrt(L))
    lv = [f.reshape(B * L, C).contiguous() for f in patch_features]
    T = epoch_text_feature.to(lv[0].device, torch.float32).contiguous()
    out = torch.empty(B, img_size, img_size, device=lv[0].device, dtype=torch.float32)
    grid = torch.empty(B * L, device=lv[0].device, dtype=torch.float32)
    k, s = _blur_for(domain)
    return ops.anomaly_map(lv, T, out, grid, g=g, ksize=k, sigma=s, normalize=normalize)


def metrics_eval(pixel_label, image_label, pixel_preds, image_preds, class_names: str, domain: str,
                 pro: bool = False, f1: bool = False):
    """forward_utils.py:233-280 on the device (aaclip_metrics_eval: class min-max, score
    fusion, exact tie-aware AUROC / AP). Tensors or numpy arrays; the rounding and the
    dict layout are the reference's. There is no CPU path: without a GPU this raises.
    pro=True adds "pixel AUPRO" (aaclip_metrics_eval_pro: the area under the per-region-overlap
    curve up to a false-positive rate of 0.3, over the 8-connected components of pixel_label),
    rounded like the other columns; pixel tensors are then [n, H, W] or [n, 1, H, W].
    f1=True adds "pixel F1-max" and "image F1-max" (aaclip_metrics_eval_f1: the maximum over the
    distinct scores t of 2 TP / (PP + P)), after "pixel AUPRO" when that is present and rounded
    like the other columns. The thresholds that reach them are in metrics_eval_deferred(...).values()."""
    return metrics_eval_deferred(pixel_label, image_label, pixel_preds, image_preds, class_names, domain, pro=pro,
                                 f1=f1)()


_F1_NAMES = [f"{level} F1{what}" for level in ("pixel", "image") for what in ("-max", " threshold", " precision",
                                                                             " recall")]


class _DeferredMetrics:
    """One class's metrics, enqueued on the device: call it for the reference's dict, or read
    values() for every computed number."""

    def __init__(self, res, class_names, pro, f1):
        self._res, self._class_names, self._pro, self._f1 = res, class_names, pro, f1

    def values(self):
        """Sync and return every computed number, unrounded (fractions, not per cent), by name:
        "pixel AUC", "pixel AP", "image AUC", "image AP", with pro "pixel AUPRO", with f1
        "pixel F1-max", "pixel F1 threshold", "pixel F1 precision", "pixel F1 recall" and the
        four "image F1 ..." counterparts. Thresholds are in the normalised score domains: the
        class min-max normalised map value (fp32; the raw value when the class maximum is 1) for
        pixels, the fused image score (the normalised map maximum for Medical, else the mean of
        that and the normalised image score) for images; a score >= threshold is a detection.
        The pixel numbers are NaN when pixel_label holds one class only."""
        names = ["pixel AUC", "pixel AP", "image AUC", "image AP"] + (["pixel AUPRO"] if self._pro else []) \
            + (_F1_NAMES if self._f1 else [])
        return dict(zip(names, self._res.tolist()))

    def __call__(self):
        v = self.values()
        if v["pixel AUC"] != v["pixel AUC"]:  # NaN: one pixel class only, sklearn raises here
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        out = {"class name": self._class_names}
        for k in ["pixel AUC", "pixel AP", "image AUC", "image AP"] + (["pixel AUPRO"] if self._pro else []) \
                + (["pixel F1-max", "image F1-max"] if self._f1 else []):
            out[k] = round(v[k], 4) * 100
        return out


def metrics_eval_deferred(pixel_label, image_label, pixel_preds, image_preds, class_names: str, domain: str,
                          pro: bool = False, f1: bool = False):
    """metrics_eval enqueued on the device now, read later: returns a callable that syncs
    and builds the reference's dict. The harness enqueues every class before reading any,
    so no class waits for the previous one's metrics on the host. The returned object also has
    .values(): every computed number unrounded, by name, among them with f1=True the F1
    thresholds, precisions and recalls (thresholds in the normalised score domains, see there)."""
    if not torch.cuda.is_available():
        raise RuntimeError("metrics_eval runs on the MI355X kernels (aaclip_metrics_eval); no GPU is visible "
                           "and there is no CPU path")
    dev = next((t.device for t in (pixel_preds, pixel_label) if isinstance(t, torch.Tensor) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    t = [x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
         for x in (pixel_preds, pixel_label, image_preds, image_label)]
    t = [x.to(dev, non_blocking=True) for x in t]
    res = ops.metrics_eval_device(t[0], t[1], t[2], t[3], medical=(domain == "Medical"), pro=pro, f1=f1)
    return _DeferredMetrics(res, class_names, pro, f1)


def anomaly_regions(pixel_preds, threshold, pixel_label=None, *, normalise=True, min_area=1, max_regions=64):
    """The defects of one class's maps as regions (aaclip_extract_regions): the 8-connected components
    of the pixels whose score reaches `threshold`, per image. With normalise=True the score is the
    class-normalised fp32 map value of metrics_eval, so the threshold may be the "pixel F1 threshold"
    of metrics_eval_deferred(..., f1=True).values(); with normalise=False it is the raw map value.
    Tensors or numpy arrays, [n, H, W] or [n, 1, H, W]; pixel_label (nonzero = anomalous) is optional.
    Syncs and returns one entry per image:
      {"n_regions": int, "regions": [{"label", "area", "bbox": [x0, y0, x1, y1], "centroid": [cx, cy],
                                      "peak", "peak_xy": [x, y], "gt_area"}, ...]}
    n_regions counts the regions of at least min_area pixels; "regions" holds the first max_regions of
    them by area descending, then label ascending (label = 1 + the smallest linear index y * W + x of
    the region; bbox inclusive; centroid in float64; peak the highest score and peak_xy the first pixel
    in row-major order that reaches it; gt_area the region's pixels with pixel_label != 0, 0 without
    one). There is no CPU path: without a GPU this raises."""
    if not torch.cuda.is_available():
        raise RuntimeError("anomaly_regions runs on the MI355X kernels (aaclip_extract_regions); no GPU is visible "
                           "and there is no CPU path")
    dev = next((t.device for t in (pixel_preds, pixel_label) if isinstance(t, torch.Tensor) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    preds, lab = [x if x is None or isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
                  for x in (pixel_preds, pixel_label)]
    preds = preds.to(dev, non_blocking=True)
    lab = None if lab is None else lab.to(dev, non_blocking=True)
    out = ops.extract_regions(preds, threshold, pixel_label=lab, normalise=normalise, min_area=min_area,
                              max_regions=max_regions)
    W = preds.shape[-1]
    out = {k: v.cpu().tolist() for k, v in out.items()}  # (the first copy syncs)
    images = []
    for i, count in enumerate(out["n_regions"]):
        if count == 0xFFFFFFFF:
            raise RuntimeError(f"aaclip_extract_regions: the component labelling of image {i} hit its loop cap")
        regions = [{"label": out["label"][i][j], "area": out["area"][i][j], "bbox": out["bbox"][i][j],
                    "centroid": out["centroid"][i][j], "peak": out["peak"][i][j],
                    "peak_xy": [out["peak_index"][i][j] % W, out["peak_index"][i][j] // W],
                    "gt_area": out["gt_area"][i][j]} for j in range(min(count, int(max_regions)))]
        images.append({"n_regions": count, "regions": regions})
    return images


_VIS_CHUNK = 32  # images rendered, copied and handed to the encoders at a time


def visualization_path(save_dir, dataset_name, class_name, file_name):
    """forward_utils.py:306, :316-317: save_dir/visualization/<dataset>/<class>/<damage>_<image name>,
    from the last two components of the file name. The reference raises for every dataset but
    MVTec; the same naming serves all of them here."""
    damage_name, image_name = file_name.split("/")[-2:]
    return os.path.join(save_dir, "visualization", dataset_name, class_name, f"{damage_name}_{image_name}")


def _thumbnails(sources, S, dev):
    """uint8 [h, w, 3] sources (numpy arrays or tensors) -> device uint8 [n, S, S, 3]: grouped by
    size, one aaclip_resize_bilinear_u8 launch per size and chunk."""
    srcs = [s if isinstance(s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s)) for s in sources]
    for s in srcs:
        if s.dtype != torch.uint8 or s.dim() != 3 or s.shape[2] != 3:
            raise ValueError(f"images must be uint8 [h, w, 3], got {s.dtype} {tuple(s.shape)}")
    out = torch.empty(len(srcs), S, S, 3, device=dev, dtype=torch.uint8)
    by_size = {}
    for i, s in enumerate(srcs):
        by_size.setdefault(tuple(s.shape), []).append(i)
    for idx in by_size.values():
        for a in range(0, len(idx), _VIS_CHUNK):
            part = idx[a:a + _VIS_CHUNK]
            batch = torch.stack([srcs[i] for i in part]).to(dev, non_blocking=True)
            out[torch.tensor(part, device=dev)] = ops.resize_bilinear_u8(batch, S)
    return out


def visualize(pixel_label, pixel_preds, file_names, save_dir, dataset_name, class_name, *, images=None,
              true_color=False, workers=4):
    """forward_utils.py:288-327 without cv2: per test image one picture of three panels stacked top
    to bottom (the photo, the ground truth over it, the prediction over it), rendered on the device
    (aaclip_resize_bilinear_u8, aaclip_overlay_range, aaclip_overlay_panels; the recipe is stated in
    include/aaclip.h and restated in numpy by tests/visualize_ref.py) and written with Pillow to
    visualization_path(...), at the source's extension. The first six arguments are the reference's;
    labels [n, 1, S, S] or [n, S, S] and maps [n, S, S] or [n, 1, S, S] may be numpy arrays or device
    tensors. images: the photos, as a list of uint8 [h, w, 3] RGB arrays or as a device uint8
    [n, S, S, 3] tensor of thumbnails already resized; without it the files are read from
    DATA_PATH[dataset_name] (Pillow, convert("RGB")). true_color=False keeps the reference's files,
    whose photo has red and blue exchanged under a true-coloured ramp (it blends an RGB photo with a
    BGR ramp and writes BGR); true_color=True writes the photo as it is. workers: encoder threads.
    Returns the written paths. There is no CPU path: without a GPU this raises."""
    if not torch.cuda.is_available():
        raise RuntimeError("visualize renders on the MI355X kernels (aaclip_overlay_panels); no GPU is visible "
                           "and there is no CPU path")
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image
    dev = next((t.device for t in (pixel_preds, pixel_label, images) if isinstance(t, torch.Tensor) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    preds, lab = [x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
                  for x in (pixel_preds, pixel_label)]
    preds = preds.to(dev, non_blocking=True)
    lab = lab.to(dev, non_blocking=True)
    if preds.dim() == 4 and preds.shape[1] == 1:
        preds = preds[:, 0]
    if preds.dim() != 3 or preds.shape[1] != preds.shape[2]:
        raise ValueError(f"pixel_preds must be [n, S, S] or [n, 1, S, S], got {tuple(preds.shape)}")
    n, S, _ = preds.shape
    if lab.numel() != preds.numel() or len(file_names) != n:
        raise ValueError(f"{n} maps of {S} x {S} need as many labels and file names, got {tuple(lab.shape)} and "
                         f"{len(file_names)}")
    lab = lab.reshape(n, S, S)
    paths = [visualization_path(save_dir, dataset_name, class_name, f) for f in file_names]
    if n == 0:
        return paths
    os.makedirs(os.path.dirname(paths[0]), exist_ok=True)
    preds = preds.to(torch.float32).contiguous()
    workers = max(1, int(workers))

    def load(file):
        with Image.open(os.path.join(DATA_PATH[dataset_name], file)) as im:
            return np.array(im.convert("RGB"))

    def save(array, path):
        Image.fromarray(array).save(path)

    with torch.cuda.device(dev), ThreadPoolExecutor(max_workers=workers) as pool:
        value_range = ops.overlay_range(preds)  # of the whole class, as the metrics take it
        thumbs = None
        if isinstance(images, torch.Tensor):
            if images.dtype != torch.uint8 or tuple(images.shape) != (n, S, S, 3):
                raise ValueError(f"a thumbnail tensor must be uint8 {(n, S, S, 3)}, got {tuple(images.shape)}")
            thumbs = images.to(dev)
        elif images is not None and len(images) != n:
            raise ValueError(f"{n} maps need {n} images, got {len(images)}")
        pinned = [torch.empty(min(n, _VIS_CHUNK), 3 * S, S, 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
        busy = [[], []]  # the encodes still reading each pinned buffer
        for k, a in enumerate(range(0, n, _VIS_CHUNK)):
            b = min(a + _VIS_CHUNK, n)
            if thumbs is not None:
                part = thumbs[a:b]
            else:
                part = _thumbnails(list(pool.map(load, file_names[a:b])) if images is None else images[a:b], S, dev)
            out = ops.overlay_panels(preds[a:b], part, labels=lab[a:b], value_range=value_range,
                                     swap_rb=not true_color)
            host = pinned[k % 2]
            for f in busy[k % 2]:
                f.result()
            host[:b - a].copy_(out, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            busy[k % 2] = [pool.submit(save, host[i].numpy(), paths[a + i]) for i in range(b - a)]
        for fs in busy:
            for f in fs:
                f.result()
    return paths
