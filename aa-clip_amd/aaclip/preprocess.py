"""Device test-time preprocessing — drop-in for the reference's per-item
transforms (dataset/__init__.py:127-143: transform_x = Resize((S,S), BICUBIC)
-> ToTensor -> Normalize(CLIP mean/std); transform_mask = Resize((S,S),
NEAREST) -> ToTensor, then `(mask != 0).float()` at :158).

Decoded uint8 images go to HBM as they are (HWC RGB / L) and one kernel per
batch resamples + normalises them (aaclip_preprocess_images), bit-exact with
Pillow's 8-bit resampling, so the maps downstream are identical to the
reference's CPU-worker path. Plans (per-axis tap tables) are built on the host
by the C ABI in Pillow's double-precision arithmetic and cached per source size.

TrainPreprocessor is the train split's counterpart (reference dataset/__init__.py:30-63,
89-94): colour jitter on the uint8 source (aaclip_color_jitter_u8, bit-exact with Pillow's
ImageEnhance), the same bicubic / nearest kernels, then rotation, translation and the two
flips of image + mask as one gather (aaclip_geom_augment). The random parameters are drawn
on the host (`sample`) and can be replayed on the Pillow / grid_sample path of the dataset
workers (`cpu_item`), which is what the tests compare the kernels with.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from ._lib import call
from .ops import _dev, _ptr, _stream

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def bicubic_plan(in_size: int, out_size: int):
    """Pillow BICUBIC tables for one axis: bounds int32 [out, 2] = (first tap, taps),
    coeffs int32 [out, ksize] (22 fraction bits). Host only."""
    k = ctypes.c_int()
    call("aaclip_bicubic_taps", in_size, out_size, ctypes.byref(k))
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, k.value), np.int32)
    call("aaclip_bicubic_plan", in_size, out_size, bounds.ctypes.data_as(ctypes.c_void_p),
         coeffs.ctypes.data_as(ctypes.c_void_p), k.value)
    return bounds, coeffs


def nearest_plan(in_size: int, out_size: int) -> np.ndarray:
    idx = np.zeros(out_size, np.int32)
    call("aaclip_nearest_plan", in_size, out_size, idx.ctypes.data_as(ctypes.c_void_p))
    return idx


class Preprocessor:
    """`images(u8 [B,H,W,3]) -> fp32 [B,3,S,S]`, `masks(u8 [B,H,W]) -> fp32 [B,1,S,S]`
    on the device of the inputs, on torch's current stream."""

    def __init__(self, img_size: int, mean=CLIP_MEAN, std=CLIP_STD):
        self.S = int(img_size)
        self._ms = (ctypes.c_float * 6)(*mean, *std)
        self._plans: dict = {}

    def _bicubic(self, n: int, dev):
        key = ("b", n, dev)
        if key not in self._plans:
            b, k = bicubic_plan(n, self.S)
            self._plans[key] = (torch.from_numpy(b).to(dev), torch.from_numpy(k).to(dev), k.shape[1])
        return self._plans[key]

    def _nearest(self, n: int, dev):
        key = ("n", n, dev)
        if key not in self._plans:
            self._plans[key] = torch.from_numpy(nearest_plan(n, self.S)).to(dev)
        return self._plans[key]

    @staticmethod
    def _check_u8(x: torch.Tensor, channels: int):
        _dev(x)
        if x.dtype != torch.uint8:
            raise TypeError("preprocess inputs are decoded uint8 images")
        if channels == 3:
            if x.dim() != 4 or x.shape[-1] != 3:
                raise ValueError(f"expected uint8 [B,H,W,3], got {tuple(x.shape)}")
            dense = x.stride(3) == 1 and x.stride(2) == 3
        else:
            if x.dim() != 3:
                raise ValueError(f"expected uint8 [B,H,W], got {tuple(x.shape)}")
            dense = x.stride(2) == 1
        if not dense or x.shape[0] > 65535:
            raise ValueError("pixel rows must be contiguous (row pitch may be padded); batch <= 65535")

    def _workspace(self, B, H, W, dev):
        n = ctypes.c_size_t()
        call("aaclip_preprocess_workspace", B, H, W, self.S, ctypes.byref(n))
        ws = self._plans.get(("ws", dev))
        if ws is None or ws.numel() < n.value:
            ws = torch.empty(max(n.value, 1), device=dev, dtype=torch.uint8)
            self._plans[("ws", dev)] = ws
        return ws, n.value

    def images(self, u8: torch.Tensor, out: torch.Tensor | None = None, two_pass: bool = True) -> torch.Tensor:
        """two_pass: horizontal pass into a uint8 intermediate (a cached workspace), then
        the vertical pass (default, faster); False = one tiled kernel, no workspace."""
        self._check_u8(u8, 3)
        B, H, W, _ = u8.shape
        dev = u8.device
        xb, xk, kx = self._bicubic(W, dev)
        yb, yk, ky = self._bicubic(H, dev)
        if out is None:
            out = torch.empty(B, 3, self.S, self.S, device=dev, dtype=torch.float32)
        if out.shape != (B, 3, self.S, self.S) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be contiguous fp32 [B,3,S,S]")
        ws, nbytes = self._workspace(B, H, W, dev) if two_pass else (None, 0)
        call("aaclip_preprocess_images", _ptr(u8), u8.stride(0), u8.stride(1), B, H, W, _ptr(xb), _ptr(xk), kx,
             _ptr(yb), _ptr(yk), ky, self.S, ctypes.cast(self._ms, ctypes.c_void_p), _ptr(out), _ptr(ws), nbytes,
             _stream())
        return out

    def masks(self, u8: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        self._check_u8(u8, 1)
        B, H, W = u8.shape
        dev = u8.device
        if out is None:
            out = torch.empty(B, 1, self.S, self.S, device=dev, dtype=torch.float32)
        if out.shape != (B, 1, self.S, self.S) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be contiguous fp32 [B,1,S,S]")
        call("aaclip_resize_masks_nearest", _ptr(u8), u8.stride(0), u8.stride(1), B, H, W,
             _ptr(self._nearest(W, dev)), _ptr(self._nearest(H, dev)), self.S, _ptr(out), _stream())
        return out


# columns of the uniform draws of TrainPreprocessor.sample, one row per image
_DRAWS = ("brightness_p", "brightness", "contrast_p", "contrast", "saturation_p", "saturation",
          "rotate_p", "angle", "translate_p", "tx", "ty", "hflip_p", "vflip_p")


def rotation_grid(S: int, cos_r, sin_r, dtype=torch.float32) -> torch.Tensor:
    """The sampling grid [1, S, S, 2] of torchvision's tensor rotate (_gen_affine_grid with the
    matrix of _get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1, [0, 0]) = [[c, s], [-s, c]],
    c = cos r, s = sin r, r = radians(-angle)), for F.grid_sample(align_corners=False). The
    formula is include/aaclip.h's (aaclip_geom_augment), evaluated in `dtype`."""
    c, s = torch.tensor(cos_r, dtype=dtype), torch.tensor(sin_r, dtype=dtype)
    half = 0.5 * S
    base = torch.arange(S, dtype=dtype) + 0.5 - half
    xb, yb = base[None, :], base[:, None]
    gx = xb * (c / half) + yb * (s / half)
    gy = xb * (-s / half) + yb * (c / half)
    return torch.stack([gx, gy], dim=-1)[None]


def geom_cpu(x: torch.Tensor, rotate: bool, cos_r: float, sin_r: float, tx: int, ty: int, hflip: bool,
             vflip: bool) -> torch.Tensor:
    """The four geometric transforms of the reference's train items, one after another, on a CPU
    tensor [C, S, S] (fp32 or fp64): rotation through F.grid_sample (nearest, zeros), the
    translation as the zero-filled shift it is (the sources are pixel centres), then the flips."""
    S = x.shape[-1]
    if rotate:
        x = torch.nn.functional.grid_sample(x[None], rotation_grid(S, cos_r, sin_r, x.dtype), mode="nearest",
                                            padding_mode="zeros", align_corners=False)[0]
    if tx or ty:
        y = torch.zeros_like(x)
        if abs(tx) < S and abs(ty) < S:
            y[:, max(ty, 0):S + min(ty, 0), max(tx, 0):S + min(tx, 0)] = \
                x[:, max(-ty, 0):S + min(-ty, 0), max(-tx, 0):S + min(-tx, 0)]
        x = y
    if hflip:
        x = torch.flip(x, (-1,))
    if vflip:
        x = torch.flip(x, (-2,))
    return x


class TrainPreprocessor(Preprocessor):
    """The train split's transforms on the device. `sample(B, generator)` draws the per-image
    parameters on the host; `apply(image_u8, mask_u8, params)` runs jitter -> bicubic + normalise
    -> nearest mask -> one geometric gather over both. text=True (stage 1's dataset) draws no
    colour jitter: the three factors are 1.0."""

    def __init__(self, img_size: int, text: bool = False, mean=CLIP_MEAN, std=CLIP_STD):
        super().__init__(img_size, mean, std)
        self.text = bool(text)

    def sample(self, B: int, generator: torch.Generator) -> dict:
        """Per-image parameters as CPU tensors. ONE torch.rand(B, 13, generator) call, columns in
        the order of _DRAWS: for each of brightness, contrast, saturation an apply draw (< 0.7) and
        a factor 0.5 + u; rotation apply (< 0.5) and angle = -30 + 60 u degrees; translation apply
        (< 0.5), tx = int(round((2 u - 1) * 0.15 S)), ty likewise; hflip, vflip (< 0.5). The same
        columns are drawn with text=True (the factors are then 1.0), so one seed gives the text and
        the image dataset the same geometry."""
        u = torch.rand(B, len(_DRAWS), generator=generator, dtype=torch.float64)
        col = {n: u[:, i] for i, n in enumerate(_DRAWS)}
        color = torch.ones(B, 3, dtype=torch.float32)
        if not self.text:
            for k, n in enumerate(("brightness", "contrast", "saturation")):
                color[:, k] = torch.where(col[n + "_p"] < 0.7, 0.5 + col[n], torch.ones(B, dtype=torch.float64)).float()
        rotate = col["rotate_p"] < 0.5
        angle = torch.where(rotate, -30.0 + 60.0 * col["angle"], torch.zeros(B, dtype=torch.float64))
        r = [math.radians(-a) for a in angle.tolist()]
        cos_sin = torch.tensor([[math.cos(v), math.sin(v)] for v in r], dtype=torch.float64).reshape(B, 2).float()
        move = col["translate_p"] < 0.5
        m = 0.15 * self.S
        shift = torch.tensor([[int(round((2 * a - 1) * m)) if on else 0, int(round((2 * b - 1) * m)) if on else 0]
                              for a, b, on in zip(col["tx"].tolist(), col["ty"].tolist(), move.tolist())],
                             dtype=torch.int32).reshape(B, 2)
        return {"color": color, "rotate": rotate, "angle": angle, "cos_sin": cos_sin, "shift": shift,
                "hflip": col["hflip_p"] < 0.5, "vflip": col["vflip_p"] < 0.5}

    # ------------------------------------------------------------------ device path
    def jitter(self, u8: torch.Tensor, color: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """aaclip_color_jitter_u8 on uint8 [B,H,W,3]; color: CPU fp32 [B,3]. out=u8 runs in place."""
        self._check_u8(u8, 3)
        B, H, W, _ = u8.shape
        if out is None:
            out = torch.empty_strided(u8.shape, u8.stride(), device=u8.device, dtype=torch.uint8)
        if out.shape != u8.shape or out.stride() != u8.stride() or out.dtype != torch.uint8 or out.device != u8.device:
            raise ValueError("out must have the input's shape, strides and device")
        f = np.ascontiguousarray(color.detach().cpu().numpy(), dtype=np.float32)
        if f.shape != (B, 3):
            raise ValueError(f"colour factors must be [B, 3], got {f.shape}")
        n = ctypes.c_size_t()
        call("aaclip_color_jitter_workspace", B, ctypes.byref(n))
        ws = self._plans.get(("jws", u8.device))
        if ws is None or ws.numel() * 8 < n.value:
            ws = torch.empty(n.value // 8, device=u8.device, dtype=torch.int64)
            self._plans[("jws", u8.device)] = ws
        call("aaclip_color_jitter_u8", _ptr(u8), u8.stride(0), u8.stride(1), B, H, W,
             f.ctypes.data_as(ctypes.c_void_p), _ptr(out), _ptr(ws), ws.numel() * 8, _stream())
        return out

    @staticmethod
    def geom_params(params: dict, lo: int = 0, hi: int | None = None):
        """(int32 [n,5] rotate, tx, ty, hflip, vflip; fp32 [n,2] cos, sin) host arrays of images lo..hi."""
        sl = slice(lo, hi)
        p = torch.stack([params["rotate"][sl].int(), params["shift"][sl, 0].int(), params["shift"][sl, 1].int(),
                         params["hflip"][sl].int(), params["vflip"][sl].int()], dim=1)
        return (np.ascontiguousarray(p.numpy(), dtype=np.int32),
                np.ascontiguousarray(params["cos_sin"][sl].numpy(), dtype=np.float32))

    def geom(self, x: torch.Tensor, params: dict, x2: torch.Tensor | None = None):
        """aaclip_geom_augment on fp32 [B,C,S,S] (and, through the same map, x2 [B,C2,S,S])."""
        _dev(x)
        if x.dim() != 4 or x.shape[2] != x.shape[3] or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("expected contiguous fp32 [B,C,S,S]")
        B, C, S, _ = x.shape
        out, out2, C2 = torch.empty_like(x), None, 0
        if x2 is not None:
            if x2.dim() != 4 or x2.shape[0] != B or tuple(x2.shape[2:]) != (S, S) or x2.dtype != torch.float32 \
                    or not x2.is_contiguous() or x2.device != x.device:
                raise ValueError("x2 must be contiguous fp32 [B,C2,S,S] on the device of x")
            out2, C2 = torch.empty_like(x2), x2.shape[1]
        ip, cs = self.geom_params(params)
        if ip.shape[0] != B:
            raise ValueError(f"{ip.shape[0]} parameter sets for {B} images")
        call("aaclip_geom_augment", _ptr(x), _ptr(x2), _ptr(out), _ptr(out2), B, C, C2, S,
             ip.ctypes.data_as(ctypes.c_void_p), cs.ctypes.data_as(ctypes.c_void_p), _stream())
        return out if x2 is None else (out, out2)

    def apply(self, image_u8, mask_u8, params: dict):
        """(image fp32 [B,3,S,S], mask fp32 [B,1,S,S]) on the inputs' device and torch's current
        stream. image_u8 / mask_u8: uint8 [B,H,W,3] / [B,H,W] device tensors, or lists of
        [H,W,3] / [H,W] of differing source sizes (one jitter + resize launch per image, as
        test.py's _device_batch does; the geometric launch is one either way). The inputs are
        not modified."""
        if isinstance(image_u8, torch.Tensor):
            img = self.images(self.jitter(image_u8, params["color"]))
            mask = self.masks(mask_u8)
        else:
            B = len(image_u8)
            img = torch.empty(B, 3, self.S, self.S, device=image_u8[0].device, dtype=torch.float32)
            mask = torch.empty(B, 1, self.S, self.S, device=image_u8[0].device, dtype=torch.float32)
            for b in range(B):
                self.images(self.jitter(image_u8[b][None], params["color"][b:b + 1]), out=img[b:b + 1])
                self.masks(mask_u8[b][None], out=mask[b:b + 1])
        return self.geom(img, params, mask)

    # ------------------------------------------------------------------ host path (loader workers)
    def cpu_item(self, image, mask, params: dict, b: int = 0):
        """The same item on the CPU, as the reference's workers make it: Pillow's ImageEnhance on
        the PIL RGB `image`, Pillow's bicubic resize, normalise; the mask (PIL L, or None) through
        Pillow's nearest resize and != 0; then geom_cpu on the 4-channel cat. Parameters: image b
        of `params`."""
        from PIL import Image, ImageEnhance
        for enh, f in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color),
                          params["color"][b].tolist()):
            if f != 1.0:
                image = enh(image).enhance(f)
        a = np.asarray(image.resize((self.S, self.S), Image.BICUBIC), dtype=np.float32).transpose(2, 0, 1) / 255.0
        ms = np.array(list(self._ms), np.float32)
        img = torch.from_numpy((a - ms[:3, None, None]) / ms[3:, None, None])
        if mask is None:
            m = torch.zeros(1, self.S, self.S)
        else:
            m = torch.from_numpy((np.asarray(mask.resize((self.S, self.S), Image.NEAREST)) != 0).astype(np.float32))[None]
        c, s = params["cos_sin"][b].tolist()
        t = geom_cpu(torch.cat([img, m], 0), bool(params["rotate"][b]), c, s, int(params["shift"][b, 0]),
                     int(params["shift"][b, 1]), bool(params["hflip"][b]), bool(params["vflip"][b]))
        return t[0:3], t[3:4]
