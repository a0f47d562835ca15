"""Yardstick of the train-time augmentation (tests/test_augment_gpu.py, tests/test_augment_host.py).

Colour: Pillow's own ImageEnhance.Brightness / .Contrast / .Color, as torchvision's ColorJitter
calls them on a PIL image (reference dataset/__init__.py:44-52).
Geometry: the reference's four transforms (dataset/__init__.py:30-39) one after another, each a
nearest resample of its predecessor's result: rotation and translation through F.grid_sample with
torchvision's affine grid (_gen_affine_grid + _get_inverse_affine_matrix, transcribed in
include/aaclip.h), the flips through torch.flip; in fp32 (what the reference computes) or fp64.
Nothing here imports the product's code.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def jitter(img_u8: np.ndarray, factors) -> np.ndarray:
    """uint8 [H, W, 3], (brightness, contrast, saturation) fp32 values -> uint8 [H, W, 3] by Pillow.
    A factor of exactly 1.0 means the op is not applied."""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(img_u8), "RGB")
    for enh, f in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), factors):
        f = float(np.float32(f))
        if f != 1.0:
            im = enh(im).enhance(f)
    return np.asarray(im).copy()


def cos_sin(angle_deg: float):
    """(cos r, sin r) as the host's doubles, r = radians(-angle): what the device entry is given
    (rounded to fp32) and what the matrix of torchvision's tensor rotate holds."""
    r = math.radians(-angle_deg)
    return math.cos(r), math.sin(r)


def _affine_grid(S, m, dtype):
    """torchvision _gen_affine_grid for a square S: m = (m00, m01, m02, m10, m11, m12)."""
    half = 0.5 * S
    base = torch.arange(S, dtype=dtype) + 0.5 - half
    xb, yb = base[None, :], base[:, None]
    t = [torch.tensor(v, dtype=dtype) for v in m]
    gx = xb * (t[0] / half) + yb * (t[1] / half) + t[2] / half
    gy = xb * (t[3] / half) + yb * (t[4] / half) + t[5] / half
    return torch.stack([gx, gy], dim=-1)[None]


def source_coords(S, m, dtype=torch.float64):
    """Un-normalised source (x, y) [S, S] of grid_sample(align_corners=False) for the grid above."""
    g = _affine_grid(S, m, dtype)[0]
    return ((g[..., 0] + 1) * S - 1) / 2, ((g[..., 1] + 1) * S - 1) / 2


def rotate(x, angle_deg, dtype):
    """x [B, C, S, S] -> rotated by angle_deg (positive = counter-clockwise), nearest, fill 0."""
    c, s = cos_sin(angle_deg)
    c, s = float(np.float32(c)), float(np.float32(s))  # the device entry's fp32 inputs
    grid = _affine_grid(x.shape[-1], (c, s, 0.0, -s, c, 0.0), dtype).expand(x.shape[0], -1, -1, -1)
    return F.grid_sample(x.to(dtype), grid, mode="nearest", padding_mode="zeros", align_corners=False)


def translate(x, tx, ty, dtype):
    """torchvision affine(translate=(tx, ty)): the inverse matrix is [[1, 0, -tx], [0, 1, -ty]]."""
    grid = _affine_grid(x.shape[-1], (1.0, 0.0, -float(tx), 0.0, 1.0, -float(ty)), dtype).expand(x.shape[0], -1, -1,
                                                                                              -1)
    return F.grid_sample(x.to(dtype), grid, mode="nearest", padding_mode="zeros", align_corners=False)


def geom(x, rot, angle_deg, tx, ty, hflip, vflip, dtype=torch.float32):
    """One image [C, S, S] (CPU) through rotation -> translation -> hflip -> vflip, each applied only
    when its flag / value says so, as the reference's RandomApply chain does."""
    y = x[None].to(dtype)
    if rot:
        y = rotate(y, angle_deg, dtype)
    if tx or ty:
        y = translate(y, tx, ty, dtype)
    if hflip:
        y = torch.flip(y, (-1,))
    if vflip:
        y = torch.flip(y, (-2,))
    return y[0]


def tie_band(S, rot, angle_deg, tx, ty, hflip, vflip, eps=5e-4):
    """bool [S, S]: output pixels whose rotation source x or y, in fp64, lies within eps of a
    half-integer (where nearest rounding may legitimately differ between fp32 evaluations). The
    rotation is the first transform, so the band is computed on its output grid and carried
    through the later (exact) transforms like a channel."""
    if not rot:
        return torch.zeros(S, S, dtype=torch.bool)
    c, s = cos_sin(angle_deg)
    c, s = float(np.float32(c)), float(np.float32(s))
    xs, ys = source_coords(S, (c, s, 0.0, -s, c, 0.0))
    near = lambda v: ((v - torch.floor(v)) - 0.5).abs() <= eps  # noqa: E731
    band = (near(xs) | near(ys)).to(torch.float64)[None]
    out = geom(band, False, 0.0, tx, ty, hflip, vflip, torch.float64)
    return out[0] != 0
