"""The overlay recipe of forward_utils.visualize() restated in numpy: the contract the device
kernels of csrc/overlay.hip equal byte for byte (include/aaclip.h states the same arithmetic).

It is modelled on what the reference's visualize() asks of cv2 (a min-max quantisation, the jet
ramp, an 8-bit bilinear resize, a half-and-half blend, a stack), written out in full so that it
needs no cv2. cv2 is not available where this was written, so nothing here is claimed to equal an
OpenCV build's bytes; tests/test_visualize_host.py holds it to facts that can be checked."""
import os

import numpy as np


def resize_table(n_in, n_out):
    """Per-axis (s, a0, a1) int arrays of the 8-bit fixed-point bilinear resize."""
    d = np.arange(n_out, dtype=np.float64)
    scale = float(n_in) / float(n_out)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= n_in - 1
    s = np.where(low, 0, np.where(high, n_in - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return s, a0, a1


def resize(src, S):
    """uint8 [h, w, 3] -> uint8 [S, S, 3]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    h, w, _ = src.shape
    sx, a0, a1 = resize_table(w, S)
    sy, b0, b1 = resize_table(h, S)
    v = src.astype(np.int64)
    x1, y1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    r = v[:, sx] * a0[None, :, None] + v[:, x1] * a1[None, :, None]  # [h, S, 3]
    top, bottom = r[sy] >> 4, r[y1] >> 4
    dst = (((b0[:, None, None] * top) >> 16) + ((b1[:, None, None] * bottom) >> 16) + 2) >> 2
    return dst.astype(np.uint8)


def jet(u):
    """The jet ramp in RGB for integer u in 0..255 -> [..., 3]."""
    u4 = 4 * np.asarray(u).astype(np.int64)
    return np.stack([np.clip(383 - np.abs(u4 - c), 0, 255) for c in (765, 510, 255)], axis=-1)


def value_range(maps):
    maps = np.asarray(maps, np.float32)
    return np.float32(maps.min()), np.float32(maps.max())


def quantise(maps, rng=None):
    """q of the maps under the class range rng = (lo, hi), or without normalisation (None)."""
    x = np.asarray(maps, np.float32)
    with np.errstate(all="ignore"):
        if rng is not None and np.float32(rng[1]) != np.float32(1):
            lo, hi = np.float32(rng[0]), np.float32(rng[1])
            v = ((x - lo) / (hi - lo)).astype(np.float32)
        else:
            v = x
        t = np.trunc(v * np.float32(255)).astype(np.float32)
        q = np.clip(t, 0, 255)
    return np.where(np.isfinite(v), q, 0).astype(np.uint8)


def panels(maps, labels, thumbs, rng="class", true_color=False):
    """maps fp32 [n, S, S], labels [n, S, S] or None, thumbs uint8 [n, S, S, 3] -> uint8 [n, 3S, S, 3].
    rng: "class" = the range of these maps, a (lo, hi) pair, or None for no normalisation."""
    maps = np.asarray(maps, np.float32)
    thumbs = np.asarray(thumbs)
    if isinstance(rng, str):
        rng = value_range(maps)
    q = quantise(maps, rng)
    L = np.zeros(maps.shape, np.int64) if labels is None else np.where(np.asarray(labels) != 0, 255, 0)
    P = (thumbs if true_color else thumbs[..., ::-1]).astype(np.int64)
    return np.concatenate([P, (P + jet(L)) >> 1, (P + jet(q)) >> 1], axis=1).astype(np.uint8)


def render(pixel_label, pixel_preds, sources, true_color=False):
    """What visualize() writes for one class: labels [n, 1, S, S] or [n, S, S], maps [n, S, S] or
    [n, 1, S, S], sources a list of uint8 [h, w, 3]."""
    maps = np.asarray(pixel_preds, np.float32)
    maps = maps.reshape(maps.shape[0], maps.shape[-2], maps.shape[-1])
    labels = np.asarray(pixel_label).reshape(maps.shape)
    S = maps.shape[-1]
    thumbs = np.stack([resize(s, S) for s in sources])
    return panels(maps, labels, thumbs, "class", true_color)


def file_path(save_dir, dataset_name, class_name, file_name):
    damage, image_name = file_name.split("/")[-2:]
    return os.path.join(save_dir, "visualization", dataset_name, class_name, f"{damage}_{image_name}")
