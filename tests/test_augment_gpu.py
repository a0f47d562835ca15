"""The train-time augmentation kernels on the device (csrc/augment.hip) against the yardstick
tests/augment_ref.py: the colour jitter bit-equal to Pillow's ImageEnhance, the geometric gather
equal to the reference's sequential nearest resamples (exactly for flips, shifts and quarter
turns; for generic angles everywhere but on rounding ties), and TrainPreprocessor.apply equal to
the CPU path of the loader workers."""
import numpy as np
import pytest
import torch

from aaclip.preprocess import TrainPreprocessor

import augment_ref as AR

pytestmark = pytest.mark.gpu

BAND = 5e-4        # |source coordinate - half-integer| below which nearest rounding may differ
BAND_SHARE = 5e-3  # the excluded pixels stay under 0.5 % per case (a condition, not a measurement)


@pytest.fixture(scope="module")
def tp(dev):
    return TrainPreprocessor(37, text=False)


def _img(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _padded(dev, arr, pad):
    """uint8 [B,H,W,3] on the device with `pad` extra bytes per row (filled with 0xA5)."""
    B, H, W, _ = arr.shape
    buf = torch.full((B, H, W * 3 + pad), 0xA5, dtype=torch.uint8, device=dev)
    view = buf[:, :, :W * 3].view(B, H, W, 3) if pad == 0 else buf.as_strided((B, H, W, 3),
                                                                               (H * (W * 3 + pad), W * 3 + pad, 3, 1))
    view.copy_(torch.from_numpy(arr).to(dev))
    return buf, view


FACTOR_SETS = [(0.5, 0.5, 0.5), (1.5, 1.5, 1.5), (0.731, 0.731, 0.731), (0.731, 1.0, 1.0), (1.0, 1.31, 1.0),
               (1.0, 1.0, 0.64), (1.0, 1.0, 1.43), (1.27, 0.58, 1.46), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0),
               (1.0, 1.0, 0.0)]


@pytest.mark.parametrize("h,w,pad", [(1, 1, 0), (7, 5, 0), (67, 45, 0), (67, 45, 9), (67, 45, 2), (300, 259, 0),
                                     (300, 259, 3), (64, 64, 0)])
def test_jitter_is_bit_equal_to_pillow(dev, tp, h, w, pad):
    """Every factor set on every size: 1 x 1, odd sizes, padded pitches (9 with W = 45 and 3 with
    W = 259: pitch % 4 == 0, the dword path with a ragged last group; 2: a padded pitch on the
    byte path), 300 x 259 (many blocks per reduction), 64 x 64 (dword path, no ragged group)."""
    img = _img(h, w, seed=h * 1000 + w)
    f = torch.tensor(FACTOR_SETS, dtype=torch.float32)
    src = np.repeat(img[None], len(FACTOR_SETS), 0)
    buf, view = _padded(dev, src, pad)
    got = tp.jitter(view, f).cpu().numpy()
    for k, fs in enumerate(FACTOR_SETS):
        ref = AR.jitter(img, f[k].tolist())
        assert np.array_equal(got[k], ref), (fs, int(np.abs(got[k].astype(int) - ref).max()))
    assert torch.equal(view.cpu(), torch.from_numpy(src))  # the source is untouched


def test_jitter_identity_and_per_image_factors(dev, tp):
    imgs = np.stack([_img(67, 45, seed=s) for s in (1, 2, 3)])
    x = torch.from_numpy(imgs).to(dev)
    assert torch.equal(tp.jitter(x, torch.ones(3, 3)), x)
    f = torch.tensor([[1.0, 1.0, 1.0], [0.731, 1.42, 0.55], [1.5, 1.0, 0.9]])
    got = tp.jitter(x, f).cpu().numpy()
    assert np.array_equal(got[0], imgs[0])
    for b in range(3):
        assert np.array_equal(got[b], AR.jitter(imgs[b], f[b].tolist())), b


@pytest.mark.parametrize("pad", [0, 9])
def test_jitter_in_place_equals_out_of_place_and_repeats(dev, tp, pad):
    imgs = np.stack([_img(300, 259, seed=s) for s in (4, 5)])
    f = torch.tensor([[0.8, 1.3, 0.6], [1.2, 0.7, 1.4]])
    buf, view = _padded(dev, imgs, pad)
    a = tp.jitter(view, f)
    b = tp.jitter(view, f)
    assert torch.equal(a, b)  # two launches, equal bits
    assert tp.jitter(view, f, out=view) is view and torch.equal(view, a)
    if pad:
        assert torch.all(buf[:, :, 259 * 3:] == 0xA5)  # the padding bytes are not written


@pytest.mark.parametrize("value", [0, 255])
def test_jitter_of_constant_images(dev, tp, value):
    img = np.full((7, 5, 3), value, np.uint8)
    for fs in FACTOR_SETS:
        got = tp.jitter(torch.from_numpy(img[None]).to(dev), torch.tensor([fs])).cpu().numpy()[0]
        assert np.array_equal(got, AR.jitter(img, fs)), fs


@pytest.mark.parametrize("k", [0, 100, 254])
def test_contrast_mean_rounds_half_up(dev, tp, k):
    """Two grey pixels k and k + 1: the mean L is exactly k + 0.5 and int(mean + 0.5) = k + 1."""
    img = np.array([[[k, k, k], [k + 1, k + 1, k + 1]]], np.uint8)
    for fc in (0.0, 0.5, 1.5):
        got = tp.jitter(torch.from_numpy(img[None]).to(dev), torch.tensor([[1.0, fc, 1.0]])).cpu().numpy()[0]
        assert np.array_equal(got, AR.jitter(img, (1.0, fc, 1.0))), fc
    got = tp.jitter(torch.from_numpy(img[None]).to(dev), torch.tensor([[1.0, 0.0, 1.0]])).cpu().numpy()[0]
    assert np.all(got == k + 1)


# ------------------------------------------------------------------ geometry
def _params(rows):
    """rows of (rotate, angle, tx, ty, hflip, vflip) -> a TrainPreprocessor.sample-shaped dict."""
    cs = [[float(np.float32(v)) for v in AR.cos_sin(r[1])] for r in rows]
    return {"color": torch.ones(len(rows), 3), "rotate": torch.tensor([bool(r[0]) for r in rows]),
            "angle": torch.tensor([float(r[1]) for r in rows], dtype=torch.float64),
            "cos_sin": torch.tensor(cs, dtype=torch.float32),
            "shift": torch.tensor([[r[2], r[3]] for r in rows], dtype=torch.int32),
            "hflip": torch.tensor([bool(r[4]) for r in rows]), "vflip": torch.tensor([bool(r[5]) for r in rows])}


def _x(S, B=4, C=4, seed=0):
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, C, S, S)).astype(np.float32))
    x[:, -1] = (x[:, -1] > 0.3).float()  # the mask channel
    return x


def _shift(x, tx, ty):
    S = x.shape[-1]
    y = torch.zeros_like(x)
    if abs(tx) < S and abs(ty) < S:
        y[..., max(ty, 0):S + min(ty, 0), max(tx, 0):S + min(tx, 0)] = \
            x[..., max(-ty, 0):S + min(-ty, 0), max(-tx, 0):S + min(-tx, 0)]
    return y


@pytest.mark.parametrize("S", [37, 64])
def test_geom_exact_cases(dev, tp, S):
    x = _x(S, seed=S)
    xd = x.to(dev)
    off = (0, 0.0, 0, 0, 0, 0)
    assert torch.equal(tp.geom(xd, _params([off] * 4)), xd)
    got = tp.geom(xd, _params([(0, 0.0, 0, 0, 1, 0), (0, 0.0, 0, 0, 0, 1), (0, 0.0, 0, 0, 1, 1), off])).cpu()
    assert torch.equal(got[0], torch.flip(x[0], (-1,))) and torch.equal(got[1], torch.flip(x[1], (-2,)))
    assert torch.equal(got[2], torch.flip(x[2], (-1, -2))) and torch.equal(got[3], x[3])
    shifts = [(3, -5), (-S + 1, S - 1), (S, 0), (0, -S - 7)]
    got = tp.geom(xd, _params([(0, 0.0, tx, ty, 0, 0) for tx, ty in shifts])).cpu()
    for b, (tx, ty) in enumerate(shifts):
        assert torch.equal(got[b], _shift(x[b], tx, ty)), (tx, ty)
    assert got[1].count_nonzero() > 0 and got[2].count_nonzero() == 0 and got[3].count_nonzero() == 0
    # the yardstick's translation (grid_sample) is the same shift
    assert torch.equal(AR.geom(x[0], False, 0.0, 3, -5, False, False), _shift(x[0], 3, -5))
    # shift, then both flips, in the reference's order
    got = tp.geom(xd, _params([(0, 0.0, 4, 2, 1, 1)] * 4)).cpu()
    assert torch.equal(got, torch.flip(_shift(x, 4, 2), (-1, -2)))
    # a second tensor goes through the same map
    a, m = tp.geom(xd[:, :3].contiguous(), _params([(0, 0.0, 4, 2, 1, 0)] * 4), xd[:, 3:].contiguous())
    assert torch.equal(torch.cat([a, m], 1).cpu(), torch.flip(_shift(x, 4, 2), (-1,)))


def test_geom_quarter_turns_pin_the_sign(dev, tp):
    """+90 degrees is counter-clockwise (torch.rot90 k = 1), independent of the transcription."""
    x = _x(64, seed=9)
    got = tp.geom(x.to(dev), _params([(1, 90.0, 0, 0, 0, 0), (1, -90.0, 0, 0, 0, 0), (1, 90.0, 0, 0, 0, 0),
                                      (1, 0.0, 0, 0, 0, 0)])).cpu()
    assert torch.equal(got[0], torch.rot90(x[0], 1, (-2, -1)))
    assert torch.equal(got[1], torch.rot90(x[1], -1, (-2, -1)))
    assert torch.equal(got[2], torch.rot90(x[2], 1, (-2, -1))) and torch.equal(got[3], x[3])


CASES = [(1, 17.3, 0, 0, 0, 0), (1, -29.9, 0, 0, 0, 0), (1, 17.3, 3, -5, 1, 1), (1, -29.9, -4, 6, 1, 1)]


@pytest.fixture(scope="module")
def yardsticks():
    """The fp32 and fp64 sequential runs and the tie band of every case and size, made once."""
    out = {}
    for S in (37, 64):
        x = _x(S, seed=100 + S)
        for b, c in enumerate(CASES):
            out[S, b] = (AR.geom(x[b], *c, dtype=torch.float32), AR.geom(x[b], *c, dtype=torch.float64),
                         AR.tie_band(S, *c, eps=BAND))
        out[S] = x
    return out


@pytest.mark.parametrize("S", [37, 64])
def test_geom_generic_angles(dev, tp, yardsticks, S):
    x = yardsticks[S]
    got = tp.geom(x.to(dev), _params(CASES)).cpu()
    for b, c in enumerate(CASES):
        r32, r64, band = yardsticks[S, b]
        share = band.float().mean().item()
        # the yardstick's own precision: its fp32 and fp64 runs differ only inside the band
        assert not ((r32 != r64.float()).any(0) & ~band).any()
        wrong = (got[b] != r32).any(0)
        print(f"S {S} case {c}: band share {share:.4%}, device != fp32 yardstick on {int(wrong.sum())} pixels "
              f"({int((wrong & ~band).sum())} outside the band)")
        assert share < BAND_SHARE
        assert not (wrong & ~band).any()
        assert set(np.unique(got[b, -1].numpy())) <= {0.0, 1.0}  # the mask channel stays binary
        assert got[b].count_nonzero() > 0.4 * got[b].numel()  # not an empty image


def test_geom_is_deterministic(dev, tp):
    x = _x(64, seed=3).to(dev)
    p = _params(CASES)
    assert torch.equal(tp.geom(x, p), tp.geom(x, p))


def test_apply_equals_the_cpu_path(dev):
    """Two images of different source sizes (a list batch), every transform on: the device chain
    against TrainPreprocessor.cpu_item (Pillow's ImageEnhance and resize, grid_sample) under the
    same parameters; rotation ties excluded by the same rule."""
    from PIL import Image
    S = 37
    tp = TrainPreprocessor(S, text=False)
    imgs = [_img(96, 80, seed=31), _img(61, 83, seed=32)]
    masks = [np.zeros((96, 80), np.uint8), np.zeros((61, 83), np.uint8)]
    masks[0][20:70, 10:50] = 255
    masks[1][5:40, 30:80] = 7
    rows = [(1, 17.3, 3, -5, 1, 0), (1, -29.9, -2, 4, 0, 1)]
    params = _params(rows)
    params["color"] = torch.tensor([[0.731, 1.42, 0.55], [1.5, 0.6, 1.0]])
    image, mask = tp.apply([torch.from_numpy(a).to(dev) for a in imgs], [torch.from_numpy(m).to(dev) for m in masks],
                           params)
    assert image.shape == (2, 3, S, S) and mask.shape == (2, 1, S, S)
    assert image.dtype == mask.dtype == torch.float32 and image.is_contiguous() and mask.is_contiguous()
    for b in range(2):
        ri, rm = tp.cpu_item(Image.fromarray(imgs[b], "RGB"), Image.fromarray(masks[b], "L"), params, b)
        band = AR.tie_band(S, *rows[b], eps=BAND)
        assert band.float().mean().item() < BAND_SHARE
        wrong = (image[b].cpu() != ri).any(0) | (mask[b].cpu() != rm).any(0)
        assert not (wrong & ~band).any(), int((wrong & ~band).sum())
        assert set(np.unique(mask[b].cpu().numpy())) <= {0.0, 1.0} and mask[b].sum() > 0
    # a stacked batch takes the batched launches and gives the same tensors
    both = np.stack([imgs[0], _img(96, 80, seed=33)])
    mk = np.stack([masks[0], masks[0]])
    a, m = tp.apply(torch.from_numpy(both).to(dev), torch.from_numpy(mk).to(dev), params)
    a0, m0 = tp.apply([torch.from_numpy(both[0]).to(dev)], [torch.from_numpy(mk[0]).to(dev)],
                      {k: v[:1] for k, v in params.items()})
    assert torch.equal(a[:1], a0) and torch.equal(m[:1], m0)
