"""The overlays on the MI355X (aaclip_resize_bilinear_u8, aaclip_overlay_range, aaclip_overlay_panels,
forward_utils.visualize, test.py --visualize) against the numpy restatement of tests/visualize_ref.py.
Every comparison is byte for byte: the recipe is integer and fp32 arithmetic with one result."""
import numpy as np
import pytest
import torch

from aaclip import ops

import visualize_ref as VR

pytestmark = pytest.mark.gpu


def _photos(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---------------------------------------------------------------------------- resize
@pytest.mark.parametrize("h,w,S", [(7, 5, 14), (5, 7, 14), (5, 9, 14), (9, 5, 14), (28, 28, 14), (14, 14, 14),
                                   (1, 1, 14), (37, 53, 70), (53, 37, 70), (70, 70, 15)])
def test_resize_equals_the_restatement(dev, h, w, S):
    src = _photos(h * 100 + w, 3, h, w, 3)  # batch 3
    got = ops.resize_bilinear_u8(torch.from_numpy(src).to(dev), S).cpu().numpy()
    want = np.stack([VR.resize(s, S) for s in src])
    assert got.shape == (3, S, S, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if (h, w) == (S, S):
        assert np.array_equal(got, src)  # the identity
    one = ops.resize_bilinear_u8(torch.from_numpy(src[1:2]).to(dev), S).cpu().numpy()
    assert np.array_equal(one[0], want[1])  # alone as in the batch


def test_resize_padded_pitch_padded_stride_and_misaligned_output(dev):
    h, w, S = 11, 13, 15
    src = _photos(5, 2, h, w, 3)
    want = np.stack([VR.resize(s, S) for s in src])
    wide = torch.full((2, h + 3, w + 5, 3), 255, dtype=torch.uint8, device=dev)  # row pitch 54 > 39, padded stride
    wide[:, :h, :w] = torch.from_numpy(src).to(dev)
    view = wide[:, :h, :w]
    assert view.stride(1) == 3 * (w + 5) and view.stride(0) == 3 * (w + 5) * (h + 3)
    assert np.array_equal(ops.resize_bilinear_u8(view, S).cpu().numpy(), want)
    # an output that starts at an odd address takes the byte path
    flat = torch.zeros(2 * S * S * 3 + 1, dtype=torch.uint8, device=dev)
    out = flat[1:].view(2, S, S, 3)
    assert out.data_ptr() % 4 == 1
    ops.resize_bilinear_u8(torch.from_numpy(src).to(dev), S, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and int(flat[0]) == 0


def test_resize_bad_arguments_raise(dev):
    ok = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_bilinear_u8(ok.float(), 14)
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_bilinear_u8(ok[..., :2], 14)
    with pytest.raises(ValueError, match="contiguous"):
        ops.resize_bilinear_u8(ok.permute(0, 2, 1, 3), 14)
    with pytest.raises(ValueError, match="at least 1"):
        ops.resize_bilinear_u8(ok, 0)
    with pytest.raises(ValueError, match="out must be"):
        ops.resize_bilinear_u8(ok, 14, out=torch.zeros(1, 14, 14, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="device"):
        ops.resize_bilinear_u8(ok.cpu(), 14)


# ---------------------------------------------------------------------------- panels
def _class(S, n=3, seed=0):
    """Maps with repeated values at lo and hi, labels holding 0, 1, 7 and 255, random thumbnails."""
    rng = np.random.default_rng(seed + S)
    maps = rng.uniform(0.1, 0.7, (n, S, S)).astype(np.float32)
    maps[0, 0, :3] = maps[n - 1, S - 1, -2:] = 0.05  # lo, in two images
    maps[1, 2, 1:4] = maps[0, S - 1, S - 1] = 0.9  # hi, likewise
    labels = rng.choice(np.array([0, 0, 1, 7, 255], np.uint8), (n, S, S))
    thumbs = rng.integers(0, 256, (n, S, S, 3), dtype=np.uint8)
    return maps, labels, thumbs


def _render(dev, maps, labels, thumbs, rng="class", true_color=False):
    m = torch.from_numpy(maps).to(dev)
    value_range = ops.overlay_range(m) if isinstance(rng, str) else rng
    return ops.overlay_panels(m, torch.from_numpy(thumbs).to(dev),
                              labels=None if labels is None else torch.from_numpy(labels).to(dev),
                              value_range=value_range, swap_rb=not true_color).cpu().numpy()


@pytest.mark.parametrize("n,pix", [(3, 13), (2, 67), (1, 2), (4, 128), (5, 70 * 70), (300, 6)])
def test_range_is_the_min_and_max_of_the_class(dev, n, pix):
    """An image is reduced in the largest number of equal parts up to 64: 13 parts of one pixel, one
    part (67 is prime), 64 parts, 50 parts of 98, and more rows than one pass of the last block."""
    maps = np.random.default_rng(n * pix).standard_normal((n, pix)).astype(np.float32)
    got = ops.overlay_range(torch.from_numpy(maps).to(dev)).cpu().numpy()
    assert got.dtype == np.float32 and got.tolist() == [maps.min(), maps.max()]
    maps[n - 1, pix - 1], maps[0, 0] = -7.0, 9.0  # the ends of the class
    assert ops.overlay_range(torch.from_numpy(maps).to(dev)).cpu().tolist() == [-7.0, 9.0]


@pytest.mark.parametrize("true_color", [False, True])
@pytest.mark.parametrize("S", [14, 15, 37])  # 15: odd row bytes; 37: 1369 pixels, two blocks per image
def test_panels_equal_the_restatement(dev, S, true_color):
    maps, labels, thumbs = _class(S)
    lo_hi = ops.overlay_range(torch.from_numpy(maps).to(dev)).cpu().numpy()
    assert lo_hi.dtype == np.float32 and lo_hi.tolist() == [np.float32(0.05), np.float32(0.9)]
    got = _render(dev, maps, labels, thumbs, true_color=true_color)
    want = VR.panels(maps, labels, thumbs, "class", true_color)
    assert got.shape == (3, 3 * S, S, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    q = VR.quantise(maps, VR.value_range(maps))
    assert (q == 0).sum() >= 5 and (q == 255).sum() >= 4  # both ends of the ramp are in the picture
    # NULL labels are all-zero labels
    bare = _render(dev, maps, None, thumbs, true_color=true_color)
    assert np.array_equal(bare, VR.panels(maps, None, thumbs, "class", true_color))
    assert np.array_equal(bare, VR.panels(maps, np.zeros_like(labels), thumbs, "class", true_color))
    # no range: the raw value is quantised
    raw = _render(dev, maps, labels, thumbs, rng=None, true_color=true_color)
    assert np.array_equal(raw, VR.panels(maps, labels, thumbs, None, true_color))


@pytest.mark.parametrize("true_color", [False, True])
@pytest.mark.parametrize("S", [14, 15])
def test_panels_class_maximum_of_one_and_constant_class(dev, S, true_color):
    maps, labels, thumbs = _class(S)
    top1 = maps.copy()
    top1[1, 2, 1:4] = top1[0, S - 1, S - 1] = 1.0  # the class maximum is exactly 1: not normalised
    top1[2, 0, 0] = -0.5  # below 0: clamped
    got = _render(dev, top1, labels, thumbs, true_color=true_color)
    assert np.array_equal(got, VR.panels(top1, labels, thumbs, "class", true_color))
    assert np.array_equal(got, VR.panels(top1, labels, thumbs, None, true_color))
    flat = np.full_like(maps, 0.3)  # 0 / 0 everywhere: q = 0
    got = _render(dev, flat, labels, thumbs, true_color=true_color)
    assert np.array_equal(got, VR.panels(flat, labels, thumbs, "class", true_color))
    assert np.array_equal(got[:, 2 * S:], VR.panels(np.zeros_like(maps), labels, thumbs, None, true_color)[:, 2 * S:])
    wild = maps.copy()  # non-finite scores without a range: q = 0 there
    wild[0, 1, :4] = [np.nan, np.inf, -np.inf, 3e38]
    got = _render(dev, wild, labels, thumbs, rng=None, true_color=true_color)
    assert np.array_equal(got, VR.panels(wild, labels, thumbs, None, true_color))


@pytest.mark.parametrize("true_color", [False, True])
@pytest.mark.parametrize("S", [14, 15])
def test_panels_alone_as_in_the_batch(dev, S, true_color):
    maps, labels, thumbs = _class(S, n=4)
    value_range = ops.overlay_range(torch.from_numpy(maps).to(dev))
    whole = _render(dev, maps, labels, thumbs, rng=value_range, true_color=true_color)
    for i in range(4):  # (an odd S puts every image of the batch at another alignment)
        one = _render(dev, maps[i:i + 1], labels[i:i + 1], thumbs[i:i + 1], rng=value_range, true_color=true_color)
        assert np.array_equal(one[0], whole[i]), i
    again = _render(dev, maps, labels, thumbs, rng=value_range, true_color=true_color)
    assert np.array_equal(again, whole)


def test_panels_bad_arguments_raise(dev):
    maps, labels, thumbs = (torch.from_numpy(x).to(dev) for x in _class(14))
    with pytest.raises(ValueError, match="maps must be"):
        ops.overlay_panels(maps[:, :, :-1], thumbs)
    with pytest.raises(ValueError, match="maps must be"):
        ops.overlay_panels(maps[:0], thumbs[:0])
    with pytest.raises(ValueError, match="thumbs must be"):
        ops.overlay_panels(maps, thumbs[:, :-1])
    with pytest.raises(ValueError, match="thumbs must be"):
        ops.overlay_panels(maps, thumbs.float())
    with pytest.raises(ValueError, match="labels must match"):
        ops.overlay_panels(maps, thumbs, labels=labels[:2])
    with pytest.raises(ValueError, match="value_range"):
        ops.overlay_panels(maps, thumbs, value_range=torch.zeros(3, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        ops.overlay_panels(maps, thumbs, out=torch.zeros(3, 14, 14, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="device"):
        ops.overlay_panels(maps, thumbs.cpu())
    with pytest.raises(ValueError, match="non-empty"):
        ops.overlay_range(maps[:0])


# ---------------------------------------------------------------------------- visualize()
def test_visualize_groups_sources_by_size_and_reads_files(dev, tmp_path, monkeypatch):
    from PIL import Image

    import forward_utils as fu
    S, n = 15, 5
    maps, labels, _ = _class(S, n=n)
    shapes = [(7, 5), (20, 31), (7, 5), (15, 15), (20, 31)]  # three sizes, interleaved
    photos = [_photos(40 + i, h, w, 3) for i, (h, w) in enumerate(shapes)]
    names = [f"bottle/test/{'good' if i % 2 else 'broken'}/{i:03d}.png" for i in range(n)]
    want = VR.render(labels, maps, photos)
    paths = fu.visualize(labels[:, None], maps, names, str(tmp_path / "a"), "MVTec", "bottle", images=photos)
    assert paths == [VR.file_path(str(tmp_path / "a"), "MVTec", "bottle", f) for f in names]
    for p, w in zip(paths, want):
        assert np.array_equal(np.asarray(Image.open(p)), w), p
    # device tensors in, thumbnails already resized, true colours, bmp
    thumbs = torch.from_numpy(np.stack([VR.resize(p, S) for p in photos])).to(dev)
    bmp = [f.replace(".png", ".bmp") for f in names]
    paths = fu.visualize(torch.from_numpy(labels).to(dev), torch.from_numpy(maps[:, None]).to(dev), bmp,
                         str(tmp_path / "b"), "VisA", "candle", images=thumbs, true_color=True, workers=1)
    assert all(p.endswith(".bmp") and "/visualization/VisA/candle/" in p for p in paths)
    for p, w in zip(paths, VR.render(labels, maps, photos, true_color=True)):
        assert np.array_equal(np.asarray(Image.open(p)), w), p
    # without images the files are read from DATA_PATH[dataset_name]
    root = tmp_path / "data"
    for f, photo in zip(names, photos):
        (root / f).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(photo).save(root / f)
    monkeypatch.setitem(fu.DATA_PATH, "MVTec", str(root))
    paths = fu.visualize(labels, maps, names, str(tmp_path / "c"), "MVTec", "bottle")
    for p, w in zip(paths, want):
        assert np.array_equal(np.asarray(Image.open(p)), w), p
    with pytest.raises(ValueError, match="need 5 images"):
        fu.visualize(labels, maps, names, str(tmp_path / "d"), "MVTec", "bottle", images=photos[:4])
    with pytest.raises(ValueError, match="file names"):
        fu.visualize(labels, maps, names[:4], str(tmp_path / "d"), "MVTec", "bottle", images=photos)


def test_visualize_more_than_one_chunk(dev, tmp_path):
    from PIL import Image

    import forward_utils as fu
    S, n = 14, 70  # chunks of 32, 32 and 6: both pinned buffers are reused
    maps, labels, thumbs = _class(S, n=n)
    names = [f"c/test/bad/{i:03d}.png" for i in range(n)]
    paths = fu.visualize(labels, maps, names, str(tmp_path), "MVTec", "bottle", images=list(thumbs), workers=3)
    want = VR.panels(maps, labels, thumbs)
    assert len(paths) == n
    for p, w in zip(paths, want):
        assert np.array_equal(np.asarray(Image.open(p)), w), p


# ---------------------------------------------------------------------------- the harness
@pytest.mark.parametrize("true_color", [False, True])
def test_harness_visualize(dev, tmp_path, true_color):
    from PIL import Image

    import test as harness
    from dataset import SyntheticSingleClassDataset
    args = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4", "--visualize",
            "--save_path", str(tmp_path)] + (["--visualize_true_color"] if true_color else [])
    df, ctx = harness.run(harness.parse_args(args))
    masks, labels, preds, preds_image = ctx["classes"]["bottle"]
    ds = SyntheticSingleClassDataset(4, 70)
    want = VR.render(masks.cpu().numpy(), preds.cpu().numpy(), [ds.source_u8(i) for i in range(4)],
                     true_color=true_color)
    folder = tmp_path / "visualization" / "synthetic" / "bottle"
    assert sorted(p.name for p in folder.iterdir()) == [f"synthetic_{i:05d}.png" for i in range(4)]
    for i in range(4):
        with Image.open(folder / f"synthetic_{i:05d}.png") as im:
            assert im.size == (70, 210) and im.mode == "RGB"
            assert np.array_equal(np.asarray(im), want[i]), i
    assert masks.cpu().numpy().any() and len(np.unique(want[:, 140:])) > 50  # there is something to see


def test_harness_thumbnails_at_batch_time(dev):
    """Single-process raw mode: get_predictions appends each batch's thumbnails, resized from the
    photos already on the device, to `sources`; the 5-tuple it returns is unchanged."""
    import test as harness
    from aaclip.preprocess import Preprocessor
    from dataset import collate_raw
    S = 28
    photos = [_photos(70 + i, *shape, 3) for i, shape in enumerate([(40, 30), (40, 30), (40, 30), (33, 47), (40, 30)])]
    items = [{"image_u8": torch.from_numpy(p), "mask_u8": torch.zeros(p.shape[:2], dtype=torch.uint8), "label": i % 2,
              "file_name": f"c/test/good/{i}.png", "class_name": "c"} for i, p in enumerate(photos)]

    class Model:
        def predict(self, image, T, domain, streams=1):
            return image.mean(1), image.mean((1, 2, 3))

    def run(sources):
        loader = torch.utils.data.DataLoader(items, batch_size=3, shuffle=False, collate_fn=collate_raw)
        return harness.get_predictions(Model(), None, loader, dev, S, dataset="MVTec", prep=Preprocessor(S),
                                       sources=sources)
    sources = []
    with_thumbs, without = run(sources), run(None)
    assert len(with_thumbs) == 5 and [tuple(t.shape) for t in sources] == [(3, S, S, 3), (2, S, S, 3)]
    assert np.array_equal(torch.cat(sources).cpu().numpy(), np.stack([VR.resize(p, S) for p in photos]))
    for a, b in zip(with_thumbs, without):
        assert a == b if isinstance(a, list) else np.array_equal(torch.as_tensor(a).cpu().numpy(),
                                                                 torch.as_tensor(b).cpu().numpy())
