"""Host-side checks of the overlays (no GPU). tests/visualize_ref.py, the numpy restatement that the
GPU tests demand exact equality with, is first held to facts that need no cv2: the jet endpoints,
the resize as identity and on constant images, weight sums of 2048, less than one grey level from a
float64 bilinear, and the blend as an integer shift. Then the file naming, the C ABI (declared,
bound, exported, bad arguments refused without a launch, the plan equal to the restatement's) and
the Python surface. The ABI version stays 9."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from aaclip import _lib

import visualize_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_bilinear_plan", "aaclip_resize_bilinear_u8", "aaclip_overlay_workspace", "aaclip_overlay_range",
       "aaclip_overlay_panels"]
# (h, w) -> S: the GPU tests' shapes, and the setting of tools/visualize_timing.py
SHAPES = [((7, 5), 14), ((5, 9), 14), ((28, 28), 14), ((14, 14), 14), ((1, 1), 14), ((37, 53), 70),
          ((1024, 1024), 518), ((900, 700), 518), ((3, 1000), 15), ((70, 70), 70), ((96, 80), 70), ((2, 2), 15)]


def _bilinear64(src, S):
    """Float64 bilinear at the same sample positions (pixel centres, edges clamped)."""
    h, w, _ = src.shape
    def axis(n):
        f = (np.arange(S) + 0.5) * (n / S) - 0.5
        f = np.clip(f, 0, n - 1)
        s = np.minimum(np.floor(f).astype(int), max(n - 2, 0))
        return s, np.minimum(s + 1, n - 1), f - s
    y0, y1, fy = axis(h)
    x0, x1, fx = axis(w)
    v = src.astype(np.float64)
    top = v[y0][:, x0] * (1 - fx)[None, :, None] + v[y0][:, x1] * fx[None, :, None]
    bot = v[y1][:, x0] * (1 - fx)[None, :, None] + v[y1][:, x1] * fx[None, :, None]
    return top * (1 - fy)[:, None, None] + bot * fy[:, None, None]


# ---------------------------------------------------------------------------- the restatement
def test_jet_endpoints_and_shape_of_the_ramp():
    assert VR.jet(0).tolist() == [0, 0, 128] and VR.jet(255).tolist() == [128, 0, 0]
    ramp = VR.jet(np.arange(256))
    assert ramp.shape == (256, 3) and ramp.min() == 0 and ramp.max() == 255
    assert ramp[128].tolist() == [130, 255, 126]  # 383 - |512 - 765|, saturated green, 383 - |512 - 255|
    assert (np.diff(ramp[:, 0]) >= 0)[:223].all() and (np.diff(ramp[:, 2]) <= 0)[32:].all()


@pytest.mark.parametrize("shape,S", SHAPES)
def test_resize_weights_and_accuracy(shape, S):
    h, w = shape
    for n in (h, w):
        s, a0, a1 = VR.resize_table(n, S)
        assert ((a0 + a1) == 2048).all() and (a0 >= 0).all() and (a1 >= 0).all()
        assert (s >= 0).all() and (s <= n - 1).all()
    rng = np.random.default_rng(h * 1000 + w)
    src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = VR.resize(src, S)
    assert got.shape == (S, S, 3) and got.dtype == np.uint8
    err = np.abs(got.astype(np.float64) - _bilinear64(src, S)).max()
    print(shape, S, "max distance from float64 bilinear", err)
    assert err < 1.0
    for value in (0, 255, 77):
        assert (VR.resize(np.full((h, w, 3), value, np.uint8), S) == value).all()


def test_resize_is_the_identity_at_equal_sizes():
    src = np.random.default_rng(3).integers(0, 256, (14, 14, 3), dtype=np.uint8)
    assert np.array_equal(VR.resize(src, 14), src)
    s, a0, a1 = VR.resize_table(14, 14)
    assert s.tolist() == list(range(14)) and (a0 == 2048).all() and (a1 == 0).all()


def test_blend_is_an_integer_shift():
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = (0.5 * a.astype(np.uint8) + 0.5 * b.astype(np.uint8)).astype(np.uint8)
    assert np.array_equal((a + b) >> 1, want)


def test_quantise_defined_cases():
    m = np.array([[[0.25, 0.75], [0.5, 0.25]]], np.float32)
    assert VR.quantise(m, VR.value_range(m)).tolist() == [[[0, 255], [127, 0]]]
    top1 = np.array([[[1.0, 0.5], [-0.25, 0.999]]], np.float32)  # class maximum 1: raw, clamped
    assert VR.quantise(top1, VR.value_range(top1)).tolist() == [[[255, 127], [0, 254]]]
    assert VR.quantise(top1, None).tolist() == [[[255, 127], [0, 254]]]
    assert VR.quantise(np.array([2.0, -3.0], np.float32), None).tolist() == [255, 0]
    flat = np.full((2, 3, 3), 0.3, np.float32)  # constant: 0 / 0
    assert not VR.quantise(flat, VR.value_range(flat)).any()
    assert VR.quantise(np.array([np.nan, np.inf, -np.inf], np.float32), None).tolist() == [0, 0, 0]


def test_panels_layout_and_channel_order():
    maps = np.array([[[0.0, 1.0], [0.5, 2.0]]], np.float32)  # range [0, 2]: q = 0, 127, 63, 255
    labels = np.array([[[0, 7], [255, 0]]], np.uint8)
    thumbs = np.zeros((1, 2, 2, 3), np.uint8)
    thumbs[..., 0], thumbs[..., 2] = 200, 10  # a red photo
    out = VR.panels(maps, labels, thumbs)
    assert out.shape == (1, 6, 2, 3)
    assert (out[0, :2] == [10, 0, 200]).all()  # the reference's files: red and blue exchanged
    assert out[0, 2, 0].tolist() == [5, 0, (200 + 128) >> 1] and out[0, 2, 1].tolist() == [(10 + 128) >> 1, 0, 100]
    assert out[0, 3, 0].tolist() == [(10 + 128) >> 1, 0, 100]
    assert out[0, 4, 0].tolist() == [5, 0, (200 + 128) >> 1] and out[0, 5, 1].tolist() == [(10 + 128) >> 1, 0, 100]
    true = VR.panels(maps, labels, thumbs, true_color=True)
    assert (true[0, :2] == [200, 0, 10]).all() and true[0, 2, 1].tolist() == [(200 + 128) >> 1, 0, 5]
    assert np.array_equal(VR.panels(maps, None, thumbs)[0, 2:4], VR.panels(maps, labels * 0, thumbs)[0, 2:4])
    assert np.array_equal(VR.render(labels[:, None], maps, [thumbs[0]]), out)


# ---------------------------------------------------------------------------- files
def test_file_naming_and_directories():
    import forward_utils as fu
    for fn in (VR.file_path, fu.visualization_path):
        assert fn("out", "MVTec", "bottle", "bottle/test/broken_large/000.png") == os.path.join(
            "out", "visualization", "MVTec", "bottle", "broken_large_000.png")
        assert fn("/a/b", "VisA", "candle", "candle/Data/Images/Anomaly/012.JPG") == os.path.join(
            "/a/b", "visualization", "VisA", "candle", "Anomaly_012.JPG")
        assert fn("s", "synthetic", "bottle", "synthetic/00003.png").endswith(
            os.path.join("visualization", "synthetic", "bottle", "synthetic_00003.png"))


# ---------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9
    assert "overlay.hip" in open(os.path.join(ROOT, "aa-clip_amd", "csrc", "Makefile")).read()
    assert "tests/visualize_ref.py" in src and "is not claimed" in src
    kernels = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "overlay.hip")).read()
    assert "pixel_score(" in kernels and "row_minmax_kernel" in kernels  # the one normalisation, reused
    assert "forward_utils.py:283-327" in kernels


@pytest.mark.parametrize("n_in,n_out", [(1, 14), (5, 14), (7, 14), (9, 14), (28, 14), (14, 14), (37, 70), (53, 70),
                                        (1024, 518), (700, 518), (3, 1000)])
def test_host_plan_equals_the_restatement(n_in, n_out):
    from aaclip import ops
    table = ops.bilinear_plan(n_in, n_out)
    assert table.dtype == np.int32 and table.shape == (n_out, 3)
    for got, want in zip(table.T, VR.resize_table(n_in, n_out)):
        assert np.array_equal(got, want)


def test_argument_validation_rejects_without_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)  # non-null and aligned; never dereferenced on the host
    table = (ctypes.c_int32 * 9)()
    assert lib.aaclip_bilinear_plan(0, 3, table) == 1 and lib.aaclip_bilinear_plan(3, 0, table) == 1
    assert lib.aaclip_bilinear_plan(3, 3, None) == 1 and lib.aaclip_bilinear_plan(3, 3, table) == 0

    def resize(ptrs=(p,) * 4, stride=30 * 20, pitch=30, batch=2, h=20, w=10, S=7):
        return lib.aaclip_resize_bilinear_u8(ptrs[0], stride, pitch, batch, h, w, ptrs[1], ptrs[2], S, ptrs[3], None)
    for bad in range(4):
        assert resize(ptrs=tuple(None if i == bad else p for i in range(4))) == 1, bad
    assert resize(batch=0) == 1 and resize(h=0) == 1 and resize(w=-1) == 1 and resize(S=0) == 1
    assert resize(pitch=29) == 1 and resize(stride=30 * 20 - 1) == 1  # rows or images that overlap
    assert resize(batch=40000, S=256) == 1  # 2^31 output pixels and more

    size = ctypes.c_size_t(0)
    assert lib.aaclip_overlay_workspace(3, None) == 1 and lib.aaclip_overlay_workspace(0, ctypes.byref(size)) == 1
    assert lib.aaclip_overlay_workspace(3, ctypes.byref(size)) == 0 and size.value >= 2 * 3 * 4

    def span(ptrs=(p,) * 3, n=3, pix=100, ws_bytes=size.value):
        return lib.aaclip_overlay_range(ptrs[0], n, pix, ptrs[1], ws_bytes, ptrs[2], None)
    for bad in range(3):
        assert span(ptrs=tuple(None if i == bad else p for i in range(3))) == 1, bad
    assert span(n=0) == 1 and span(pix=0) == 1 and span(ws_bytes=size.value - 1) == 1

    def panels(ptrs=(p,) * 5, batch=2, S=14, swap=1):
        return lib.aaclip_overlay_panels(ptrs[0], ptrs[1], ptrs[2], ptrs[3], batch, S, swap, ptrs[4], None)
    for bad in (0, 2, 4):  # the labels, 1, and the range, 3, may be null
        assert panels(ptrs=tuple(None if i == bad else p for i in range(5))) == 1, bad
    assert panels(batch=0) == 1 and panels(S=0) == 1 and panels(batch=-2) == 1 and panels(batch=65536) == 1


# ---------------------------------------------------------------------------- Python surface
def test_python_surface():
    import forward_utils as fu
    from aaclip import ops
    par = inspect.signature(fu.visualize).parameters
    assert list(par)[:6] == ["pixel_label", "pixel_preds", "file_names", "save_dir", "dataset_name", "class_name"]
    assert all(par[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(par)[:6])
    for k, default in (("images", None), ("true_color", False), ("workers", 4)):
        assert par[k].kind is inspect.Parameter.KEYWORD_ONLY and par[k].default == default
    assert "aaclip_overlay_panels" in fu.__doc__ and "visualize() (cv2)" not in fu.__doc__
    assert callable(ops.resize_bilinear_u8) and callable(ops.overlay_panels) and callable(ops.overlay_range)
    assert inspect.signature(ops.overlay_panels).parameters["swap_rb"].default is True
    import test as harness
    off = harness.parse_args([])
    assert off.visualize is False and off.visualize_true_color is False
    on = harness.parse_args(["--visualize", "--visualize_true_color"])
    assert on.visualize is True and on.visualize_true_color is True
    assert inspect.signature(harness.get_predictions).parameters["sources"].default is None


def test_synthetic_source_u8_undoes_the_normalisation():
    from dataset import MEAN, STD, SyntheticSingleClassDataset
    ds = SyntheticSingleClassDataset(3, 10)
    u8 = ds.source_u8(1)
    assert u8.dtype == np.uint8 and u8.shape == (10, 10, 3) and u8.flags["C_CONTIGUOUS"]
    img = ds[1]["image"].numpy()
    want = np.clip(np.rint((img * STD + MEAN) * 255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(u8.transpose(2, 0, 1), want)
    inside = (u8 > 0) & (u8 < 255)  # where nothing was clipped the item comes back within half a grey level
    back = ((u8.astype(np.float32) / 255.0).transpose(2, 0, 1) - MEAN) / STD
    assert inside.any() and np.abs(back - img)[inside.transpose(2, 0, 1)].max() <= 0.5 / 255 / STD.min() + 1e-5
    assert np.array_equal(ds.source_u8(1), u8) and not np.array_equal(ds.source_u8(2), u8)


def test_visualize_needs_a_gpu(monkeypatch):
    import torch

    import forward_utils as fu
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no GPU is visible"):
        fu.visualize(np.zeros((1, 1, 4, 4), np.uint8), np.zeros((1, 4, 4), np.float32), ["a/b.png"], "out", "MVTec",
                     "bottle")
