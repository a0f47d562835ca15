"""Host-side checks of the region extraction (no GPU): tests/regions_ref.py, the scipy reference the
GPU tests demand exact equality with, on hand-drawn cases with known answers; the two entry points
are declared, bound and exported and reject bad arguments without a launch; the Python surface.

The ABI version stays 9: seven earlier test files pin it, and the project's rule for additions
(include/aaclip.h) is that the loader refuses a library that lacks a symbol it binds."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from aaclip import _lib

import regions_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_regions_workspace", "aaclip_extract_regions"]


def _draw(H, W, *boxes):
    """Raw fp32 scores: 0 everywhere, 0.5 inside the (y0, y1, x0, x1) half-open boxes."""
    v = np.zeros((H, W), np.float32)
    for y0, y1, x0, x1 in boxes:
        v[y0:y1, x0:x1] = 0.5
    return v


# ---------------------------------------------------------------------------- the reference
def test_two_squares_touching_at_a_corner_are_one_region():
    v = _draw(8, 9, (1, 3, 1, 3), (3, 5, 3, 5))
    got = RR.image_regions(v, 0.5)
    assert len(got) == 1
    assert got[0]["label"] == 1 * 9 + 1 + 1 and got[0]["area"] == 8 and got[0]["bbox"] == [1, 1, 4, 4]
    assert got[0]["centroid"] == [2.5, 2.5]
    # one pixel further apart they are two, equal in area: ordered by label
    two = RR.image_regions(_draw(8, 9, (1, 3, 1, 3), (3, 5, 4, 6)), 0.5)
    assert [g["label"] for g in two] == [1 * 9 + 1 + 1, 3 * 9 + 4 + 1] and [g["area"] for g in two] == [4, 4]


def test_l_shape_bbox_centroid_and_peak_index():
    v = _draw(7, 10, (1, 5, 2, 3), (4, 5, 3, 6))  # a 4-pixel column at x = 2, a 3-pixel foot to its right
    v[2, 2] = v[4, 4] = 0.75  # two pixels share the peak: the first in row-major order counts
    gt = np.zeros((7, 10), np.uint8)
    gt[4:, 3:] = 1
    (g,) = RR.image_regions(v, 0.5, gt)
    assert g["label"] == 1 * 10 + 2 + 1 and g["area"] == 7 and g["bbox"] == [2, 1, 5, 4]
    assert g["centroid"] == [(4 * 2 + 3 + 4 + 5) / 7, (1 + 2 + 3 + 4 + 3 * 4) / 7]
    assert g["peak"] == np.float32(0.75) and g["peak_index"] == 2 * 10 + 2 and g["gt_area"] == 3
    # >= : a threshold equal to the peak keeps exactly the two peak pixels, as two regions
    assert [r["peak_index"] for r in RR.image_regions(v, 0.75)] == [2 * 10 + 2, 4 * 10 + 4]
    assert RR.image_regions(v, np.nextafter(np.float32(0.75), np.float32(1))) == []


def test_area_order_ties_by_label_min_area_and_max_regions():
    v = np.stack([_draw(9, 12, (0, 2, 0, 2), (0, 3, 4, 7), (5, 7, 0, 2), (5, 6, 5, 6), (8, 9, 11, 12)),
                  np.zeros((9, 12), np.float32)])
    every = RR.image_regions(v[0], 0.5)
    assert [(g["area"], g["label"]) for g in every] == [(9, 5), (4, 1), (4, 5 * 12 + 1), (1, 5 * 12 + 6), (1, 8 * 12 + 12)]
    assert [g["area"] for g in RR.image_regions(v[0], 0.5, min_area=4)] == [9, 4, 4]
    out = RR.extract(v, 0.5, normalise=False, min_area=2, max_regions=2)
    assert out["n_regions"].tolist() == [3, 0]  # the filtered total, not the listed ones
    assert out["area"].tolist() == [[9, 4], [0, 0]] and out["label"].tolist() == [[5, 1], [0, 0]]
    wide = RR.extract(v, 0.5, normalise=False, max_regions=7)
    assert wide["n_regions"].tolist() == [5, 0] and wide["area"][0].tolist() == [9, 4, 4, 1, 1, 0, 0]
    assert not wide["bbox"][0, 5:].any() and not wide["centroid"][0, 5:].any() and not wide["peak"][0, 5:].any()
    entries = RR.as_entries(v, 0.5, normalise=False, max_regions=2)
    assert entries[1] == {"n_regions": 0, "regions": []} and entries[0]["n_regions"] == 5
    assert [g["bbox"] for g in entries[0]["regions"]] == [[4, 0, 6, 2], [0, 0, 1, 1]]
    assert list(entries[0]["regions"][0]) == ["label", "area", "bbox", "centroid", "peak", "peak_xy", "gt_area"]


def test_normalisation_is_the_metrics_one_and_nan_is_background():
    v = np.stack([_draw(5, 6, (1, 3, 1, 4)), np.zeros((5, 6), np.float32)])  # class range [0, 0.5]
    assert RR.scores(v).max() == 1.0 and RR.extract(v, 1.0)["area"][:, 0].tolist() == [6, 0]
    assert RR.extract(v, 0.75, normalise=False)["n_regions"].tolist() == [0, 0]
    top1 = v * 2  # class maximum exactly 1: taken as it is
    assert RR.scores(top1) is not None and (RR.scores(top1) == top1).all()
    flat = np.full((2, 5, 6), 0.25, np.float32)  # constant: 0 / 0, no region whatever the threshold
    assert np.isnan(RR.scores(flat)).all()
    assert RR.extract(flat, 0.0)["n_regions"].tolist() == [0, 0]
    assert RR.extract(flat, 0.25, normalise=False)["area"][:, 0].tolist() == [30, 30]
    assert RR.extract(np.ones((2, 5, 6), np.float32), 1.0)["area"][:, 0].tolist() == [30, 30]  # constant 1: raw
    holed = _draw(5, 6, (0, 5, 0, 6))
    holed[2, 3] = np.nan
    assert RR.image_regions(holed, 0.5)[0]["area"] == 29


# ---------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert lib.aaclip_abi_version() == _lib.ABI_VERSION
    assert "regions.hip" in open(os.path.join(ROOT, "aa-clip_amd", "csrc", "Makefile")).read()
    assert "area descending" in src and "0xFFFFFFFF" in src and "scorenorm.h" in src


def test_argument_validation_rejects_without_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)  # non-null and 256-B aligned; never dereferenced on the host
    size = ctypes.c_size_t(0)
    assert lib.aaclip_regions_workspace(1000, 2, None) == 1
    assert lib.aaclip_regions_workspace(0, 2, ctypes.byref(size)) == 1
    assert lib.aaclip_regions_workspace(1000, 0, ctypes.byref(size)) == 1
    assert lib.aaclip_regions_workspace(1001, 2, ctypes.byref(size)) == 1  # not n_images equal images
    assert lib.aaclip_regions_workspace(2 ** 32 - 1, 3, ctypes.byref(size)) == 1

    def run(ptrs=(p,) * 11, n=2, h=20, w=25, thr=0.5, normalise=1, min_area=1, max_regions=4, ws_bytes=1 << 20):
        return lib.aaclip_extract_regions(ptrs[0], ptrs[1], n, h, w, thr, normalise, min_area, max_regions, ptrs[2],
                                          ws_bytes, *ptrs[3:], None)
    for bad in [0] + list(range(2, 11)):  # null pointers (the label pointer, 1, may be null)
        assert run(ptrs=tuple(None if i == bad else p for i in range(11))) == 1, bad
    assert run(n=0) == 1 and run(h=0) == 1 and run(w=-1) == 1  # empty shapes
    assert run(h=65536, w=32768) == 1 and run(n=4, h=32768, w=32768) == 1  # the labelling's size limits
    assert run(min_area=0) == 1 and run(max_regions=0) == 1 and run(n=2, max_regions=2 ** 30) == 1
    assert run(ws_bytes=0) == 1 and run(ws_bytes=17 * 1000 - 1) == 1  # smaller than the pixel arrays alone
    assert run(ptrs=(p, p, ctypes.c_void_p(256 + 64)) + (p,) * 8) == 1  # a misaligned workspace


# ---------------------------------------------------------------------------- Python surface
def test_python_surface():
    import forward_utils as fu
    from aaclip import ops
    for fn in (ops.extract_regions, fu.anomaly_regions):
        par = inspect.signature(fn).parameters
        assert par["normalise"].default is True and par["min_area"].default == 1 and par["max_regions"].default == 64
        assert par["normalise"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(fu.anomaly_regions).parameters)[:3] == ["pixel_preds", "threshold", "pixel_label"]
    import test as harness
    off, on = harness.parse_args([]), harness.parse_args(["--regions"])
    assert off.regions is False and off.f1 is False
    assert on.regions is True and on.f1 is True and on.regions_min_area == 1 and on.regions_max == 64
    assert harness.parse_args(["--f1"]).regions is False
    got = harness.parse_args(["--regions", "--regions_min_area", "5", "--regions_max", "3"])
    assert (got.regions_min_area, got.regions_max) == (5, 3)


def test_anomaly_regions_needs_a_gpu(monkeypatch):
    import torch

    import forward_utils as fu
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no GPU is visible"):
        fu.anomaly_regions(np.zeros((1, 4, 4), np.float32), 0.5)
