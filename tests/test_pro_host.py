"""Host-side checks of the pixel AUPRO feature (no GPU): tests/pro_ref.py, the float64
restatement the GPU tests compare with, against a brute-force loop over the distinct
thresholds and on hand-written masks; the three new entry points are declared, bound and
exported and reject bad arguments without a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from aaclip import _lib

import pro_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_label_components", "aaclip_metrics_pro_workspace", "aaclip_metrics_eval_pro"]


# ---------------------------------------------------------------------------- the references
def _brute_aupro(masks, scores, L):
    """The definition, threshold by threshold: per-region fractions and the ok-pixel fraction
    at every distinct score, then trapezoids with interpolation at L."""
    masks = np.asarray(masks) != 0
    s = PR.normalise(scores).astype(np.float64)
    labels, _, counts = PR.label_ref(masks)
    regions = [(i, v) for i in range(masks.shape[0]) for v in np.unique(labels[i]) if v]
    n_ok = (~masks).sum()
    pts = [(0.0, 0.0)]
    for t in sorted(np.unique(s), reverse=True):
        hit = s >= t
        fpr = (hit & ~masks).sum() / n_ok
        pro = sum((hit[i] & (labels[i] == v)).sum() / (labels[i] == v).sum() for i, v in regions) / len(regions)
        pts.append((fpr, pro))
    pts.append((1.0, 1.0))
    assert len(regions) == counts.sum()
    area = 0.0
    for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]):
        if x0 >= L or x1 == x0:
            continue
        xe = min(x1, L)
        ye = y0 + (y1 - y0) * (xe - x0) / (x1 - x0)
        area += (xe - x0) * (y0 + ye) / 2.0
    return area / L


def _small_case(levels):
    r = np.random.default_rng(5)
    masks = np.zeros((3, 9, 9), dtype=np.uint8)
    masks[0, 1:4, 1:3] = 1
    masks[0, 6, 6] = 1
    masks[0, 7, 7] = 1  # diagonal contact: one component with (6, 6)
    masks[1, 0, 8] = 1
    masks[1, 1, 0] = 1  # row end / row start: two components
    masks[1, 5:8, 4] = 1
    scores = r.standard_normal((3, 9, 9)) + 1.2 * masks
    scores = (np.round(scores * levels) / levels).astype(np.float32)
    return masks, scores


@pytest.mark.parametrize("levels", [1, 2, 8])
@pytest.mark.parametrize("L", [0.05, 0.3, 1.0])
def test_aupro_ref_matches_brute_force(levels, L):
    masks, scores = _small_case(levels)
    assert PR.label_ref(masks)[2].tolist() == [2, 3, 0]
    assert abs(PR.aupro_ref(masks, scores, L) - _brute_aupro(masks, scores, L)) <= 1e-12


def test_aupro_ref_all_equal_and_separated():
    masks, _ = _small_case(1)
    for const in (1.0, 0.5):  # 1.0 skips the normalisation; 0.5 normalises to one tie group
        assert abs(PR.aupro_ref(masks, np.full(masks.shape, const, np.float32), 0.3) - 0.15) <= 1e-12
        assert abs(PR.aupro_ref(masks, np.full(masks.shape, const, np.float32), 1.0) - 0.5) <= 1e-12
    sep = np.random.default_rng(0).random(masks.shape).astype(np.float32) + 2.0 * masks
    for L in (0.05, 0.3, 1.0):
        assert abs(PR.aupro_ref(masks, sep, L) - 1.0) <= 1e-12
    assert np.isnan(PR.aupro_ref(np.zeros_like(masks), sep, 0.3))
    assert np.isnan(PR.aupro_ref(np.ones_like(masks), sep, 0.3))


def test_label_ref_hand_written():
    m = np.array([[[1, 0, 0, 0, 0],
                   [0, 1, 0, 0, 1],
                   [1, 0, 0, 0, 0],
                   [0, 0, 0, 1, 1],
                   [0, 0, 1, 0, 0]]], dtype=np.uint8)
    labels, areas, counts = PR.label_ref(m)
    # diagonal contact joins: (0,0)-(1,1)-(2,0) and (4,2)-(3,3)-(3,4); (1,4) and (2,0) do not
    # join across the row end, so (1,4) stands alone
    assert counts.tolist() == [3]
    assert labels[0].tolist() == [[1, 0, 0, 0, 0],
                                  [0, 1, 0, 0, 10],
                                  [1, 0, 0, 0, 0],
                                  [0, 0, 0, 19, 19],
                                  [0, 0, 19, 0, 0]]
    assert areas[0].tolist() == [[3, 0, 0, 0, 0],
                                 [0, 3, 0, 0, 1],
                                 [3, 0, 0, 0, 0],
                                 [0, 0, 0, 3, 3],
                                 [0, 0, 3, 0, 0]]
    # no wrap across the row end: column W-1 of row y and column 0 of row y+1
    w = np.zeros((1, 5, 5), dtype=np.uint8)
    w[0, 1, 4] = w[0, 2, 0] = 1
    labels, areas, counts = PR.label_ref(w)
    assert counts.tolist() == [2] and labels[0, 1, 4] == 10 and labels[0, 2, 0] == 11 and areas.max() == 1


# ---------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9  # additions only
    assert "forward_utils.py:233-280" in src and "PRO(t)" in src


def test_argument_validation_rejects_without_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)  # non-null and 256-B aligned; never dereferenced on the host
    size = ctypes.c_size_t(0)
    # labelling: null pointers, empty shapes, height * width >= 2^31, n * height * width >= 2^32 - 1
    for bad in range(4):
        ptrs = [None if i == bad else p for i in range(4)]
        assert lib.aaclip_label_components(ptrs[0], 2, 8, 8, ptrs[1], ptrs[2], ptrs[3], None) == 1
    assert lib.aaclip_label_components(p, 0, 8, 8, p, p, p, None) == 1
    assert lib.aaclip_label_components(p, 1, 0, 8, p, p, p, None) == 1
    assert lib.aaclip_label_components(p, 1, 65536, 32768, p, p, p, None) == 1
    assert lib.aaclip_label_components(p, 1, 2 ** 31 - 1, 2 ** 31 - 1, p, p, p, None) == 1
    assert lib.aaclip_label_components(p, 4, 32768, 32768, p, p, p, None) == 1
    # workspace query
    assert lib.aaclip_metrics_pro_workspace(1000, 2, None) == 1
    assert lib.aaclip_metrics_pro_workspace(0, 2, ctypes.byref(size)) == 1
    assert lib.aaclip_metrics_pro_workspace(1000, 0, ctypes.byref(size)) == 1
    assert lib.aaclip_metrics_pro_workspace(2 ** 32 - 1, 2, ctypes.byref(size)) == 1

    def run(ptrs=(p,) * 6, n=2, h=20, w=25, limit=0.3, ws_bytes=1 << 20):
        return lib.aaclip_metrics_eval_pro(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, h, w, 0, limit, ptrs[4],
                                           ws_bytes, ptrs[5], None)
    for bad in range(6):  # null pointers
        assert run(ptrs=tuple(None if i == bad else p for i in range(6))) == 1, bad
    for limit in (0.0, 1.5, -0.3, float("nan")):
        assert run(limit=limit) == 1, limit
    assert run(h=65536, w=65536) == 1 and run(h=2 ** 31 - 1, w=2 ** 31 - 1) == 1  # height * width overflow
    assert run(n=4, h=32768, w=32768) == 1
    assert run(n=0) == 1 and run(h=0) == 1 and run(w=-1) == 1
    # a workspace smaller than the per-pixel arrays alone (32 B per pixel), or misaligned
    assert run(ws_bytes=0) == 1 and run(ws_bytes=32 * 1000 - 1) == 1
    assert run(ptrs=(p, p, p, p, ctypes.c_void_p(256 + 64), p)) == 1


def test_python_surface():
    import inspect

    import forward_utils as fu
    from aaclip import ops
    for fn in (ops.metrics_eval, ops.metrics_eval_device):
        sig = inspect.signature(fn).parameters
        assert sig["pro"].default is False and sig["fpr_limit"].default == 0.3
    for fn in (fu.metrics_eval, fu.metrics_eval_deferred):
        assert inspect.signature(fn).parameters["pro"].default is False
    assert callable(ops.label_components)
    import test as harness
    assert harness.parse_args([]).pro is False and harness.parse_args(["--pro"]).pro is True
