"""Host-side checks of the F1-max feature (no GPU): tests/f1_ref.py, the float64 restatement the
GPU tests demand bits of, against a brute-force loop over the distinct thresholds, against
sklearn.metrics.precision_recall_curve and on hand-written cases; the two new entry points are
declared, bound and exported and reject bad arguments without a launch; the Python surface."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib

import f1_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_metrics_f1_workspace", "aaclip_metrics_eval_f1"]


# ---------------------------------------------------------------------------- the reference
def _brute(y, v):
    """The definition, threshold by threshold, ascending, keeping the first maximum."""
    y = np.asarray(y).ravel() != 0
    v = np.asarray(v, dtype=np.float32).ravel()
    P = int(y.sum())
    best = None
    for t in np.unique(v):
        hit = v >= t
        pp, tp = int(hit.sum()), int((hit & y).sum())
        f = float(2 * tp) / float(pp + P)
        if best is None or f > best[0]:
            best = (f, float(t), tp / pp, tp / P)
    return best


def _sklearn(y, v):
    """(F1-max, the thresholds that reach it within 1e-12) from precision_recall_curve, as the
    VAND code computes it: 2 p r / (p + r) over the curve."""
    from sklearn.metrics import precision_recall_curve
    p, r, thr = precision_recall_curve(np.asarray(y).ravel() != 0, np.asarray(v, dtype=np.float32).ravel())
    p, r = p[:-1].astype(np.float64), r[:-1].astype(np.float64)  # the last point has no threshold
    f1 = np.where(p + r > 0, 2 * p * r / np.where(p + r > 0, p + r, 1.0), 0.0)
    return float(f1.max()), {float(t) for t in thr[f1 >= f1.max() - 1e-12]}


def _random_case(seed, n, levels, frac):
    r = np.random.default_rng(seed)
    y = r.random(n) < frac
    y[0], y[1] = True, False
    v = r.standard_normal(n) + 0.8 * y
    if levels == 1:
        v = np.full(n, 0.25)
    elif levels:
        v = np.round((v - v.min()) / (v.max() - v.min()) * (levels - 1)) / (levels - 1)
    return y, v.astype(np.float32)


@pytest.mark.parametrize("levels", [1, 2, 8, 0])
@pytest.mark.parametrize("seed,n,frac", [(0, 12, 0.5), (1, 97, 0.1), (2, 400, 0.03), (3, 1000, 0.6)])
def test_f1_ref_matches_brute_force_and_sklearn(levels, seed, n, frac):
    y, v = _random_case(seed, n, levels, frac)
    got, want = FR.f1_max(y, v), _brute(y, v)
    assert got == want, (got, want)  # the same integers, the same divisions: the same bits
    sk_f1, sk_thr = _sklearn(y, v)
    assert abs(got[0] - sk_f1) <= 1e-12, (got, sk_f1)
    assert got[1] in sk_thr, (got, sorted(sk_thr)[:5])


def test_hand_written_tie_takes_the_lowest_threshold():
    y, v = [1, 0, 0, 1], [1.0, 0.75, 0.5, 0.0]
    # F1 at 0.0: 4 / 6; at 0.5: 2 / 5; at 0.75: 2 / 4; at 1.0: 2 / 3 -- two maximisers
    assert FR.f1_max(y, v) == (2 / 3, 0.0, 0.5, 1.0)
    assert _brute(y, v) == (2 / 3, 0.0, 0.5, 1.0)
    sk_f1, sk_thr = _sklearn(y, v)
    assert abs(sk_f1 - 2 / 3) <= 1e-12 and sk_thr == {0.0, 1.0}


def test_hand_written_small_cases():
    # one positive on top: perfect at its score
    assert FR.f1_max([0, 0, 1], [0.1, 0.2, 0.9]) == (1.0, float(np.float32(0.9)), 1.0, 1.0)
    # positives at both ends, negatives between: everything flagged beats the top one alone (4/5 > 2/3)
    assert FR.f1_max([1, 0, 1], [0.0, 0.5, 1.0]) == (0.8, 0.0, 2 / 3, 1.0)
    # a tie group holding both labels counts as one threshold
    assert FR.f1_max([1, 0, 0], [0.5, 0.5, 0.0]) == (2 / 3, 0.5, 0.5, 1.0)
    # -0.0 and +0.0 are one score, reported as +0.0
    got = FR.f1_max([1, 1], np.array([-0.0, 0.0], np.float32))
    assert got == (1.0, 0.0, 1.0, 1.0) and math.copysign(1.0, got[1]) == 1.0


def test_all_equal_scores():
    y = np.zeros((3, 9, 9), dtype=np.uint8)
    y[0, 1:4, 1:3] = 1
    n, P = y.size, int(y.sum())
    for const in (1.0, 0.5):
        f1, thr, prec, rec = FR.pixel_f1(y, np.full(y.shape, const, np.float32))
        assert f1 == (2 * P) / (n + P) and prec == P / n and rec == 1.0
        # 1.0 skips the normalisation; 0.5 normalises to 0 / 0, whose threshold is NaN
        assert thr == 1.0 if const == 1.0 else math.isnan(thr)


def test_separated_scores_and_no_positives():
    r = np.random.default_rng(0)
    y = np.zeros((2, 9, 9), dtype=np.uint8)
    y[1, 2:5, 3:7] = 1
    v = (r.random(y.shape) + 2.0 * y).astype(np.float32)
    f1, thr, prec, rec = FR.pixel_f1(y, v)
    lowest_positive = FR.normalise(v)[y != 0].min()
    assert (f1, prec, rec) == (1.0, 1.0, 1.0) and thr == float(lowest_positive)
    assert all(math.isnan(x) for x in FR.pixel_f1(np.zeros_like(y), v))
    assert all(math.isnan(x) for x in FR.pixel_f1(np.ones_like(y), v))
    assert FR.image_f1(v, [0.1, 0.2], [1, 1], False) == (0.0,) * 4
    assert FR.image_f1(v, [0.1, 0.2], [0, 0], True) == (0.0,) * 4


def test_fused_scores_are_float32_and_exact():
    v = np.arange(2 * 4 * 4, dtype=np.float32).reshape(2, 4, 4) / 8  # max 3.875: normalised
    ip = np.array([0.25, 0.75], np.float32)
    med, ind = FR.fused_scores(v, ip, True), FR.fused_scores(v, ip, False)
    assert med.dtype == ind.dtype == np.float32
    assert med.tolist() == [float(np.float32(15) / np.float32(31)), 1.0]
    assert ind.tolist() == [float(np.float32(0.5) * med[0]), 1.0]


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
    assert "forward_utils.py:233-280" in src and "F1(t)" in src and "LOWEST" in src


def test_argument_validation_rejects_without_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)  # non-null and 256-B aligned; never dereferenced on the host
    size = ctypes.c_size_t(0)
    for with_pro in (0, 1):
        assert lib.aaclip_metrics_f1_workspace(1000, 2, with_pro, None) == 1
        assert lib.aaclip_metrics_f1_workspace(0, 2, with_pro, ctypes.byref(size)) == 1
        assert lib.aaclip_metrics_f1_workspace(1000, 0, with_pro, ctypes.byref(size)) == 1
        assert lib.aaclip_metrics_f1_workspace(2 ** 32 - 1, 2, with_pro, ctypes.byref(size)) == 1

        def run(ptrs=(p,) * 6, n=2, h=20, w=25, limit=0.3, ws_bytes=1 << 20):
            return lib.aaclip_metrics_eval_f1(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, h, w, 0, with_pro, limit,
                                              ptrs[4], ws_bytes, ptrs[5], None)
        for bad in range(6):  # null pointers
            assert run(ptrs=tuple(None if i == bad else p for i in range(6))) == 1, bad
        assert run(n=0) == 1 and run(h=0) == 1 and run(w=-1) == 1  # empty shapes
        assert run(h=65536, w=32768) == 1 and run(h=2 ** 31 - 1, w=2 ** 31 - 1) == 1  # height * width >= 2^31
        assert run(n=4, h=32768, w=32768) == 1  # n >= 2^32 - 1
        # a workspace smaller than the per-pixel arrays alone (24 B per pixel, 32 with the areas), or misaligned
        assert run(ws_bytes=0) == 1 and run(ws_bytes=(32 if with_pro else 24) * 1000 - 1) == 1
        assert run(ptrs=(p, p, p, p, ctypes.c_void_p(256 + 64), p)) == 1
        if with_pro:  # (ignored without: tests/test_f1_gpu.py passes a bad one there)
            for limit in (0.0, 1.5, -0.3, float("nan")):
                assert run(limit=limit) == 1, limit


# ---------------------------------------------------------------------------- Python surface
def test_python_surface():
    import forward_utils as fu
    from aaclip import ops
    for fn in (ops.metrics_eval, ops.metrics_eval_device, fu.metrics_eval, fu.metrics_eval_deferred):
        assert inspect.signature(fn).parameters["f1"].default is False, fn
    import test as harness
    assert harness.parse_args([]).f1 is False and harness.parse_args(["--f1"]).f1 is True
    assert harness.parse_args(["--f1", "--pro"]).pro is True


def test_deferred_object_dict_and_values():
    """The object metrics_eval_deferred returns, built here on a host tensor: callable as before,
    .values() by name and unrounded."""
    import forward_utils as fu
    raw = [0.91234567, 0.5, 0.75, 0.25, 0.123456, 0.66666666, 0.375, 0.5, 1.0, 0.8, 0.625, 2 / 3, 1.0]
    base = ["class name", "pixel AUC", "pixel AP", "image AUC", "image AP"]
    for pro in (False, True):
        nums = raw if pro else raw[:4] + raw[5:]
        d = fu._DeferredMetrics(torch.tensor(nums, dtype=torch.float64), "cls", pro, True)
        assert callable(d) and callable(d.values)
        row, v = d(), d.values()
        assert list(row) == base + (["pixel AUPRO"] if pro else []) + ["pixel F1-max", "image F1-max"]
        assert row["pixel F1-max"] == round(raw[5], 4) * 100 and row["image F1-max"] == round(raw[9], 4) * 100
        assert row["pixel AUC"] == round(raw[0], 4) * 100 and row["class name"] == "cls"
        assert list(v) == base[1:] + (["pixel AUPRO"] if pro else []) + [
            "pixel F1-max", "pixel F1 threshold", "pixel F1 precision", "pixel F1 recall",
            "image F1-max", "image F1 threshold", "image F1 precision", "image F1 recall"]
        assert list(v.values()) == nums
    plain = fu._DeferredMetrics(torch.tensor(raw[:4], dtype=torch.float64), "cls", False, False)
    assert list(plain()) == base and list(plain.values()) == base[1:]
    nan = fu._DeferredMetrics(torch.tensor([float("nan")] * 2 + raw[2:4] + [float("nan")] * 4 + raw[9:],
                                           dtype=torch.float64), "cls", False, True)
    with pytest.raises(ValueError, match="Only one class present"):
        nan()
    assert math.isnan(nan.values()["pixel F1 threshold"]) and nan.values()["image F1-max"] == raw[9]
