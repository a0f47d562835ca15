"""F1-max and its threshold on the MI355X (aaclip_metrics_eval_f1) against the float64 restatement
of tests/f1_ref.py: bit for bit wherever the fp32 normalisation is exact (score grids, block
seams, ties across blocks), within 1e-9 / one fp32 ulp for continuous scores; the leading numbers
unchanged in bits; degenerate inputs; the drop-in dict and the harness's --f1 columns.
"Same bits" lets any NaN stand for any NaN: a NaN's sign and payload carry no meaning."""
import json
import math
import struct

import numpy as np
import pytest
import torch
from scipy import ndimage

from aaclip import ops

import f1_ref as FR

pytestmark = pytest.mark.gpu

NAMES = ["F1-max", "threshold", "precision", "recall"]


def _bits(xs):
    return ["nan" if x != x else struct.pack("<d", x).hex() for x in xs]


def _blobs(seed, N, S, sigma=2.5, q=0.9):
    """Smooth random blobs (a thresholded blurred noise field); the last image is defect-free."""
    r = np.random.default_rng(seed)
    field = np.stack([ndimage.gaussian_filter(r.standard_normal((S, S)), sigma) for _ in range(N)])
    masks = (field > np.quantile(field, q)).astype(np.uint8)
    masks[-1] = 0
    scores = (field / field.std() + 0.8 * r.standard_normal((N, S, S))).astype(np.float32)
    return masks, scores


def _with_images(masks, scores, seed=0):
    N = masks.shape[0]
    ip = np.random.default_rng(seed).random(N).astype(np.float32)
    il = (masks.reshape(N, -1).max(1) > 0).astype(np.int64)
    return masks, scores, ip, il


def _grid(scores, levels, top):
    """`levels` values k / 16 in [0, 1] that include 0 and 1, times top: top = 1 skips the
    normalisation (class maximum 1), top = 2 gives k / 8 in [0, 2], normalised by an exact division."""
    lo, hi = scores.min(), scores.max()
    j = np.floor((scores - lo) / (hi - lo) * levels).clip(0, levels - 1)
    k = np.round(j * 16 / (levels - 1))
    assert len(np.unique(k)) == levels and k.min() == 0 and k.max() == 16
    return (k / 16 * top).astype(np.float32)


def _separated(masks, top, seed=2):
    r = np.random.default_rng(seed)
    k = np.where(masks != 0, r.integers(9, 17, masks.shape), r.integers(0, 8, masks.shape)).astype(np.float64)
    pos, neg = np.argwhere(masks != 0)[0], np.argwhere(masks == 0)[0]
    k[tuple(pos)], k[tuple(neg)] = 16, 0
    return (k / 16 * top).astype(np.float32)


GRID = [f"{lv} levels, top {top}" for lv in (2, 4, 16) for top in (1, 2)] + [
    "all equal 1.0", "all equal 0.5", "separated, top 1", "separated, top 2"]


@pytest.fixture(scope="module")
def cases():
    masks, scores = _blobs(11, 4, 37)
    out = {"continuous": _with_images(masks, scores)}
    for lv in (2, 4, 16):
        for top in (1, 2):
            out[f"{lv} levels, top {top}"] = _with_images(masks, _grid(scores, lv, top))
    out["all equal 1.0"] = _with_images(masks, np.ones_like(scores))
    out["all equal 0.5"] = _with_images(masks, np.full_like(scores, 0.5))
    for top in (1, 2):
        out[f"separated, top {top}"] = _with_images(masks, _separated(masks, top))
    m3, s3 = _blobs(12, 3, 37)
    out["continuous, 3 maps"] = _with_images(m3, s3, seed=1)
    return out


def _tensors(dev, case):
    masks, scores, ip, il = case
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (scores, masks, ip, il)]


def _device(dev, case, medical=False, pro=False, **kw):
    out = ops.metrics_eval_device(*_tensors(dev, case), medical=medical, pro=pro, f1=True, **kw)
    assert out.dtype == torch.float64 and out.shape == (13 if pro else 12,)
    return out.tolist()


def _check_bits(dev, case, medical, what):
    got = _device(dev, case, medical)[4:]
    want = FR.all_eight(*case, medical)
    for level, g, w in (("pixel", got[:4], want[:4]), ("image", got[4:], want[4:])):
        print(what, "medical" if medical else "industrial", level, dict(zip(NAMES, g)), "reference", w)
    assert _bits(got) == _bits(want), (what, medical, got, want)
    return got


# ---------------------------------------------------------------------------- bits on exact grids
@pytest.mark.parametrize("medical", [False, True])
@pytest.mark.parametrize("name", GRID)
def test_f1_grid_cases_bit_equal(dev, cases, name, medical):
    case = cases[name]
    got = _check_bits(dev, case, medical, name)
    n, P = case[0].size, int(case[0].sum())
    if name.startswith("all equal"):
        assert got[0] == (2 * P) / (n + P) and got[2] == P / n and got[3] == 1.0
        assert got[1] == 1.0 if name.endswith("1.0") else math.isnan(got[1])
    if name.startswith("separated"):
        assert got[0] == 1.0 and got[2] == 1.0 and got[3] == 1.0


@pytest.mark.parametrize("medical", [False, True])
@pytest.mark.parametrize("name", ["continuous", "continuous, 3 maps"])
def test_f1_continuous_scores(dev, cases, name, medical):
    case = cases[name]
    got = _device(dev, case, medical)[4:]
    want = FR.all_eight(*case, medical)
    print(name, medical, "device", got, "reference", want, "bit-equal", _bits(got) == _bits(want))
    for at in (0, 4):
        f1, thr, prec, rec = got[at:at + 4]
        assert abs(f1 - want[at]) <= 1e-9
        assert abs(thr - want[at + 1]) <= float(np.spacing(np.float32(abs(want[at + 1]))))
        assert abs(prec - want[at + 2]) <= 1e-9 and abs(rec - want[at + 3]) <= 1e-9


# ---------------------------------------------------------------------------- block seams
N_SEAM, SEAM_SHAPE = 24000, (3, 80, 100)  # two blocks of the candidate pass: 16384 + 7616 sorted positions


def _scatter(values, labels, seed):
    """Values and labels given in any order, scattered over the maps by a fixed permutation."""
    perm = np.random.default_rng(seed).permutation(N_SEAM)
    v, y = np.empty(N_SEAM, np.float32), np.empty(N_SEAM, np.uint8)
    v[perm], y[perm] = values, labels
    ip = np.random.default_rng(seed + 1).random(3).astype(np.float32)
    return y.reshape(SEAM_SHAPE), v.reshape(SEAM_SHAPE), ip, np.array([1, 0, 1])


def _ladder(n_pos):
    """24000 distinct scores k / 32768 with the top one 1.0 (no normalisation), the n_pos highest
    positive: F1 = 1 only at sorted position 24000 - n_pos."""
    v = np.arange(N_SEAM, dtype=np.float64) / 32768
    v[-1] = 1.0
    y = np.zeros(N_SEAM, np.uint8)
    y[N_SEAM - n_pos:] = 1
    return v.astype(np.float32), y


@pytest.mark.parametrize("n_pos,block", [(12000, 0), (100, 1), (7616, 1), (7617, 0)])
def test_f1_unique_maximiser_in_either_block(dev, n_pos, block):
    v, y = _ladder(n_pos)
    at = N_SEAM - n_pos
    assert at // 16384 == block
    got = _check_bits(dev, _scatter(v, y, n_pos), False, f"maximiser at sorted position {at}")
    assert got[:4] == [1.0, float(v[at]), 1.0, 1.0]


def test_f1_one_tie_group_leaves_a_block_without_candidate(dev):
    y = (np.arange(N_SEAM) % 7 == 0).astype(np.uint8)
    P = int(y.sum())
    got = _check_bits(dev, _scatter(np.ones(N_SEAM, np.float32), y, 5), False, "one tie group")
    assert got[:4] == [(2 * P) / (N_SEAM + P), 1.0, P / N_SEAM, 1.0]


def test_f1_tie_across_blocks_takes_the_lowest_threshold(dev):
    """Group starts at sorted positions 0 (block 0) and 18000 (block 1) both reach 2 / 3."""
    v = np.r_[np.full(6000, 1.0), np.full(6000, 0.75), np.full(6000, 0.5), np.full(6000, 0.0)].astype(np.float32)
    y = np.r_[np.ones(6000), np.zeros(12000), np.ones(6000)].astype(np.uint8)
    for medical in (False, True):
        got = _check_bits(dev, _scatter(v, y, 9), medical, "cross-block tie")
        assert got[:4] == [2 / 3, 0.0, 0.5, 1.0]
        assert math.copysign(1.0, got[1]) == 1.0


@pytest.mark.parametrize("n_img", [300, 256, 257])
def test_f1_images_over_two_blocks_of_the_image_pass(dev, n_img):
    """More than 256 images (two blocks of the image kernel), tiny maps and scores on grids that
    keep the fused fp32 score exact: many ties among images, bits demanded. The best threshold's
    image is moved from block to block by reversing the order of the images."""
    r = np.random.default_rng(n_img)
    il = (r.random(n_img) < 0.4).astype(np.int64)
    scores = (r.integers(0, 9, (n_img, 4, 4)) + 4 * il[:, None, None] * (r.random((n_img, 1, 1)) < 0.7)) / 16
    scores = scores.clip(0, 1).astype(np.float32)
    scores[0, 0, 0], scores[1, 0, 0] = 0.0, 1.0  # class minimum 0, maximum 1: no normalisation
    masks = ((scores > 0.5) & (il[:, None, None] != 0)).astype(np.uint8)
    ip = (r.integers(0, 9, n_img) / 8).astype(np.float32)
    ip[2], ip[3] = 0.0, 1.0
    for flip in (False, True):
        case = tuple(x[::-1].copy() for x in (masks, scores, ip, il)) if flip else (masks, scores, ip, il)
        for medical in (False, True):
            got = _check_bits(dev, case, medical, f"{n_img} images")
            assert 0.0 < got[4] < 1.0  # a curve with a real maximum, not a separated one


def test_f1_image_tie_across_blocks_takes_the_lowest_score(dev):
    """Image scores 1.0 (positive), 0.75 / 0.5 (negative), 0.0 (positive), 75 each: thresholds 0.0
    and 1.0 both reach 2 / 3, and their images sit in different blocks of the image pass."""
    lv = np.r_[np.full(75, 1.0), np.full(75, 0.75), np.full(75, 0.5), np.full(75, 0.0)].astype(np.float32)
    il = np.r_[np.ones(75), np.zeros(150), np.ones(75)].astype(np.int64)
    scores = np.zeros((300, 4, 4), np.float32)
    scores[:, 1, 2] = lv  # the row maximum; Medical fuses to it
    masks = np.zeros((300, 4, 4), np.uint8)
    masks[:, 1, 2] = il
    for flip in (False, True):
        case = (masks, scores, lv, il)
        if flip:
            case = tuple(x[::-1].copy() for x in case)
        for medical in (False, True):  # Industrial: 0.5 * lv + 0.5 * lv, the same scores
            got = _check_bits(dev, case, medical, "image tie across blocks")
            assert got[4:] == [2 / 3, 0.0, 0.5, 1.0]


# ---------------------------------------------------------------------------- unchanged bits
@pytest.mark.parametrize("name", ["continuous", "4 levels, top 2", "all equal 0.5", "separated, top 1"])
def test_f1_leaves_the_other_numbers_bit_identical(dev, cases, name):
    case = cases[name]
    t = _tensors(dev, case)
    flat = [t[0].reshape(4, -1), t[1].reshape(4, -1), t[2], t[3]]
    for medical in (False, True):
        plain = ops.metrics_eval_device(*t, medical=medical).tolist()
        pro = ops.metrics_eval_device(*t, medical=medical, pro=True).tolist()
        f1 = _device(dev, case, medical)
        f1_pro = _device(dev, case, medical, pro=True)
        assert len(plain) == 4 and len(pro) == 5
        assert _bits(f1[:4]) == _bits(plain) and _bits(f1_pro[:5]) == _bits(pro)
        assert _bits(f1_pro[5:]) == _bits(f1[4:])  # the same F1 numbers with and without the AUPRO
        assert _bits(_device(dev, case, medical)) == _bits(f1)  # two launches, the same bits
        assert _bits(_device(dev, case, medical, pro=True)) == _bits(f1_pro)
        # flattened maps stay legal without pro; fpr_limit is ignored without pro
        again = ops.metrics_eval_device(*flat, medical=medical, f1=True, fpr_limit=7.0).tolist()
        assert _bits(again) == _bits(f1)
        assert _bits(ops.metrics_eval(*t, medical=medical, f1=True)) == _bits(f1)
    with pytest.raises(ValueError, match="H, W"):
        ops.metrics_eval_device(*flat, medical=False, pro=True, f1=True)
    with pytest.raises(ValueError, match="fpr_limit"):
        ops.metrics_eval_device(*t, medical=False, pro=True, f1=True, fpr_limit=0.0)


# ---------------------------------------------------------------------------- 518 x 518
def test_f1_518(dev):
    """4 maps of 518 x 518 (4-byte arrays that are no multiple of 256 B), 512 score levels whose
    class maximum is 511 / 512: normalised by an inexact division, so held as the continuous cases."""
    masks, scores = _blobs(12, 4, 518, sigma=9.0, q=0.97)
    lo, hi = scores.min(), scores.max()
    scores = (np.floor((scores - lo) / (hi - lo) * 512).clip(0, 511) / 512).astype(np.float32)
    case = _with_images(masks, scores)
    want_px = FR.pixel_f1(masks, scores)
    for medical in (False, True):
        got = _device(dev, case, medical, pro=medical)
        got = got[5:] if medical else got[4:]
        want = want_px + FR.image_f1(scores, case[2], case[3], medical)
        print("518", medical, "device", got, "reference", want, "bit-equal", _bits(got) == _bits(want))
        for at in (0, 4):
            assert abs(got[at] - want[at]) <= 1e-9
            assert abs(got[at + 1] - want[at + 1]) <= float(np.spacing(np.float32(abs(want[at + 1]))))
            assert abs(got[at + 2] - want[at + 2]) <= 1e-9 and abs(got[at + 3] - want[at + 3]) <= 1e-9


# ---------------------------------------------------------------------------- degenerate inputs
@pytest.mark.parametrize("fill", [0, 1])
def test_f1_one_pixel_class_is_nan(dev, cases, fill):
    from forward_utils import metrics_eval
    masks, scores, ip, il = cases["continuous"]
    masks = np.full_like(masks, fill)
    for pro in (False, True):
        out = _device(dev, (masks, scores, ip, il), pro=pro)
        assert np.isnan(out[0]) and all(np.isnan(x) for x in out[-8:-4]), out
        assert _bits(out[-4:]) == _bits(FR.image_f1(scores, ip, il, False))  # the image numbers stand
        with pytest.raises(ValueError, match="Only one class present"):
            metrics_eval(masks[:, None], il, scores, ip, "c", "Industrial", pro=pro, f1=True)


@pytest.mark.parametrize("fill", [0, 1])
def test_f1_equal_image_labels_give_zeros(dev, cases, fill):
    masks, scores, ip, il = cases["4 levels, top 1"]
    il = np.full_like(il, fill)
    for medical in (False, True):
        out = _device(dev, (masks, scores, ip, il), medical)
        assert out[2:4] == [0.0, 0.0] and out[8:] == [0.0] * 4, out
        assert _bits(out[4:8]) == _bits(FR.pixel_f1(masks, scores))


# ---------------------------------------------------------------------------- public API, harness
BASE = ["class name", "pixel AUC", "pixel AP", "image AUC", "image AP"]


def test_forward_utils_f1_dict(dev, cases):
    from forward_utils import metrics_eval, metrics_eval_deferred
    masks, scores, ip, il = cases["16 levels, top 2"]
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (masks[:, None], il, scores, ip)]
    want = FR.all_eight(masks, scores, ip, il, False)
    plain = metrics_eval(*t, "cls", "Industrial")
    assert list(plain) == BASE
    r = metrics_eval(*t, "cls", "Industrial", f1=True)
    assert list(r) == BASE + ["pixel F1-max", "image F1-max"]
    rp = metrics_eval(*t, "cls", "Industrial", pro=True, f1=True)
    assert list(rp) == BASE + ["pixel AUPRO", "pixel F1-max", "image F1-max"]
    assert rp == {**metrics_eval(*t, "cls", "Industrial", pro=True), "pixel F1-max": r["pixel F1-max"],
                  "image F1-max": r["image F1-max"]}
    assert all(r[k] == plain[k] for k in plain)
    assert r["pixel F1-max"] == round(want[0], 4) * 100 and r["image F1-max"] == round(want[4], 4) * 100
    # numpy inputs, as the reference passes them
    assert metrics_eval(masks[:, None], il, scores, ip, "cls", "Industrial", f1=True) == r
    d = metrics_eval_deferred(*t, "cls", "Industrial", pro=True, f1=True)
    assert d() == rp
    v = d.values()
    assert list(v) == BASE[1:] + ["pixel AUPRO"] + [f"{lv} F1{w}" for lv in ("pixel", "image")
                                                    for w in ("-max", " threshold", " precision", " recall")]
    assert _bits([v[f"{lv} F1{w}"] for lv in ("pixel", "image") for w in ("-max", " threshold", " precision",
                                                                          " recall")]) == _bits(want)
    assert list(metrics_eval_deferred(*t, "cls", "Industrial").values()) == BASE[1:]


@pytest.mark.parametrize("pro", [False, True])
def test_harness_f1_columns(dev, tmp_path, caplog, pro):
    import logging

    import test as harness
    from dataset import DOMAINS
    caplog.set_level(logging.INFO)
    path = tmp_path / "table.json"
    args = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4", "--f1",
            "--save_path", str(tmp_path), "--results_json", str(path)] + (["--pro"] if pro else [])
    df, ctx = harness.run(harness.parse_args(args))
    cols = ["pixel F1-max", "image F1-max"]
    assert list(df.columns) == BASE + (["pixel AUPRO"] if pro else []) + cols
    assert df.iloc[-1]["class name"] == "Average" and len(df) == len(ctx["classes"]) + 1
    assert list(ctx["operating_points"]) == list(ctx["classes"])
    medical = DOMAINS["synthetic"] == "Medical"
    seen = {c: [] for c in cols}
    for cls, (masks, labels, preds, preds_image) in ctx["classes"].items():
        want = FR.all_eight(masks.cpu().numpy(), preds.cpu().numpy(), preds_image.cpu().numpy(), labels, medical)
        row, op = df[df["class name"] == cls].iloc[0], ctx["operating_points"][cls]
        print(cls, dict(row), op, want)
        for level, at in (("pixel", 0), ("image", 4)):
            assert abs(float(row[f"{level} F1-max"]) - round(want[at], 4) * 100) <= 1e-9 * 100
            seen[f"{level} F1-max"].append(float(row[f"{level} F1-max"]))
            assert list(op[level]) == ["threshold", "precision", "recall"]
            assert abs(op[level]["threshold"] - want[at + 1]) <= float(np.spacing(np.float32(abs(want[at + 1]))))
            assert abs(op[level]["precision"] - want[at + 2]) <= 1e-9
            assert abs(op[level]["recall"] - want[at + 3]) <= 1e-9
    for c in cols:
        assert abs(float(df.iloc[-1][c]) - np.mean(seen[c])) <= 1e-9
    table = json.loads(path.read_text())
    assert table["operating_points"] == ctx["operating_points"]
    assert [abs(r[c] - s) <= 1e-9 for c in cols for r, s in zip(table["rows"], seen[c])] == [True] * (2 * len(seen[cols[0]]))
    for cls in ctx["classes"]:  # one log line per class with both operating points
        lines = [m for m in caplog.messages if m.startswith(f"{cls} F1-max operating points: pixel threshold")]
        assert len(lines) == 1 and "; image threshold" in lines[0] and "recall" in lines[0], lines
