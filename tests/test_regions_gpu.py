"""Region extraction on the MI355X (aaclip_extract_regions) against the scipy reference of
tests/regions_ref.py. Every field is compared exactly: the integers are equal, the peak has the
fp32 reference's bits, the centroids the bits of the float64 division. No tolerances."""
import json
import struct

import numpy as np
import pytest
import torch
from scipy import ndimage

from aaclip import ops

import regions_ref as RR

pytestmark = pytest.mark.gpu

INTS = ["n_regions", "label", "area", "bbox", "peak_index", "gt_area"]


def _device(dev, preds, thr, label=None, stream=None, **kw):
    p = torch.from_numpy(np.ascontiguousarray(preds)).to(dev)
    lab = None if label is None else torch.from_numpy(np.ascontiguousarray(label)).to(dev)
    if stream is None:
        out = ops.extract_regions(p, thr, pixel_label=lab, **kw)
    else:
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            out = ops.extract_regions(p, thr, pixel_label=lab, **kw)
        stream.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in INTS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert got["peak"].dtype == np.float32 and got["centroid"].dtype == np.float64
    assert np.array_equal(got["peak"].view(np.uint32), want["peak"].view(np.uint32)), (what, got["peak"], want["peak"])
    assert np.array_equal(got["centroid"].view(np.uint64), want["centroid"].view(np.uint64)), (what, "centroid")


def _check(dev, preds, thr, label=None, what="", **kw):
    got = _device(dev, preds, thr, label, **kw)
    want = RR.extract(preds, thr, label, kw.get("normalise", True), kw.get("min_area", 1), kw.get("max_regions", 64))
    print(what, kw, "threshold", float(thr), "regions per image", got["n_regions"].tolist(), "reference",
          want["n_regions"].tolist())
    _same(got, want, (what, kw))
    return got


# ---------------------------------------------------------------------------- wave-segment edges
def _designed(H, W):
    """One image of foreground bits around the 64-column seams: a bar across every seam, a pair that
    meets only diagonally across every seam, a column over all rows, the last column's ends."""
    m = np.zeros((H, W), bool)
    m[:, 0] = True  # spans all rows
    for seam in range(64, W, 64):
        m[0, max(seam - 3, 2):min(seam + 3, W)] = True  # crosses the seam in one row
        if H >= 4:
            m[2, seam - 1] = m[3, seam] = True  # (2, 63) and (3, 64) touch only diagonally
        if H >= 8:
            m[6, seam] = m[7, seam - 1] = True  # and the other diagonal
    if H >= 12 and W >= 3:
        m[10:, W - 1] = True
        m[H - 1, 2:] = True  # the whole last row
    return m


def _edge_case(H, W, seed, designed):
    r = np.random.default_rng(seed)
    m = np.zeros((3, H, W), bool)
    m[0] = _designed(H, W) if designed else r.random((H, W)) < 0.5
    m[2] = True  # an empty image (1) and a full image (2) in the same batch
    levels = r.integers(2, 5, (3, H, W)) / 8  # foreground scores 0.25 .. 0.5 in eighths: many shared peaks
    preds = np.where(m, levels, 0.0).astype(np.float32)
    preds[1, 0, 0] = -0.5  # class range [-0.5, 0.5]: normalised by an exact division
    gt = (r.random((3, H, W)) < 0.4).astype(np.uint8)
    return m, preds, gt


@pytest.mark.parametrize("designed", [True, False])
@pytest.mark.parametrize("H", [1, 2, 37])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 130])
def test_regions_at_the_wave_segment_edges(dev, H, W, designed):
    m, preds, gt = _edge_case(H, W, 1000 * H + W, designed)
    most = ((H + 1) // 2) * ((W + 1) // 2)
    raw = _check(dev, preds, 0.25, gt, f"{H}x{W} raw", normalise=False, max_regions=most)
    assert raw["n_regions"][1] == 0 and raw["n_regions"][2] == 1 and raw["area"][2, 0] == H * W
    assert raw["area"][0].sum() == m[0].sum()  # nothing was cut off: every region is listed
    assert RR.scores(preds)[m].min() >= 0.75  # (0.25 + 0.5) / 1: the lowest foreground score
    _check(dev, preds, 0.75, None, f"{H}x{W} normalised", normalise=True, max_regions=most)
    _check(dev, preds, 0.75, gt, f"{H}x{W} normalised, 2 slots", normalise=True, max_regions=2, min_area=2)


def test_designed_image_holds_the_contacts_it_is_meant_to():
    m = _designed(37, 130)
    lab, k = ndimage.label(m, structure=np.ones((3, 3)))
    assert lab[2, 63] == lab[3, 64] != 0 and lab[6, 64] == lab[7, 63] != 0  # joined diagonally across a seam
    assert lab[2, 127] == lab[3, 128] != 0 and lab[0, 62] == lab[0, 66] != 0
    four, _ = ndimage.label(m)
    assert four[2, 63] != four[3, 64]  # and only diagonally
    assert (lab[:, 0] == lab[0, 0]).all() and k >= 6


# ---------------------------------------------------------------------------- random blobs
@pytest.fixture(scope="module")
def blobs():
    r = np.random.default_rng(5)
    field = np.stack([ndimage.gaussian_filter(r.standard_normal((37, 70)), 2.5) for _ in range(3)])
    masks = (field > np.quantile(field, 0.9)).astype(np.uint8)
    preds = (field / field.std() + 0.3 * r.standard_normal(field.shape)).astype(np.float32)
    return masks, preds


MOST = 19 * 35  # the most components a 37 x 70 image can hold


@pytest.mark.parametrize("with_label", [False, True])
@pytest.mark.parametrize("normalise", [True, False])
def test_regions_of_random_blobs(dev, blobs, normalise, with_label):
    masks, preds = blobs
    v = RR.scores(preds, normalise)
    for q in (0.05, 0.5, 0.8, 0.95, 0.999):
        thr = np.quantile(v, q, method="lower")  # one pixel's own score: >= keeps that pixel
        assert thr.dtype == np.float32 and (v == thr).sum() >= 1
        got = _check(dev, preds, thr, masks if with_label else None, f"quantile {q}", normalise=normalise,
                     max_regions=MOST)
        assert got["area"].sum() == (v >= thr).sum()
        if not with_label:
            assert not got["gt_area"].any()
        just_above = np.nextafter(thr, np.float32(np.inf))
        assert _device(dev, preds, just_above, normalise=normalise, max_regions=MOST)["area"].sum() == (v > thr).sum()


@pytest.mark.parametrize("min_area", [1, 4])
def test_min_area_and_max_regions(dev, blobs, min_area):
    masks, preds = blobs
    thr = np.quantile(RR.scores(preds), 0.8, method="lower")
    full = _check(dev, preds, thr, masks, "all slots", min_area=min_area, max_regions=MOST)
    counts = full["n_regions"]
    assert counts.min() > 3 and (full["area"][full["area"] > 0] >= min_area).all()
    if min_area > 1:
        assert (counts < _device(dev, preds, thr, max_regions=MOST)["n_regions"]).all()
    for R in (1, 3, int(counts.max()) + 5):
        got = _check(dev, preds, thr, masks, f"{R} slots", min_area=min_area, max_regions=R)
        assert np.array_equal(got["n_regions"], counts)  # the filtered total, whatever is listed
        for i, c in enumerate(counts):
            for k in INTS[1:] + ["peak", "centroid"]:
                assert np.array_equal(got[k][i, :min(c, R)], full[k][i, :min(c, R)])
                assert not got[k][i, min(c, R):].any(), (k, i)


def test_shared_peak_class_maximum_one_and_constant_maps(dev, blobs):
    masks, preds = blobs
    p = preds.copy()
    thr = np.quantile(p, 0.9, method="lower")
    first = RR.extract(p, thr, None, False, 1, 4)
    lab, _ = ndimage.label(p[0] >= thr, structure=np.ones((3, 3)))
    region = np.argwhere(lab == lab.ravel()[first["label"][0, 0] - 1])
    assert len(region) == first["area"][0, 0] > 1
    a, b = region[0], region[-1]  # the region's first and last pixel share a new peak
    p[0, a[0], a[1]] = p[0, b[0], b[1]] = p.max() + 1
    got = _check(dev, p, thr, masks, "two pixels share the peak", normalise=False, max_regions=4)
    assert got["peak_index"][0, 0] == a[0] * 70 + a[1] and got["peak"][0, 0] == p.max()
    # a class maximum of exactly 1 is taken raw: its minimum, 0.25, would otherwise move every score
    q = (0.25 + 0.75 * (preds - preds.min()) / (preds.max() - preds.min())).astype(np.float32)
    q[1, 5, 5] = 1.0
    assert q.max() == 1.0 and q.min() > 0.2
    got = _check(dev, q, 0.5, masks, "class maximum 1", normalise=True, max_regions=MOST)
    _same(got, _device(dev, q, 0.5, masks, normalise=False, max_regions=MOST), "raw")
    assert got["area"].sum() == (q >= 0.5).sum() != ((q - q.min()) / (1 - q.min()) >= 0.5).sum()
    # constant maps: 0 / 0 has no region at any threshold; constant 1 is raw and all foreground
    flat = np.full((3, 37, 70), 0.5, np.float32)
    for t in (0.0, 0.5, -1.0):
        got = _check(dev, flat, t, masks, "constant 0.5", normalise=True, max_regions=3)
        assert not got["n_regions"].any()
    assert _check(dev, flat, 0.5, masks, "constant 0.5 raw", normalise=False, max_regions=3)["area"][:, 0].tolist() \
        == [37 * 70] * 3
    assert _check(dev, np.ones_like(flat), 1.0, None, "constant 1", max_regions=3)["n_regions"].tolist() == [1, 1, 1]


def test_wide_region_sums_need_64_bits(dev):
    """One 2100 x 2100 region: the sum of x is 2100 * (2099 * 2100 / 2) > 2^32."""
    S = 2100
    r = np.random.default_rng(3)
    preds = (1 + r.random((1, S, S))).astype(np.float32)
    preds[0, 1234, 567] = preds[0, 2000, 1] = 3.0
    gt = np.zeros((1, S, S), np.uint8)
    gt[0, 100:1500, 300:2000] = 1
    assert S * (S - 1) * S // 2 > 2 ** 32
    got = _check(dev, preds, 0.5, gt, "2100 x 2100", normalise=False, max_regions=2)
    assert got["n_regions"].tolist() == [1] and got["area"][0].tolist() == [S * S, 0]
    assert got["centroid"][0, 0].tolist() == [(S - 1) / 2, (S - 1) / 2] and got["bbox"][0, 0].tolist() == [0, 0, S - 1, S - 1]
    assert got["peak_index"][0, 0] == 1234 * S + 567 and got["gt_area"][0, 0] == 1400 * 1700


# ---------------------------------------------------------------------------- the shipped metrics
def _bits(x):
    return struct.pack("<d", x).hex()


def test_regions_at_the_f1_threshold_reproduce_its_precision_and_recall(dev, blobs):
    masks, preds = blobs
    t = [torch.from_numpy(x).to(dev) for x in (preds, masks, np.array([0.2, 0.9, 0.4], np.float32),
                                               np.array([1, 1, 0], np.uint8))]
    f1 = ops.metrics_eval_device(*t, medical=False, f1=True).tolist()
    thr, precision, recall = f1[5], f1[6], f1[7]
    assert 0 < precision < 1 and 0 < recall < 1 and thr == float(np.float32(thr))
    got = _check(dev, preds, thr, masks, "F1 threshold", min_area=1, max_regions=MOST)
    assert (got["n_regions"] <= MOST).all()
    hit, flagged, P = int(got["gt_area"].sum()), int(got["area"].sum()), int(masks.sum())
    print("TP", hit, "PP", flagged, "P", P, "precision", precision, "recall", recall)
    assert _bits(float(hit) / float(flagged)) == _bits(precision)
    assert _bits(float(hit) / float(P)) == _bits(recall)


def test_two_launches_one_on_a_side_stream_give_the_same_bytes(dev, blobs):
    masks, preds = blobs
    thr = np.quantile(RR.scores(preds), 0.7, method="lower")
    a = _device(dev, preds, thr, masks, max_regions=40)
    b = _device(dev, preds, thr, masks, stream=torch.cuda.Stream(device=dev), max_regions=40)
    c = _device(dev, preds, thr, masks, max_regions=40)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


# ---------------------------------------------------------------------------- public API, harness
def test_forward_utils_anomaly_regions(dev, blobs):
    from forward_utils import anomaly_regions
    masks, preds = blobs
    thr = float(np.quantile(RR.scores(preds), 0.8, method="lower"))
    want = RR.as_entries(preds, thr, masks, True, 2, 5)
    assert anomaly_regions(preds, thr, masks, min_area=2, max_regions=5) == want  # numpy in
    t = [torch.from_numpy(x).to(dev) for x in (preds[:, None], masks[:, None])]
    assert anomaly_regions(t[0], thr, t[1], min_area=2, max_regions=5) == want  # [n, 1, H, W] tensors in
    assert max(e["n_regions"] for e in want) > 5 and all(len(e["regions"]) <= 5 for e in want)
    bare = anomaly_regions(preds, thr, normalise=True)
    assert bare == RR.as_entries(preds, thr) and not any(g["gt_area"] for e in bare for g in e["regions"])
    with pytest.raises(ValueError, match="pixel_label must match"):
        ops.extract_regions(t[0], thr, pixel_label=t[1][:, :, :-1])
    with pytest.raises(ValueError, match="at least 1"):
        ops.extract_regions(t[0], thr, max_regions=0)


def test_harness_regions(dev, tmp_path, caplog):
    import logging

    import test as harness
    caplog.set_level(logging.INFO)
    path = tmp_path / "table.json"
    base = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4",
            "--save_path", str(tmp_path), "--results_json", str(path)]
    df, ctx = harness.run(harness.parse_args(base + ["--regions"]))
    assert list(ctx["regions"]) == list(ctx["classes"]) == list(ctx["operating_points"])
    table = json.loads(path.read_text())
    for cls, (masks, labels, preds, preds_image) in ctx["classes"].items():
        thr = ctx["operating_points"][cls]["pixel"]["threshold"]
        found = ctx["regions"][cls]
        assert found["threshold"] == thr and list(found) == ["threshold", "images"]
        want = RR.as_entries(preds.cpu().numpy(), thr, masks.cpu().numpy())
        assert [list(e) for e in found["images"]] == [["file_name", "n_regions", "regions"]] * 4
        assert [e["file_name"] for e in found["images"]] == [f"synthetic/{i:05d}.png" for i in range(4)]
        assert [{k: e[k] for k in ("n_regions", "regions")} for e in found["images"]] == want
        total = sum(e["n_regions"] for e in want)
        print(cls, "threshold", thr, "regions", total)
        assert total > 0
        assert table["regions"][cls] == found  # floats survive JSON exactly
        lines = [m for m in caplog.messages if m.startswith(f"{cls} regions at pixel threshold")]
        assert len(lines) == 1 and f": {total} in " in lines[0] and "overlap the ground truth" in lines[0], lines
    # the columns are the --f1 ones: the same table without --regions, and no "regions" anywhere
    df2, ctx2 = harness.run(harness.parse_args(base + ["--f1"]))
    assert df2.equals(df) and list(df2.columns) == list(df.columns)
    assert "regions" not in ctx2 and ctx2["operating_points"] == ctx["operating_points"]
    again = json.loads(path.read_text())
    assert "regions" not in again and again == {k: v for k, v in table.items() if k != "regions"}
