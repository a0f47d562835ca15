"""scipy reference for the region extraction (aaclip_extract_regions): scipy.ndimage.label with the
8-neighbour structure for the components, find_objects for the boxes, ndimage.sum / minimum /
maximum for the rest. Scores are normalised in fp32 as tests/pro_ref.py does it, except
that a constant class stays 0 / 0 = NaN, which no threshold reaches: background. Centroids are one
float64 division of integer sums; regions are ordered by (area descending, label ascending)."""
import numpy as np
from scipy import ndimage

from pro_ref import EIGHT

FIELDS = ["label", "area", "bbox", "centroid", "peak", "peak_index", "gt_area"]


def scores(pixel_preds, normalise=True):
    """The score v the threshold is applied to, fp32: the class min-max of the metrics (skipped when
    the class maximum is 1), or the raw value."""
    s = np.asarray(pixel_preds, dtype=np.float32)
    if normalise and s.max() != 1:
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (s - s.min()) / (s.max() - s.min())  # (a constant class: 0 / 0, NaN everywhere)
    return s


def image_regions(v, threshold, gt=None, min_area=1):
    """Every region of one image's scores v [H, W] (fp32) with at least min_area pixels, ordered:
    dicts of label (1 + the smallest linear index), area, bbox [x0, y0, x1, y1] inclusive,
    centroid [cx, cy] (float64), peak (np.float32), peak_index (the smallest linear index that
    reaches the peak), gt_area."""
    H, W = v.shape
    with np.errstate(invalid="ignore"):
        fg = v >= np.float32(threshold)  # (False for a NaN)
    lab, k = ndimage.label(fg, structure=EIGHT)
    if k == 0:
        return []
    idx = np.arange(1, k + 1)
    lin = np.arange(H * W, dtype=np.int64).reshape(H, W)
    ys, xs = np.divmod(lin, W)
    first = ndimage.minimum(lin, lab, idx).astype(np.int64)
    area = ndimage.sum(fg, lab, idx).astype(np.int64)
    sum_x = ndimage.sum(xs, lab, idx).astype(np.int64)  # (float64 sums of integers far below 2^53: exact)
    sum_y = ndimage.sum(ys, lab, idx).astype(np.int64)
    truth = np.zeros(k, dtype=np.int64) if gt is None else ndimage.sum(np.asarray(gt) != 0, lab, idx).astype(np.int64)
    # ndimage.maximum_position breaks ties between equal maxima by an unstable sort: take the
    # maximum, then the smallest linear index among the pixels that reach it
    peak = ndimage.maximum(np.where(fg, v, -np.inf), lab, idx).astype(np.float32)
    at_peak = fg & (v == peak[np.maximum(lab, 1) - 1])
    where = ndimage.minimum(np.where(at_peak, lin, H * W), lab, idx).astype(np.int64)
    out = []
    for r, box in enumerate(ndimage.find_objects(lab)):
        if area[r] < min_area:
            continue
        py, px = divmod(int(where[r]), W)
        out.append({"label": int(first[r]) + 1, "area": int(area[r]),
                    "bbox": [box[1].start, box[0].start, box[1].stop - 1, box[0].stop - 1],
                    "centroid": [float(np.float64(sum_x[r]) / np.float64(area[r])),
                                 float(np.float64(sum_y[r]) / np.float64(area[r]))],
                    "peak": np.float32(v[py, px]), "peak_index": int(py) * W + int(px), "gt_area": int(truth[r])})
    out.sort(key=lambda g: (-g["area"], g["label"]))
    return out


def extract(pixel_preds, threshold, pixel_label=None, normalise=True, min_area=1, max_regions=64):
    """The device's outputs as numpy arrays: {"n_regions" int64 [n], and per slot [n, max_regions]
    "label", "area", "bbox" [.., 4], "peak_index", "gt_area" int64, "centroid" float64 [.., 2], "peak"
    float32}, zero past min(n_regions, max_regions)."""
    p = np.asarray(pixel_preds)
    if p.ndim == 4:
        p = p[:, 0]
    gt = None if pixel_label is None else np.asarray(pixel_label).reshape(p.shape)
    v = scores(p, normalise)
    n, R = p.shape[0], max_regions
    out = {"n_regions": np.zeros(n, np.int64), "label": np.zeros((n, R), np.int64), "area": np.zeros((n, R), np.int64),
           "bbox": np.zeros((n, R, 4), np.int64), "centroid": np.zeros((n, R, 2), np.float64),
           "peak": np.zeros((n, R), np.float32), "peak_index": np.zeros((n, R), np.int64),
           "gt_area": np.zeros((n, R), np.int64)}
    for i in range(n):
        regions = image_regions(v[i], threshold, None if gt is None else gt[i], min_area)
        out["n_regions"][i] = len(regions)
        for j, g in enumerate(regions[:R]):
            for f in FIELDS:
                out[f][i, j] = g[f]
    return out


def as_entries(pixel_preds, threshold, pixel_label=None, normalise=True, min_area=1, max_regions=64):
    """The same in the layout of forward_utils.anomaly_regions: one {"n_regions", "regions"} per image."""
    p = np.asarray(pixel_preds)
    W = p.shape[-1]
    a = extract(p, threshold, pixel_label, normalise, min_area, max_regions)
    images = []
    for i, count in enumerate(a["n_regions"].tolist()):
        regions = [{"label": int(a["label"][i, j]), "area": int(a["area"][i, j]), "bbox": a["bbox"][i, j].tolist(),
                    "centroid": a["centroid"][i, j].tolist(), "peak": float(a["peak"][i, j]),
                    "peak_xy": [int(a["peak_index"][i, j]) % W, int(a["peak_index"][i, j]) // W],
                    "gt_area": int(a["gt_area"][i, j])} for j in range(min(count, max_regions))]
        images.append({"n_regions": count, "regions": regions})
    return images
