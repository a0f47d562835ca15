"""float64 / integer references for the component labelling (aaclip_label_components) and the
pixel AUPRO (aaclip_metrics_eval_pro): scipy.ndimage.label for the components, and the
per-region-overlap curve walked point by point as MVTec AD's evaluation code does (sorted
sweep, ties collapsed to distinct thresholds, (0, 0) prepended, (1, 1) appended, trapezoids
with linear interpolation at the FPR limit)."""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=np.int64)


def label_ref(mask):
    """mask [n, H, W] (foreground = nonzero) -> (labels, areas, counts) as the device defines
    them: labels int64 [n, H, W], 0 for background, else 1 + the smallest linear index
    y * W + x of the pixel's 8-connected component within its image; areas int64 [n, H, W],
    the pixel's component's area (0 for background); counts int64 [n]."""
    mask = np.asarray(mask) != 0
    n, H, W = mask.shape
    labels = np.zeros((n, H, W), dtype=np.int64)
    areas = np.zeros((n, H, W), dtype=np.int64)
    counts = np.zeros(n, dtype=np.int64)
    lin = np.arange(H * W, dtype=np.int64).reshape(H, W)
    for i in range(n):
        lab, k = ndimage.label(mask[i], structure=EIGHT)
        counts[i] = k
        if k == 0:
            continue
        idx = np.arange(1, k + 1)
        first = ndimage.minimum(lin, lab, idx).astype(np.int64)
        size = ndimage.sum(mask[i], lab, idx).astype(np.int64)
        fg = lab > 0
        labels[i][fg] = first[lab[fg] - 1] + 1
        areas[i][fg] = size[lab[fg] - 1]
    return labels, areas, counts


def normalise(scores):
    """The class min-max of forward_utils.py:241-242 in fp32 (tests/test_metrics_gpu.py::_sk),
    so that ties are the device's ties."""
    s = np.asarray(scores, dtype=np.float32)
    if s.max() != 1:
        if s.max() == s.min():  # 0 / 0: the same NaN for every pixel, i.e. one tie group
            return np.zeros_like(s)
        s = (s - s.min()) / (s.max() - s.min())
    return s


def pro_curve(masks, scores):
    """(fpr, pro) float64 arrays of the curve: (0, 0), one point per distinct normalised score
    in descending order, (1, 1). None when there is no component or no ok pixel."""
    masks = np.asarray(masks) != 0
    if masks.ndim == 4:
        masks = masks[:, 0]
    s = normalise(scores).reshape(masks.shape).astype(np.float64)
    labels, areas, counts = label_ref(masks)
    R, n_ok = int(counts.sum()), int((~masks).sum())
    if R == 0 or n_ok == 0:
        return None
    flat = s.ravel()
    order = np.argsort(-flat, kind="stable")
    fs = flat[order]
    ok = (~masks).ravel()[order].astype(np.float64)
    a = areas.ravel()[order].astype(np.float64)
    w = np.where(a > 0, 1.0 / np.maximum(a, 1.0), 0.0) / R
    last = np.r_[np.nonzero(np.diff(fs))[0], fs.size - 1]  # last position of every tie group
    fpr = np.cumsum(ok)[last] / n_ok
    pro = np.cumsum(w)[last]
    return np.r_[0.0, fpr, 1.0], np.r_[0.0, pro, 1.0]


def aupro_ref(masks, scores, L=0.3):
    """AUPRO = (1/L) * integral_0^L PRO dFPR over the piecewise-linear curve; NaN without a
    component or without an ok pixel."""
    c = pro_curve(masks, scores)
    if c is None:
        return float("nan")
    fpr, pro = c
    area = 0.0
    for k in range(1, fpr.size):
        x0, x1, y0, y1 = fpr[k - 1], fpr[k], pro[k - 1], pro[k]
        if x0 >= L:
            break
        if x1 <= L:
            area += (x1 - x0) * (y0 + y1) / 2.0
        else:  # the limit falls inside this segment (x1 > x0 here)
            yl = y0 + (y1 - y0) * (L - x0) / (x1 - x0)
            area += (L - x0) * (y0 + yl) / 2.0
    return area / L
