"""float64 restatement of F1-max and its threshold (aaclip_metrics_eval_f1): a stable ascending
sort, the group starts, and for every distinct score t
    PP = #{v >= t},  TP = #{y = 1, v >= t},  F1 = float64(2 TP) / float64(PP + P),
the maximum with the LOWEST maximising t (np.argmax on ascending thresholds), precision TP / PP
and recall TP / P there. Integers below 2^53 and one division each, so the device's fp64 numbers
are these bit for bit whenever the fp32 scores are. Pixels use the class normalisation of
pro_ref.normalise; images the fused fp32 score restated below (image_scores_kernel)."""
import numpy as np

from pro_ref import normalise

NAN4 = (float("nan"),) * 4


def f1_max(y, v):
    """(F1-max, threshold, precision, recall) of labels y (nonzero = positive) and fp32 scores v."""
    y = np.asarray(y).ravel() != 0
    v = np.asarray(v, dtype=np.float32).ravel()
    n, P = y.size, int(y.sum())
    order = np.argsort(v, kind="stable")
    vs, ys = v[order], y[order]
    starts = np.r_[0, 1 + np.nonzero(vs[1:] != vs[:-1])[0]].astype(np.int64)
    before = np.r_[0, np.cumsum(ys, dtype=np.int64)][starts]  # positives below the group
    tp, pp = P - before, n - starts
    f1 = (2 * tp).astype(np.float64) / (pp + P).astype(np.float64)
    k = int(np.argmax(f1))  # the first maximum: the lowest threshold
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = np.float64(tp[k]) / np.float64(P)
    return float(f1[k]), float(np.float64(vs[starts[k]]) + 0.0), float(np.float64(tp[k]) / np.float64(pp[k])), float(rec)


def pixel_f1(masks, scores):
    """The four pixel numbers of one class; NaN with no positive or no negative pixel. A constant
    class whose value is not 1 normalises to 0 / 0 on the device: one tie group (as
    pro_ref.normalise has it) whose score, and so the threshold, is NaN."""
    y = np.asarray(masks).ravel() != 0
    if y.all() or not y.any():
        return NAN4
    s = np.asarray(scores, dtype=np.float32)
    f1, thr, prec, rec = f1_max(y, normalise(s))
    if s.max() != 1 and s.max() == s.min():
        thr = float("nan")
    return f1, thr, prec, rec


def fused_scores(scores, image_preds, medical):
    """image_scores_kernel in numpy float32: the class-normalised row maximum for Medical, else
    0.5 * that + 0.5 * the normalised image score (both products are exact)."""
    s = np.asarray(scores, dtype=np.float32)
    s = s.reshape(s.shape[0], -1)
    lo, hi, rmax = s.min(), s.max(), s.max(axis=1)
    pm = (rmax - lo) / (hi - lo) if hi != 1 else rmax
    ip = np.asarray(image_preds, dtype=np.float32).ravel()
    ilo, ihi = ip.min(), ip.max()
    im = (ip - ilo) / (ihi - ilo) if ihi != 1 else ip
    out = pm if medical else pm * np.float32(0.5) + im * np.float32(0.5)
    assert out.dtype == np.float32
    return out


def image_f1(scores, image_preds, image_label, medical):
    """The four image numbers; zeros when the image labels are all equal (forward_utils.py:264-271).
    Fused scores that are all NaN (a constant class normalised to 0 / 0) are one tie group with a
    NaN threshold, as for pixels: the device compares image scores as it compares the pixel keys."""
    y = np.asarray(image_label).ravel() != 0
    if y.all() or not y.any():
        return (0.0,) * 4
    with np.errstate(invalid="ignore"):
        fused = fused_scores(scores, image_preds, medical)
    if np.isnan(fused).all():
        f1, _, prec, rec = f1_max(y, np.zeros_like(fused))
        return f1, float("nan"), prec, rec
    return f1_max(y, fused)


def all_eight(masks, scores, image_preds, image_label, medical):
    return pixel_f1(masks, scores) + image_f1(scores, image_preds, image_label, medical)
