"""Time the device metrics with and without the pixel AUPRO on an MI355X.

  python tools/pro_timing.py [--images 32] [--sizes 336 518] [--warmup 5] [--reps 30]
                             [--out profiles/r14/pro_timing.json]

One class of --images maps per size: smooth random defect blobs (a thresholded blurred noise
field, a quarter of the images defect-free), scores = the field plus noise. HIP events around
ops.metrics_eval_device with pro=False (aaclip_metrics_eval, the yardstick) and with pro=True
(aaclip_metrics_eval_pro), the two alternating in one process after warm-up, and around the
labelling launch alone (ops.label_components' C call on preallocated outputs); the median and
the min-max of --reps runs. The pro=True result is also compared with the float64
curve-walking reference of tests/pro_ref.py on the same class. Nothing is gated on these
numbers. Needs a GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "aa-clip_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aaclip import _lib, ops  # noqa: E402


def make_class(n, S, seed):
    from scipy import ndimage
    r = np.random.default_rng(seed)
    field = np.stack([ndimage.gaussian_filter(r.standard_normal((S, S)), S / 40.0) for _ in range(n)])
    masks = (field > np.quantile(field, 0.97)).astype(np.uint8)
    masks[::4] = 0
    scores = (field / field.std() + 0.8 * r.standard_normal((n, S, S))).astype(np.float32)
    ip = r.random(n).astype(np.float32)
    il = (masks.reshape(n, -1).max(1) > 0).astype(np.uint8)
    return masks, scores, ip, il


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 1), "min_us": round(min(ms) * 1e3, 1),
            "max_us": round(max(ms) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[336, 518])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "pro_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pro_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    import pro_ref
    dev = torch.device("cuda:0")
    runs = []
    for S in a.sizes:
        masks, scores, ip, il = make_class(a.images, S, S)
        t = [torch.from_numpy(x).to(dev) for x in (scores, masks, ip, il)]
        n = a.images
        labels = torch.empty(n, S, S, device=dev, dtype=torch.int32)
        areas = torch.empty_like(labels)
        counts = torch.empty(n, device=dev, dtype=torch.int32)
        stream = torch.cuda.current_stream().cuda_stream

        def plain():
            return ops.metrics_eval_device(*t, medical=False)

        def pro():
            return ops.metrics_eval_device(*t, medical=False, pro=True)

        def label():
            _lib.call("aaclip_label_components", ctypes.c_void_p(t[1].data_ptr()), n, S, S,
                      ctypes.c_void_p(labels.data_ptr()), ctypes.c_void_p(areas.data_ptr()),
                      ctypes.c_void_p(counts.data_ptr()), stream)

        for _ in range(a.warmup):
            plain(), pro(), label()
        torch.cuda.synchronize()
        tp, tq, tl = [], [], []
        for _ in range(a.reps):
            tp.append(timed(plain))
            tq.append(timed(pro))
            tl.append(timed(label))
        got = pro().tolist()
        want = pro_ref.aupro_ref(masks, scores, 0.3)
        run = {"img_size": S, "images": n, "pixels": n * S * S, "components": int(counts.sum()),
               "metrics_eval": spread(tp), "metrics_eval_pro": spread(tq), "label_components": spread(tl),
               "pro_over_plain": round(statistics.median(tq) / statistics.median(tp), 3),
               "label_share_of_extra": round(statistics.median(tl) / max(statistics.median(tq) - statistics.median(tp),
                                                                         1e-9), 3),
               "aupro": got[4], "aupro_ref": want, "abs_err": abs(got[4] - want)}
        print(json.dumps(run))
        runs.append(run)
    res = {"tool": "tools/pro_timing.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps,
           "fpr_limit": 0.3,
           "method": "HIP events around ops.metrics_eval_device (workspace allocation from the caching allocator "
                     "included) with pro=False and pro=True alternating in one process after warm-up, and around "
                     "the labelling launches alone; median and min-max",
           "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
