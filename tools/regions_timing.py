"""Time the region extraction against the F1 metrics pass on an MI355X.

  python tools/regions_timing.py [--images 32] [--sizes 336 518] [--warmup 5] [--reps 30] [--out FILE]

One class of --images maps per size (the class of tools/f1_timing.py: smooth random defect blobs,
scores = the field plus noise). The class's pixel F1-max threshold comes from
ops.metrics_eval_device(f1=True); ops.extract_regions at that threshold (with the masks, the
defaults min_area=1, max_regions=64) and metrics_eval_device(f1=True) on the same data, the
yardstick, alternate in one process after warm-up, each between HIP events: the median and the
min-max of --reps runs (at least 20). The pixel noise breaks the foreground into thousands of
regions per map; a second pair of numbers times the same maps at min_area=16, which changes what
is compacted and listed but not what is labelled and sorted. A third pair times the class with its
scores blurred (Gaussian, sigma 4, as the model's maps are before they are upsampled) at that
class's own F1 threshold: a few blobs per map instead of thousands of specks.

The regions are compared with tests/regions_ref.py on the first two maps' worth of the class
(the whole class is normalised, two maps are labelled by scipy). The JSON goes to --out, by
default regions_timing.json in the next free profiles/r<N>. Nothing is gated on these numbers.
Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT, os.path.join(ROOT, "aa-clip_amd")):
    sys.path.insert(0, p)

from f1_timing import make_class, next_round_dir, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[336, 518])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("regions_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    import regions_ref
    from aaclip import ops
    dev = torch.device("cuda:0")
    runs = []
    for S in a.sizes:
        masks, scores, ip, il = make_class(a.images, S, S)
        t = [torch.from_numpy(x).to(dev) for x in (scores, masks, ip, il)]
        thr = ops.metrics_eval_device(*t, medical=False, f1=True).tolist()[5]
        from scipy import ndimage
        smooth = torch.from_numpy(ndimage.gaussian_filter(scores, (0, 4, 4))).to(dev)
        thr_smooth = ops.metrics_eval_device(smooth, *t[1:], medical=False, f1=True).tolist()[5]
        variants = {"f1_metrics": lambda: ops.metrics_eval_device(*t, medical=False, f1=True),
                    "regions": lambda: ops.extract_regions(t[0], thr, pixel_label=t[1]),
                    "regions_min_area_16": lambda: ops.extract_regions(t[0], thr, pixel_label=t[1], min_area=16),
                    "f1_metrics_smooth": lambda: ops.metrics_eval_device(smooth, *t[1:], medical=False, f1=True),
                    "regions_smooth": lambda: ops.extract_regions(smooth, thr_smooth, pixel_label=t[1])}
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        run = {"img_size": S, "images": a.images, "pixels": a.images * S * S, "threshold": thr,
               "threshold_smooth": thr_smooth}
        run.update({k: spread(v) for k, v in ms.items()})
        for k, base in (("regions", "f1_metrics"), ("regions_min_area_16", "f1_metrics"),
                        ("regions_smooth", "f1_metrics_smooth")):
            run[f"{k}_over_{base}"] = round(statistics.median(ms[k]) / statistics.median(ms[base]), 3)
        found = variants["regions_smooth"]()
        run["regions_smooth_found"] = int(found["n_regions"].sum())
        run["foreground_share"] = round(float((regions_ref.scores(scores) >= np.float32(thr)).mean()), 4)
        run["foreground_share_smooth"] = round(float(found["area"].sum()) / (a.images * S * S), 4)
        for k, kw in (("regions", {}), ("regions_min_area_16", {"min_area": 16})):
            got = {f: v.cpu().numpy() for f, v in variants[k]().items()}
            run[f"{k}_found"] = int(got["n_regions"].sum())
            run[f"{k}_images_with_one"] = int((got["n_regions"] > 0).sum())
            run[f"{k}_listed_overlapping_gt"] = int((got["gt_area"] > 0).sum())
            v = regions_ref.scores(scores)[:2]  # the class's normalisation, two maps' labelling
            want = regions_ref.extract(v, thr, masks[:2], normalise=False, **kw)
            run[f"{k}_equal_to_regions_ref_on_2_maps"] = all(
                np.array_equal(got[f][:2].view(np.uint8), want[f].astype(got[f].dtype).view(np.uint8)) for f in want)
        runs.append(run)
        print(json.dumps(run))
    res = {"tool": "tools/regions_timing.py", "warmup": a.warmup, "reps": a.reps,
           "method": "HIP events around ops.extract_regions and ops.metrics_eval_device(f1=True) (workspace allocation "
                     "from the caching allocator included), alternating in one process after warm-up; median and "
                     "min-max",
           "device": torch.cuda.get_device_name(0), "runs": runs}
    out = a.out or os.path.join(next_round_dir(), "regions_timing.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
