"""Time the device metrics with and without F1-max on an MI355X.

  python tools/f1_timing.py [--images 32] [--sizes 336 518] [--warmup 5] [--reps 30]
                            [--f1 both|off] [--tree DIR] [--baseline-tree DIR] [--out FILE]

One class of --images maps per size (the class of tools/pro_timing.py: smooth random defect
blobs, scores = the field plus noise), plain and with pro=True, each with f1 off and on: HIP
events around ops.metrics_eval_device, the variants alternating in one process after warm-up;
the median and the min-max of --reps runs (at least 20), and the extra time of f1=True.

--f1 off measures the f1-less calls only and passes no f1 keyword, so it runs on a checkout
from before the feature. --tree DIR imports the package from that checkout (built there)
instead of this one. --baseline-tree DIR does both in a child process before the measurement:
the parent commit's metrics_eval, timed by the same tool on the same machine in the same
session, is stored as "baseline" and the extra time is also given as a share of it.

The f1=True results are compared with tests/f1_ref.py on the same class. The JSON goes to
--out, by default f1_timing.json in the next free profiles/r<N>. Nothing is gated on these
numbers. Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_class(n, S, seed):
    import numpy as np
    from scipy import ndimage
    r = np.random.default_rng(seed)
    field = np.stack([ndimage.gaussian_filter(r.standard_normal((S, S)), S / 40.0) for _ in range(n)])
    masks = (field > np.quantile(field, 0.97)).astype(np.uint8)
    masks[::4] = 0
    scores = (field / field.std() + 0.8 * r.standard_normal((n, S, S))).astype(np.float32)
    ip = r.random(n).astype(np.float32)
    il = (masks.reshape(n, -1).max(1) > 0).astype(np.uint8)
    return masks, scores, ip, il


def spread(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 1), "min_us": round(min(ms) * 1e3, 1),
            "max_us": round(max(ms) * 1e3, 1)}


def next_round_dir():
    rounds = [int(m.group(1)) for d in os.listdir(os.path.join(ROOT, "profiles")) if (m := re.fullmatch(r"r(\d+)", d))]
    return os.path.join(ROOT, "profiles", f"r{max(rounds, default=0) + 1}")


def measure(a):
    tree = os.path.abspath(a.tree) if a.tree else ROOT
    for p in (os.path.join(ROOT, "tests"), tree, os.path.join(tree, "aa-clip_amd")):
        sys.path.insert(0, p)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("f1_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    from aaclip import ops
    assert os.path.abspath(ops.__file__).startswith(tree + os.sep), (ops.__file__, tree)
    dev = torch.device("cuda:0")
    runs = []
    for S in a.sizes:
        masks, scores, ip, il = make_class(a.images, S, S)
        t = [torch.from_numpy(x).to(dev) for x in (scores, masks, ip, il)]
        variants = {"plain": lambda: ops.metrics_eval_device(*t, medical=False),
                    "pro": lambda: ops.metrics_eval_device(*t, medical=False, pro=True)}
        if a.f1 == "both":
            variants["plain_f1"] = lambda: ops.metrics_eval_device(*t, medical=False, f1=True)
            variants["pro_f1"] = lambda: ops.metrics_eval_device(*t, medical=False, pro=True, f1=True)
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
        run = {"img_size": S, "images": a.images, "pixels": a.images * S * S}
        run.update({k: spread(v) for k, v in ms.items()})
        if a.f1 == "both":
            import f1_ref
            for k in ("plain", "pro"):
                run[f"{k}_f1_extra_us"] = round((statistics.median(ms[k + "_f1"]) - statistics.median(ms[k])) * 1e3, 1)
            got = variants["pro_f1"]().tolist()[5:]
            want = f1_ref.all_eight(masks, scores, ip, il, False)
            run["f1"] = dict(zip(["pixel F1-max", "pixel threshold", "pixel precision", "pixel recall",
                                  "image F1-max", "image threshold", "image precision", "image recall"], got))
            run["max_abs_err_vs_f1_ref"] = max(abs(g - w) for g, w in zip(got, want))
            run["bit_equal_to_f1_ref"] = got == list(want)
        runs.append(run)
    return {"tree": os.path.relpath(tree, ROOT), "device": torch.cuda.get_device_name(0), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[336, 518])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--f1", choices=["both", "off"], default="both")
    ap.add_argument("--tree", default="", help="import the package from this checkout instead (with --f1 off)")
    ap.add_argument("--baseline-tree", default="", help="a built checkout of the parent commit to time first")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    baseline = None
    if a.baseline_tree:  # a fresh process: its own import of the other checkout's package and library
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", a.baseline_tree, "--f1", "off", "--out", "-",
               "--images", str(a.images), "--warmup", str(a.warmup), "--reps", str(a.reps), "--sizes"]
        done = subprocess.run(cmd + [str(s) for s in a.sizes], check=True, capture_output=True, text=True,
                              timeout=600)
        baseline = json.loads(done.stdout.strip().splitlines()[-1])
    res = measure(a)
    if a.out == "-":
        print(json.dumps(res))
        return
    if baseline:
        for run, base in zip(res["runs"], baseline["runs"]):
            for k in ("plain", "pro"):
                if f"{k}_f1_extra_us" in run:
                    run[f"{k}_f1_extra_over_baseline_plain"] = round(run[f"{k}_f1_extra_us"]
                                                                     / base["plain"]["median_us"], 3)
    res = {"tool": "tools/f1_timing.py", "warmup": a.warmup, "reps": a.reps,
           "method": "HIP events around ops.metrics_eval_device (workspace allocation from the caching allocator "
                     "included), the variants alternating in one process after warm-up; median and min-max; "
                     "baseline = the same tool with --f1 off on a checkout of the parent commit, in a child "
                     "process just before",
           **res, "baseline": baseline}
    for run in res["runs"]:
        print(json.dumps(run))
    if baseline:
        for run in baseline["runs"]:
            print("baseline", json.dumps(run))
    out = a.out or os.path.join(next_round_dir(), "f1_timing.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
