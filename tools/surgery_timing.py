"""Time the frozen surgery tower against the plain tower on an MI355X.

  python tools/surgery_timing.py [--batch 16] [--sizes 518 336] [--dtypes fp16 bf16]
                                 [--warmup 3] [--reps 10] [--out profiles/r07/surgery_timing.json]

For every (image size, dtype): FrozenVisualEngine.encode(x, [6, 12, 18, 24]) of a tower
with surgery from block 5 (DAPM_replace(20)) and of the plain tower, on synthetic weights
and images, IN THE SAME RUN, alternating the two (HIP events around each call, after
warm-up; the median and the spread of --reps calls). Then the surgery step again under an
ops.set_probe probe (HIP events around every launch, averaged over --reps steps): the v-v
kernel's time per launch and per step, its share of the sum of launch times, and its
achieved bytes/s (2 x R x 1024 elements over its time) against the 6.29 TB/s a float4 copy
was measured at on this chip. Needs a GPU; there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "aa-clip_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from aaclip import ops  # noqa: E402
from aaclip.engine import FrozenVisualEngine  # noqa: E402
from oracle import synth  # noqa: E402

COPY_CEILING_TBS = 6.29  # float4 copy measured on the MI355X (HBM3E, 8.0 TB/s spec)
LEVELS = [6, 12, 18, 24]
DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


class Probe:
    def __init__(self):
        self.recs = []

    def begin(self, kind, name, flops, nbytes):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return (kind, name, flops, nbytes, e)

    def end(self, tok):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.recs.append(tok + (e,))


def timed(eng, x):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.encode(x, LEVELS)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def probe_step(eng, x, reps):
    by_kind, total = {}, 0.0
    for _ in range(reps):
        probe = Probe()
        ops.set_probe(probe)
        try:
            eng.encode(x, LEVELS)
        finally:
            ops.set_probe(None)
        torch.cuda.synchronize()
        for kind, _, flops, nbytes, b, e in probe.recs:
            ms = b.elapsed_time(e)
            d = by_kind.setdefault(kind, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += ms
            d["flops"] += flops
            d["bytes"] += nbytes
            total += ms
    out = {}
    for kind, d in by_kind.items():
        ms = d["ms"] / reps
        out[kind] = {"launches_per_step": d["launches"] // reps, "ms_per_step": round(ms, 4),
                     "avg_launch_us": round(d["ms"] / d["launches"] * 1e3, 2),
                     "GBs": round(d["bytes"] / (d["ms"] * 1e-3) / 1e9, 1),
                     "tflops": round(d["flops"] / (d["ms"] * 1e-3) / 1e12, 2)}
    return out, total / reps


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--sizes", type=int, nargs="+", default=[518, 336])
    ap.add_argument("--dtypes", nargs="+", default=["fp16", "bf16"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "surgery_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surgery_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/surgery_timing.py", "device": torch.cuda.get_device_name(0), "batch": a.batch,
           "out_layers": LEVELS, "surgery_from_block": 5, "warmup": a.warmup, "reps": a.reps,
           "copy_ceiling_TBs": COPY_CEILING_TBS,
           "method": "HIP events around each encode(), surgery and plain alternating in one process; per-op times "
                     "from HIP events around every launch (ops.set_probe), eager", "runs": []}
    for size in a.sizes:
        sd = synth.clip_state_dict(111, img_size=size)
        vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
        x = torch.from_numpy(synth.images(7, a.batch, size)).to(dev)
        for name in a.dtypes:
            surg = FrozenVisualEngine(vp, dtype=DT[name], surgery_from=5)
            plain = FrozenVisualEngine(vp, dtype=DT[name])
            for _ in range(a.warmup):
                surg.encode(x, LEVELS)
                plain.encode(x, LEVELS)
            torch.cuda.synchronize()
            ts, tp = [], []
            for _ in range(a.reps):
                ts.append(timed(surg, x))
                tp.append(timed(plain, x))
            by_kind, launch_sum = probe_step(surg, x, a.reps)
            by_kind_plain, launch_sum_plain = probe_step(plain, x, a.reps)
            vv = by_kind["vv_attention"]
            n_tok = (size // 14) ** 2 + 1
            run = {"img_size": size, "n_tok": n_tok, "rows": a.batch * n_tok, "dtype": name,
                   "surgery_encode": spread(ts), "plain_encode": spread(tp),
                   "surgery_over_plain": round(statistics.median(ts) / statistics.median(tp), 4),
                   "surgery_sum_of_launch_ms": round(launch_sum, 3), "plain_sum_of_launch_ms": round(launch_sum_plain, 3),
                   "vv_attention": dict(vv, share_of_launch_time=round(vv["ms_per_step"] / launch_sum, 4),
                                        share_of_copy_ceiling=round(vv["GBs"] / (COPY_CEILING_TBS * 1e3), 3)),
                   "surgery_by_op": by_kind, "plain_by_op": by_kind_plain}
            print(json.dumps({k: run[k] for k in ("img_size", "dtype", "surgery_encode", "plain_encode",
                                                  "surgery_over_plain", "vv_attention")}), flush=True)
            res["runs"].append(run)
            del surg, plain
        del vp, x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
