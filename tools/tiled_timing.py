"""Time tiled inference on an MI355X: the tile gather, the stitch + score, and a whole tiled step.

  python tools/tiled_timing.py [--warmup 2] [--reps 7] [--out FILE] [--shapes 32:518:2:129,32:518:3:129,32:336:2:84]
                               [--step 32:518:2:129:32]

Measured, each after warm-up in one process, between HIP events, the variants alternating, median
and min-max (the method of tools/fewshot_timing.py):
  (a) per batch:side:grid:overlap of --shapes, on seeded random operands: ops.tile_gather of the
      whole batch, and ops.tile_stitch + ops.tile_score with a global view (a = 0.5); the bytes each
      must move (gather: tiles read + written; stitch: tile maps and global maps read once, canvas
      written) and the share of the 6.29 TB/s measured copy ceiling that amounts to; and a torch
      eager restatement on the same operands: the gather as G^2 slice copies per batch, the stitch as
      G^2 slice-multiply-accumulates into a zeroed canvas plus F.interpolate, the blend and the
      score's amax. How far the two stitches differ is recorded.
  (b) --step batch:side:grid:overlap:tile_batch on an engine with seeded synthetic weights in the
      fp16 mode: VisualEngine.predict_tiled (global view, a = 0.5) against G^2 + 1 plain predict_cached
      calls of tile_batch images at the same side, i.e. the same tower work without the tiling; the
      difference is the share of a tiled step that is tiling overhead (gather, copies, stitch, score).
The JSON goes to --out, by default profiles/r20/tiled_timing.json. Nothing is gated on these numbers.
RANDOM-INIT weights and synthetic images: this measures time, not whether tiling finds more defects.
Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), ROOT, os.path.join(ROOT, "aa-clip_amd")):
    sys.path.insert(0, p)

from f1_timing import spread  # noqa: E402
from fewshot_timing import timed  # noqa: E402

COPY_CEILING_BYTES_PER_S = 6.29e12  # measured device copy ceiling (read + write bytes per second)
ALPHA = 0.5


def eager_weights(S, G, O, dev):
    """[G, S] float32 1-D blend weights, as the plan rounds them."""
    import torch
    u = torch.arange(S, device=dev, dtype=torch.float64)
    w = torch.ones(G, S, device=dev, dtype=torch.float64)
    if O:
        w[1:, :O] = ((u[:O] + 0.5) / O)[None]
        w[:-1, S - O:] = ((S - u[S - O:] - 0.5) / O)[None]
    return w.float()


def time_kernels(B, S, G, O, a, dev):
    import torch
    import torch.nn.functional as F

    from aaclip import ops
    C, step, n = ops.tile_canvas(S, G, O), S - O, G * G
    gen = torch.Generator(device=dev).manual_seed(S + G + O)
    canvas = torch.randn(B, 3, C, C, device=dev, generator=gen)
    tile_maps = torch.rand(B * n, S, S, device=dev, generator=gen) * 4
    global_maps = torch.rand(B, S, S, device=dev, generator=gen) * 4
    tile_scores = torch.rand(B * n, device=dev, generator=gen)
    global_scores = torch.rand(B, device=dev, generator=gen)
    tiles = torch.empty(B * n, 3, S, S, device=dev)
    out_map, out_score = torch.empty(B, C, C, device=dev), torch.empty(B, device=dev)
    w = eager_weights(S, G, O, dev)
    keep = {}

    def gather():
        ops.tile_gather(canvas, G, O, out=tiles)

    def gather_eager():
        t = tiles.view(B, n, 3, S, S)
        for ty in range(G):
            for tx in range(G):
                t[:, ty * G + tx].copy_(canvas[:, :, ty * step:ty * step + S, tx * step:tx * step + S])

    def stitch():
        ops.tile_stitch(tile_maps, G, O, global_maps=global_maps, global_weight=ALPHA, out=out_map)
        ops.tile_score(tile_scores, G, global_scores=global_scores, global_weight=ALPHA, out=out_score)

    def stitch_eager():
        acc = torch.zeros(B, C, C, device=dev)
        t = tile_maps.view(B, n, S, S)
        for ty in range(G):
            for tx in range(G):
                acc[:, ty * step:ty * step + S, tx * step:tx * step + S] += \
                    (w[ty][:, None] * w[tx][None, :]) * t[:, ty * G + tx]
        up = F.interpolate(global_maps[:, None], size=(C, C), mode="bilinear", align_corners=False)[:, 0]
        keep["map"] = (1 - ALPHA) * acc + ALPHA * up
        keep["score"] = (1 - ALPHA) * tile_scores.view(B, n).amax(1) + ALPHA * global_scores

    ms = timed({"tile_gather": gather, "torch_eager_gather": gather_eager, "tile_stitch_plus_score": stitch,
                "torch_eager_stitch": stitch_eager}, a.warmup, a.reps)
    torch.cuda.synchronize()
    gather_bytes = 2 * tiles.numel() * 4
    stitch_bytes = (tile_maps.numel() + global_maps.numel() + out_map.numel()) * 4
    res = {"batch": B, "side": S, "grid": G, "overlap": O, "canvas": C, "gather_bytes": gather_bytes,
           "stitch_bytes": stitch_bytes,
           "stitch_vs_eager_max_abs": float((out_map - keep["map"]).abs().max()),
           "score_vs_eager_max_abs": float((out_score - keep["score"]).abs().max())}
    for k, v in ms.items():
        nbytes = gather_bytes if "gather" in k else stitch_bytes
        rate = nbytes / (statistics.median(v) * 1e-3)
        res[k] = dict(spread(v), bytes_per_s=round(rate, 1), share_of_copy_ceiling=round(rate / COPY_CEILING_BYTES_PER_S, 4))
    res["eager_over_device_gather"] = round(statistics.median(ms["torch_eager_gather"])
                                            / statistics.median(ms["tile_gather"]), 3)
    res["eager_over_device_stitch"] = round(statistics.median(ms["torch_eager_stitch"])
                                            / statistics.median(ms["tile_stitch_plus_score"]), 3)
    return res


def time_step(B, S, G, O, tile_batch, a, dev):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from aaclip import ops
    from aaclip.engine import VisualEngine
    from oracle import synth
    sd = synth.clip_state_dict(111, S)
    ia, _ = synth.adapter_state_dicts(111)
    vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
    eng = VisualEngine(vp, {k: torch.from_numpy(v).to(dev) for k, v in ia.items()}, dtype=torch.float16)
    C = ops.tile_canvas(S, G, O)
    canvas = torch.randn(B, 3, C, C, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    view = F.adaptive_avg_pool2d(canvas, S).contiguous()
    T = torch.from_numpy(np.linalg.qr(np.random.default_rng(0).standard_normal((768, 2)))[0].astype(np.float32)).to(dev)
    x = torch.randn(tile_batch, 3, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(10))
    calls = -(-B * G * G // tile_batch)

    def tiled():
        eng.predict_tiled(canvas, T, G, O, global_view=view, global_weight=ALPHA, tile_batch=tile_batch)

    def plain():
        for _ in range(calls):
            eng.predict_cached(x, T, "Industrial")
        eng.predict_cached(view, T, "Industrial")

    ms = timed({"predict_tiled": tiled, "plain_predict_calls": plain}, a.warmup, a.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"batch": B, "side": S, "grid": G, "overlap": O, "canvas": C, "tile_batch": tile_batch,
            "tile_calls": calls, "global_call_batch": B, "weights": "random-init (seeded synthetic), synthetic images",
            **{k: spread(v) for k, v in ms.items()},
            "tiling_overhead_share": round(1.0 - med["plain_predict_calls"] / med["predict_tiled"], 4),
            "tiled_images_per_s": round(B / (med["predict_tiled"] * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="32:518:2:129,32:518:3:129,32:336:2:84")
    ap.add_argument("--step", default="32:518:2:129:32", help="batch:side:grid:overlap:tile_batch, or none")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "tiled_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tiled_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/tiled_timing.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "reps": a.reps, "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S, "global_weight": ALPHA,
           "method": "HIP events around each call, variants alternating in one process after warm-up, median and "
                     "min-max; bytes from the shapes", "kernels": {}}
    for item in a.shapes.split(","):
        B, S, G, O = (int(v) for v in item.split(":"))
        entry = time_kernels(B, S, G, O, a, dev)
        torch.cuda.empty_cache()
        res["kernels"][item] = entry
        print(item, json.dumps(entry), flush=True)
    if a.step != "none":
        B, S, G, O, tb = (int(v) for v in a.step.split(":"))
        res["step"] = time_step(B, S, G, O, tb, a, dev)
        print("step", json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
