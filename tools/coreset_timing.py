"""Time the greedy k-centre coreset selection of the few-shot memory bank on an MI355X.

  python tools/coreset_timing.py [--warmup 1] [--reps 5] [--out FILE] [--sizes 2304:0.1,43808:0.1,273800:0.01]

Measured, each after warm-up in one process, between HIP events, alternating, median and min-max
(the method of tools/fewshot_timing.py):
  * one level's selection, ops.bank_coreset on fp16 unit rows (seeded random, K = 768), at each
    rows:ratio of --sizes (by default the c2 bank at 10 %, the reference's defaults 518 px / --shot 32
    at 10 % and a full-shot MVTec class at 1 %), against a torch eager greedy loop on the same
    operands (index_select of the centre, mv, maximum, masked argmin; the pick stays on the device,
    so neither arm synchronises inside the loop). Per step: the time, the bank bytes per second it
    amounts to (N K 2 bytes are read once per step; the 8.6 TB/s the Infinity Cache serves a 38 MB
    table at is the ceiling this is quoted against, not a bar) and the bytes of the redundant
    candidate reduction, blocks^2 x 8. Whether the two arms pick the same rows is recorded (eager
    rounds every similarity to fp16, so they may part at a near-tie);
  * the whole step at 518 px / --shot 32 on an engine with seeded synthetic weights in the fp16
    mode: VisualEngine.predict_few_shot with a 10 % coreset bank against the full bank and against
    the plain predict, with the fp16 and the MX fp8 search, and build_bank with and without the
    selection;
  * how far the few-shot map moves against the full bank's on that engine: RANDOM-INIT weights and
    synthetic images, so it says what the subsampling does to this map, not to a detector's accuracy.
The JSON goes to --out, by default profiles/r19/coreset_timing.json. Nothing is gated on these
numbers. Needs a GPU.
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
from fewshot_timing import K, timed, unit_rows  # noqa: E402

INFINITY_CACHE_BYTES_PER_S = 8.6e12  # measured read rate on a 38 MB table (the microarchitecture guide)


def eager_greedy(rows, m):
    """The same selection as torch eager calls; returns the picks (device int64 [m])."""
    import torch
    n = rows.shape[0]
    maxsim = torch.full((n,), float("-inf"), device=rows.device)
    taken = torch.zeros(n, dtype=torch.bool, device=rows.device)
    inf = torch.full((), float("inf"), device=rows.device)
    sel = torch.empty(m, dtype=torch.int64, device=rows.device)
    c = torch.zeros(1, dtype=torch.int64, device=rows.device)
    for t in range(m):
        sel[t:t + 1] = c
        taken.index_fill_(0, c, True)
        maxsim = torch.maximum(maxsim, torch.mv(rows, rows.index_select(0, c).view(-1)).float())
        c = torch.argmin(torch.where(taken, inf, maxsim)).view(1)
    return sel


def time_selection(n, ratio, a, dev):
    import torch

    from aaclip import ops
    rows = unit_rows(n, 3, dev)
    m = ops.coreset_rows(n, ratio)
    blocks = ops.coreset_blocks(n)
    out = {}

    def device():
        out["device"] = ops.bank_coreset(rows, m, 0)

    def eager():
        out["eager"] = eager_greedy(rows, m)
    ms = timed({"bank_coreset": device, "torch_eager_greedy": eager}, a.warmup, a.reps)
    torch.cuda.synchronize()
    sel, cover, maxsim = out["device"]
    bank_bytes = n * K * rows.element_size()
    res = {"rows": n, "ratio": ratio, "picks": m, "K": K, "dtype": "float16", "blocks": blocks,
           "bank_bytes": bank_bytes, "candidate_reduction_bytes_per_step": blocks * blocks * 8,
           "coverage": float(maxsim.min()), "last_cover": float(cover[-1]),
           "same_picks_as_eager": bool(torch.equal(sel.long(), out["eager"])),
           "common_picks_with_eager": len(set(sel.cpu().tolist()) & set(out["eager"].cpu().tolist()))}
    for k, v in ms.items():
        per_step = statistics.median(v) * 1e-3 / m
        res[k] = dict(spread(v), us_per_step=round(per_step * 1e6, 3),
                      bank_bytes_per_s=round(bank_bytes / per_step, 1),
                      share_of_infinity_cache_rate=round(bank_bytes / per_step / INFINITY_CACHE_BYTES_PER_S, 4))
    res["eager_over_device"] = round(statistics.median(ms["torch_eager_greedy"])
                                     / statistics.median(ms["bank_coreset"]), 3)
    return res


def time_step(batch, S, shot, ratio, a, dev):
    import numpy as np
    import torch

    from aaclip.engine import VisualEngine
    from oracle import synth
    sd = synth.clip_state_dict(111, S)
    ia, _ = synth.adapter_state_dicts(111)
    vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
    eng = VisualEngine(vp, {k: torch.from_numpy(v).to(dev) for k, v in ia.items()}, dtype=torch.float16)
    x = torch.from_numpy(synth.images(7, batch, S)).to(dev)
    support = torch.from_numpy(synth.images(8, shot, S)).to(dev)
    T = torch.from_numpy(np.linalg.qr(np.random.default_rng(0).standard_normal((K, 2)))[0].astype(np.float32)).to(dev)
    fp8 = torch.float8_e4m3fn
    banks = {"full_fp16": eng.build_bank(support), "coreset_fp16": eng.build_bank(support, None, ratio),
             "full_fp8": eng.build_bank(support, fp8), "coreset_fp8": eng.build_bank(support, fp8, ratio)}
    variants = {"predict": lambda: eng.predict(x, T, "Industrial")}
    for name, bank in banks.items():
        variants["predict_few_shot_" + name] = lambda bank=bank: eng.predict_few_shot(x, T, bank, "Industrial")
    variants.update({"build_bank_full_fp16": lambda: eng.build_bank(support),
                     "build_bank_coreset_fp16": lambda: eng.build_bank(support, None, ratio),
                     "build_bank_full_fp8": lambda: eng.build_bank(support, fp8),
                     "build_bank_coreset_fp8": lambda: eng.build_bank(support, fp8, ratio)})
    ms = timed(variants, a.warmup, a.reps)
    res = {k: spread(v) for k, v in ms.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    res["rows_per_level"] = {k: [b.rows, b.source_rows] for k, b in banks.items()}
    res["coverage_per_level"] = [float(c) for c in banks["coreset_fp16"].coverage]
    for name in banks:
        res[f"few_shot_{name}_over_predict"] = round(med["predict_few_shot_" + name] / med["predict"], 3)
    # quality: the few-shot map against the full bank's, per search dtype
    res["fs_map_shift"] = {"weights": "random-init (seeded synthetic), synthetic images"}
    for dt in ("fp16", "fp8"):
        full = eng.predict_few_shot(x, T, banks["full_" + dt], "Industrial")[2]
        kept = eng.predict_few_shot(x, T, banks["coreset_" + dt], "Industrial")[2]
        d = kept - full
        res["fs_map_shift"][dt] = {"full_min": float(full.min()), "full_max": float(full.max()),
                                   "full_mean": float(full.mean()), "max_abs": float(d.abs().max()),
                                   "mean_abs": float(d.abs().mean()), "min_signed": float(d.min()),
                                   "pearson": float(torch.corrcoef(torch.stack([full.flatten(), kept.flatten()]))[0, 1])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="2304:0.1,43808:0.1,273800:0.01")
    ap.add_argument("--step", default="32:518:32:0.1", help="batch:img_size:shot:ratio of the whole step, or none")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "coreset_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("coreset_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/coreset_timing.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "reps": a.reps, "infinity_cache_bytes_per_s": INFINITY_CACHE_BYTES_PER_S,
           "method": "HIP events around each call, variants alternating in one process after warm-up, median and "
                     "min-max; bytes from the shapes", "selection_one_level": {}}
    for item in a.sizes.split(","):
        n, ratio = item.split(":")
        entry = time_selection(int(n), float(ratio), a, dev)
        torch.cuda.empty_cache()
        res["selection_one_level"][item] = entry
        print(item, json.dumps(entry), flush=True)
    if a.step != "none":
        batch, S, shot, ratio = a.step.split(":")
        res["step"] = dict(batch=int(batch), img_size=int(S), shot=int(shot), ratio=float(ratio),
                           **time_step(int(batch), int(S), int(shot), float(ratio), a, dev))
        print("step", json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
