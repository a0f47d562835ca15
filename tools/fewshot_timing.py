"""Time the few-shot memory-bank scoring on an MI355X.

  python tools/fewshot_timing.py [--warmup 3] [--reps 20] [--out FILE] [--shapes c2,ref518]

Two settings: c2 (batch 32 at 336 px, --shot 4: 18 432 query rows against a bank of 2 304 rows per
level) and ref518, the reference's defaults (batch 32 at 518 px, --shot 32: 43 808 x 43 808 per level).
Measured, each after warm-up in one process, between HIP events, alternating, median and min-max:
  * one level's search, ops.bank_nn + ops.bank_distance, on fp16 unit rows (seeded random), against
    torch eager amax(q @ bank.T, 1) in fp16 on the same operands, which writes the [M, Nb] matrix
    (its bytes are recorded; where it does not fit in memory that is recorded instead, not forced).
    The 2 M Nb K operations over the median give the achieved FLOP/s, set against the 2.5 PFLOP/s
    dense fp16 peak; the largest difference between the two results is recorded;
  * the whole step on an engine with seeded synthetic weights in the fp16 mode:
    VisualEngine.predict_few_shot (zero-shot map and score, four searches, the few-shot map) against
    the plain VisualEngine.predict (one stream, eager) on the same batch.
The JSON goes to --out, by default profiles/r13/fewshot_timing.json. Nothing is gated on these
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

PEAK_F16 = 2.5e15  # dense fp16 MFMA FLOP/s
SHAPES = {"c2": dict(batch=32, img_size=336, shot=4), "ref518": dict(batch=32, img_size=518, shot=32)}
K = 768


def timed(variants, warmup, reps):
    """{name: [ms]} of the callables, alternating, HIP events around each call."""
    import torch
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def unit_rows(n, seed, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, K, device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.float16)


def time_search(M, Nb, a, dev):
    import torch

    from aaclip import ops
    q, bank = unit_rows(M, 1, dev), unit_rows(Nb, 2, dev)
    n_splits, _ = ops.bank_nn_plan(M, Nb)
    part = torch.empty(M, n_splits, device=dev)
    grid = torch.empty(M, device=dev)

    def fused():
        ops.bank_nn(q, bank, part)
        ops.bank_distance(part, grid, accumulate=False)
    variants = {"bank_nn_plus_distance": fused}
    eager_out, res = {}, {"M": M, "Nb": Nb, "K": K, "n_splits": n_splits, "blocks": -(-M // ops.BANK_TM) * n_splits,
                          "flops": 2.0 * M * Nb * K, "eager_matrix_bytes": 2 * M * Nb}
    try:
        eager_out["d"] = 1.0 - torch.amax(q @ bank.T, 1).float()
        torch.cuda.synchronize()

        def eager():
            eager_out["d"] = 1.0 - torch.amax(q @ bank.T, 1).float()
        variants["torch_eager_fp16"] = eager
    except torch.OutOfMemoryError:
        res["torch_eager_fp16"] = "did not fit in memory"
        torch.cuda.empty_cache()
    ms = timed(variants, a.warmup, a.reps)
    for k, v in ms.items():
        med = statistics.median(v) * 1e-3
        res[k] = dict(spread(v), flops_per_s=round(res["flops"] / med, 1),
                      share_of_fp16_peak=round(res["flops"] / med / PEAK_F16, 4))
    if "torch_eager_fp16" in ms:
        res["eager_over_fused"] = round(statistics.median(ms["torch_eager_fp16"])
                                        / statistics.median(ms["bank_nn_plus_distance"]), 3)
        # eager rounds every similarity to fp16 before the maximum: half an ulp of values near 1
        res["max_abs_difference_from_eager"] = float((grid - eager_out["d"]).abs().max())
    return res


def time_step(batch, S, shot, a, dev):
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
    bank = eng.build_bank(support)
    ms = timed({"predict": lambda: eng.predict(x, T, "Industrial"),
                "predict_few_shot": lambda: eng.predict_few_shot(x, T, bank, "Industrial"),
                "build_bank": lambda: eng.build_bank(support)}, a.warmup, a.reps)
    res = {k: spread(v) for k, v in ms.items()}
    res["bank_rows_per_level"] = int(bank.levels[0].shape[0])
    res["few_shot_over_predict"] = round(statistics.median(ms["predict_few_shot"]) / statistics.median(ms["predict"]),
                                         3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="c2,ref518")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "fewshot_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fewshot_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/fewshot_timing.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "reps": a.reps, "fp16_peak_flops_per_s": PEAK_F16,
           "method": "HIP events around each call, variants alternating in one process after warm-up, median and "
                     "min-max; operations from the shapes", "shapes": {}}
    for name in a.shapes.split(","):
        s = SHAPES[name]
        P = (s["img_size"] // 14) ** 2
        entry = dict(s, patches=P)
        entry["search_one_level"] = time_search(s["batch"] * P, s["shot"] * P, a, dev)
        torch.cuda.empty_cache()
        entry["step"] = time_step(s["batch"], s["img_size"], s["shot"], a, dev)
        torch.cuda.empty_cache()
        res["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
