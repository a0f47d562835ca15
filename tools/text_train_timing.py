"""Time one class's text anchors, forward + backward into the text adapter, on an MI355X.

  python tools/text_train_timing.py [--cls bottle] [--warmup 5] [--reps 30]
                                    [--out profiles/r09/text_train_timing.json]

What a stage-1 step (train.py:62-72, :99) does per distinct class of its batch:
get_adapted_single_class_text_embedding (6 + 10 prompts through the adapted 12-block text
tower, the anchor reduction) and, under loss.backward(), the backward down to the lowest
adapter, filling .grad of the four text_adapter weights. The model is the full-size tower on
the synthetic weights (oracle/synth.py); the loss is sum G * T + 0.1 (T0 . T1)^2. Timed with HIP
events around forward + backward after warm-up, median (min-max) of --reps runs. The identical
formula in torch-ROCm eager ops with autograd (tests/textbwd_ref.py, fp32, on the same device
tensors, truncated to the longest prompt like the engine) runs IN THE SAME PROCESS, the two
alternating. Then the library sequence again under an ops.set_probe probe (HIP events around
every probed launch): time per kernel name. text_embed_ln, eot_ln and anchor_reduce report to
no probe; the sum of kernel times against the end-to-end time shows how much of the step is
launch latency and host time. The share of a stage-1 step uses the tower times of
profiles/r07/surgery_timing.json (B = 16, 518 px, fp16: surgery + plain encode). Nothing is
gated on these numbers. Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "aa-clip_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import textbwd_ref as TR  # noqa: E402
from aaclip import ops  # noqa: E402
from dataset.constants import REAL_NAMES  # noqa: E402
from forward_utils import _sentences, get_adapted_single_class_text_embedding  # noqa: E402
from model.tokenizer import tokenize  # noqa: E402
from oracle import synth  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


class Probe:
    def __init__(self):
        self.recs = []

    def begin(self, kind, name, flops, nbytes):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return (name, e)

    def end(self, tok):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.recs.append(tok + (e,))


def spread(ms, unit="ms"):
    k = 1.0 if unit == "ms" else 1e3
    return {f"median_{unit}": round(statistics.median(ms) * k, 3), f"min_{unit}": round(min(ms) * k, 3),
            f"max_{unit}": round(max(ms) * k, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cls", default="bottle")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "text_train_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_train_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    dev = torch.device("cuda:0")
    sd = synth.clip_state_dict(111)
    clip = create_model("ViT-L-14-336", 336, pretrained=None, device=dev)
    clip.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = AdaptedCLIP(clip, relu=False, compute_dtype=torch.float32).to(dev).eval()
    _, ta = synth.adapter_state_dicts(111)
    model.text_adapter.load_state_dict({k: torch.from_numpy(v) for k, v in ta.items()})
    weights = [m.fc[0].weight for m in model.text_adapter]
    G = torch.from_numpy(TR.loss_weights()).to(dev)
    tn, tb = (tokenize(s).to(dev) for s in _sentences(REAL_NAMES["MVTec"][a.cls]))
    ctx = max(int(tn.argmax(-1).max()), int(tb.argmax(-1).max())) + 1

    def hip_step():
        for w in weights:
            w.grad = None
        T = get_adapted_single_class_text_embedding(model, "MVTec", a.cls, dev)
        loss = TR.fixture_loss(T, G)
        loss.backward()
        return loss

    P = {k: v.to(dev) for k, v in TR.params(sd, torch.float32).items()}
    ew = [w.detach().clone().requires_grad_() for w in weights]

    def eager_step():
        for w in ew:
            w.grad = None
        loss = TR.fixture_loss(TR.class_anchors(P, ew, tn, tb), G)
        loss.backward()
        return loss

    for _ in range(a.warmup):
        lh, le = hip_step(), eager_step()
    torch.cuda.synchronize()
    grad_gap = [TR.rel_l2(w.grad.cpu().numpy(), e.grad.cpu().numpy()) for w, e in zip(weights, ew)]
    th, te = [], []
    for _ in range(a.reps):
        th.append(timed(hip_step))
        te.append(timed(eager_step))
    by_name = {}
    for _ in range(a.reps):
        probe = Probe()
        ops.set_probe(probe)
        try:
            hip_step()
        finally:
            ops.set_probe(None)
        torch.cuda.synchronize()
        run = {}
        for name, b, e in probe.recs:
            t, c = run.get(name, (0.0, 0))
            run[name] = (t + b.elapsed_time(e), c + 1)
        for name, (t, c) in run.items():
            by_name.setdefault(name, {"launches": c, "ms": []})["ms"].append(t)
    kernels = {name: dict(launches=v["launches"], **spread(v["ms"], "us")) for name, v in sorted(by_name.items())}
    n_probed = sum(k["launches"] for k in kernels.values())
    sum_us = sum(k["median_us"] for k in kernels.values())
    step_ms = statistics.median(th)
    res = {"tool": "tools/text_train_timing.py", "device": torch.cuda.get_device_name(0), "class": a.cls,
           "sentences": [int(tn.shape[0]), int(tb.shape[0])], "context_after_truncation": ctx,
           "token_rows": [int(tn.shape[0]) * (int(tn.argmax(-1).max()) + 1), int(tb.shape[0]) * (int(tb.argmax(-1).max()) + 1)],
           "warmup": a.warmup, "reps": a.reps,
           "method": "HIP events around one class's anchors forward + backward, library and torch eager (fp32, autograd, "
                     "same device tensors) alternating in one process after warm-up; per-kernel times from HIP events "
                     "around every probed launch (ops.set_probe), summed per kernel name and run",
           "loss_library": float(lh.detach()), "loss_eager": float(le.detach()), "grad_rel_l2_library_vs_eager": grad_gap,
           "library_fwd_bwd": spread(th), "eager_fwd_bwd": spread(te),
           "eager_over_library": round(statistics.median(te) / step_ms, 3),
           "kernels": kernels, "probed_launches": n_probed, "sum_of_kernel_us": round(sum_us, 1),
           "kernel_time_share_of_step": round(sum_us * 1e-3 / step_ms, 3),
           "mean_us_per_probed_launch_end_to_end": round(step_ms * 1e3 / max(n_probed, 1), 2)}
    r07 = os.path.join(ROOT, "profiles", "r07", "surgery_timing.json")
    if os.path.exists(r07):
        d = json.load(open(r07))
        runs = [r for r in d["runs"] if r["img_size"] == 518 and r["dtype"] == "fp16"]
        if runs:
            towers = runs[0]["surgery_encode"]["median_ms"] + runs[0]["plain_encode"]["median_ms"]
            res["stage1_step"] = {
                "towers_ms_quoted_from": f"profiles/r07/surgery_timing.json (B = {d['batch']}, 518 px, fp16, surgery + plain encode)",
                "towers_ms": round(towers, 3), "text_class_ms": round(step_ms, 3),
                **{f"share_{n}_classes": round(n * step_ms / (towers + n * step_ms), 4) for n in (1, 4, 15)}}
    print(json.dumps({k: res[k] for k in res if k != "kernels"}))
    for name, k in kernels.items():
        print(name, json.dumps(k))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
