"""Time one stage-2 step's visual forward + backward into the image adapter on an MI355X.

  python tools/image_train_timing.py [--batch 2] [--img 518] [--warmup 5] [--reps 30] [--dtype fp32|bf16]
                                     [--out profiles/r10/image_train_timing.json]

What a stage-2 step (train.py:145-156) does on the visual side: AdaptedCLIP.forward under grad
(VisualEngine.forward_train: the 24-block tower with the activations of the blocks above the
lowest trainable adapter kept) and, under loss.backward(), the HIP backward down to that adapter,
filling .grad of the 11 image_adapter weights. The model is the full-size tower on the synthetic
weights (oracle/synth.py) at the reference's own shape (B = 2, 518 px, fp32); the loss is
sum_j sum(G_j seg_j) + sum(G_d det). Timed with HIP events around forward + backward after
warm-up, median (min-max) of --reps runs. The identical formula in torch-ROCm eager ops with
autograd (tests/imagebwd_ref.py, fp32, on the same device tensors) runs IN THE SAME PROCESS, the
two alternating. Then the library sequence again under an ops.set_probe probe (HIP events around
every probed launch): time per kernel name, with the achieved TFLOP/s of attention_bwd_tiled
against the 157 TFLOP/s fp32-MFMA peak. --dtype bf16 times the bf16 mixed-precision step instead
(AdaptedCLIP(compute_dtype = train_dtype = bfloat16); the eager formula stays fp32), reports
attention_bwd16 against the 2.5 PFLOP/s bf16 dense peak and writes
profiles/r12/image_train_timing_bf16.json by default. Both report the peak device memory of one
library step. Nothing is gated on these numbers. Needs a GPU.
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

import imagebwd_ref as IR  # noqa: E402
from aaclip import ops  # noqa: E402
from oracle import synth  # noqa: E402

FP32_MFMA_PEAK_TF = 157.0
BF16_MFMA_PEAK_TF = 2500.0


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
        return (kind if kind.startswith("gemm") else name, flops, e)  # GEMMs by shape and epilogue, the rest by kernel

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
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--img", type=int, default=518)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = (os.path.join(ROOT, "profiles", "r10", "image_train_timing.json") if a.dtype == "fp32" else
                 os.path.join(ROOT, "profiles", "r12", "image_train_timing_bf16.json"))
    if not torch.cuda.is_available():
        raise SystemExit("image_train_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    dev = torch.device("cuda:0")
    sd = synth.clip_state_dict(111, img_size=a.img)
    clip = create_model("ViT-L-14-336", a.img, pretrained=None, device=dev,
                        force_image_size=a.img if a.img != 336 else None)
    clip.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    if a.dtype == "bf16":
        model = AdaptedCLIP(clip, relu=False, compute_dtype=torch.bfloat16, train_dtype=torch.bfloat16).to(dev).eval()
    else:
        model = AdaptedCLIP(clip, relu=False, compute_dtype=torch.float32).to(dev).eval()
    ia, _ = synth.adapter_state_dicts(111)
    model.image_adapter.load_state_dict({k: torch.from_numpy(v) for k, v in ia.items()})
    for p in model.parameters():
        p.requires_grad_(False)
    weights = model._adapter_weights()
    for w in weights:
        w.requires_grad_(True)
    n_patch = (a.img // 14) ** 2
    G = [torch.from_numpy(g).to(dev) for g in IR.loss_weights(n_patch, batch=a.batch)]
    x = torch.from_numpy(synth.images(IR.X_SEED, a.batch, a.img)).to(dev)

    def hip_step():
        for w in weights:
            w.grad = None
        seg, det = model(x)
        loss = IR.fixture_loss(seg, det, G)
        loss.backward()
        return loss

    # peak device memory of one library step (the packed tower, its transposes and the kept
    # activations), before the eager formula's own copy of the weights exists
    hip_step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    hip_step()
    torch.cuda.synchronize()
    peak_mib = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)

    P = {k: v.to(dev) for k, v in IR.params(sd, torch.float32).items()}
    ew = [w.detach().clone().requires_grad_() for w in weights]

    def eager_step():
        for w in ew:
            w.grad = None
        seg, det = IR.forward(P, ew, x)
        loss = IR.fixture_loss(seg, det, G)
        loss.backward()
        return loss

    for _ in range(a.warmup):
        lh, le = hip_step(), eager_step()
    torch.cuda.synchronize()
    grad_gap = [IR.rel_l2(w.grad.cpu().numpy(), e.grad.cpu().numpy()) for w, e in zip(weights, ew)]
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
        for name, flops, b, e in probe.recs:
            t, c, f = run.get(name, (0.0, 0, 0.0))
            run[name] = (t + b.elapsed_time(e), c + 1, f + flops)
        for name, (t, c, f) in run.items():
            by_name.setdefault(name, {"launches": c, "flops": f, "ms": []})["ms"].append(t)
    step_ms = statistics.median(th)
    kernels = {}
    for name, v in sorted(by_name.items()):
        k = dict(launches=v["launches"], **spread(v["ms"], "us"))
        k["share_of_step"] = round(statistics.median(v["ms"]) / step_ms, 4)
        if v["flops"] > 0:
            k["tflops"] = round(v["flops"] / (statistics.median(v["ms"]) * 1e-3) / 1e12, 2)
        kernels[name] = k
    n_probed = sum(k["launches"] for k in kernels.values())
    sum_us = sum(k["median_us"] for k in kernels.values())
    res = {"tool": "tools/image_train_timing.py", "device": torch.cuda.get_device_name(0), "batch": a.batch,
           "img_size": a.img, "tokens_per_image": n_patch + 1, "dtype": a.dtype, "warmup": a.warmup, "reps": a.reps,
           "method": "HIP events around one visual forward + backward, library and torch eager (fp32, autograd, same "
                     "device tensors) alternating in one process after warm-up; per-kernel times from HIP events "
                     "around every probed launch (ops.set_probe), summed per kernel name and run",
           "loss_library": float(lh.detach()), "loss_eager": float(le.detach()), "grad_rel_l2_library_vs_eager": grad_gap,
           "library_fwd_bwd": spread(th), "eager_fwd_bwd": spread(te), "library_step_peak_memory_mib": peak_mib,
           "eager_over_library": round(statistics.median(te) / step_ms, 3),
           "kernels": kernels, "probed_launches": n_probed, "sum_of_kernel_us": round(sum_us, 1),
           "kernel_time_share_of_step": round(sum_us * 1e-3 / step_ms, 3)}
    if "attention_bwd_tiled" in kernels:
        tf = kernels["attention_bwd_tiled"]["tflops"]
        res["attention_bwd_tiled"] = {"tflops": tf, "fp32_mfma_peak_tflops": FP32_MFMA_PEAK_TF,
                                      "fraction_of_peak": round(tf / FP32_MFMA_PEAK_TF, 3)}
    if "attention_bwd16" in kernels:
        tf = kernels["attention_bwd16"]["tflops"]
        res["attention_bwd16"] = {"tflops": tf, "bf16_mfma_peak_tflops": BF16_MFMA_PEAK_TF,
                                  "fraction_of_peak": round(tf / BF16_MFMA_PEAK_TF, 3)}
    print(json.dumps({k: res[k] for k in res if k != "kernels"}))
    for name, k in kernels.items():
        print(name, json.dumps(k))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
