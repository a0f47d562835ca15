"""Time one level of the stage-1 loss head (train.py:86-100) on an MI355X.

  python tools/segloss_timing.py [--batch 16] [--size 518] [--warmup 5] [--reps 30]
                                 [--out profiles/r08/segloss_timing.json]

Shape of record: B = 16 at 518 px (g = 37), per-image anchors [B, 768, 2], fp32 features.
One level's forward + backward -- calculate_similarity_map -> calculate_seg_loss ->
backward() to the anchors AND the features -- is timed with HIP events around the whole
sequence, after warm-up; the median and the spread of --reps runs. The identical formula
written in torch-ROCm eager ops (matmul, F.interpolate, softmax, the focal / dice terms,
autograd) runs on the same tensors IN THE SAME PROCESS, the two alternating. Then the
library sequence again under an ops.set_probe probe (HIP events around every launch): each
kernel's time and its bytes/s against the byte count derived from its operands. The share of
a stage-1 step uses the tower times of profiles/r07/surgery_timing.json (same batch, size,
fp16) when that file is there. Nothing is gated on these numbers. Needs a GPU.
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
import torch.nn.functional as F  # noqa: E402

from aaclip import ops  # noqa: E402
from forward_utils import calculate_seg_loss, calculate_similarity_map  # noqa: E402

COPY_CEILING_TBS = 6.29  # float4 copy measured on the MI355X (HBM3E, 8.0 TB/s spec)


def derived_bytes(B, g, S, C=768):
    """Bytes each launch must move at least once (fp32 operands, per-image anchors)."""
    L, px = g * g, S * S
    return {
        "patch_logits_per_image": 4 * (B * L * C + B * C * 2 + B * 2 * L),
        "blur_upsample": 4 * (B * 2 * L + B * 2 * px),
        "seg_loss": 4 * (B * 2 * px + B * px),
        "seg_loss_bwd": 4 * (B * 2 * px + B * px + B * 2 * px),
        "upsample_softmax_bwd": 4 * (B * 2 * px + 2 * B * 2 * L),
        "patch_logits_bwd": 4 * (B * L * C + B * L * C + B * C * 2 + B * 2 * L) + 2 * 4 * B * -(-L // 16) * 2 * C,
    }


def hip_step(f, T, mask, S):
    f.grad = T.grad = None
    loss = calculate_seg_loss(calculate_similarity_map(f, T, S), mask)
    loss.backward()
    return loss


def eager_step(f, T, mask, S):
    """forward_utils.py:196-227 of the reference, op for op, on device tensors."""
    f.grad = T.grad = None
    B, L, _ = f.shape
    g = int(round(L ** 0.5))
    z = (100.0 * torch.matmul(f, T)).permute(0, 2, 1).reshape(B, 2, g, g)
    p = torch.softmax(F.interpolate(z, size=S, mode="bilinear", align_corners=True), dim=1)
    m = mask.reshape(B, -1)
    k = m.long()
    lo, hi = 1e-5, 1.0 - 1e-5
    one_hot = torch.clamp(torch.stack([(k == 0).float(), (k == 1).float()], dim=1), lo, hi)
    pt = (one_hot * p.reshape(B, 2, -1)).sum(1) + 1e-5
    loss = (-1 * torch.pow(1 - pt, 2) * pt.log()).mean()
    for c, t in ((0, 1 - m), (1, m)):
        pc = p[:, c].reshape(B, -1)
        loss = loss + (1 - ((2 * (pc * t).sum(1) + 1) / (pc.sum(1) + t.sum(1) + 1)).sum() / B)
    loss.backward()
    return loss


def timed(fn, *args):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*args)
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


def spread(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 1), "min_us": round(min(ms) * 1e3, 1),
            "max_us": round(max(ms) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "segloss_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segloss_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    g = S // 14
    gen = torch.Generator(device="cpu").manual_seed(8)
    f = F.normalize(torch.randn(B, g * g, 768, generator=gen), dim=-1).to(dev).requires_grad_()
    T = F.normalize(torch.randn(B, 2, 768, generator=gen), dim=-1).transpose(1, 2).contiguous().to(dev).requires_grad_()
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    mask = (((yy - 0.4 * S) ** 2 + (xx - 0.6 * S) ** 2) <= (0.3 * S) ** 2).float()[None, None].repeat(B, 1, 1, 1).to(dev)

    for _ in range(a.warmup):
        lh, le = hip_step(f, T, mask, S), eager_step(f, T, mask, S)
    torch.cuda.synchronize()
    th, te = [], []
    for _ in range(a.reps):
        th.append(timed(hip_step, f, T, mask, S))
        te.append(timed(eager_step, f, T, mask, S))
    by_name = {}
    for _ in range(a.reps):
        probe = Probe()
        ops.set_probe(probe)
        try:
            hip_step(f, T, mask, S)
        finally:
            ops.set_probe(None)
        torch.cuda.synchronize()
        for name, b, e in probe.recs:
            by_name.setdefault(name, []).append(b.elapsed_time(e))
    # blur_upsample reports to no probe: timed on its own, on the same grid
    grid = torch.empty(B, 2, g, g, device=dev)
    ops.patch_logits_per_image(f.detach().reshape(B * g * g, 768), T.detach(), grid, group=g * g)
    out = torch.empty(B, 2, S, S, device=dev)
    by_name["blur_upsample"] = [timed(lambda: ops.blur_upsample(grid, out, ksize=0, sigma=0.0, softmax=True))
                                for _ in range(a.reps)]
    need = derived_bytes(B, g, S)
    kernels = {}
    for name in need:
        ms = by_name[name]
        med = statistics.median(ms)
        kernels[name] = dict(spread(ms), derived_bytes=need[name], GBs=round(need[name] / (med * 1e-3) / 1e9, 1),
                             share_of_copy_ceiling=round(need[name] / (med * 1e-3) / 1e12 / COPY_CEILING_TBS, 3))
    res = {"tool": "tools/segloss_timing.py", "device": torch.cuda.get_device_name(0), "batch": B, "img_size": S, "g": g,
           "anchors": "per image [B, 768, 2]", "features": "fp32", "leaves": "anchors and features",
           "warmup": a.warmup, "reps": a.reps, "copy_ceiling_TBs": COPY_CEILING_TBS,
           "method": "HIP events around one level's forward + backward, library and torch eager alternating in one "
                     "process after warm-up; per-kernel times from HIP events around every launch (ops.set_probe)",
           "loss_library": float(lh.detach()), "loss_eager": float(le.detach()),
           "library_fwd_bwd": spread(th), "eager_fwd_bwd": spread(te),
           "eager_over_library": round(statistics.median(te) / statistics.median(th), 3),
           "kernels": kernels, "sum_of_kernel_us": round(sum(k["median_us"] for k in kernels.values()), 1)}
    r07 = os.path.join(ROOT, "profiles", "r07", "surgery_timing.json")
    if os.path.exists(r07):
        runs = [r for r in json.load(open(r07))["runs"] if r["img_size"] == S and r["dtype"] == "fp16"]
        if runs and json.load(open(r07))["batch"] == B:
            towers = runs[0]["surgery_encode"]["median_ms"] + runs[0]["plain_encode"]["median_ms"]
            level_ms = statistics.median(th)
            res["stage1_step"] = {"towers_ms_quoted_from": "profiles/r07/surgery_timing.json (fp16, surgery + plain encode)",
                                  "towers_ms": round(towers, 3), "loss_head_level_ms": round(level_ms, 4),
                                  "share_one_level": round(level_ms / (towers + level_ms), 4),
                                  "share_four_levels": round(4 * level_ms / (towers + 4 * level_ms), 4)}
    print(json.dumps({k: res[k] for k in res if k != "kernels"}))
    for name, k in kernels.items():
        print(name, json.dumps(k))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
