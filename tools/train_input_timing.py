"""Time the train split's input pipeline on an MI355X, next to the training steps it feeds.

  python tools/train_input_timing.py [--src 1024] [--img 518] [--warmup 5] [--reps 30]
                                     [--cpu_items 6] [--out profiles/r11/train_input_timing.json]

Device path (aaclip.preprocess.TrainPreprocessor.apply): colour jitter on the uint8 source ->
bicubic resize + normalise -> nearest mask -> one geometric gather, on --src x --src sources to
--img pixels, at B = 16 (stage 1's batch) and B = 2 (stage 2's), every transform applied to every
image (the most work a batch can ask for). HIP events around each part and around the whole
apply, after warm-up; median (min-max) of --reps runs. For the two new kernels the bytes the
algorithm moves (csrc/augment.hip's header) over the median give the achieved bytes/s and its
share of the 8.0 TB/s HBM peak (and of the 6.29 TB/s float4-copy ceiling).

CPU path (TrainPreprocessor.cpu_item, what --no-gpu_preprocess runs in each loader worker):
wall time per image on ONE thread (torch.set_num_threads(1)), from PIL images already decoded,
--cpu_items images, alternating with the device path's B = 2 apply in the same loop. Decoding
(both paths do it in the workers) is timed on its own from an in-memory PNG.

The step times the input has to keep up with are QUOTED from profiles/r07, r09 and r10, not
measured again. Nothing is gated on these numbers. Needs a GPU.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "aa-clip_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aaclip.preprocess import TrainPreprocessor  # noqa: E402

HBM_PEAK_TBS = 8.0
COPY_CEILING_TBS = 6.29  # float4 copy, measured (profiles/r07/surgery_timing.json uses the same figure)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, unit="ms"):
    k = 1.0 if unit == "ms" else 1000.0
    return {f"median_{unit}": round(statistics.median(ms) * k, 3), f"min_{unit}": round(min(ms) * k, 3),
            f"max_{unit}": round(max(ms) * k, 3)}


def params_all_on(tp, B, seed):
    """A sampled batch with every transform switched on (factors and angles as drawn)."""
    g = torch.Generator().manual_seed(seed)
    while True:
        p = tp.sample(64 * B, g)
        keep = ((p["color"] != 1).all(1) & p["rotate"] & (p["shift"] != 0).all(1)).nonzero()[:, 0]
        if len(keep) >= B:
            p = {k: v[keep[:B]] for k, v in p.items()}
            p["hflip"][:] = True
            p["vflip"][:] = True
            return p


def device_arm(tp, B, src, S, warmup, reps, dev):
    rng = np.random.default_rng(B)
    u8 = torch.from_numpy(rng.integers(0, 256, (B, src, src, 3), dtype=np.uint8)).to(dev)
    mk = torch.from_numpy((rng.random((B, src, src)) > 0.9).astype(np.uint8) * 255).to(dev)
    p = params_all_on(tp, B, 7)
    jit = torch.empty_like(u8)
    img, mask = tp.images(u8), tp.masks(mk)
    parts = {
        "color_jitter_u8": lambda: tp.jitter(u8, p["color"], out=jit),
        "preprocess_images": lambda: tp.images(jit),
        "resize_masks_nearest": lambda: tp.masks(mk),
        "geom_augment": lambda: tp.geom(img, p, mask),
        "apply": lambda: tp.apply(u8, mk, p),
    }
    for fn in parts.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in parts}
    for _ in range(reps):  # the parts take turns, so a slow spell of the machine lands on all of them
        for k, fn in parts.items():
            t[k].append(timed(fn))
    out = {k: stats(v, "us") for k, v in t.items()}
    # bytes the algorithm moves (csrc/augment.hip): jitter with contrast = 3 reads (reduce), 3 reads + 3 writes
    # (apply) per pixel; geometry = 4 C S^2 written and at most as much read
    nbytes = {"color_jitter_u8": 9 * src * src * B, "geom_augment": 2 * 4 * 4 * S * S * B}
    for k, n in nbytes.items():
        tbs = n / (out[k]["median_us"] * 1e-6) / 1e12
        out[k].update(bytes_moved=n, achieved_TBs=round(tbs, 3), share_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 4),
                      share_of_copy_ceiling=round(tbs / COPY_CEILING_TBS, 4))
    out["apply"]["us_per_image"] = round(out["apply"]["median_us"] / B, 2)
    return out, (u8, mk, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=int, default=1024)
    ap.add_argument("--img", type=int, default=518)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu_items", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "train_input_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_input_timing needs a GPU: nothing here is measured on the CPU alone")
    from PIL import Image
    dev = torch.device("cuda:0")
    tp = TrainPreprocessor(a.img, text=False)
    res = {"tool": "tools/train_input_timing.py", "device": torch.cuda.get_device_name(0), "src": a.src,
           "img_size": a.img, "warmup": a.warmup, "reps": a.reps, "hbm_peak_TBs": HBM_PEAK_TBS,
           "copy_ceiling_TBs": COPY_CEILING_TBS,
           "method": "HIP events around each launch sequence after warm-up, the parts taking turns inside one loop; "
                     "every transform applied to every image; CPU path: perf_counter around cpu_item on one "
                     "thread, alternating with the B = 2 device apply",
           "device_path": {}}
    keep = None
    for B in (16, 2):
        res["device_path"][f"B{B}"], keep = device_arm(tp, B, a.src, a.img, a.warmup, a.reps, dev)
    u8, mk, p = keep  # B = 2

    # CPU path, one thread, alternating with the device apply
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    rng = np.random.default_rng(99)
    src_img = rng.integers(0, 256, (a.src, a.src, 3), dtype=np.uint8)
    pil = Image.fromarray(src_img, "RGB")
    pmask = Image.fromarray(((rng.random((a.src, a.src)) > 0.9) * 255).astype(np.uint8), "L")
    png = io.BytesIO()
    pil.save(png, format="PNG")
    cpu_ms, dev_ms, dec_ms = [], [], []
    tp.cpu_item(pil, pmask, p, 0)  # warm-up
    for i in range(a.cpu_items):
        t0 = time.perf_counter()
        tp.cpu_item(pil, pmask, p, i % 2)
        cpu_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(timed(lambda: tp.apply(u8, mk, p)))
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(png.getvalue())).convert("RGB"))
        dec_ms.append((time.perf_counter() - t0) * 1e3)
    torch.set_num_threads(threads)
    res["cpu_path_one_worker"] = {"per_image": stats(cpu_ms), "device_apply_B2_alternating": stats(dev_ms),
                                  "png_decode_per_image_noise_source": stats(dec_ms),
                                  "note": "decode of a noise image is an upper bound for a PNG of this size; "
                                          "both paths decode in the workers"}

    # the steps the input feeds (quoted)
    def quoted(path, *keys):
        v = json.load(open(os.path.join(ROOT, path)))
        for k in keys:
            v = v[k]
        return v
    towers = quoted("profiles/r09/text_train_timing.json", "stage1_step", "towers_ms")
    per_class = quoted("profiles/r09/text_train_timing.json", "stage1_step", "text_class_ms")
    stage2 = quoted("profiles/r10/image_train_timing.json", "library_fwd_bwd", "median_ms")
    cpu = res["cpu_path_one_worker"]["per_image"]["median_ms"]
    workers = 4
    steps = {"stage1_B16_1_class": (16, towers + per_class), "stage1_B16_4_classes": (16, towers + 4 * per_class),
             "stage2_B2": (2, stage2)}
    res["steps_quoted"] = {"stage1_towers_ms": towers, "stage1_per_class_ms": per_class, "stage2_fwd_bwd_ms": stage2,
                           "from": "profiles/r07/surgery_timing.json via profiles/r09/text_train_timing.json; "
                                   "profiles/r10/image_train_timing.json"}
    res["verdict"] = {}
    dec = res["cpu_path_one_worker"]["png_decode_per_image_noise_source"]["median_ms"]
    for name, (B, step_ms) in steps.items():
        # four workers, one image each at a time: the transforms alone, and with the decode both paths pay
        cpu_batch, cpu_dec_batch, dec_batch = B * cpu / workers, B * (cpu + dec) / workers, B * dec / workers
        dev_batch = res["device_path"][f"B{B}"]["apply"]["median_us"] / 1e3
        res["verdict"][name] = {"step_ms": round(step_ms, 3), "cpu_4_workers_ms_per_batch": round(cpu_batch, 3),
                                "cpu_4_workers_with_decode_ms_per_batch": round(cpu_dec_batch, 3),
                                "cpu_workers_bound_the_step": bool(cpu_batch > step_ms),
                                "cpu_workers_with_decode_bound_the_step": bool(cpu_dec_batch > step_ms),
                                "decode_only_4_workers_ms_per_batch": round(dec_batch, 3),
                                "decode_only_workers_bound_the_step": bool(dec_batch > step_ms),
                                "device_apply_ms_per_batch": round(dev_batch, 3),
                                "device_apply_share_of_step": round(dev_batch / step_ms, 4)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
