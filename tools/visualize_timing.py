"""Time the overlay rendering of forward_utils.visualize() on an MI355X.

  python tools/visualize_timing.py [--images 32] [--size 518] [--source 1024] [--warmup 5] [--reps 30] [--out FILE]

One class of --images maps at --size pixels (the class of tools/f1_timing.py) with --source-square
uint8 photos (blurred noise plus a little pixel noise, so that PNG has something to compress).
Measured, each after warm-up in one process:
  * the three kernels (ops.resize_bilinear_u8, ops.overlay_range, ops.overlay_panels) between HIP
    events, median and min-max of --reps runs (at least 20), alternating; the bytes each must move,
    computed from the shapes, over the median give its achieved bytes/s, set against the 6.3 TB/s
    that HBM streams on this chip (8 TB/s peak);
  * the device-to-host copy of the class's panels into pinned memory, between HIP events;
  * Pillow's PNG encode of the class's pictures, on one thread and on the 4 threads visualize()
    uses by default (host clock);
  * visualize() end to end (host clock around the call, which ends synchronised), given the photos
    as a list and given thumbnails on the device;
  * for scale, the numpy restatement tests/visualize_ref.py on the same class on a pool of 16
    threads (host clock).
The device pictures of the first two images are compared with the restatement, byte for byte.
The JSON goes to --out, by default profiles/r13/visualize_timing.json. Nothing is gated on these
numbers. Needs a GPU.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT, os.path.join(ROOT, "aa-clip_amd")):
    sys.path.insert(0, p)

from f1_timing import make_class, spread  # noqa: E402

HBM_STREAM = 6.3e12  # bytes/s achievable; the peak is 8e12


def make_photos(n, side, seed):
    import numpy as np
    from scipy import ndimage
    r = np.random.default_rng(seed)
    out = np.empty((n, side, side, 3), np.uint8)
    for i in range(n):
        field = ndimage.gaussian_filter(r.standard_normal((side, side, 3)), (6, 6, 0))
        field = 128 + 60 * field / field.std() + 3 * r.standard_normal((side, side, 3))
        out[i] = np.clip(field, 0, 255).astype(np.uint8)
    return out


def host_clock(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--source", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "visualize_timing.json"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("visualize_timing needs an MI355X: no GPU found (nothing is measured on the CPU)")
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    import forward_utils as fu
    import visualize_ref as VR
    from aaclip import ops
    dev = torch.device("cuda:0")
    n, S, side = a.images, a.size, a.source
    masks, maps, _, _ = make_class(n, S, S)
    photos = make_photos(n, side, S)
    d_maps, d_masks, d_photos = (torch.from_numpy(x).to(dev) for x in (maps, masks, photos))
    thumbs = ops.resize_bilinear_u8(d_photos, S)
    value_range = ops.overlay_range(d_maps)
    panels = ops.overlay_panels(d_maps, thumbs, labels=d_masks, value_range=value_range)
    pinned = torch.empty(panels.shape, dtype=torch.uint8).pin_memory()
    variants = {"resize_bilinear_u8": lambda: ops.resize_bilinear_u8(d_photos, S, out=thumbs),
                "overlay_range": lambda: ops.overlay_range(d_maps),
                "overlay_panels": lambda: ops.overlay_panels(d_maps, thumbs, labels=d_masks, value_range=value_range,
                                                             out=panels),
                "d2h_copy_pinned": lambda: pinned.copy_(panels, non_blocking=True)}
    pix = n * S * S
    need = {"resize_bilinear_u8": n * side * side * 3 + pix * 3,  # every source pixel is a tap at this ratio
            "overlay_range": pix * 4,
            "overlay_panels": pix * (4 + 1 + 3) + pix * 9,
            "d2h_copy_pinned": pix * 9}
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
    res = {"tool": "tools/visualize_timing.py", "device": torch.cuda.get_device_name(0), "images": n, "img_size": S,
           "source": [side, side], "warmup": a.warmup, "reps": a.reps,
           "method": "HIP events around each op (output and workspace from the caching allocator where the op "
                     "allocates), alternating in one process after warm-up, median and min-max; host clock around "
                     "the host work; bytes from the shapes",
           "hbm_stream_bytes_per_s": HBM_STREAM, "device_ops": {}}
    for k, v in ms.items():
        med = statistics.median(v) * 1e-3
        entry = dict(spread(v), bytes=need[k], bytes_per_s=round(need[k] / med, 1))
        if k != "d2h_copy_pinned":
            entry["share_of_hbm_stream"] = round(need[k] / med / HBM_STREAM, 4)
        res["device_ops"][k] = entry
    host = pinned.numpy()

    def encode(i):
        Image.fromarray(host[i]).save(io.BytesIO(), format="PNG")

    def encode_all(workers):
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(encode, range(n)))
    encode_all(4)
    res["png_encode_class_1_thread"] = spread(host_clock(lambda: [encode(i) for i in range(n)], 3))
    res["png_encode_class_4_threads"] = spread(host_clock(lambda: encode_all(4), 3))
    names = [f"timing/test/defect/{i:03d}.png" for i in range(n)]
    with tempfile.TemporaryDirectory() as tmp:
        listed = [p for p in photos]
        fu.visualize(d_masks, d_maps, names, tmp, "timing", "class", images=listed)
        res["visualize_from_host_photos"] = spread(host_clock(
            lambda: fu.visualize(d_masks, d_maps, names, tmp, "timing", "class", images=listed), 3))
        res["visualize_from_device_thumbnails"] = spread(host_clock(
            lambda: fu.visualize(d_masks, d_maps, names, tmp, "timing", "class", images=thumbs), 3))
        res["png_bytes_per_picture"] = int(statistics.mean(os.path.getsize(os.path.join(
            tmp, "visualization", "timing", "class", f"defect_{i:03d}.png")) for i in range(n)))
    rng = VR.value_range(maps)

    def restate(i):
        return VR.panels(maps[i:i + 1], masks[i:i + 1], VR.resize(photos[i], S)[None], rng)[0]

    def restate_all():
        with ThreadPoolExecutor(max_workers=16) as pool:
            return list(pool.map(restate, range(n)))
    res["numpy_restatement_16_threads"] = spread(host_clock(restate_all, 2))
    res["equal_to_restatement_on_2_images"] = all(np.array_equal(host[i], restate(i)) for i in range(2))
    kernels = sum(res["device_ops"][k]["median_us"] for k in ("resize_bilinear_u8", "overlay_range", "overlay_panels"))
    res["kernels_median_us_sum"] = round(kernels, 1)
    res["png_encode_4_threads_over_kernels"] = round(res["png_encode_class_4_threads"]["median_us"] / kernels, 1)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
