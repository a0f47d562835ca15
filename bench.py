"""AA-CLIP anomaly-map inference benchmark on MI355X (BASELINE.json metric:
images/sec at 336x336, ViT-L/14, + pixel-map parity vs the CPU reference).

One step = one batch of 32 synthetic 336x336 images per GPU through the full
hot path, inputs already resident in HBM: ViT-L/14-336 visual tower with the 6
residual adapters, 4 level taps + seg/det projections, fused anomaly map
(Industrial blur) and image scores; for N > 1 the per-image scores are
all-gathered over RCCL (the path's only exchange). Weights: random-init
synthetic (no checkpoint in the image), bf16 compute.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 32] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...   (one process per GPU)

Prints ONE JSON line on rank 0. A plain run sets up,
warms up, times the K steps and prints the headline fields (`value`, `ms_per_step`, ...);
--dump-outputs DIR also writes the last timed step's maps and scores as DIR/<name>.npy
(same arguments -> same seeded inputs, so two builds compare output for output).
Everything else runs only with --full: the timed outputs checked against the eager path
and the CPU oracle (the parity gate and the exit status), the N-rank gather check, a
`roofline` object for the dominant kernel (bf16 GEMM, MFMA-bound), a
`roofline_map` object for the anomaly-map stream kernel (HBM-bound) and a
`cpu_baseline` measured with the torch-CPU oracle (oracle/aaclip_torch.py: the
reference's fp32 arithmetic on ATen's CPU kernels, calibrated against the
reference itself) on this host's cores.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "aa-clip_amd"))
sys.path.insert(0, ROOT)


def _self_launch():
    """`python bench.py --gpus N` with no torchrun environment: start the N ranks
    ourselves (torch.distributed.run as a CHILD process, one rank per GPU over
    RCCL) and exit with its code. Runs before torch is imported, so this parent
    never touches the GPU (no exec from a GPU-initialised process)."""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gpus", type=int, default=1)
    known, _ = ap.parse_known_args()
    if known.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={known.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    _self_launch()

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from aaclip import ops  # noqa: E402
from aaclip.engine import HEADS, LAYERS, WIDTH, VisualEngine  # noqa: E402
from aaclip.parallel import shard_range, sharded_step, verify_gather  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "pmc_traffic.json")


def pmc_traffic(key):
    """HBM bytes per launch measured by rocprofv3 PMC passes on the same kernels
    and shapes (profiles/pmc_traffic.json, written by tools/pmc_summary.py)."""
    try:
        with open(TRAFFIC_FILE) as f:
            t = json.load(f)
        return t[key]["bytes_per_launch"], t["source"]
    except (OSError, KeyError, ValueError):
        return None, None
HBM_PEAK_GBS = 8000.0      # HBM3E spec peak


def synthetic_visual_weights(dev, seed=111, n_levels=4, adapt_until=6, n_tok=577):
    """Random-init ViT-L/14 (+ adapters), generated on device (reference key names);
    n_tok = 577 at 336 px, 1025 at 448 px (config C5)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=g) * std  # noqa: E731
    W = WIDTH
    vp = {
        "visual.conv1.weight": r(W, 3, 14, 14, std=588 ** -0.5),
        "visual.class_embedding": r(W, std=W ** -0.5),
        "visual.positional_embedding": r(n_tok, W, std=W ** -0.5),
        "visual.ln_pre.weight": 1 + r(W, std=0.1), "visual.ln_pre.bias": r(W, std=0.05),
        "visual.ln_post.weight": 1 + r(W, std=0.1), "visual.ln_post.bias": r(W, std=0.05),
    }
    for i in range(LAYERS):
        p = f"visual.transformer.resblocks.{i}."
        vp.update({
            p + "ln_1.weight": 1 + r(W, std=0.1), p + "ln_1.bias": r(W, std=0.05),
            p + "ln_2.weight": 1 + r(W, std=0.1), p + "ln_2.bias": r(W, std=0.05),
            p + "attn.in_proj_weight": r(3 * W, W, std=W ** -0.5), p + "attn.in_proj_bias": r(3 * W, std=0.02),
            p + "attn.out_proj.weight": r(W, W, std=W ** -0.5), p + "attn.out_proj.bias": r(W, std=0.02),
            p + "mlp.c_fc.weight": r(4 * W, W, std=(2 * W) ** -0.5), p + "mlp.c_fc.bias": r(4 * W, std=0.02),
            p + "mlp.c_proj.weight": r(W, 4 * W, std=(4 * W) ** -0.5), p + "mlp.c_proj.bias": r(W, std=0.02),
        })
    ad = {f"layer_adapters.{i}.fc.0.weight": r(W, W, std=0.03) for i in range(adapt_until)}
    ad.update({f"seg_proj.{i}.fc.weight": r(768, W, std=0.03) for i in range(n_levels)})
    ad["det_proj.fc.weight"] = r(768, W, std=0.03)
    return vp, ad


def flops_per_image(n_tok=577, levels=4, adapt=6):
    """Algorithmic FLOPs: GEMMs 2MKN, attention 4 N^2 d per layer."""
    P = n_tok - 1
    W = WIDTH
    blocks = LAYERS * (2 * n_tok * W * 3 * W + 4 * n_tok * n_tok * W + 2 * n_tok * W * W + 2 * 2 * n_tok * W * 4 * W)
    return blocks + 2 * P * 588 * W + adapt * 2 * n_tok * W * W + levels * 2 * P * W * 768 + 2 * P * W * 768


def time_launches(fn, reps, stream=None):
    """GPU time per launch of fn (ms): `reps` launches captured into one hipGraph and
    replayed between HIP events on the replay stream, so host launch overhead (ctypes,
    argument checks) is not in the number; the dependent-kernel boundary (~1.5 us) is."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # warm-up outside the capture (kernel attributes, lazy allocations)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record(st)
    graph.replay()
    end.record(st)
    end.synchronize()
    return start.elapsed_time(end) / reps  # ms per launch


def latency_b1(eng, size, T, reps=30):
    """Config C1's shape on the GPU: one image (bs=1) through the whole path as one
    hipGraph replay, input already on device; HIP events on the replay stream."""
    run = eng.graphed_predict(1, size, "Industrial", streams=1)
    x = torch.randn(1, 3, size, size, device=T.device)
    st = torch.cuda.current_stream()
    run(x, T)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(st)
    for _ in range(reps):
        run(x, T)
    end.record(st)
    end.synchronize()
    ms = start.elapsed_time(end) / reps
    return {"batch": 1, "ms_per_image": round(ms, 3), "images_per_sec": round(1e3 / ms, 1)}


def step_bounds(eng, run, x, T, streams, steps=10, rounds=2):
    """Diagnostic (never `value`): what the GEMM epilogues cost in the timed step. The
    shipped captured step vs the same step captured with every GEMM epilogue skipped
    (aaclip_set_gemm_variant bit 9) or only its global stores skipped (bit 10), replayed on
    the graph's own workspaces after a normal replay filled them with this batch's
    activations (fresh zero buffers would let every later kernel multiply zeros and the chip
    clock up). The skipped arms compute garbage; interleaved rounds, min per arm.
    tools/epi_bound.py is the standalone form (profiles/r03/gemm_epilogue_bound.txt)."""
    from aaclip import _lib
    S = x.shape[-1]
    slot0 = run.slot0  # `run`'s private workspace slots (graphed_predict)
    graphs = {}
    try:
        for name, v in (("epilogue_skipped", 512), ("stores_skipped", 1024)):
            _lib.call("aaclip_set_gemm_variant", v)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                eng.predict(x, T, "Industrial", streams=streams, _slot0=slot0)
            graphs[name] = gr
    finally:
        _lib.call("aaclip_set_gemm_variant", 0)
    arms = {"shipped": lambda: run(x, T)}
    arms.update({k: g.replay for k, g in graphs.items()})
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = {}
    for _ in range(rounds):
        for name, fn in arms.items():
            run(x, T)  # real activations in the workspaces before every arm
            fn()
            e0.record(st)
            for _ in range(steps):
                fn()
            e1.record(st)
            e1.synchronize()
            best[name] = min(best.get(name, 1e9), e0.elapsed_time(e1) / steps)
    run(x, T)
    torch.cuda.synchronize()
    base = best["shipped"]
    return {"note": "diagnostic arms skip work (garbage outputs); never the timed value",
            "ms_per_step": {k: round(v, 3) for k, v in best.items()},
            "gemm_epilogue_ms": round(base - best["epilogue_skipped"], 3),
            "gemm_epilogue_share": round((base - best["epilogue_skipped"]) / base, 3),
            "gemm_store_ms": round(base - best["stores_skipped"], 3)}


def preprocess_leg(dev, batch, size, reps=20):
    """SURVEY 8(f)-3 on device: B decoded uint8 RGB images (1024x1024, MVTec's size)
    -> Pillow-exact BICUBIC resize + ToTensor + Normalize -> fp32 [B,3,S,S]
    (aaclip_preprocess_images, two-pass), and the NEAREST mask resize. HIP events
    on the launch stream; algorithmic bytes = B*H*W*3 read + B*3*S*S*4 written."""
    from aaclip.preprocess import Preprocessor
    H = W = 1024
    g = torch.Generator(device=dev).manual_seed(5)
    u8 = torch.randint(0, 256, (batch, H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    m8 = (torch.rand(batch, H, W, device=dev, generator=g) < 0.05).to(torch.uint8)
    pp = Preprocessor(size)
    out = torch.empty(batch, 3, size, size, device=dev)
    mo = torch.empty(batch, 1, size, size, device=dev)
    st = torch.cuda.current_stream()
    t_img = time_launches(lambda: pp.images(u8, out), reps, st)
    t_mask = time_launches(lambda: pp.masks(m8, mo), reps, st)
    alg = batch * H * W * 3 + batch * 3 * size * size * 4
    gbs = alg / (t_img * 1e-3) / 1e9
    return {"workload": f"{batch} x {H}x{W} uint8 RGB -> fp32 [{batch},3,{size},{size}] (Pillow BICUBIC exact)",
            "images_per_sec": round(batch / (t_img * 1e-3), 1), "us_per_batch": round(t_img * 1e3, 1),
            "mask_us_per_batch": round(t_mask * 1e3, 1),
            "roofline": {"kernel": "resample_h_kernel + resample_v_kernel", "bound": "hbm", "unit": "GB/s",
                         "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes_per_launch": alg, "traffic": None}}


def metrics_leg(dev, size, reps=5):
    """SURVEY 8(f)-1 on device: one class's metrics_eval (class min-max, pixel-max score
    fusion, exact tie-aware pixel/image AUROC + AP: rocPRIM radix sort of 33-bit keys,
    scans, fixed-order reductions), graph-timed, at a C4 batch (32 images) and at the
    largest MVTec test class (167 images). Synthetic maps (uniform scores) and masks
    (5 % anomalous pixels). Sort-bound, not a streaming kernel: the exact tie-aware
    metrics need the class's pixels in score order (one radix sort of 64-bit keys), so
    the figure is pixels ranked per second, with the per-class time beside the class's
    forward (32 images: ~14 ms)."""
    import ctypes
    from aaclip import _lib
    out = {}
    for n_img in (32, 167):
        pix = size * size
        g = torch.Generator(device=dev).manual_seed(9)
        preds = torch.rand(n_img, pix, device=dev, generator=g)
        lab = (torch.rand(n_img, pix, device=dev, generator=g) < 0.05).to(torch.uint8)
        ip = torch.rand(n_img, device=dev, generator=g)
        il = (torch.arange(n_img, device=dev) % 2).to(torch.uint8)
        need = ctypes.c_size_t(0)
        _lib.call("aaclip_metrics_workspace", n_img * pix, n_img, ctypes.byref(need))
        wsb = torch.empty(int(need.value) + 256, device=dev, dtype=torch.uint8)
        off = (-wsb.data_ptr()) % 256
        res = torch.empty(4, device=dev, dtype=torch.float64)

        def run():
            _lib.call("aaclip_metrics_eval", preds.data_ptr(), lab.data_ptr(), ip.data_ptr(), il.data_ptr(), n_img,
                      pix, 0, wsb.data_ptr() + off, need.value, res.data_ptr(),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        t = time_launches(run, reps, torch.cuda.current_stream())
        out[f"class_{n_img}_images"] = {"pixels": n_img * pix, "ms": round(t, 3),
                                        "mpixels_per_sec": round(n_img * pix / (t * 1e-3) / 1e6, 1)}
    out["bound"] = "sort (rocPRIM radix sort of 64-bit keys + scans), exact sklearn-equivalent AUROC/AP"
    return out


class StepProbe:
    """HIP timing events around every launch of the step (aaclip.ops.set_probe): an event
    recorded on the launch's stream right before and right after each kernel, so
    elapsed_time(begin, end) = that launch's GPU duration inside the running step (its
    neighbours, the clock the sustained step holds and, with two streams, the other
    chunk's concurrent kernels included). The step runs EAGERLY here (same kernels,
    same streams as the timed graph): ROCm's torch refuses event-record nodes inside a
    captured graph ("External events are disallowed in rocm")."""

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


# op categories of the block GEMMs (ops.gemm's probe kind: N, K and epilogue)
GEMM_OPS = {"gemm N3072 K1024": "qkv", "gemm N1024 K1024 resid": "out_proj", "gemm N4096 K1024 gelu": "c_fc",
            "gemm N1024 K4096 resid": "c_proj", "gemm N1024 K1024 leaky": "adapter",
            # fp8 MX block GEMMs (config C5's fp8 modes)
            "gemm8 N3072 K1024": "qkv", "gemm8 N1024 K1024 resid": "out_proj", "gemm8 N4096 K1024 gelu": "c_fc",
            "gemm8 N1024 K4096 resid": "c_proj"}


def in_step_profile(eng, x, T, streams, replays=8):
    """Run the C2 step (same engine, batch, domain and stream count as the timed graph)
    eagerly with a StepProbe `replays` times and average every launch's duration.
    Returns per-kernel-name and per-op totals per step, the probed step's time and the
    sum of launch durations."""
    for _ in range(2):
        eng.predict(x, T, "Industrial", streams=streams)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    acc, recs0, t_step = None, None, 0.0
    for _ in range(replays):
        probe = StepProbe()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.set_probe(probe)
        try:
            e0.record(st)
            eng.predict(x, T, "Industrial", streams=streams)
            e1.record(st)
        finally:
            ops.set_probe(None)
        e1.synchronize()
        torch.cuda.synchronize()
        t_step += e0.elapsed_time(e1)
        ms = [r[4].elapsed_time(r[5]) for r in probe.recs]
        if acc is None:
            acc, recs0 = ms, probe.recs
        else:
            acc = [u + v for u, v in zip(acc, ms)]
    by_name, by_op = {}, {}
    for (kind, name, flops, nbytes, _, _), ms in zip(recs0, acc):
        ms /= replays
        op = GEMM_OPS.get(kind, kind if not kind.startswith("gemm") else
                          "level_proj" if " scores" in kind or kind.startswith("gemm N768 K1024") or
                          kind.startswith("gemm N1536 K1024") else "other_gemm")
        for d, k in ((by_name, name), (by_op, op)):
            e = d.setdefault(k, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            e["launches"] += 1
            e["ms"] += ms
            e["flops"] += flops
            e["bytes"] += nbytes
    for d in (by_name, by_op):
        for e in d.values():
            e["avg_launch_us"] = round(e["ms"] / e["launches"] * 1e3, 2)
            if e["flops"]:
                e["tflops"] = round(e["flops"] / (e["ms"] * 1e-3) / 1e12, 1)
            else:
                e["GBs"] = round(e["bytes"] / (e["ms"] * 1e-3) / 1e9, 1)
            e["ms"] = round(e["ms"], 4)
    return {"streams": streams, "replays": replays, "launches_per_step": len(recs0),
            "method": "eager step, HIP events recorded on each launch's stream right before and after it",
            "step_ms_probed": round(t_step / replays, 3),
            "sum_of_launch_ms": round(sum(acc) / replays, 3), "by_kernel": by_name, "by_op": by_op}


def roofline_from_profiles(p1, p2, B, n_tok):
    """`roofline` (dominant kernel), its attention + MLP block and the anomaly map, from
    the in-step profiles: p1 = one-stream step (each launch alone on the chip: the
    per-launch durations a rocprofv3 kernel trace of the same step reproduces), p2 =
    the two-stream step that `value` times (per-launch durations there include the
    other chunk's concurrent kernels, so they overstate each kernel's own cost)."""
    gemms = {k: v for k, v in p1["by_kernel"].items() if v["flops"] and "attn" not in k}
    dom = max(gemms, key=lambda k: gemms[k]["ms"])
    e = gemms[dom]
    ach = e["flops"] / (e["ms"] * 1e-3) / 1e12
    traffic, src = pmc_traffic("gemm")
    ops_of = sorted(op for op, v in p1["by_op"].items() if op in GEMM_OPS.values())
    R = B * n_tok
    roof = {"kernel": dom, "bound": "mfma", "unit": "TFLOP/s", "achieved": round(ach, 1),
            "peak": BF16_PEAK_TFLOPS, "frac": round(ach / BF16_PEAK_TFLOPS, 4),
            "traffic": traffic, "traffic_source": src,
            "avg_launch_us": e["avg_launch_us"], "launches_per_step": e["launches"],
            "flops_per_launch": e["flops"] / e["launches"],
            "context": (f"in-step: the C2 step (B = {B}, M = {R} rows per GEMM) on ONE stream, HIP events "
                        "recorded right before and after every launch, durations averaged over the probed "
                        "steps; the dominant kernel = the GEMM kernel with the most step time"),
            "ops_on_this_kernel": [op for op in ops_of if _plan_name(op, R) == dom]}
    blk = [p1["by_op"][k] for k in ("qkv", "attention", "out_proj", "c_fc", "c_proj")]
    bf, bm = sum(v["flops"] for v in blk), sum(v["ms"] for v in blk)
    roof["attn_mlp_block"] = {"tflops": round(bf / (bm * 1e-3) / 1e12, 1),
                              "frac": round(bf / (bm * 1e-3) / 1e12 / BF16_PEAK_TFLOPS, 4),
                              "ms_per_step": {k: p1["by_op"][k]["ms"] for k in
                                              ("qkv", "attention", "out_proj", "c_fc", "c_proj")},
                              "attention_tflops": p1["by_op"]["attention"]["tflops"],
                              "attention_frac": round(p1["by_op"]["attention"]["tflops"] / BF16_PEAK_TFLOPS, 4),
                              "context": "in-step, one stream (same profile as the dominant kernel)"}
    if p2 is not None:
        e2 = p2["by_kernel"].get(dom)
        blk2 = [p2["by_op"][k] for k in ("qkv", "attention", "out_proj", "c_fc", "c_proj")]
        bf2, bm2 = sum(v["flops"] for v in blk2), sum(v["ms"] for v in blk2)
        roof["in_step_2stream"] = {
            "note": "the timed two-stream step: per-launch durations include the other chunk's concurrent "
                    "kernels (two launches sharing the CUs each take longer), so these understate each "
                    "kernel's own rate; the throughput of the overlap is in `value`",
            "dominant_kernel_avg_launch_us": e2["avg_launch_us"] if e2 else None,
            "dominant_kernel_tflops_per_launch": e2.get("tflops") if e2 else None,
            "attn_mlp_block_tflops": round(bf2 / (bm2 * 1e-3) / 1e12, 1),
            "attention_tflops": p2["by_op"]["attention"]["tflops"]}
    return roof


def _plan_name(op, R):
    from aaclip import _lib
    N, K = {"qkv": (3 * WIDTH, WIDTH), "out_proj": (WIDTH, WIDTH), "c_fc": (4 * WIDTH, WIDTH),
            "c_proj": (WIDTH, 4 * WIDTH), "adapter": (WIDTH, WIDTH)}[op]
    return ops.gemm_plan(_lib.BF16, R, N, K)


def map_from_profile(p1, p2, B=32, S=336, L=4):
    """The anomaly map in the step. In the partials form (the default predict) the map entry
    is aaclip_anomaly_map_partials (partial_scores_kernel + blur_upsample_score_kernel):
    `achieved` is its own bytes (the (L+1)*384-B partial rows read + the S*S*4 map written)
    per launch time; `frac_vs_survey_bytes` prices the same launch time against SURVEY
    §8(d)'s algorithmic map bytes (L*P*768*2 bf16 features + S*S*4 per image, the bytes a
    map kernel reading the projected rows would move) -- the north_star's >= 0.60 target
    is quoted on those. The norm / anchor-dot work moved into the level / det projection
    GEMM epilogues (aaclip_gemm_scores), so `projections_plus_map_us` is the end-to-end
    figure to compare against the row form."""
    m = p1["by_op"]["anomaly_map"]
    gbs = m["bytes"] / (m["ms"] * 1e-3) / 1e9
    traffic, src = pmc_traffic("map")
    kern = next((k for k in p1["by_kernel"] if k.startswith("anomaly_map")), "anomaly_map")
    partials = "partial" in kern
    entry = ("aaclip_anomaly_map_partials (partial_scores_kernel + blur_upsample_score_kernel)" if partials
             else "aaclip_anomaly_map (patch_scores_kernel + blur_upsample_kernel)")
    out = {"kernel": entry, "bound": "hbm",
           "unit": "GB/s", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 4),
           "traffic": traffic, "traffic_source": src, "avg_launch_us": m["avg_launch_us"],
           "bytes_per_launch": m["bytes"] / m["launches"],
           "context": "in-step, one stream: the B=32 map after the level projections, HIP events around the op"}
    g = S // 14
    survey_bytes = B * (L * g * g * 768 * 2 + S * S * 4)
    sgbs = survey_bytes / (m["ms"] / m["launches"] * 1e-3) / 1e9
    out["survey_bytes_per_launch"] = survey_bytes
    out["frac_vs_survey_bytes"] = round(sgbs / HBM_PEAK_GBS, 4)
    out["target_frac"] = 0.60
    sc = p1["by_op"].get("image_score")
    out["map_plus_score_us"] = round((m["ms"] + (sc["ms"] if sc else 0.0)) / m["launches"] * 1e3, 2)
    pr = p1["by_op"].get("level_proj")
    if pr is not None:
        out["level_projections_us"] = round(pr["ms"] / m["launches"] * 1e3, 2)
        out["projections_plus_map_us"] = round(out["map_plus_score_us"] + out["level_projections_us"], 2)
    out["form"] = ("partials: the level/det projection GEMMs emit per-(row, 32-column) {||v||^2, v.t0, v.t1} "
                   "(aaclip_gemm_scores), the map + image score read those (aaclip_anomaly_map_partials)"
                   if partials else "rows: the map and the image score stream the projected rows")
    if p2 is not None:
        m2 = p2["by_op"]["anomaly_map"]
        out["in_step_2stream"] = {"avg_launch_us": m2["avg_launch_us"], "GBs": m2["GBs"],
                                  "note": "per 16-image chunk, beside the other chunk's kernels"}
    return out


def roofline_gemm_isolated(eng, ws, reps=20):
    """Dominant kernel = the bf16 MFMA GEMM (QKV and c_fc launches; which tile family
    the per-shape dispatch picks is reported). Average HIP-event launch duration over
    the two shapes."""
    s = torch.cuda.current_stream()
    blk = eng.blocks[0]
    R = ws["x"].shape[0]
    t_qkv = time_launches(lambda: ops.gemm(ws["h"], blk["w_qkv"], ws["qkv"], bias=blk["b_qkv"]), reps, s)
    t_fc = time_launches(lambda: ops.gemm(ws["h"], blk["w_fc"], ws["fc"], bias=blk["b_fc"], gelu=True), reps, s)
    f_qkv = 2.0 * R * WIDTH * 3 * WIDTH
    f_fc = 2.0 * R * WIDTH * 4 * WIDTH
    t_avg = (t_qkv + t_fc) / 2
    achieved = (f_qkv + f_fc) / 2 / (t_avg * 1e-3) / 1e12
    # attention + MLP block GEMMs incl. the 256x128 launches (out-proj, c_proj)
    t_o = time_launches(lambda: ops.gemm(ws["attn"], blk["w_o"], ws["u"], bias=blk["b_o"]), reps, s)
    t_pr = time_launches(lambda: ops.gemm(ws["fc"], blk["w_pr"], ws["u"], bias=blk["b_pr"]), reps, s)
    t_at = time_launches(lambda: ops.attention(ws["qkv"], ws["attn"], R // ws["n_tok"], ws["n_tok"], HEADS), reps, s)
    n = ws["n_tok"]
    B = R // n
    f_at = 4.0 * B * n * n * WIDTH
    block_flops = f_qkv + f_fc + 2.0 * R * WIDTH * WIDTH + 2.0 * R * 4 * WIDTH * WIDTH + f_at
    block_ms = t_qkv + t_fc + t_o + t_pr + t_at
    traffic, src = pmc_traffic("gemm")
    from aaclip import _lib
    k_qkv = _lib.lib().aaclip_gemm_plan(_lib.BF16, R, 3 * WIDTH, WIDTH).decode()
    k_fc = _lib.lib().aaclip_gemm_plan(_lib.BF16, R, 4 * WIDTH, WIDTH).decode()
    return {
        "kernel": f"{k_qkv} (QKV) + {k_fc} (c_fc) at M = {R}",
        "bound": "mfma", "unit": "TFLOP/s", "achieved": round(achieved, 1), "peak": BF16_PEAK_TFLOPS,
        "frac": round(achieved / BF16_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_source": src,
        "algorithmic_bytes_per_launch": (R * WIDTH * 2 + 3 * WIDTH * WIDTH * 2 + R * 3 * WIDTH * 2
                                         + R * WIDTH * 2 + 4 * WIDTH * WIDTH * 2 + R * 4 * WIDTH * 2) / 2,
        "avg_launch_us": round(t_avg * 1e3, 2),
        "flops_per_launch": (f_qkv + f_fc) / 2,
        "attn_mlp_block": {"tflops": round(block_flops / (block_ms * 1e-3) / 1e12, 1),
                           "frac": round(block_flops / (block_ms * 1e-3) / 1e12 / BF16_PEAK_TFLOPS, 4),
                           "ms": {"qkv": round(t_qkv, 4), "attn": round(t_at, 4), "out": round(t_o, 4),
                                  "fc": round(t_fc, 4), "proj": round(t_pr, 4)},
                           "attention_tflops": round(f_at / (t_at * 1e-3) / 1e12, 1)},
    }


def roofline_map_isolated(eng, ws, T, reps=50):
    """The anomaly map as ONE operation (aaclip_anomaly_map = stage 1 patch_scores +
    stage 2 blur_upsample, HIP events around both launches): algorithmic bytes =
    L*P*768*4 (fp32 level features) + 768*2*4 (anchors) read + S*S*4 (map) written per
    image (the P*4-byte score grid between the stages is counted once
    each way). Stage times are reported beside it."""
    s = torch.cuda.current_stream()
    L = ws["segbuf"].shape[1] // 768 - 1
    seg = [ws["segbuf"][:, j * 768:(j + 1) * 768] for j in range(L)]
    rows = seg[0].shape[0]
    B = rows // ws["P"]
    S = ws["map"].shape[-1]
    g = ws["g"]
    t_all = time_launches(lambda: ops.anomaly_map(seg, T, ws["map"], ws["grid"], g=g, ksize=7, sigma=1.0), reps, s)
    t_ps = time_launches(lambda: ops.patch_scores(seg, T, ws["grid"][:rows]), reps, s)
    t_bu = time_launches(lambda: ops.blur_upsample(ws["grid"][:rows].view(B, 1, g, g), ws["map"].view(B, 1, S, S),
                                                   ksize=7, sigma=1.0), reps, s)
    read1 = len(seg) * rows * 768 * seg[0].element_size() + 768 * 2 * 4
    write2 = B * S * S * 4
    nbytes = read1 + write2 + 2 * rows * 4
    gbs = nbytes / (t_all * 1e-3) / 1e9
    traffic, src = pmc_traffic("map")
    return {"kernel": "aaclip_anomaly_map (patch_scores_kernel + blur_upsample_kernel)", "bound": "hbm",
            "unit": "GB/s", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 4),
            "traffic": traffic, "traffic_source": src, "avg_launch_us": round(t_all * 1e3, 2),
            "bytes_per_launch": nbytes,
            "stage1_patch_scores": {"us": round(t_ps * 1e3, 2), "bytes": read1 + rows * 4,
                                    "GBs": round((read1 + rows * 4) / (t_ps * 1e-3) / 1e9, 1)},
            "stage2_blur_upsample": {"us": round(t_bu * 1e3, 2), "bytes": write2 + rows * 4,
                                     "GBs": round((write2 + rows * 4) / (t_bu * 1e-3) / 1e9, 1)}}


def c5_leg(dev, steps: int, warmup: int, streams: int, batch: int = 32):
    """Config C5 (BASELINE.json configs[4]): 448 px (1025 tokens), 6 feature levels,
    MLP GEMMs on fp8 ("fp8": e4m3 weights + MX e4m3 activations, K=128 MFMA; QKV,
    attention, out-proj bf16), all four block GEMMs on fp8 ("fp8_all"), and bf16,
    batch of 32 on one GPU. Accuracy: anomaly maps against the fp32 parity mode of
    this path (itself pinned to the reference's C5 golden within 1e-5) on 2 images."""
    S, lv = 448, (4, 8, 12, 16, 20, 24)
    vp, ad = synthetic_visual_weights(dev, seed=448, n_levels=len(lv), n_tok=(S // 14) ** 2 + 1)
    g = torch.Generator(device=dev).manual_seed(448)
    x = torch.randn(batch, 3, S, S, device=dev, generator=g)
    T = torch.nn.functional.normalize(torch.randn(768, 2, device=dev, generator=g), dim=0).contiguous()
    out = {"workload": "C5: 448x448 (32x32 patch grid, 1025 tokens), 6 levels, batch 32, 1 GPU",
           "gflop_per_image": round(flops_per_image(1025, levels=6) / 1e9, 2)}
    maps = {}
    modes = (("fp8", dict(dtype=ops.FP8, fp8_scope="mlp")), ("fp8_all", dict(dtype=ops.FP8, fp8_scope="all")),
             ("bf16", dict(dtype=torch.bfloat16)))
    for tag, kw in modes:
        eng = VisualEngine(vp, ad, levels=lv, **kw)
        run = eng.graphed_predict(batch, S, "Medical", streams=streams)
        for _ in range(warmup):
            run(x, T)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            run(x, T)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        out[tag] = {"images_per_sec": round(batch * steps / dt_s, 2), "ms_per_step": round(dt_s / steps * 1e3, 3)}
        maps[tag] = eng.predict(x[:2], T, "Medical")[0].clone()
        if tag == "fp8_all":  # the fp8 MX GEMM roofline (QKV + c_fc shapes at this size)
            ws = eng._workspace(batch, S)
            blk, R = eng.blocks[0], ws["x"].shape[0]
            a8, asc = ws["a8"], ws["asc"]
            ops.quant_fp8_mx(ws["h"], a8, asc)
            st = torch.cuda.current_stream()
            t_q = time_launches(lambda: ops.gemm_fp8mx(a8, asc, *blk["w_qkv"], ws["qkv"], bias=blk["b_qkv"]), 10, st)
            t_f = time_launches(lambda: ops.gemm_fp8mx(a8, asc, *blk["w_fc"], ws["f8"], out_sc=ws["fsc"],
                                                       bias=blk["b_fc"], gelu=True), 10, st)
            t_qa = time_launches(lambda: ops.quant_fp8_mx(ws["h"], a8, asc), 10, st)
            fl = 2.0 * R * WIDTH * 7 * WIDTH / 2
            ach = fl / ((t_q + t_f) / 2 * 1e-3) / 1e12
            out["fp8_gemm_roofline"] = {"kernel": "gemm_fp8mx_8ph_kernel (QKV + c_fc launches)",
                                        "bound": "mfma", "unit": "TFLOP/s", "achieved": round(ach, 1),
                                        "peak": 2 * BF16_PEAK_TFLOPS, "frac": round(ach / (2 * BF16_PEAK_TFLOPS), 4),
                                        "avg_launch_us": round((t_q + t_f) / 2 * 1e3, 2),
                                        "quant_mx_us": round(t_qa * 1e3, 2)}
        del eng, run
        torch.cuda.empty_cache()
    eng = VisualEngine(vp, ad, levels=lv, dtype=torch.float32)
    ref = eng.predict(x[:2], T, "Medical")[0]
    for tag, _ in modes:
        d = maps[tag] - ref
        out[tag]["map_rel_l2_vs_fp32"] = float(d.norm() / ref.norm())
        out[tag]["map_max_abs_err_vs_fp32"] = float(d.abs().max())
        out[tag]["frac_pixels_within_fp32_contract"] = float((d.abs() <= 1e-3 + 1e-2 * ref.abs()).float().mean())
    return out


def _host_cores():
    """(nproc, physical cores from lscpu) of this host, for the record."""
    import subprocess
    nproc = os.cpu_count() or 1
    phys = None
    try:
        out = subprocess.run(["lscpu", "-p=CORE,SOCKET"], capture_output=True, text=True, timeout=10).stdout
        phys = len({ln for ln in out.splitlines() if ln and not ln.startswith("#")}) or None
    except (OSError, subprocess.SubprocessError):
        pass
    return nproc, phys


CALIBRATION_FILE = os.path.join(ROOT, "profiles", "r03", "cpu_calibration.json")


def _calibration():
    """The torch-CPU port's images/sec over the REFERENCE's own, both timed in the build
    container (tools/cpu_calibrate.py; the reference cannot run on the GPU box)."""
    try:
        with open(CALIBRATION_FILE) as f:
            c = json.load(f)
        legs = {k: v["ratio_torch_port_over_reference"] for k, v in c["legs"].items()}
        return {"ratio_port_over_reference": legs, "host": c["host"], "workload": c["workload"],
                "map_max_abs_diff_port_vs_reference": c["map_max_abs_diff_vs_reference"]["torch_port"],
                "source": "tools/cpu_calibrate.py -> profiles/r03/cpu_calibration.json (build container)"}
    except (OSError, KeyError, ValueError):
        return None


def _cpu_refs(RT, w, x, T, idx, threads):
    """Torch-CPU oracle outputs for images idx (bs = 1): per-level anchor grids
    100 f.T [L, P, 2], Industrial map [S, S], image score."""
    out = {}
    torch.set_num_threads(threads)
    with torch.no_grad():
        for i in idx:
            seg, det = RT.visual_forward(w, x[i:i + 1])
            out[i] = (torch.stack([100.0 * (f[0] @ T) for f in seg]).numpy(),
                      RT.anomaly_map(seg, T, x.shape[-1], "Industrial")[0].numpy(),
                      float(RT.image_score(det, T)[0]))
    return out


def cpu_baseline_and_parity(dev, streams: int, min_seconds: float = 12.0, warmup: int = 2, parity_images: int = 8):
    """CPU leg on rank 0. Timed: the torch-CPU oracle (oracle/aaclip_torch.py:
    the reference's fp32 arithmetic on the same ATen CPU kernels, pinned to the reference's
    golden vectors) over the per-batch path -- forward + 4-level map + image score, bs = 1 --
    on this host's cores: 2 warm-up images, then >= min_seconds of steady state, at 4
    threads (the reference's own setting, test.py:28-35) and at every thread this job may
    use (`value`). `calibration` = that port's rate over the reference's own, measured side
    by side in the build container. The first `parity_images` images' outputs are also the
    parity reference for the GPU modes, at 336 px and at the reference's default 518 px."""
    import numpy as np

    from oracle import aaclip_torch as RT
    from oracle import synth
    threads0 = torch.get_num_threads()
    sd = synth.clip_state_dict(111)
    ia, _ = synth.adapter_state_dicts(111)
    T = np.linalg.qr(np.random.default_rng(0).standard_normal((768, 2)))[0].astype(np.float32)
    Tt = torch.from_numpy(T)
    pool = 64
    x = torch.from_numpy(synth.images(111, pool, 336))
    w = RT.prepare(sd, ia)
    nproc, phys = _host_cores()
    allowed = int(os.environ.get("OMP_NUM_THREADS", nproc))
    refs = {336: {}}

    @torch.no_grad()
    def one(i):
        seg, det = RT.visual_forward(w, x[i:i + 1])
        m, sc = RT.anomaly_map(seg, Tt, 336, "Industrial"), RT.image_score(det, Tt)
        if i < parity_images and i not in refs[336]:
            refs[336][i] = (torch.stack([100.0 * (f[0] @ Tt) for f in seg]).numpy(), m[0].numpy(), float(sc[0]))

    legs = {}
    for threads in sorted({4, allowed}):
        torch.set_num_threads(threads)
        for i in range(warmup):
            one(i)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < min_seconds:
            one((warmup + n) % pool)
            n += 1
        dt = time.perf_counter() - t0
        legs[threads] = {"value": round(n / dt, 4), "images": n, "seconds": round(dt, 2)}
    main_t = allowed if allowed in legs else max(legs)
    cal = _calibration()
    base = {"value": legs[main_t]["value"], "unit": "images/sec", "cores": main_t, "kind": "port",
            "threads_4": legs.get(4), f"threads_{main_t}": legs[main_t],
            "host": {"nproc": nproc, "physical_cores_lscpu": phys, "threads_allowed": allowed},
            "calibration": cal,
            "sample": (f"fp32 torch-CPU oracle of the reference (oracle/aaclip_torch.py: the reference's "
                       f"arithmetic on the same ATen CPU kernels), bs=1 synthetic 336px images through forward "
                       f"+ 4-level map + image score; {warmup} warm-up images then >= {min_seconds:.0f} s steady "
                       f"state per leg; legs at 4 threads (reference test.py:28-35) and {main_t} threads (the "
                       f"cores this job may use; 'value')")}
    if cal:
        r8 = cal["ratio_port_over_reference"].get("threads_8")
        if r8:
            base["reference_equivalent_value"] = round(base["value"] / r8, 4)
    missing = [i for i in range(parity_images) if i not in refs[336]]
    refs[336].update(_cpu_refs(RT, w, x, Tt, missing, main_t))
    # the reference's default test size (test.py:111): 518 px, 1370 tokens
    sd518 = synth.clip_state_dict(111, img_size=518)
    w518 = RT.prepare(sd518, ia)
    x518 = torch.from_numpy(synth.images(111, parity_images, 518))
    t0 = time.perf_counter()
    refs[518] = _cpu_refs(RT, w518, x518, Tt, range(parity_images), main_t)
    base["parity_518_cpu_seconds"] = round(time.perf_counter() - t0, 1)
    torch.set_num_threads(threads0)
    parity = {"images_per_size": parity_images, "sizes": [336, 518],
              "tolerance": "maps |gpu - ref| <= 1e-3 + 1e-2*|ref| (north_star); patch labels = argmax over the 2 "
                           "anchors of 100 f.T per (image, level, patch); 'sure' = reference margin > 1e-3 on that "
                           "x100 scale (closer margins are ties at fp32 resolution)",
              "reference": "CPU fp32 torch oracle (pinned to the reference's golden vectors), same synthetic "
                           "weights/images/masks"}
    for S, sdS, xS in ((336, sd, x[:parity_images]), (518, sd518, x518)):
        parity[str(S)] = _parity_size(dev, streams, S, sdS, ia, xS, T, refs[S], synth)
    return base, parity


def parity_stats(grid, maps, scores, ref_grid, ref_maps, ref_scores, lab, auc_cpu=None):
    """One compute mode's outputs against the CPU oracle's on the same images (pure numpy):
    grid [n, L, P, 2] = 100 f.T per (image, level, patch), maps [n, S, S], scores [n];
    lab = the pixel labels for the AUROC. The fields the parity gate reads."""
    import numpy as np
    from sklearn.metrics import roc_auc_score
    if auc_cpu is None:
        auc_cpu = float(roc_auc_score(lab, ref_maps.reshape(-1)))
    tol = 1e-3 + 1e-2 * np.abs(ref_maps)
    margin = np.abs(ref_grid[..., 1] - ref_grid[..., 0])
    sure = margin > 1e-3
    err = np.abs(maps - ref_maps)
    flips = grid.argmax(-1) != ref_grid.argmax(-1)
    finite = bool(np.isfinite(maps).all() and np.isfinite(scores).all() and np.isfinite(grid).all())
    auc_gpu = float(roc_auc_score(lab, maps.reshape(-1))) if finite else float("nan")
    # per level (grid axis 1): a kernel change that doubles one level's flips shows here
    per_level = [int(flips[:, lv][sure[:, lv]].sum()) for lv in range(flips.shape[1])]
    return {"patch_label_flips_sure": int(flips[sure].sum()), "patch_label_flips_all": int(flips.sum()),
            "patch_label_flips_sure_per_level": per_level,
            "patch_label_flip_rate_sure": round(float(flips[sure].mean()), 6) if sure.any() else 0.0,
            "anchor_logit_max_abs_err": float(np.abs(grid - ref_grid).max()),
            "pixel_auroc_gpu": round(auc_gpu, 6), "pixel_auroc_abs_diff": abs(auc_gpu - auc_cpu) if finite else 1.0,
            "map_max_abs_err": float(err.max()) if finite else float("inf"),
            "map_within_tol": bool((err <= tol).all()),
            "frac_pixels_within_tol": float((err <= tol).mean()),
            "image_score_max_abs_err": float(np.abs(scores - ref_scores).max()) if finite else float("inf"),
            "image_labels_equal": bool(np.array_equal(scores > 0.5, ref_scores > 0.5)), "finite": finite}


def _parity_size(dev, streams, S, sd, ia, x, T, refs, synth):
    import numpy as np
    from sklearn.metrics import roc_auc_score
    n = x.shape[0]
    ref_grid = np.stack([refs[i][0] for i in range(n)])        # [n, L, P, 2]
    ref_maps = np.stack([refs[i][1] for i in range(n)])
    ref_scores = np.array([refs[i][2] for i in range(n)], dtype=np.float32)
    masks = synth.masks(111, n, S)[:, 0]
    lab = masks.reshape(-1) > 0
    auc_cpu = float(roc_auc_score(lab, ref_maps.reshape(-1)))
    margin = np.abs(ref_grid[..., 1] - ref_grid[..., 0])
    out = {"pixel_auroc_cpu_ref": round(auc_cpu, 6), "patch_labels": int(margin.size),
           "patch_labels_sure": int((margin > 1e-3).sum())}
    vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
    iad = {k: torch.from_numpy(v).to(dev) for k, v in ia.items()}
    xs, Td = x.to(dev), torch.from_numpy(T).to(dev)
    for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16), ("fp32", torch.float32)):
        eng = VisualEngine(vp, iad, dtype=dt)
        seg, _ = eng.forward(xs)
        grid = torch.stack([100.0 * (f @ Td) for f in seg], 1).cpu().numpy()
        m, sc = eng.predict(xs, Td, "Industrial", streams=streams)
        out[tag] = parity_stats(grid, m.cpu().numpy(), sc.cpu().numpy(), ref_grid, ref_maps, ref_scores, lab,
                                auc_cpu)
        del eng, seg, m, sc
        torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------- parity gate
# The bounds every bench line is held to (exit status 1 and "parity_gate": false otherwise):
# the tests' bounds (tests/test_e2e_gpu.py, test_fp16_gpu.py) applied to the bench's own
# parity leg against the CPU oracle. bf16 sure patch-label flips: the counts this tree
# measures on the parity leg's 8 images (per size; per level), held to 2x in total and
# 2x + 2 per level; fp16 / fp32: the north_star contract in full (every pixel within
# 1e-3 + 1e-2 |ref|, 0 sure flips). Reference: test.py:80-93.
BF16_PARITY_FLIPS = {"336": (33, (4, 0, 29, 0)), "518": (87, (12, 0, 71, 4))}
BF16_MIN_FRAC_WITHIN_TOL = 0.999
MAX_PIXEL_AUROC_DIFF = 2e-3
# the timed step's own outputs (images of the timed batch, the bench's own weights) vs the
# oracle, checked on every line (every N, rank 0's shard). These are corruption bounds, not
# the contract: bf16 maps against fp32 measure rel-L2 0.002-0.012 and 32-100 % of pixels in
# the fp32 envelope depending on the anchor draw (the contract is the parity leg's, on the
# fixed parity data); a wrong or racing kernel moves rel-L2 by orders of magnitude
TIMED_MAX_MAP_REL_L2 = 5e-2
TIMED_MAX_SCORE_ABS_ERR = 2e-3
# C5 (448 px, 6 levels) against the fp32 parity mode of the same path
C5_BF16_MIN_FRAC_WITHIN_TOL = 0.999
C5_FP8_MAX_MAP_REL_L2 = 1.5e-2


def parity_gate(line: dict) -> dict:
    """Check a bench line's parity legs against the bounds above. Returns {"pass": bool,
    "checked": [leg names], "failed": [reasons]}; a line with no parity leg at all fails
    (every line carries at least timed_step_vs_oracle)."""
    failed, checked = [], []
    tv = line.get("timed_step_vs_oracle")
    if tv is not None:
        checked.append("timed_step_vs_oracle")
        if not tv.get("finite", False):
            failed.append("timed step: non-finite outputs")
        if not tv["map_rel_l2"] <= TIMED_MAX_MAP_REL_L2:
            failed.append(f"timed step: map rel-L2 {tv['map_rel_l2']:.3e} > {TIMED_MAX_MAP_REL_L2}")
        if not tv["image_score_max_abs_err"] <= TIMED_MAX_SCORE_ABS_ERR:
            failed.append(f"timed step: image score err {tv['image_score_max_abs_err']:.3e} > "
                          f"{TIMED_MAX_SCORE_ABS_ERR}")
        if not tv["image_labels_equal"]:
            failed.append("timed step: image labels differ")
    par = line.get("parity")
    if par is not None:
        for size in par["sizes"]:
            leg = par[str(size)]
            for tag in ("bf16", "fp16", "fp32"):
                r = leg[tag]
                where = f"parity {size}px {tag}"
                checked.append(where)
                if not r.get("finite", True):
                    failed.append(f"{where}: non-finite outputs")
                if not r["image_labels_equal"]:
                    failed.append(f"{where}: image labels differ")
                if not r["pixel_auroc_abs_diff"] <= MAX_PIXEL_AUROC_DIFF:
                    failed.append(f"{where}: pixel AUROC differs by {r['pixel_auroc_abs_diff']:.2e}")
                if tag == "bf16":
                    tot, lv = BF16_PARITY_FLIPS[str(size)]
                    if r["patch_label_flips_sure"] > 2 * tot:
                        failed.append(f"{where}: {r['patch_label_flips_sure']} sure flips > 2 x {tot}")
                    got = r["patch_label_flips_sure_per_level"]
                    if len(got) != len(lv) or any(f > 2 * m + 2 for f, m in zip(got, lv)):
                        failed.append(f"{where}: sure flips per level {got} exceed 2 x {list(lv)} + 2")
                    if r["frac_pixels_within_tol"] < BF16_MIN_FRAC_WITHIN_TOL:
                        failed.append(f"{where}: {r['frac_pixels_within_tol']:.6f} of pixels within tol "
                                      f"< {BF16_MIN_FRAC_WITHIN_TOL}")
                else:  # fp16 / fp32: the full north_star contract
                    if not r["map_within_tol"]:
                        failed.append(f"{where}: map outside 1e-3 + 1e-2 |ref| (max {r['map_max_abs_err']:.3e})")
                    if r["patch_label_flips_sure"] != 0:
                        failed.append(f"{where}: {r['patch_label_flips_sure']} sure patch-label flips")
    c5 = line.get("c5")
    if c5 is not None:
        checked.append("c5")
        if c5["bf16"]["frac_pixels_within_fp32_contract"] < C5_BF16_MIN_FRAC_WITHIN_TOL:
            failed.append(f"c5 bf16: {c5['bf16']['frac_pixels_within_fp32_contract']:.6f} of pixels within the "
                          "fp32 contract")
        if not c5["fp8"]["map_rel_l2_vs_fp32"] <= C5_FP8_MAX_MAP_REL_L2:
            failed.append(f"c5 fp8: map rel-L2 {c5['fp8']['map_rel_l2_vs_fp32']:.3e} > {C5_FP8_MAX_MAP_REL_L2}")
    if not checked:
        failed.append("no parity leg in the line")
    return {"pass": not failed, "checked": checked, "failed": failed}


def timed_step_vs_oracle(vp, ad, x, maps, scores, T, idx=(0, -1), threads=None):
    """The TIMED step's own outputs (the graph replay's maps / scores for images idx of this
    rank's shard) against the CPU oracle (oracle/aaclip_torch.py, fp32) on the bench's own
    synthetic weights and images: the line proves what it timed, not an eager re-run of the
    same library. Runs after timing, on rank 0."""
    import numpy as np

    from oracle import aaclip_torch as RT
    n = x.shape[0]
    idx = sorted({i % n for i in idx})
    cpu = lambda d: {k: v.detach().float().cpu() for k, v in d.items()}  # noqa: E731
    w = RT.prepare(cpu(vp), cpu(ad))
    Tc = T.detach().float().cpu()
    t0 = time.perf_counter()
    threads0 = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    ref_m, ref_s = [], []
    with torch.no_grad():
        for i in idx:
            seg, det = RT.visual_forward(w, x[i:i + 1].float().cpu())
            ref_m.append(RT.anomaly_map(seg, Tc, x.shape[-1], "Industrial")[0].numpy())
            ref_s.append(float(RT.image_score(det, Tc)[0]))
    torch.set_num_threads(threads0)
    ref_m, ref_s = np.stack(ref_m), np.array(ref_s, dtype=np.float32)
    got_m = maps[idx].float().cpu().numpy()
    got_s = scores[idx].float().cpu().numpy()
    finite = bool(np.isfinite(got_m).all() and np.isfinite(got_s).all())
    err = np.abs(got_m - ref_m)
    tol = 1e-3 + 1e-2 * np.abs(ref_m)
    return {"images": [int(i) for i in idx], "reference": "CPU fp32 torch oracle, the bench's own weights and images",
            "finite": finite, "map_max_abs_err": float(err.max()) if finite else float("inf"),
            "map_rel_l2": float(np.linalg.norm(got_m - ref_m) / np.linalg.norm(ref_m)) if finite else float("inf"),
            "frac_pixels_within_tol": float((err <= tol).mean()),
            "image_score_max_abs_err": float(np.abs(got_s - ref_s).max()) if finite else float("inf"),
            "image_labels_equal": bool(np.array_equal(got_s > 0.5, ref_s > 0.5)),
            "cpu_seconds": round(time.perf_counter() - t0, 1)}


def emit(line: dict, rank: int = 0) -> int:
    """Gate the line on its parity legs, print it (rank 0) and return the exit status:
    0 when every bound holds, 1 otherwise ("parity_gate": false and the reasons in
    "parity_gate_failed")."""
    g = parity_gate(line)
    line["parity_gate"] = g["pass"]
    line["parity_gate_checked"] = g["checked"]
    if g["failed"]:
        line["parity_gate_failed"] = g["failed"]
    if rank == 0:
        print(json.dumps(line), flush=True)
        if g["failed"]:
            print("bench.py: PARITY GATE FAILED: " + "; ".join(g["failed"]), file=sys.stderr, flush=True)
    return 0 if g["pass"] else 1


def modes_leg(vp, ad, x, T, steps: int, warmup: int, streams: int):
    """The C2 step (same weights, images, graph) in the other compute modes:
    fp16 (fp16 MFMA, same rate as bf16, 8x finer operand rounding: the mode that
    meets the north_star map contract) and fp32 (fp32 MFMA parity mode)."""
    out = {}
    B, S = x.shape[0], x.shape[-1]
    for tag, dt, k in (("fp16", torch.float16, steps), ("fp32", torch.float32, max(2, steps // 5))):
        eng = VisualEngine(vp, ad, dtype=dt)
        run = eng.graphed_predict(B, S, "Industrial", streams=streams)
        for _ in range(warmup):
            run(x, T)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            run(x, T)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        out[tag] = {"images_per_sec": round(B * k / dt_s, 2), "ms_per_step": round(dt_s / k * 1e3, 3), "steps": k,
                    "tflops_whole_path": round(flops_per_image((S // 14) ** 2 + 1) * B * k / dt_s / 1e12, 1)}
        del eng, run
        torch.cuda.empty_cache()
    return out


DUMP_MAX_BYTES = 64 * 1000 * 1000  # --dump-outputs: everything written stays under this


def dump_outputs(path: str, maps, scores, scores_all=None) -> dict:
    """--dump-outputs: what the timed path returned in its last timed step, as float32
    .npy files under `path`: maps.npy [b, S, S] and scores.npy [b] (this rank's shard), and
    for N > 1 scores_gathered.npy [n_total] (the all-gathered image scores). A map tensor
    over the byte budget is written as a fixed sample instead: the flat elements at
    numpy.random.default_rng(0).choice(maps.size, k, replace=False), sorted, as a 1-D array
    (the same elements for the same shape in every run). Returns {name: shape} as written."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    out = {"scores": scores.detach().float().cpu().numpy()}
    if scores_all is not None:
        out["scores_gathered"] = scores_all.detach().float().cpu().numpy()
    m = maps.detach().float().cpu().numpy()
    budget = DUMP_MAX_BYTES - sum(v.nbytes for v in out.values()) - 1024 * (len(out) + 1)  # .npy headers
    if m.nbytes > budget:
        keep = np.sort(np.random.default_rng(0).choice(m.size, budget // 4, replace=False))
        m = m.reshape(-1)[keep]
    out["maps"] = m
    for name, arr in out.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float32))
    return {name: list(arr.shape) for name, arr in out.items()}


def _streams_arg(v: str):
    """--streams N (equal chunks) or an explicit chunk-size list 'a,b,...' (summing to --batch)."""
    return tuple(int(t) for t in v.split(",")) if "," in v else int(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU per step")
    ap.add_argument("--img-size", type=int, default=336)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg (output checks against the eager path and "
                         "the CPU oracle + parity gate, N-rank gather check, rooflines, compute modes, CPU baseline "
                         "and parity, preprocessing, metrics, C5); the --no-* / --cpu-seconds / --isolated switches "
                         "below pick among those legs and mean nothing without --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0: maps, scores; N > 1 also the gathered scores) "
                         "as float32 DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0,
                    help="steady-state seconds per CPU-baseline leg (0 = skip the CPU leg and parity)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--isolated", action="store_true",
                    help="also time the dominant GEMMs / attention / map as isolated graph-replayed launches")
    ap.add_argument("--streams", type=_streams_arg, default=2,
                    help="concurrent image chunks per GPU (HIP streams); 'a,b,...' = explicit chunk sizes")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-c5", action="store_true", help="skip the config-C5 leg (448 px, 6 levels, fp8)")
    ap.add_argument("--no-modes", action="store_true", help="skip the fp16 / fp32 mode throughput leg")
    ap.add_argument("--gemm-variant", type=int, default=0, help="aaclip_set_gemm_variant value (A/B runs)")
    ap.add_argument("--attn-variant", type=int, default=0, help="aaclip_set_attn_variant value (A/B runs)")
    ap.add_argument("--no-oracle-check", action="store_true",
                    help="skip the timed step's check against the CPU oracle AND the parity gate (A/B timing runs "
                         "only; such a line carries no parity_gate)")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16",
                    help="compute dtype of the timed step (C2 is quoted in bf16; fp16 = the contract mode, for A/B)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    n_streams = args.streams if isinstance(args.streams, int) else len(args.streams)  # for the other legs
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch one rank per GPU "
                 "(plain `python bench.py --gpus N` starts them itself)")
    # AACLIP_BENCH_REHEARSAL=1: every rank on cuda:0 over gloo -- exercises the N-rank launch,
    # sharding, all-gather and max-over-ranks timing on a one-GPU box (not a scaling number)
    rehearsal = os.environ.get("AACLIP_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local = 0
    if world > 1:
        torch.cuda.set_device(local)
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    if args.gemm_variant or args.attn_variant:
        from aaclip import _lib
        _lib.call("aaclip_set_gemm_variant", args.gemm_variant)
        _lib.call("aaclip_set_attn_variant", args.attn_variant)
    vp, ad = synthetic_visual_weights(dev, n_tok=(args.img_size // 14) ** 2 + 1)
    eng = VisualEngine(vp, ad, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float16)
    B, S = args.batch, args.img_size
    # one global batch of B * world images (the same seeded tensor on every rank);
    # each rank owns its shard_range slice (C3: 256 = 8 x 32), weights replicated
    n_total = B * world
    g = torch.Generator(device=dev).manual_seed(111)
    x_global = torch.randn(n_total, 3, S, S, device=dev, generator=g)
    # the anchors from a generator of their own: the same T at every world size
    gt = torch.Generator(device=dev).manual_seed(112)
    T = torch.nn.functional.normalize(torch.randn(768, 2, device=dev, generator=gt), dim=0).contiguous()
    a, b = shard_range(n_total, rank, world)
    x = x_global[a:b].contiguous()
    del x_global

    def images_of(i0, i1):
        """Images [i0, i1) of the seeded global batch (regenerated: the same tensor on every rank)."""
        gg = torch.Generator(device=dev).manual_seed(111)
        return torch.randn(n_total, 3, S, S, device=dev, generator=gg)[i0:i1].contiguous()

    run = None if args.no_graph else eng.graphed_predict(B, S, "Industrial", streams=args.streams)

    def predict(xl, Tl):
        if run is not None:
            return run(xl, Tl)
        return eng.predict(xl, Tl, "Industrial", streams=args.streams)

    def step():
        return sharded_step(predict, x, T, n_total)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_rank = None
    if world > 1:
        # every rank's own elapsed time (load balance of the shards), then the MAX the line reports
        t_all = torch.empty(world, device=dev, dtype=torch.float64)
        dist.all_gather_into_tensor(t_all, torch.tensor([elapsed], device=dev, dtype=torch.float64))
        per_rank = [round(v / args.steps * 1e3, 3) for v in t_all.tolist()]
        elapsed = max(t_all.tolist())
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, last[0], last[1], last[2] if world > 1 else None)
    dist_check = None
    if world > 1 and args.full:
        # the N-rank line proves its own result: own slices + a foreign shard recomputed
        # on rank 0 (eager, one stream: a different launch path from the timed graph)
        dist_check = verify_gather(lambda xi: eng.predict(xi, T, "Industrial", streams=1)[1].clone(), images_of,
                                   last[2], last[1], n_total)
        dist_check["ms_per_step_per_rank"] = per_rank

    images = n_total * args.steps
    ms_per_step = elapsed / args.steps * 1e3
    line = {
        "metric": "images/sec (336x336, ViT-L/14) + pixel-AUROC parity vs CPU ref",
        "value": round(images / elapsed, 2),
        "unit": "images/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic (N(0,1) images on device, random-init ViT-L/14-336 + adapters)"
                + (" [REHEARSAL: all ranks on cuda:0 over gloo]" if rehearsal else ""),
        "config": {"workload": f"C2: AA-CLIP anomaly-map inference, ViT-L/14-336, {args.dtype}, 4 levels, 2 anchors, "
                               "Industrial blur, per-GPU batch of images",
                   "global_batch": n_total, "img_size": S, "per_gpu_batch": B,
                   "parallelism": f"image-sharded dp{world} (shard_range slices of one global batch "
                                  "+ RCCL all-gather of image scores)",
                   "streams_per_gpu": args.streams, "hipgraph": not args.no_graph,
                   "gflop_per_image": round(flops_per_image((S // 14) ** 2 + 1) / 1e9, 2)},
    }
    line["tflops_whole_path"] = round(flops_per_image((S // 14) ** 2 + 1) * images / elapsed / 1e12, 1)
    if dumped is not None:
        line["dumped_outputs"] = {"dir": args.dump_outputs, "float32": dumped}
    if not args.full:
        # the plain run ends here: set-up, warm-up, the timed steps, the dump, the line
        if rank == 0:
            print(json.dumps(line), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    ws = eng._workspace(B, S)
    if dist_check is not None:
        line["distributed"] = dist_check
    # the timed step's own outputs, checked after the fact: finite, and bit-identical to an
    # eager one-stream predict of the same images (per-image bits do not depend on chunking)
    m_t, s_t = last[0].clone(), last[1].clone()
    m_e, s_e = eng.predict(x, T, "Industrial", streams=1)
    line["step_outputs_verified"] = {
        "finite": bool(torch.isfinite(m_t).all() and torch.isfinite(s_t).all()),
        "equal_to_one_stream_eager": bool(torch.equal(m_t, m_e) and torch.equal(s_t, s_e))}
    if rank == 0 and not args.no_oracle_check:
        # ... and against the CPU oracle: first and last image of rank 0's shard, the timed
        # replay's own maps / scores (parity_gate holds them to the TIMED_* bounds)
        line["timed_step_vs_oracle"] = timed_step_vs_oracle(vp, ad, x, m_t, s_t, T)
    del m_t, s_t
    if rank == 0 and not args.no_roofline:
        # in-step per-launch durations: the one-stream step (the roofline; a rocprofv3 kernel
        # trace of the same step reproduces it) and the timed two-stream step
        n_tok = (S // 14) ** 2 + 1
        try:
            p1 = in_step_profile(eng, x, T, 1)
            p2 = in_step_profile(eng, x, T, args.streams) if args.streams != 1 else None
            line["roofline"] = roofline_from_profiles(p1, p2, B, n_tok)
            line["roofline_map"] = map_from_profile(p1, p2, B, S, len(eng.levels))
            line["step_profile"] = {"one_stream": p1, "timed_streams": p2}
        except RuntimeError as exc:  # event-record nodes unsupported: fall back to isolated launches
            line["in_step_error"] = str(exc)[:300]
            line["roofline"] = roofline_gemm_isolated(eng, ws)
            line["roofline_map"] = roofline_map_isolated(eng, ws, T)
        if args.isolated:
            line["isolated"] = {"gemm": roofline_gemm_isolated(eng, ws), "map": roofline_map_isolated(eng, ws, T)}
        line["latency_b1"] = latency_b1(eng, S, T)
        if world == 1 and run is not None:
            line["step_bounds"] = step_bounds(eng, run, x, T, args.streams)
    if rank == 0 and world == 1 and not args.no_modes:
        del run
        run = None
        line["modes"] = modes_leg(vp, ad, x, T, args.steps, args.warmup, args.streams)
    if rank == 0 and world == 1 and args.cpu_seconds > 0:
        line["cpu_baseline"], line["parity"] = cpu_baseline_and_parity(dev, n_streams, args.cpu_seconds)
        if "modes" in line:
            p = line["parity"]
            line["contract_mode"] = {
                "dtype": "fp16", "images_per_sec": line["modes"]["fp16"]["images_per_sec"],
                "why": "the north_star map contract (1e-3 abs + 1e-2 rel fp32, argmax labels exact) on the 16-bit "
                       "MFMA path: fp16 operands carry 11 significant bits (bf16: 8) at the same MFMA rate",
                "patch_label_flips_sure": {str(sz): p[str(sz)]["fp16"]["patch_label_flips_sure"] for sz in p["sizes"]},
                "all_pixels_within_tol": all(p[str(sz)]["fp16"]["map_within_tol"] for sz in p["sizes"]),
                "image_labels_equal": all(p[str(sz)]["fp16"]["image_labels_equal"] for sz in p["sizes"]),
                "headline_bf16_patch_label_flips_sure": {str(sz): p[str(sz)]["bf16"]["patch_label_flips_sure"]
                                                         for sz in p["sizes"]}}
    if rank == 0 and world == 1 and not args.no_roofline:
        line["preprocess"] = preprocess_leg(dev, B, S)
        line["metrics"] = metrics_leg(dev, S)
    if rank == 0 and world == 1 and not args.no_c5:
        del eng, run, vp, ad
        torch.cuda.empty_cache()
        line["c5"] = c5_leg(dev, max(3, args.steps // 2), args.warmup, n_streams)
    rc = emit(line, rank) if (rank == 0 and not args.no_oracle_check) else 0
    if rank == 0 and args.no_oracle_check:
        print(json.dumps(line), flush=True)
    if world > 1:
        # every rank leaves with rank 0's parity verdict
        flag = torch.tensor([rc], dtype=torch.int32, device="cpu" if rehearsal else dev)
        dist.broadcast(flag, 0)
        rc = int(flag.item())
        dist.barrier()
        dist.destroy_process_group()
    if dist_check is not None and not (dist_check["gather_verified"] and dist_check["own_slice_verified"]):
        sys.exit("bench.py: the gathered image scores do not match the ranks' own / recomputed shards")
    if rc:
        sys.exit(rc)


if __name__ == "__main__":
    main()
