"""Evaluation harness — the counterpart of the reference test.py (same flags,
same flow, same outputs), running AdaptedCLIP on the MI355X kernels.

    python test.py --dataset MVTec --img_size 336 --save_path ckpt/...     (needs weights + data)
    python test.py --dataset synthetic --allow_random_init --img_size 336  (C1: no files needed)
    python test.py --dataset synthetic_mvtec --allow_random_init --img_size 336  (C4's 15-class flow)
    torchrun --nproc-per-node 8 test.py ...   (C3-style: each class's images sharded over 8 GPUs)
    AACLIP_REHEARSAL=1 torchrun --nproc-per-node 2 test.py ...   (the same ranks, all on cuda:0 over gloo)

Differences from the reference, all on the host side:
  * the per-batch loop calls the fused AdaptedCLIP.predict (map + score in one
    device pass) and keeps results on the device (the reference syncs twice per
    batch, test.py:85,93); metrics_eval ranks the class's pixels on the device;
  * checkpoints load with torch.load(weights_only=True);
  * --allow_random_init / --dataset synthetic run without the OpenAI weights;
  * batch k+1 is copied to the device on a copy stream while batch k runs; masks
    stay on the device until metrics_eval;
  * under torchrun (WORLD_SIZE > 1, one process per GPU) every class's test set is
    sharded by image (aaclip.parallel.shard_range), each rank predicts its shard and
    the maps / scores / masks / labels are gathered (RCCL) onto rank 0, which runs
    metrics_eval and prints and logs the table;
  * --visualize hands visualize() the device tensors: the overlays are rendered on the
    device, from thumbnails made at batch time out of the photos already there (single
    process, --gpu_preprocess), from the files otherwise (rank 0 in a sharded run), and
    for the synthetic datasets from the items un-normalised (source_u8);
  * --few_shot reads --shot, which the reference parses and never uses (its test.py:39-50
    get_support_features and utils.py:86-93 cos_sim are wired to nothing): per class a memory
    bank of --shot normal support images (get_dataset stage "support"; real datasets list them
    in --support_meta), every test patch scored by its distance to the nearest bank patch at
    every level on the device, and that map fused with the zero-shot one (single process).
    --few_shot_search fp8 keeps the bank and the test patches in MX fp8 (e4m3, a scale per 64
    values) and searches on the block-scaled fp8 MFMA, the cosine taken between the stored rows;
    the default searches in the engine's own search dtype. --bank_coreset RATIO keeps per level
    only that share of the bank's rows, a greedy k-centre coreset selected on the device (the
    subsampling of the PatchCore family of memory-bank detectors; the reference has none);
  * --tile_grid G (G >= 2; the reference has one input shape) runs sliding-window inference at the
    native scale: every photo is brought to a canvas of C = G S - (G - 1) O pixels (S = --img_size,
    O = --tile_overlap), cut into G x G tiles of S pixels, each tile goes through the tower, and the
    tile maps are stitched on the device and mixed with the map of the whole photo at S
    (--tile_global_weight). Masks, maps, metrics, regions and overlays are then C x C.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from glob import glob

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dataset import DOMAINS, get_dataset  # noqa: E402
from forward_utils import anomaly_regions, get_adapted_text_embedding, metrics_eval_deferred, visualize  # noqa: E402
from model.adapter import AdaptedCLIP  # noqa: E402
from model.clip import create_model  # noqa: E402
from utils import setup_seed  # noqa: E402


def _device_batch(input_data, prep, device, thumbs=None, *, views=None, global_prep=None, global_size=None):
    """One loader batch -> (image fp32 [B,3,S,S], mask uint8 [B,1,S,S]) on the device:
    raw uint8 batches (dataset raw=True) go through aaclip_preprocess_images /
    aaclip_resize_masks_nearest, normalised ones are copied (non_blocking from the
    DataLoader's pinned memory). Runs on the caller's current stream. thumbs (a list, raw
    batches only): the batch's uint8 [B,S,S,3] thumbnails for visualize() are appended to it,
    resized from the same device copy of the photos (aaclip_resize_bilinear_u8). views (a list,
    --tile_grid): the batch's global view fp32 [B,3,global_size,global_size] is appended to it, for
    raw batches made by global_prep from the same device copy of the photos (prep then makes the
    canvas), for normalised ones pooled from the canvas."""
    if prep is not None:
        def to_dev(u8):
            if isinstance(u8, torch.Tensor):
                return u8.to(device, non_blocking=True)
            return [t.to(device, non_blocking=True)[None] for t in u8]

        def run(fn, u8):
            return fn(u8) if isinstance(u8, torch.Tensor) else torch.cat([fn(t) for t in u8])
        image_u8 = to_dev(input_data["image_u8"])
        image, mask = run(prep.images, image_u8), run(prep.masks, to_dev(input_data["mask_u8"]))
        if thumbs is not None:
            from aaclip import ops
            thumbs.append(run(lambda t: ops.resize_bilinear_u8(t, prep.S), image_u8))
        if views is not None:
            views.append(run(global_prep.images, image_u8))
    else:
        image = input_data["image"].to(device, non_blocking=True)
        mask = torch.as_tensor(input_data["mask"]).to(device, non_blocking=True)
        if views is not None:
            # harness code, not a model of any camera: the synthetic items exist only at the canvas
            # size, so their "whole photo at S" is the canvas area-averaged down to S
            views.append(torch.nn.functional.adaptive_avg_pool2d(image, int(global_size)))
    return image, (mask != 0).to(torch.uint8)


def get_predictions(model, class_text_embeddings, test_loader, device, img_size, dataset="MVTec", prep=None,
                    n_total=None, streams=1, sources=None, tiling=None, global_prep=None, tile_batch=32):
    """test.py:53-99. Batch k+1 is copied to the device (and preprocessed, with prep) on a
    copy stream while batch k runs; maps, scores and masks stay on the device (the
    reference syncs twice per batch, test.py:85,93). Returns (masks uint8 [N,1,S,S]
    device tensor, labels numpy [N], maps [N,S,S] and scores [N] device tensors, file
    names). With n_total (sharded run: test_loader holds this rank's shard_range slice
    of a class's n_total images) the class is gathered in shard order onto rank 0, which
    alone runs metrics_eval; the other ranks return None for the tensors. A rank with an
    empty shard still takes part. streams: concurrent image chunks per batch (HIP
    streams) for batches of at least 8 images per chunk; results do not depend on it.
    sources (a list; single-process raw mode, i.e. with prep and without n_total): each batch's
    uint8 [B,S,S,3] thumbnails are appended to it, made at batch time from the photos already
    on the device, so visualize() decodes nothing twice. Otherwise it is left empty.
    tiling ({"grid", "overlap", "canvas", "global_weight"}, --tile_grid): every batch arrives at
    the canvas size (prep, or the dataset, makes it) and goes through model.predict_tiled, tile_batch
    tiles per tower call, with the global view at img_size (global_prep for raw batches); masks and
    maps, the empty shard's zero rows included, are then canvas x canvas."""
    masks, labels, preds, preds_image, file_names = [], [], [], [], []
    device = torch.device(device)
    on_gpu = device.type == "cuda"  # (a CPU device only in the host-logic tests, with a stand-in model)
    main = torch.cuda.current_stream(device) if on_gpu else None
    copy = torch.cuda.Stream(device=device) if on_gpu else None

    want_thumbs = sources is not None and prep is not None and n_total is None
    want_view = tiling is not None and tiling["global_weight"] > 0
    out_size = tiling["canvas"] if tiling is not None else img_size

    def stage(batch):
        thumbs = [] if want_thumbs else None
        views = [] if want_view else None
        extra = dict(views=views, global_prep=global_prep, global_size=img_size) if want_view else {}
        if not on_gpu:
            return (batch,) + _device_batch(batch, prep, device, thumbs, **extra) + (None, thumbs, views)
        with torch.cuda.stream(copy):
            image, mask = _device_batch(batch, prep, device, thumbs, **extra)
        ev = torch.cuda.Event()
        ev.record(copy)
        return batch, image, mask, ev, thumbs, views

    it = iter(test_loader)
    first = next(it, None)
    staged = stage(first) if first is not None else None
    while staged is not None:
        input_data, image, mask, ready, thumbs, views = staged
        if on_gpu:
            main.wait_event(ready)
            image.record_stream(main)
            mask.record_stream(main)
            if views:
                views[0].record_stream(main)
        if thumbs:
            if on_gpu:
                thumbs[0].record_stream(main)
            sources.append(thumbs[0])
        class_name = input_data["class_name"]
        assert len(set(class_name)) == 1, "mixed class not supported"
        labels.append(np.asarray(input_data["label"]))
        file_names.extend(input_data["file_name"])
        if tiling is not None:  # fresh tensors
            n_tiles = min(int(tile_batch), image.shape[0] * tiling["grid"] ** 2)
            pmap, score = model.predict_tiled(image, class_text_embeddings, tiling["grid"], tiling["overlap"],
                                              DOMAINS[dataset], global_view=views[0] if views else None,
                                              global_weight=tiling["global_weight"],
                                              streams=streams if n_tiles >= 8 * streams else 1, tile_batch=tile_batch)
            preds.append(pmap)
            preds_image.append(score)
        else:
            nst = streams if image.shape[0] >= 8 * streams else 1
            pmap, score = model.predict(image, class_text_embeddings, DOMAINS[dataset], streams=nst)
            preds.append(pmap.clone())
            preds_image.append(score.clone())
        masks.append(mask)
        nxt = next(it, None)  # host: the next batch (loader workers) while this one runs
        staged = stage(nxt) if nxt is not None else None
    if preds:
        masks, labels = torch.cat(masks), np.concatenate(labels, axis=0)
        preds, preds_image = torch.cat(preds), torch.cat(preds_image)
    else:  # empty shard (fewer images than ranks): zero rows of the right shapes
        masks = torch.zeros(0, 1, out_size, out_size, device=device, dtype=torch.uint8)
        labels = np.zeros(0, dtype=np.int64)
        preds = torch.zeros(0, out_size, out_size, device=device)
        preds_image = torch.zeros(0, device=device)
    if n_total is not None:
        import torch.distributed as dist
        from aaclip.parallel import gather_rows_to
        lab = gather_rows_to(torch.from_numpy(labels.astype(np.int64)).to(device), n_total)
        masks, preds, preds_image = (gather_rows_to(t, n_total) for t in (masks, preds, preds_image))
        names = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
        dist.gather_object(file_names, names, dst=0)
        if dist.get_rank() != 0:
            return None, None, None, None, None
        labels = lab.cpu().numpy()
        file_names = [f for part in names for f in part]
    return masks, labels, preds, preds_image, file_names


def get_few_shot_predictions(model, class_text_embeddings, test_loader, support_loader, device, img_size,
                             dataset="MVTec", prep=None, sources=None, search="default", coreset=1.0):
    """get_predictions for --few_shot (single process): the class's memory bank is built from the
    support loader's normal images (reference test.py:39-50), every test batch goes through
    AdaptedCLIP.predict_few_shot, and the class's zero-shot and few-shot maps and scores are fused
    on the device (aaclip_fewshot_fuse). Returns get_predictions' tuple with the fused maps and
    scores in the place of the zero-shot ones, and a dict of the device tensors behind them:
    zs_map, fs_map, fused_map [N,S,S], zs_score, fs_score, fused_score [N]. The bank is dropped
    on return. Eager and on one stream; sources as in get_predictions. search "fp8": the bank and
    the search in MX fp8 (--few_shot_search). coreset: the share of the bank's rows kept per level,
    a greedy k-centre coreset (--bank_coreset; 1.0 keeps all). The dict also carries "bank":
    {"rows", "source_rows": kept and source rows per level, "coverage": per level the smallest
    cosine between a source row and its nearest kept row, None for a full bank}."""
    from aaclip import ops
    device = torch.device(device)
    support = [_device_batch(batch, prep, device)[0] for batch in support_loader]
    if not support:
        raise ValueError("few-shot scoring needs at least one support image per class")
    bank = model.build_memory_bank(torch.cat(support), torch.float8_e4m3fn if search == "fp8" else None,
                                   None if coreset == 1.0 else coreset)
    bank_info = {"rows": bank.rows, "source_rows": bank.source_rows,
                 "coverage": None if bank.coverage is None else [float(c) for c in bank.coverage]}
    del support
    masks, labels, zs_maps, zs_scores, fs_maps, file_names = [], [], [], [], [], []
    for input_data in test_loader:
        thumbs = [] if (sources is not None and prep is not None) else None
        image, mask = _device_batch(input_data, prep, device, thumbs)
        if thumbs:
            sources.append(thumbs[0])
        assert len(set(input_data["class_name"])) == 1, "mixed class not supported"
        labels.append(np.asarray(input_data["label"]))
        file_names.extend(input_data["file_name"])
        zs_map, zs_score, fs_map = model.predict_few_shot(image, class_text_embeddings, bank, DOMAINS[dataset])
        zs_maps.append(zs_map)
        zs_scores.append(zs_score)
        fs_maps.append(fs_map)
        masks.append(mask)
    del bank
    if not zs_maps:
        raise ValueError("few-shot scoring needs at least one test image per class")
    masks, labels = torch.cat(masks), np.concatenate(labels, axis=0)
    zs_map, zs_score, fs_map = torch.cat(zs_maps), torch.cat(zs_scores), torch.cat(fs_maps)
    fused_map, fs_score, fused_score = ops.fewshot_fuse(zs_map, fs_map, zs_score)
    parts = {"zs_map": zs_map, "fs_map": fs_map, "fused_map": fused_map, "zs_score": zs_score,
             "fs_score": fs_score, "fused_score": fused_score, "bank": bank_info}
    return masks, labels, fused_map, fused_score, file_names, parts


def _coreset_ratio(text):
    value = float(text)
    if not 0.0 < value <= 1.0:
        raise argparse.ArgumentTypeError(f"a coreset ratio lies in (0, 1], got {text}")
    return value


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Testing")
    parser.add_argument("--model_name", type=str, default="ViT-L-14-336", help="ViT-L-14-336")
    parser.add_argument("--img_size", type=int, default=518)
    parser.add_argument("--relu", action="store_true")
    parser.add_argument("--dataset", type=str, default="MVTec")
    parser.add_argument("--shot", type=int, default=4,
                        help="--few_shot: normal support images per class in the memory bank (ignored otherwise)")
    parser.add_argument("--few_shot", action="store_true",
                        help="few-shot scoring: per class a memory bank of --shot normal support images; every "
                             "test patch's distance to its nearest bank patch, over the levels, is fused with the "
                             "zero-shot map and score (single process)")
    parser.add_argument("--few_shot_search", type=str, default="default", choices=["default", "fp8"],
                        help="--few_shot: the nearest-patch search's operands: the engine's own search dtype, or "
                             "fp8 = bank and test patches in MX fp8 (half the bank's bytes) on the block-scaled "
                             "fp8 MFMA (ignored without --few_shot)")
    parser.add_argument("--bank_coreset", type=_coreset_ratio, default=1.0, metavar="RATIO",
                        help="--few_shot: keep only this share of the memory bank's rows per level, a greedy "
                             "k-centre coreset selected on the device; in (0, 1], 1.0 keeps every row (ignored "
                             "without --few_shot)")
    parser.add_argument("--support_meta", type=str, default="",
                        help="--few_shot on a real dataset: jsonl in the metadata line format listing the normal "
                             "support images (the first --shot label-0 lines of each class are used)")
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--seed", type=int, default=111)
    parser.add_argument("--save_path", type=str, default="ckpt/baseline")
    parser.add_argument("--visualize", action="store_true")
    parser.add_argument("--visualize_true_color", action="store_true",
                        help="--visualize: write the photo in its true colours (the default keeps the reference's "
                             "files, whose photo has red and blue exchanged under a true-coloured ramp)")
    parser.add_argument("--text_norm_weight", type=float, default=0.1)
    parser.add_argument("--text_adapt_weight", type=float, default=0.1)
    parser.add_argument("--image_adapt_weight", type=float, default=0.1)
    parser.add_argument("--text_adapt_until", type=int, default=3)
    parser.add_argument("--image_adapt_until", type=int, default=6)
    # build-only flags
    parser.add_argument("--allow_random_init", action="store_true",
                        help="run on random-init CLIP + adapters when no checkpoints exist")
    parser.add_argument("--synthetic_n", type=int, default=16)
    parser.add_argument("--compute_dtype", type=str, default="fp16", choices=["bf16", "fp16", "fp32", "fp8"],
                        help="visual tower MFMA dtype: fp16 (default; meets the map-parity contract at the bf16 "
                             "rate), bf16, fp32 (fp32-MFMA parity mode) or fp8 (config C5)")
    parser.add_argument("--streams", type=int, default=2,
                        help="concurrent image chunks per batch on HIP streams (bit-identical results; "
                             "batches under 8 images per chunk run as one)")
    parser.add_argument("--gpu_preprocess", action=argparse.BooleanOptionalAction, default=True,
                        help="real datasets: decode on the host, resize + normalise on the GPU (bit-exact with the "
                             "Pillow path; the default); --no-gpu_preprocess = the Pillow transform in the workers")
    parser.add_argument("--results_json", type=str, default="",
                        help="also write the final table (rank 0) to this JSON file")
    parser.add_argument("--pro", action="store_true",
                        help="add the pixel AUPRO column (per-region overlap up to FPR 0.3, on the device)")
    parser.add_argument("--f1", action="store_true",
                        help="add the pixel and image F1-max columns and log each class's operating points "
                             "(threshold, precision, recall; thresholds in the normalised score domains)")
    parser.add_argument("--regions", action="store_true",
                        help="extract each class's defect regions at its pixel F1-max threshold (area, bbox, "
                             "centroid, peak, ground-truth overlap per region; implies --f1)")
    parser.add_argument("--regions_min_area", type=int, default=1, help="--regions: drop smaller regions")
    parser.add_argument("--regions_max", type=int, default=64,
                        help="--regions: regions listed per image, the largest first (all are counted)")
    parser.add_argument("--tile_grid", type=int, default=1, metavar="G",
                        help="sliding-window inference at the native scale: G x G tiles of --img_size pixels per "
                             "photo, stitched on the device (2..8; 1 = off, the whole photo at --img_size)")
    parser.add_argument("--tile_overlap", type=int, default=None, metavar="O",
                        help="--tile_grid: pixels neighbouring tiles share, blended with linear ramps; 0 .. "
                             "img_size // 2 (default img_size // 4). The canvas is G * img_size - (G - 1) * O pixels")
    parser.add_argument("--tile_global_weight", type=float, default=0.5, metavar="A",
                        help="--tile_grid: weight in [0, 1) of the whole photo's map and score at --img_size in "
                             "the result (0 = tiles only, no global forward)")
    args = parser.parse_args(argv)
    if args.regions:
        args.f1 = True
    if args.tile_overlap is None:
        args.tile_overlap = args.img_size // 4
    if args.tile_grid != 1:
        if not 2 <= args.tile_grid <= 8:
            parser.error(f"--tile_grid takes 1 (off) or 2..8, got {args.tile_grid}")
        if args.few_shot:
            parser.error("--tile_grid with --few_shot is not supported: the memory bank would need tile-scale rows")
        if not 0 <= args.tile_overlap <= args.img_size // 2:
            parser.error(f"--tile_overlap must lie in 0 .. img_size // 2 = {args.img_size // 2}, got "
                         f"{args.tile_overlap}")
        if not 0.0 <= args.tile_global_weight < 1.0:
            parser.error(f"--tile_global_weight must lie in [0, 1), got {args.tile_global_weight}")
    return args


def main(argv=None):
    return run(parse_args(argv))[0]


def run(args):
    """main() body; returns (results DataFrame, context dict with the model, the text
    anchors and every class's (masks, labels, preds, preds_image), with --f1 also
    "operating_points": per class the pixel and image F1-max threshold, precision and
    recall, with --regions also "regions": per class {"threshold", "images": [{"file_name",
    "n_regions", "regions"}]}, see forward_utils.anomaly_regions, with --few_shot also
    "few_shot": per class the device tensors zs_map, fs_map, fused_map, zs_score, fs_score,
    fused_score and "bank", the kept / source rows and the coreset's coverage per level; the
    class's preds and preds_image are then the fused ones, with --tile_grid also "tiling": {"grid",
    "overlap", "canvas", "global_weight"}, masks and preds then canvas x canvas) for callers/tests."""
    setup_seed(args.seed)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if args.few_shot and world > 1:
        raise RuntimeError("--few_shot runs in a single process: sharded (torchrun, WORLD_SIZE > 1) few-shot "
                           "scoring is not supported")
    if not torch.cuda.is_available():
        raise RuntimeError("the AA-CLIP MI355X build needs a GPU (no CPU path)")
    if world > 1:  # one process per GPU (torchrun); image-sharded classes
        import torch.distributed as dist
        # AACLIP_REHEARSAL=1: every rank on cuda:0 over gloo -- the multi-rank harness (shards,
        # gathers onto rank 0, rank-0 metrics) on a one-GPU box, where RCCL refuses two ranks
        # on one device (bench.py's AACLIP_BENCH_REHEARSAL is the same switch)
        rehearsal = os.environ.get("AACLIP_REHEARSAL") == "1"
        local = 0 if rehearsal else int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        if not dist.is_initialized():
            if rehearsal:
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        device = torch.device("cuda", local)
    else:
        device = torch.device("cuda:0")
    os.makedirs(args.save_path, exist_ok=True)
    logger = logging.getLogger(__name__)
    if rank == 0:
        logging.basicConfig(filename=os.path.join(args.save_path, "test.log"), encoding="utf-8", level=logging.INFO)
    logger.info("args: %s", vars(args))

    clip_model = create_model(model_name=args.model_name, img_size=args.img_size, device=device,
                              pretrained=None if args.allow_random_init else "openai",
                              require_pretrained=not args.allow_random_init,
                              force_image_size=args.img_size if args.allow_random_init else None)
    clip_model.eval()
    model = AdaptedCLIP(clip_model=clip_model, text_adapt_weight=args.text_adapt_weight,
                        image_adapt_weight=args.image_adapt_weight, text_adapt_until=args.text_adapt_until,
                        image_adapt_until=args.image_adapt_until, relu=args.relu,
                        compute_dtype={"fp32": torch.float32, "fp8": torch.float8_e4m3fn, "fp16": torch.float16}.get(
                            args.compute_dtype, torch.bfloat16)).to(device)
    model.eval()

    text_file = glob(args.save_path + "/text_adapter.pth")
    if len(text_file) > 0:
        checkpoint = torch.load(text_file[0], map_location="cpu", weights_only=True)
        model.text_adapter.load_state_dict(checkpoint["text_adapter"])
        adapt_text = True
    else:
        adapt_text = False

    files = sorted(glob(args.save_path + "/image_adapter_*.pth"))
    if not files and args.allow_random_init:
        files = [None]
    assert len(files) > 0, "image adapter checkpoint not found"
    from pandas import DataFrame, Series
    for file in files:
        if file is not None:
            checkpoint = torch.load(file, map_location="cpu", weights_only=True)
            model.image_adapter.load_state_dict(checkpoint["image_adapter"])
            test_epoch = checkpoint["epoch"]
        else:
            test_epoch = -1
        logger.info("-----------------------------------------------")
        logger.info("load model from epoch %d", test_epoch)
        logger.info("-----------------------------------------------")
        synthetic = args.dataset.startswith("synthetic")
        raw = args.gpu_preprocess and not synthetic  # synthetic items are already normalised
        tiling, data_size = None, args.img_size
        if args.tile_grid > 1:  # photos, masks and thumbnails at the canvas size; the model stays at img_size
            if not raw and not synthetic:
                raise RuntimeError("--tile_grid on a real dataset needs --gpu_preprocess: the canvas and the "
                                   "global view are made from one device copy of the photo")
            data_size = args.tile_grid * args.img_size - (args.tile_grid - 1) * args.tile_overlap
            tiling = {"grid": args.tile_grid, "overlap": args.tile_overlap, "canvas": data_size,
                      "global_weight": args.tile_global_weight}
            logger.info("tiling: %s", tiling)
        image_datasets = get_dataset(args.dataset, data_size, None, args.shot, "test", logger=logger,
                                     synthetic_n=args.synthetic_n, raw=raw)
        support_datasets = None
        if args.few_shot:  # before any model work: a real dataset without --support_meta fails here
            support_datasets = get_dataset(args.dataset, args.img_size, None, args.shot, "support", raw=raw,
                                           support_meta=args.support_meta or None)
        prep = global_prep = None
        if raw:
            from aaclip.preprocess import Preprocessor
            prep = Preprocessor(data_size)
            if tiling is not None:
                global_prep = Preprocessor(args.img_size)
        with torch.no_grad():
            text_embeddings = get_adapted_text_embedding(model if adapt_text else clip_model, args.dataset, device)
        df = DataFrame(columns=["class name", "pixel AUC", "pixel AP", "image AUC", "image AP"]
                       + (["pixel AUPRO"] if args.pro else [])
                       + (["pixel F1-max", "image F1-max"] if args.f1 else []))
        pending = []
        ctx = {"model": model, "text_embeddings": text_embeddings, "classes": {}}
        if tiling is not None:
            ctx["tiling"] = tiling
        if args.f1:
            ctx["operating_points"] = {}
        if args.regions:
            ctx["regions"], names = {}, {}
        if args.few_shot:
            ctx["few_shot"] = {}
        for class_name, image_dataset in image_datasets.items():
            workers = 0 if synthetic else 4
            from dataset import collate_raw
            n_total, whole = None, image_dataset
            if world > 1:
                from aaclip.parallel import shard_range
                n_total = len(image_dataset)
                a, b = shard_range(n_total, rank, world)
                image_dataset = torch.utils.data.Subset(image_dataset, range(a, b))
            loader = torch.utils.data.DataLoader(image_dataset, batch_size=args.batch_size, shuffle=False,
                                                 num_workers=workers, pin_memory=True,
                                                 collate_fn=collate_raw if raw else None)
            sources = [] if args.visualize else None
            with torch.no_grad():
                if args.few_shot:  # the class's bank lives inside this call
                    support_loader = torch.utils.data.DataLoader(
                        support_datasets[class_name], batch_size=args.batch_size, shuffle=False,
                        num_workers=workers, pin_memory=True, collate_fn=collate_raw if raw else None)
                    masks, labels, preds, preds_image, file_names, parts = get_few_shot_predictions(
                        model=model, class_text_embeddings=text_embeddings[class_name], test_loader=loader,
                        support_loader=support_loader, device=device, img_size=args.img_size,
                        dataset=args.dataset, prep=prep, sources=sources, search=args.few_shot_search,
                        coreset=args.bank_coreset)
                    ctx["few_shot"][class_name] = parts
                    info = parts["bank"]
                    logger.info("%s few-shot bank: %d of %d rows per level%s", class_name, info["rows"],
                                info["source_rows"], "" if info["coverage"] is None else
                                ", coverage " + ", ".join("%.4f" % c for c in info["coverage"]))
                else:
                    masks, labels, preds, preds_image, file_names = get_predictions(
                        model=model, class_text_embeddings=text_embeddings[class_name], test_loader=loader,
                        device=device, img_size=args.img_size, dataset=args.dataset, prep=prep, n_total=n_total,
                        streams=args.streams, sources=sources,
                        **(dict(tiling=tiling, global_prep=global_prep, tile_batch=args.batch_size) if tiling else {}))
            if rank != 0:  # the class was gathered onto rank 0, which runs metrics_eval
                continue
            if args.visualize:
                if synthetic:  # no files: the photos are the items, un-normalised on the host
                    photos = [whole.source_u8(i) for i in range(len(whole))]
                else:  # the batches' thumbnails; a sharded or Pillow-transform run reads the files
                    photos = torch.cat(sources) if sources else None
                visualize(masks, preds, file_names, args.save_path, args.dataset, class_name=class_name,
                          images=photos, true_color=args.visualize_true_color)
            # enqueued now, read after the loop: the next class's batches start at once
            pending.append(metrics_eval_deferred(masks, labels, preds, preds_image, class_name,
                                                 domain=DOMAINS[args.dataset], pro=args.pro, f1=args.f1))
            ctx["classes"][class_name] = (masks, labels, preds, preds_image)
            if args.regions:
                names[class_name] = file_names
        for read in pending:
            row = read()
            df.loc[len(df)] = Series(row)
            if args.f1:
                v = read.values()
                op = {level: {k: v[f"{level} F1 {k}"] for k in ("threshold", "precision", "recall")}
                      for level in ("pixel", "image")}
                ctx["operating_points"][row["class name"]] = op
                logger.info("%s F1-max operating points: %s", row["class name"], "; ".join(
                    "%s threshold %.6g, precision %.4f, recall %.4f" % (level, p["threshold"], p["precision"],
                                                                        p["recall"]) for level, p in op.items()))
            if args.regions:
                name, thr = row["class name"], op["pixel"]["threshold"]
                if thr != thr:  # NaN: one pixel class only, no F1-max threshold
                    logger.info("%s regions: no pixel F1-max threshold, none extracted", name)
                    continue
                masks, _, preds, _ = ctx["classes"][name]
                found = anomaly_regions(preds, thr, masks, min_area=args.regions_min_area,
                                        max_regions=args.regions_max)
                ctx["regions"][name] = {"threshold": thr, "images": [dict(file_name=f, **r)
                                                                     for f, r in zip(names[name], found)]}
                logger.info("%s regions at pixel threshold %.6g: %d in %d of %d images, %d listed, %d of those "
                            "overlap the ground truth", name, thr, sum(r["n_regions"] for r in found),
                            sum(r["n_regions"] > 0 for r in found), len(found),
                            sum(len(r["regions"]) for r in found),
                            sum(g["gt_area"] > 0 for r in found for g in r["regions"]))
        if rank != 0:
            continue
        df.loc[len(df)] = df.drop(columns=["class name"]).mean()
        df.loc[len(df) - 1, "class name"] = "Average"
        logger.info("final results:\n%s", df.to_string(index=False, justify="center"))
        print(df.to_string(index=False, justify="center"))
        if args.results_json:  # the table as JSON (tests compare sharded and single-process runs)
            import json
            with open(args.results_json, "w") as f:
                table = {"world": world, "rows": df.astype({c: float for c in df.columns[1:]}).to_dict("records")}
                if args.f1:
                    table["operating_points"] = ctx["operating_points"]
                if args.regions:
                    table["regions"] = ctx["regions"]
                if tiling is not None:
                    table["tiling"] = tiling
                json.dump(table, f)
    return df, ctx


if __name__ == "__main__":
    main()
