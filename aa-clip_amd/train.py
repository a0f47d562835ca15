"""Training harness — the counterpart of the reference train.py (same flags, same flow, same
checkpoint files and keys), running both stages on the MI355X kernels.

    python train.py --dataset VisA --save_path ckpt/...                      (needs weights + data)
    python train.py --dataset synthetic --allow_random_init --img_size 70 --synthetic_n 4 \\
                    --text_epoch 1 --image_epoch 1                           (no files needed)
    python test.py --dataset <test set> --save_path <the same>               (loads what this wrote)

Stage 1 (train_text_adapter, reference train.py:38-114) trains `text_adapter` against the frozen
surgery tower's patch features; stage 2 (train_image_adapter, :117-174) trains `image_adapter`.
Both loop bodies are the reference's as written, including its `loss =` inside stage 1's per-level
loop (only the last level reaches backward()), `scheduler.step()` per batch in stage 2, Adam
betas (0.5, 0.999) and MultiStepLR [16000, 32000]. The adapted model computes in fp32; with
AACLIP_TRAIN_DTYPE=bf16 in the environment (default fp32) stage 2 runs in bf16 mixed precision
instead (fp32 weights, gradients, Adam and residual stream, bf16 GEMM inputs), stage 1 and the text
anchors as before, and the checkpoints keep their keys and fp32 tensors. Writes text_adapter.pth {epoch, text_adapter, text_optimizer}, image_adapter.pth
and image_adapter_<epoch>.pth {epoch, image_adapter, image_optimizer}; resumes from them as the
reference does.

Differences from the reference, all on the host side:
  * --gpu_preprocess (default): the loader workers only decode (dataset raw=True, collate_raw) and
    every batch is augmented on the device by aaclip.preprocess.TrainPreprocessor (colour jitter,
    bicubic resize + normalise, nearest mask, rotation / translation / flips); --no-gpu_preprocess
    makes the items in the workers (Pillow + grid_sample) from the same sampler;
  * checkpoints load with torch.load(weights_only=True); ipdb is not imported;
  * --allow_random_init / --dataset synthetic run without the OpenAI weights or any data;
    --max_steps N stops every epoch after N batches (tests, timing);
  * the frozen surgery tower (its packed weights too) is released before stage 2.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
import warnings
from glob import glob

import numpy as np
import torch
import torch.nn.functional as F
from torch.optim.lr_scheduler import MultiStepLR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dataset import collate_raw, get_dataset  # noqa: E402
from forward_utils import (calculate_seg_loss, calculate_similarity_map,  # noqa: E402
                           get_adapted_single_class_text_embedding, get_adapted_text_embedding)
from model.adapter import AdaptedCLIP  # noqa: E402
from model.clip import create_model  # noqa: E402
from utils import setup_seed  # noqa: E402

cpu_num = 4


def train_dtype_from_env(env=None) -> torch.dtype:
    """Stage 2's compute dtype from AACLIP_TRAIN_DTYPE: fp32 (the default) or bf16."""
    v = (os.environ if env is None else env).get("AACLIP_TRAIN_DTYPE", "fp32").strip().lower()
    if v in ("fp32", "float32", "f32"):
        return torch.float32
    if v in ("bf16", "bfloat16"):
        return torch.bfloat16
    raise ValueError(f"AACLIP_TRAIN_DTYPE={v!r}: expected fp32 or bf16")


def _batches(train_loader, prep, generator, device, max_steps):
    """The loader's batches with "image" / "mask" / "label" on the device. With prep (a
    TrainPreprocessor; the loader yields raw uint8 batches) the batch is augmented on the device
    with parameters drawn from `generator`; else the workers made the tensors."""
    for step, input_data in enumerate(train_loader):
        if max_steps and step >= max_steps:
            break
        if prep is not None:
            def dev(u8):
                return u8.to(device, non_blocking=True) if isinstance(u8, torch.Tensor) else [
                    t.to(device, non_blocking=True) for t in u8]
            params = prep.sample(len(input_data["class_name"]), generator)
            image, mask = prep.apply(dev(input_data["image_u8"]), dev(input_data["mask_u8"]), params)
            input_data = {**input_data, "image": image, "mask": mask, "label": torch.stack(input_data["label"])}
        yield input_data


def train_text_adapter(adapted_model, clip_surgery, text_norm_weight, train_loader, optimizer, device, start_epoch,
                       save_path, text_epoch, dataset_name, img_size, logger, prep=None, generator=None,
                       max_steps=0, losses=None):
    """Reference train.py:38-114. prep / generator / max_steps: see _batches; losses: a list that
    receives every step's loss (tests)."""
    for epoch in range(start_epoch, text_epoch):
        logger.info(f"training text epoch {epoch}:")

        loss_list = []
        for input_data in _batches(train_loader, prep, generator, device, max_steps):
            image = input_data["image"].to(device)
            mask = input_data["mask"].to(device)
            class_names = input_data["class_name"]

            # forward text
            epoch_text_feature_dict = {}
            for class_name in list(set(class_names)):
                text_embedding = get_adapted_single_class_text_embedding(adapted_model, dataset_name, class_name,
                                                                         device)
                epoch_text_feature_dict[class_name] = text_embedding
            epoch_text_feature = torch.stack([epoch_text_feature_dict[class_name] for class_name in class_names],
                                             dim=0)  # bs,768,2
            # forward image
            with torch.no_grad():
                _, patch_features = clip_surgery.encode_image(image, [6, 12, 18, 24])
                cls_token, _ = adapted_model.clipmodel.encode_image(image, [])
                cls_token = cls_token / cls_token.norm(dim=-1, keepdim=True)
                patch_features = [clip_surgery.visual.ln_post(t[:, 1:, :]) for t in patch_features]
                patch_features = [t @ clip_surgery.visual.proj for t in patch_features]
                patch_features = [t / t.norm(dim=-1, keepdim=True) for t in patch_features]
                patch_features = [t + cls_token.unsqueeze(1) for t in patch_features]
            # calculate similarity and get prediction
            for f in patch_features:
                # bs,patch_num,768
                patch_preds = calculate_similarity_map(f, epoch_text_feature, img_size)
                loss = calculate_seg_loss(patch_preds, mask)
                orthogonal_loss = ((epoch_text_feature[:, :, 0] * epoch_text_feature[:, :, 1]).sum(1).mean()) ** 2
                loss += orthogonal_loss * text_norm_weight
            # backward
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            loss_list.append(loss.item())
        if losses is not None:
            losses.extend(loss_list)
        logger.info(f"loss: {np.mean(loss_list)}")
        # save checkpoint
        ckp_path = os.path.join(save_path, "text_adapter.pth")
        torch.save({"epoch": epoch + 1, "text_adapter": adapted_model.text_adapter.state_dict(),
                    "text_optimizer": optimizer.state_dict()}, ckp_path)
    return adapted_model


def train_image_adapter(model, text_embeddings, train_loader, optimizer, scheduler, device, start_epoch, save_path,
                        image_epoch, img_size, logger, prep=None, generator=None, max_steps=0, losses=None):
    """Reference train.py:117-174."""
    for epoch in range(start_epoch, image_epoch):
        logger.info(f"training image epoch {epoch}:")
        loss_list = []
        for input_data in _batches(train_loader, prep, generator, device, max_steps):
            image = input_data["image"].to(device)
            mask = input_data["mask"].to(device)
            label = input_data["label"].to(device)
            B, C, H, W = image.shape
            # forward text
            class_names = input_data["class_name"]
            epoch_text_feature = torch.stack([text_embeddings[class_name] for class_name in class_names], dim=0)

            # forward image
            patch_features, det_feature = model(image)
            # calculate similarity and get prediction
            loss = 0.0
            det_feature = det_feature.unsqueeze(1)
            cls_preds = torch.matmul(det_feature, epoch_text_feature)[:, 0]
            loss += F.cross_entropy(cls_preds, label)
            for f in patch_features:
                # text-image alignment
                patch_preds = calculate_similarity_map(f, epoch_text_feature, img_size)
                loss += calculate_seg_loss(patch_preds, mask)  # backward
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            loss_list.append(loss.item())
            scheduler.step()
        if losses is not None:
            losses.extend(loss_list)
        logger.info(f"loss: {np.mean(loss_list)}")
        # save checkpoint
        model_dict = {"epoch": epoch + 1, "image_adapter": model.image_adapter.state_dict(),
                      "image_optimizer": optimizer.state_dict()}
        torch.save(model_dict, os.path.join(save_path, "image_adapter.pth"))
        if (epoch + 1) % 1 == 0:
            ckp_path = os.path.join(save_path, f"image_adapter_{epoch + 1}.pth")
            torch.save(model_dict, ckp_path)
    return model


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Training")
    # model
    parser.add_argument("--model_name", type=str, default="ViT-L-14-336",
                        help="clip model to use (default: ViT-L-14-336)")
    parser.add_argument("--img_size", type=int, default=518)
    parser.add_argument("--surgery_until_layer", type=int, default=20)
    parser.add_argument("--relu", action="store_true", help="use relu after projection")
    # training
    parser.add_argument("--dataset", type=str, default="VisA")
    parser.add_argument("--training_mode", type=str, default="few_shot", choices=["few_shot", "full_shot"])
    parser.add_argument("--shot", type=int, default=32, help="number of shots (0 means full shot)")
    parser.add_argument("--text_batch_size", type=int, default=16)
    parser.add_argument("--image_batch_size", type=int, default=2)
    parser.add_argument("--text_epoch", type=int, default=5, help="epochs for stage1")
    parser.add_argument("--image_epoch", type=int, default=20, help="epochs for stage2")
    parser.add_argument("--text_lr", type=float, default=0.00001, help="learning rate for stage1")
    parser.add_argument("--image_lr", type=float, default=0.0005, help="learning rate for stage2")
    parser.add_argument("--criterion", type=str, default=["dice_loss", "focal_loss"], nargs="+")
    # exp
    parser.add_argument("--seed", type=int, default=111)
    parser.add_argument("--save_path", type=str, default="ckpt/baseline")
    # hyper-parameters
    parser.add_argument("--text_norm_weight", type=float, default=0.1)
    parser.add_argument("--text_adapt_weight", type=float, default=0.1)
    parser.add_argument("--image_adapt_weight", type=float, default=0.1)
    parser.add_argument("--text_adapt_until", type=int, default=3)
    parser.add_argument("--image_adapt_until", type=int, default=6)
    # build-only flags
    parser.add_argument("--allow_random_init", action="store_true",
                        help="train on a random-init CLIP when the OpenAI weights are absent")
    parser.add_argument("--synthetic_n", type=int, default=16)
    parser.add_argument("--gpu_preprocess", action=argparse.BooleanOptionalAction, default=True,
                        help="decode on the host, augment + resize + normalise on the GPU (the default); "
                             "--no-gpu_preprocess = the Pillow / grid_sample transforms in the workers")
    parser.add_argument("--max_steps", type=int, default=0, help="batches per epoch (0 = all)")
    return parser.parse_args(argv)


def main(argv=None):
    # the reference's process-wide settings (train.py:25-35), for the command line only
    warnings.filterwarnings("ignore")
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "VECLIB_MAXIMUM_THREADS",
              "NUMEXPR_NUM_THREADS"):
        os.environ[k] = str(cpu_num)
    torch.set_num_threads(cpu_num)
    os.environ["TOKENIZERS_PARALLELISM"] = "false"
    run(parse_args(argv))


def run(args):
    """main() body; returns a context dict (the model, each stage's per-step losses, whether stage 1
    ran and the epochs both stages started from) for callers/tests."""
    setup_seed(args.seed)
    train_dtype = train_dtype_from_env()
    if not torch.cuda.is_available():
        raise RuntimeError("the AA-CLIP MI355X build needs a GPU (no CPU path)")
    # check save_path and setting logger
    os.makedirs(args.save_path, exist_ok=True)
    logger = logging.getLogger(__name__)
    logging.basicConfig(filename=os.path.join(args.save_path, "train.log"), encoding="utf-8", level=logging.INFO)
    logger.info("args: %s", vars(args))
    device = torch.device("cuda:0")
    # ========================================================
    # load model
    pretrained = dict(pretrained=None if args.allow_random_init else "openai",
                      require_pretrained=not args.allow_random_init,
                      force_image_size=args.img_size if args.allow_random_init else None)
    # set up model for training (the same random-init weights in both towers: one draw, one copy)
    clip_model = create_model(model_name=args.model_name, img_size=args.img_size, device=device, **pretrained)
    clip_model.eval()
    # setup image feature extractor after surgery
    clip_surgery = create_model(model_name=args.model_name, img_size=args.img_size, device=device, **pretrained)
    if args.allow_random_init:
        clip_surgery.load_state_dict(clip_model.state_dict())
    clip_surgery.eval()
    clip_surgery.visual.DAPM_replace(DPAM_layer=args.surgery_until_layer)
    model = AdaptedCLIP(clip_model=clip_model, text_adapt_weight=args.text_adapt_weight,
                        image_adapt_weight=args.image_adapt_weight, text_adapt_until=args.text_adapt_until,
                        image_adapt_until=args.image_adapt_until, relu=args.relu,
                        compute_dtype=torch.float32).to(device)
    model.eval()
    # set optimizer
    text_optimizer = torch.optim.Adam(model.text_adapter.parameters(), lr=args.text_lr, betas=(0.5, 0.999))
    image_optimizer = torch.optim.Adam(model.image_adapter.parameters(), lr=args.image_lr, betas=(0.5, 0.999))
    image_scheduler = MultiStepLR(image_optimizer, milestones=[16000, 32000], gamma=0.5)
    # ========================================================
    # load checkpoints if exists
    text_start_epoch = 0
    text_file = glob(args.save_path + "/text_adapter.pth")
    if len(text_file) > 0:
        checkpoint = torch.load(text_file[0], map_location="cpu", weights_only=True)
        model.text_adapter.load_state_dict(checkpoint["text_adapter"])
        text_optimizer.load_state_dict(checkpoint["text_optimizer"])
        text_start_epoch = checkpoint["epoch"]
        adapt_text = not (text_start_epoch == (args.text_epoch - 1))  # the reference's expression
    elif args.text_epoch == 0:
        adapt_text = False
    else:
        text_start_epoch = 0
        adapt_text = True  # check if text adapter is loaded
    file = glob(args.save_path + "/image_adapter.pth")
    if len(file) > 0:
        checkpoint = torch.load(file[0], map_location="cpu", weights_only=True)
        image_start_epoch = checkpoint["epoch"]
        model.image_adapter.load_state_dict(checkpoint["image_adapter"])
        image_optimizer.load_state_dict(checkpoint["image_optimizer"])
    else:
        image_start_epoch = 0
    # ========================================================
    # load dataset
    if args.training_mode == "full_shot":
        args.shot = -1
    synthetic = args.dataset.startswith("synthetic")
    raw = bool(args.gpu_preprocess)
    kwargs = {"num_workers": 0 if synthetic else 4, "pin_memory": True}
    if raw:
        kwargs["collate_fn"] = collate_raw
    logger.info("loading dataset ...")
    text_dataset, image_dataset = get_dataset(args.dataset, args.img_size, args.training_mode, args.shot, "train",
                                              logger, synthetic_n=args.synthetic_n, raw=raw)
    text_dataloader = torch.utils.data.DataLoader(text_dataset, batch_size=args.text_batch_size, shuffle=True,
                                                  **kwargs)
    logger.info("loading image adaptation dataset ...")
    image_dataloader = torch.utils.data.DataLoader(image_dataset, batch_size=args.image_batch_size, shuffle=True,
                                                   **kwargs)
    text_prep = image_prep = generator = None
    if raw:
        from aaclip.preprocess import TrainPreprocessor
        text_prep = TrainPreprocessor(args.img_size, text=True)
        image_prep = TrainPreprocessor(args.img_size, text=False)
        generator = torch.Generator().manual_seed(args.seed)
    # the synthetic train set draws its class names from synthetic_mvtec's prompt tables
    prompt_dataset = "synthetic_mvtec" if args.dataset == "synthetic" else args.dataset
    ctx = {"model": model, "adapt_text": adapt_text, "text_start_epoch": text_start_epoch,
           "image_start_epoch": image_start_epoch, "text_losses": [], "image_losses": []}
    # ========================================================
    # training
    if adapt_text:
        model = train_text_adapter(adapted_model=model, clip_surgery=clip_surgery,
                                   text_norm_weight=args.text_norm_weight, train_loader=text_dataloader,
                                   optimizer=text_optimizer, device=device, start_epoch=text_start_epoch,
                                   dataset_name=prompt_dataset, save_path=args.save_path,
                                   text_epoch=args.text_epoch, img_size=args.img_size, logger=logger,
                                   prep=text_prep, generator=generator, max_steps=args.max_steps,
                                   losses=ctx["text_losses"])
    # the surgery tower and its packed device weights go before stage 2 allocates its activations
    clip_surgery.visual._frozen.clear()
    clip_model.visual._frozen.clear()  # the plain frozen tower of stage 1's cls token
    del text_dataloader, text_dataset, clip_surgery, text_optimizer
    torch.cuda.empty_cache()
    with torch.no_grad():
        if args.text_epoch == 0:
            text_embeddings = get_adapted_text_embedding(clip_model, prompt_dataset, device)
        else:
            text_embeddings = get_adapted_text_embedding(model, prompt_dataset, device)
    if train_dtype == torch.bfloat16:  # stage 2 in bf16 mixed precision; the tower is packed on first use
        model.compute_dtype = model.train_dtype = torch.bfloat16
    ctx["train_dtype"] = train_dtype
    model = train_image_adapter(model=model, text_embeddings=text_embeddings, image_epoch=args.image_epoch,
                                train_loader=image_dataloader, optimizer=image_optimizer,
                                scheduler=image_scheduler, device=device, start_epoch=image_start_epoch,
                                save_path=args.save_path, img_size=args.img_size, logger=logger, prep=image_prep,
                                generator=generator, max_steps=args.max_steps, losses=ctx["image_losses"])
    return ctx


if __name__ == "__main__":
    main()
