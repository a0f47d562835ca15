"""get_dataset — drop-in for reference dataset/__init__.py:175-232 (train and test stages).

Test transform (reference :127-143): PIL bicubic resize to (S, S) -> [0,1]
tensor -> CLIP mean/std normalise; masks: nearest resize -> (mask != 0).
Implemented with PIL + numpy (torchvision is not in this image). Metadata is the
reference's jsonl layout, `./dataset/metadata/<dataset>/full-shot.jsonl`
relative to the working directory (or under $AACLIP_METADATA_ROOT, e.g. the
reference checkout's dataset/metadata — the lists are not shipped here), images
under DATA_PATH[dataset].

Extra: dataset name "synthetic" (no files needed) yields seeded N(0,1)
post-normalisation images and rectangle masks.

Train stage (reference :13-103, :188-202): `get_dataset(..., stage="train")` returns
(text_dataset, image_dataset) over `<shot>-shot.jsonl` / `full-shot.jsonl`, both BaseDataset,
the first without colour jitter (text=True). The random transforms -- ColorJitter brightness /
contrast / saturation (p = 0.7 each), rotation within 30 degrees, translation within 15 %,
the two flips (p = 0.5 each) -- are drawn by aaclip.preprocess.TrainPreprocessor.sample.
raw=False items are made in the workers (Pillow's ImageEnhance and resize, the rotation through
F.grid_sample: TrainPreprocessor.cpu_item); raw=True items carry the decoded uint8 image and
mask and the loop runs TrainPreprocessor.apply on the device (aaclip_color_jitter_u8,
aaclip_preprocess_images, aaclip_resize_masks_nearest, aaclip_geom_augment). The stream of
random numbers is this build's own (one torch.rand per item or batch), not torchvision's.
"synthetic" has a train stage too: seeded uint8 images of 96 x 80 pixels with rectangle
masks, class names cycling through three synthetic_mvtec classes.

raw=True (build extension): items carry the decoded uint8
image [H, W, 3] and mask [H, W] instead of the transformed tensors; batch them
with `collate_raw` and transform on the GPU with aaclip.preprocess.Preprocessor,
which is bit-exact with the Pillow transform above (tests/test_preprocess.py).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .constants import CLASS_NAMES, DATA_PATH, DOMAINS, PROMPTS, REAL_NAMES  # noqa: F401

MEAN = np.array((0.48145466, 0.4578275, 0.40821073), np.float32)[:, None, None]
STD = np.array((0.26862954, 0.26130258, 0.27577711), np.float32)[:, None, None]


class BaseSingleClassDataset(Dataset):
    def __init__(self, data_path: str, meta_path: str, img_size: int, class_name: str, logger=None,
                 raw: bool = False):
        assert class_name is not None, "class_name should be provided"
        self.data_path, self.img_size, self.raw = data_path, img_size, raw
        self.meta = []
        with open(meta_path) as f:
            for line in f:
                m = json.loads(line.strip())
                if m["class_name"] == class_name:
                    self.meta.append(m)
        if logger:
            logger.info(f"Class name: {class_name}")
            logger.info(f"Sample number: {len(self.meta)}")
            logger.info("=====================================")

    def __len__(self):
        return len(self.meta)

    def _image(self, path):
        from PIL import Image
        img = Image.open(path).convert("RGB").resize((self.img_size, self.img_size), Image.BICUBIC)
        a = np.asarray(img, dtype=np.float32).transpose(2, 0, 1) / 255.0
        return torch.from_numpy((a - MEAN) / STD)

    def _mask(self, path):
        from PIL import Image
        m = Image.open(path).convert("L").resize((self.img_size, self.img_size), Image.NEAREST)
        return torch.from_numpy((np.asarray(m) != 0).astype(np.float32))[None]

    def _raw_item(self, meta):
        from PIL import Image
        img = np.asarray(Image.open(os.path.join(self.data_path, meta["image_path"])).convert("RGB"))
        if meta["label"]:
            m = np.asarray(Image.open(os.path.join(self.data_path, meta["mask_path"])).convert("L"))
        else:
            m = np.zeros(img.shape[:2], np.uint8)
        return {"image_u8": torch.from_numpy(img.copy()), "mask_u8": torch.from_numpy(m.copy()),
                "label": meta["label"], "file_name": meta["image_path"], "class_name": meta["class_name"]}

    def __getitem__(self, idx):
        meta = self.meta[idx]
        if self.raw:
            return self._raw_item(meta)
        img = self._image(os.path.join(self.data_path, meta["image_path"]))
        if meta["label"]:
            mask = self._mask(os.path.join(self.data_path, meta["mask_path"]))
        else:
            mask = torch.zeros([1, self.img_size, self.img_size])
        return {"image": img, "mask": mask, "label": meta["label"], "file_name": meta["image_path"],
                "class_name": meta["class_name"]}


class BaseDataset(Dataset):
    """Reference dataset/__init__.py:13-103: every line of the jsonl, all classes mixed, with the
    train-time transforms. text=True leaves the colour jitter out (stage 1). `generator` (a CPU
    torch.Generator) drives the raw=False items' parameters; left None, one is seeded from
    torch.initial_seed() on first use, which in a DataLoader worker is that worker's own seed."""

    def __init__(self, data_path: str, meta_path: str, img_size: int, text: bool = False, raw: bool = False,
                 generator: torch.Generator | None = None):
        self.data_path, self.img_size, self.text, self.raw = data_path, img_size, text, raw
        self.full_shot = "full-shot" in meta_path
        self.generator = generator
        self.meta = []
        with open(meta_path) as f:
            for line in f:
                if line.strip():
                    self.meta.append(json.loads(line))
        self._prep = None

    def __len__(self):
        return len(self.meta)

    def _load(self, idx):
        """(PIL RGB image, PIL L mask or None, label, file name, class name) of item idx."""
        from PIL import Image
        meta = self.meta[idx]
        img = Image.open(os.path.join(self.data_path, meta["image_path"])).convert("RGB")
        mask = Image.open(os.path.join(self.data_path, meta["mask_path"])).convert("L") if meta["label"] else None
        return img, mask, meta["label"], meta["image_path"], meta["class_name"]

    def prep(self):
        if self._prep is None:
            from aaclip.preprocess import TrainPreprocessor
            self._prep = TrainPreprocessor(self.img_size, text=self.text)
        return self._prep

    def item(self, idx, params=None):
        """Item idx; raw=False with `params` (image 0 of a TrainPreprocessor.sample result) replays
        those instead of drawing."""
        img, mask, label, file_name, class_name = self._load(idx)
        out = {"label": torch.tensor(label).to(torch.int64), "file_name": file_name, "class_name": class_name}
        if self.raw:
            a = np.asarray(img)
            m = np.asarray(mask) if mask is not None else np.zeros(a.shape[:2], np.uint8)
            return {"image_u8": torch.from_numpy(a.copy()), "mask_u8": torch.from_numpy(m.copy()), **out}
        if params is None:
            if self.generator is None:
                self.generator = torch.Generator().manual_seed(torch.initial_seed() % (2 ** 63))
            params = self.prep().sample(1, self.generator)
        image, m = self.prep().cpu_item(img, mask, params)
        return {"image": image, "mask": m, **out}

    def __getitem__(self, idx):
        return self.item(idx)


class SyntheticTrainDataset(BaseDataset):
    """Seeded synthetic train set: uint8 RGB noise images of 96 x 80 pixels (a non-square source)
    over a smooth ramp, a rectangle mask (255) of 1-10% of the pixels in every other image, class
    names cycling through the first three synthetic_mvtec classes."""
    H, W = 96, 80

    def __init__(self, n: int, img_size: int, text: bool = False, raw: bool = False, seed: int = 111,
                 generator: torch.Generator | None = None):
        self.n, self.img_size, self.text, self.raw, self.seed = n, img_size, text, raw, seed
        self.generator, self._prep, self.full_shot = generator, None, True
        self.classes = CLASS_NAMES["synthetic_mvtec"][:3]

    def __len__(self):
        return self.n

    def _load(self, idx):
        from PIL import Image
        rng = np.random.Generator(np.random.Philox(key=(self.seed << 20) + idx))
        H, W = self.H, self.W
        ramp = np.linspace(40, 200, W)[None, :, None] + np.linspace(-30, 30, H)[:, None, None]
        img = np.clip(ramp + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)
        mask = None
        if idx % 2 == 1:
            area = rng.uniform(0.01, 0.10) * H * W
            h = int(max(1, min(H, round(np.sqrt(area) * rng.uniform(0.6, 1.4)))))
            w = int(max(1, min(W, round(area / h))))
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            m = np.zeros((H, W), np.uint8)
            m[y:y + h, x:x + w] = 255
            mask = Image.fromarray(m, "L")
        return (Image.fromarray(img, "RGB"), mask, int(mask is not None), f"synthetic/train/{idx:05d}.png",
                self.classes[idx % len(self.classes)])


class SyntheticSingleClassDataset(Dataset):
    """Seeded synthetic test set: N(0,1) images (already in normalised space) and
    rectangles covering 1-10% of pixels in every other image (label = mask non-empty)."""

    def __init__(self, n: int, img_size: int, class_name: str = "bottle", seed: int = 111):
        self.n, self.img_size, self.class_name, self.seed = n, img_size, class_name, seed

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        rng = np.random.Generator(np.random.Philox(key=(self.seed << 20) + idx))
        S = self.img_size
        img = rng.standard_normal((3, S, S), dtype=np.float32)
        mask = np.zeros((1, S, S), np.float32)
        if idx % 2 == 1:
            area = rng.uniform(0.01, 0.10) * S * S
            h = int(max(1, min(S, round(np.sqrt(area) * rng.uniform(0.6, 1.4)))))
            w = int(max(1, min(S, round(area / h))))
            y, x = int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1))
            mask[0, y:y + h, x:x + w] = 1.0
        return {"image": torch.from_numpy(img), "mask": torch.from_numpy(mask), "label": int(mask.max() > 0),
                "file_name": f"synthetic/{idx:05d}.png", "class_name": self.class_name}

    def source_u8(self, idx):
        """Item idx as the photo it would have come from: the normalisation undone, uint8 RGB
        [S, S, 3] (host numpy; values outside 0..255 are clipped). What visualize() is given for
        the synthetic datasets, which have no files."""
        img = self[idx]["image"].numpy()
        return np.clip(np.rint((img * STD + MEAN) * 255.0), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


class SyntheticSupportDataset(SyntheticSingleClassDataset):
    """The `shot` normal support images of a synthetic class (few-shot memory bank): the even
    (label 0) items of a SyntheticSingleClassDataset whose seed lies SEED_OFFSET above the test
    set's, so no support item is a test item (the test seeds of the synthetic datasets span 15)."""
    SEED_OFFSET = 1000

    def __init__(self, shot: int, img_size: int, class_name: str = "bottle", seed: int = 111):
        super().__init__(shot, img_size, class_name, seed + self.SEED_OFFSET)

    def __getitem__(self, idx):
        if not 0 <= idx < self.n:
            raise IndexError(idx)
        item = super().__getitem__(2 * idx)
        item["file_name"] = f"synthetic/support/{idx:05d}.png"
        return item

    def source_u8(self, idx):
        raise NotImplementedError("support items are not visualised")


class SupportDataset(BaseSingleClassDataset):
    """The first `shot` normal (label 0) lines of a class in a jsonl of the reference's line format:
    the support images of the few-shot memory bank."""

    def __init__(self, data_path: str, meta_path: str, img_size: int, class_name: str, shot: int,
                 raw: bool = False):
        super().__init__(data_path, meta_path, img_size, class_name, raw=raw)
        self.meta = [m for m in self.meta if m["label"] == 0][:shot]
        if len(self.meta) < shot:
            raise ValueError(f"{meta_path} lists {len(self.meta)} normal images of class {class_name}, "
                             f"--shot {shot} needs {shot}")


SUPPORT_META_MISSING = ("few-shot scoring of a real dataset needs --support_meta PATH: a jsonl in the metadata "
                        "line format listing normal (label 0) support images per class; the reference's lists "
                        "hold test images only, so there is no default")


def collate_raw(items):
    """Batch raw items: uint8 images/masks stacked when the sizes agree (one
    preprocessing launch), else kept as lists (one launch per size)."""
    out = {k: [it[k] for it in items] for k in items[0]}
    for k in ("image_u8", "mask_u8"):
        if len({tuple(t.shape) for t in out[k]}) == 1:
            out[k] = torch.stack(out[k])
    return out


def metadata_root() -> str:
    """Where the per-dataset jsonl test lists live. The reference reads
    ./dataset/metadata relative to the working directory (dataset/__init__.py:204);
    the same relative path is used here when it exists, else $AACLIP_METADATA_ROOT
    (e.g. <reference checkout>/dataset/metadata: the lists ship with the reference,
    not with this build)."""
    local = "./dataset/metadata"
    if os.path.isdir(local) or "AACLIP_METADATA_ROOT" not in os.environ:
        return local
    return os.environ["AACLIP_METADATA_ROOT"]


def get_dataset(dataset_name: str, img_size: int, training_mode: str, shot: int = -1, stage: str = "train",
                logger=None, synthetic_n: int = 16, raw: bool = False, support_meta: str | None = None):
    """stage "support" (few-shot memory bank): per class the `shot` normal support images -- for the
    synthetic datasets seeded items that are no test items (SyntheticSupportDataset), for a real
    dataset the first `shot` label-0 lines of the class in the jsonl `support_meta`."""
    if stage == "support" and shot < 1:
        raise ValueError(f"stage support needs a positive shot, got {shot}")
    if dataset_name in ("synthetic", "synthetic_mvtec"):
        if stage == "support":
            if dataset_name == "synthetic":
                return {"bottle": SyntheticSupportDataset(shot, img_size)}
            return {c: SyntheticSupportDataset(shot, img_size, class_name=c, seed=111 + i)
                    for i, c in enumerate(CLASS_NAMES["synthetic_mvtec"])}
        if stage == "train":
            if dataset_name != "synthetic":
                raise ValueError("of the synthetic datasets only 'synthetic' has a train stage")
            return (SyntheticTrainDataset(synthetic_n, img_size, text=True, raw=raw),
                    SyntheticTrainDataset(synthetic_n, img_size, text=False, raw=raw))
        if stage not in ("test", "visualize"):
            raise ValueError(f"stage {stage} not found; available stages: train, test, support")
        if dataset_name == "synthetic":
            return {"bottle": SyntheticSingleClassDataset(synthetic_n, img_size)}
        # config C4's shape: every MVTec class, its own seed
        return {c: SyntheticSingleClassDataset(synthetic_n, img_size, class_name=c, seed=111 + i)
                for i, c in enumerate(CLASS_NAMES["synthetic_mvtec"])}
    if "Med" not in dataset_name:
        assert dataset_name in DATA_PATH, (
            f"Dataset {dataset_name} not found; available datasets: {list(DATA_PATH.keys())}")
    if stage == "train":  # reference :188-202
        if training_mode == "few_shot":
            assert shot > 0, "shot should be positive"
            meta_path = os.path.join(metadata_root(), dataset_name, f"{shot}-shot.jsonl")
        else:
            meta_path = os.path.join(metadata_root(), dataset_name, "full-shot.jsonl")
        data_path = DATA_PATH[dataset_name.split("-")[0]]
        return (BaseDataset(data_path, meta_path, img_size, text=True, raw=raw),
                BaseDataset(data_path, meta_path, img_size, text=False, raw=raw))
    if stage == "support":
        if not support_meta:
            raise ValueError(SUPPORT_META_MISSING)
        return {c: SupportDataset(DATA_PATH[dataset_name], support_meta, img_size, c, shot, raw=raw)
                for c in CLASS_NAMES[dataset_name]}
    if stage in ("test", "visualize"):
        meta_path = os.path.join(metadata_root(), dataset_name, "full-shot.jsonl")
        return {c: BaseSingleClassDataset(DATA_PATH[dataset_name], meta_path, img_size, c,
                                          logger=logger if stage == "test" else None, raw=raw)
                for c in CLASS_NAMES[dataset_name]}
    raise ValueError(f"stage {stage} not found; available stages: train, test, support")
