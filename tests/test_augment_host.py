"""Host-side checks of the train split (no GPU): the new C entries exist and validate their
arguments without a launch, the parameter sampler is deterministic and has the reference's
ranges and frequencies, get_dataset(stage="train") yields the reference's item layout, and
train.py keeps the reference's flags and defaults (tests/golden/train_args.json, written by
tests/golden/make_golden_train_args.py from the real reference)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib
from aaclip.preprocess import TrainPreprocessor

import augment_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aaclip_color_jitter_workspace", "aaclip_color_jitter_u8", "aaclip_geom_augment")


def test_entries_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9
    # each cites the reference lines it replaces
    assert "dataset/__init__.py:44-52" in src and "dataset/__init__.py:30-39, 89-94" in src


def test_loader_refuses_a_library_without_the_gather(tmp_path):
    import subprocess
    others = [s for s in _lib.SIGNATURES if s not in ("aaclip_abi_version", "aaclip_geom_augment")]
    src = tmp_path / "stale.c"
    src.write_text(f"int aaclip_abi_version(void) {{ return {_lib.ABI_VERSION}; }}\n"
                   + "".join(f"int {s}(void) {{ return 0; }}\n" for s in others))
    out = tmp_path / "stale.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(out), str(src)], check=True)
    with pytest.raises(RuntimeError, match=r"lacks aaclip_geom_augment.*stale"):
        _lib.load(str(out))


def _f32(*v):
    return (ctypes.c_float * len(v))(*v)


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_bad_arguments_fail_before_any_launch():
    """Every call below returns AACLIP_ERR_ARG (1) on a machine without a GPU: the checks come
    before the first launch. The device pointers are never dereferenced on the host."""
    lib = _lib.lib()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    one, ws = _f32(1.0, 1.0, 1.0), ctypes.c_void_p(1 << 24)
    n = ctypes.c_size_t()
    assert lib.aaclip_color_jitter_workspace(3, ctypes.byref(n)) == 0 and n.value >= 3 * 8
    assert lib.aaclip_color_jitter_workspace(0, ctypes.byref(n)) == 1
    assert lib.aaclip_color_jitter_workspace(3, None) == 1
    jit = lambda src, dst, f, B=1, H=4, W=4, pitch=12, stride=48, w=ws, wb=1 << 20: \
        lib.aaclip_color_jitter_u8(src, stride, pitch, B, H, W, f, dst, w, wb, None)  # noqa: E731
    assert jit(None, q, one) == 1 and jit(p, None, one) == 1 and jit(p, q, None) == 1     # null pointers
    assert jit(p, q, one, B=0) == 1                                                       # B = 0
    assert jit(p, q, one, H=0) == 1 and jit(p, q, one, W=0) == 1
    assert jit(p, q, one, pitch=11) == 1                                                  # pitch < 3 W
    assert jit(p, q, _f32(1, 1, 1, 1, 1, 1), B=2, stride=47) == 1                         # images overlap
    assert jit(p, ctypes.c_void_p(4096 + 5), one) == 1                                    # partial overlap
    for bad in (float("nan"), float("inf"), -float("inf")):                               # non-finite factors
        for k in range(3):
            f = [1.0, 1.0, 1.0]
            f[k] = bad
            assert jit(p, q, _f32(*f)) == 1
    assert jit(p, q, _f32(1.0, 0.5, 1.0), w=None, wb=0) == 1                              # contrast needs workspace
    assert jit(p, q, _f32(1.0, 0.5, 1.0), wb=8) == 1                                      # ... of the right size

    par, cs = _i32(0, 0, 0, 0, 0), _f32(1.0, 0.0)
    geo = lambda src, dst, B=1, C=4, S=8, src2=None, dst2=None, C2=0, pr=par, c=cs: \
        lib.aaclip_geom_augment(src, src2, dst, dst2, B, C, C2, S, pr, c, None)  # noqa: E731
    assert geo(None, q) == 1 and geo(p, None) == 1                                        # null pointers
    assert geo(p, q, pr=None) == 1 and geo(p, q, c=None) == 1
    assert geo(p, q, B=0) == 1 and geo(p, q, C=0) == 1 and geo(p, q, S=0) == 1            # B = 0, C = 0
    assert geo(p, p) == 1                                                                 # dst == src
    assert geo(p, ctypes.c_void_p(4096 + 4 * 8 * 8 * 4 - 4)) == 1                         # overlapping
    assert geo(p, q, C2=1) == 1                                                           # second pair missing
    assert geo(p, q, C2=1, src2=q, dst2=ctypes.c_void_p(1 << 22)) == 1                    # src2 aliases dst
    assert geo(p, q, pr=_i32(2, 0, 0, 0, 0)) == 1 and geo(p, q, pr=_i32(0, 0, 0, 0, -1)) == 1  # flags are 0 / 1
    assert geo(p, q, c=_f32(float("nan"), 0.0)) == 1 and geo(p, q, c=_f32(0.0, float("inf"))) == 1


def test_sampler_is_deterministic_per_seed():
    tp = TrainPreprocessor(518, text=False)
    a = tp.sample(16, torch.Generator().manual_seed(7))
    b = tp.sample(16, torch.Generator().manual_seed(7))
    c = tp.sample(16, torch.Generator().manual_seed(8))
    assert a.keys() == b.keys()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    assert all(not v.is_cuda for v in a.values())
    assert a["color"].dtype == torch.float32 and a["color"].shape == (16, 3)
    assert a["cos_sin"].dtype == torch.float32 and a["cos_sin"].shape == (16, 2)
    assert a["shift"].dtype == torch.int32 and a["shift"].shape == (16, 2)


def test_text_sampler_has_no_colour_and_the_same_geometry():
    img = TrainPreprocessor(518, text=False).sample(64, torch.Generator().manual_seed(3))
    txt = TrainPreprocessor(518, text=True).sample(64, torch.Generator().manual_seed(3))
    assert torch.equal(txt["color"], torch.ones(64, 3))
    assert not torch.equal(img["color"], txt["color"])
    for k in ("rotate", "angle", "cos_sin", "shift", "hflip", "vflip"):
        assert torch.equal(img[k], txt[k]), k


@pytest.mark.parametrize("S", [70, 518])
def test_sampler_ranges_and_frequencies(S):
    """4000 draws: every apply-frequency within 5 binomial standard deviations of its p
    (5 * sqrt(0.7 * 0.3 / 4000) = 0.036, 5 * sqrt(0.25 / 4000) = 0.040), values in range."""
    n = 4000
    p = TrainPreprocessor(S, text=False).sample(n, torch.Generator().manual_seed(11))
    col = p["color"]
    for k in range(3):
        on = col[:, k] != 1.0
        assert abs(on.float().mean().item() - 0.7) <= 5 * math.sqrt(0.7 * 0.3 / n)
        assert col[on, k].min() >= 0.5 and col[on, k].max() <= 1.5
        assert col[on, k].max() - col[on, k].min() > 0.9  # the whole range is used
    for k in ("rotate", "hflip", "vflip"):
        assert abs(p[k].float().mean().item() - 0.5) <= 5 * math.sqrt(0.25 / n), k
    moved = (p["shift"] != 0).any(1)
    # a translation that was applied can still round to (0, 0): p = 0.5 less a share below 1 / (0.3 S)^2
    assert -5 * math.sqrt(0.25 / n) - 1.0 / (0.3 * S) ** 2 <= moved.float().mean().item() - 0.5 <= 5 * math.sqrt(0.25 / n)
    assert p["shift"].abs().max().item() <= round(0.15 * S)
    assert p["shift"].abs().max().item() >= round(0.15 * S) - 1
    rot = p["rotate"]
    assert p["angle"][rot].abs().max() <= 30.0 and p["angle"][rot].abs().max() > 29.0
    assert torch.all(p["angle"][~rot] == 0)
    for a, (c, s) in zip(p["angle"].tolist()[:50], p["cos_sin"].tolist()[:50]):
        ec, es = AR.cos_sin(a)
        assert c == float(np.float32(ec)) and s == float(np.float32(es))  # r = radians(-angle), doubles -> fp32


@pytest.fixture()
def tiny_set(tmp_path, monkeypatch):
    """Three PNGs (two sizes), one mask and a 2-shot jsonl under tmp_path, wired into the dataset
    tables as 'TinySet'."""
    from PIL import Image
    import dataset
    rng = np.random.default_rng(5)
    meta = []
    for i, (h, w) in enumerate(((40, 52), (40, 52), (33, 47))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(tmp_path / f"im{i}.png")
        m = {"image_path": f"im{i}.png", "label": int(i == 1), "class_name": ("nut", "bolt", "nut")[i], "mask_path": ""}
        if i == 1:
            mk = np.zeros((h, w), np.uint8)
            mk[5:30, 10:40] = 255
            Image.fromarray(mk, "L").save(tmp_path / "mask1.png")
            m["mask_path"] = "mask1.png"
        meta.append(m)
    os.makedirs(tmp_path / "metadata" / "TinySet")
    with open(tmp_path / "metadata" / "TinySet" / "2-shot.jsonl", "w") as f:
        f.write("\n".join(json.dumps(m) for m in meta) + "\n")
    monkeypatch.setitem(dataset.DATA_PATH, "TinySet", str(tmp_path))
    monkeypatch.setenv("AACLIP_METADATA_ROOT", str(tmp_path / "metadata"))
    monkeypatch.chdir(tmp_path)
    return meta


def test_train_stage_items(tiny_set):
    import dataset
    S = 28
    text_ds, image_ds = dataset.get_dataset("TinySet", S, "few_shot", 2, "train")
    assert isinstance(text_ds, dataset.BaseDataset) and isinstance(image_ds, dataset.BaseDataset)
    assert text_ds.text and not image_ds.text and len(text_ds) == len(image_ds) == 3
    for ds in (text_ds, image_ds):
        ds.generator = torch.Generator().manual_seed(21)
        for i in range(3):
            it = ds[i]
            assert set(it) == {"image", "mask", "label", "file_name", "class_name"}
            assert it["image"].shape == (3, S, S) and it["image"].dtype == torch.float32
            assert it["mask"].shape == (1, S, S) and it["mask"].dtype == torch.float32
            assert set(np.unique(it["mask"].numpy())) <= {0.0, 1.0}
            assert it["label"].dtype == torch.int64 and it["label"].dim() == 0 and int(it["label"]) == int(i == 1)
            assert it["file_name"] == f"im{i}.png" and it["class_name"] == tiny_set[i]["class_name"]
    # a batch collates as the reference's does
    b = next(iter(torch.utils.data.DataLoader(image_ds, batch_size=3)))
    assert b["image"].shape == (3, 3, S, S) and b["label"].dtype == torch.int64 and b["label"].shape == (3,)

    # the same parameters: the text item is the image item without the colour jitter
    tp = TrainPreprocessor(S, text=False)
    params = tp.sample(1, torch.Generator().manual_seed(2))
    params["color"] = torch.tensor([[0.62, 1.31, 0.77]])
    plain = {**params, "color": torch.ones(1, 3)}
    a, t = image_ds.item(1, params), text_ds.item(1, plain)
    assert torch.equal(a["mask"], t["mask"]) and not torch.equal(a["image"], t["image"])
    assert torch.equal(image_ds.item(1, plain)["image"], t["image"])
    # ... and with nothing applied it is the test split's transform of the same file
    off = {"color": torch.ones(1, 3), "rotate": torch.zeros(1, dtype=torch.bool), "angle": torch.zeros(1),
           "cos_sin": torch.tensor([[1.0, 0.0]]), "shift": torch.zeros(1, 2, dtype=torch.int32),
           "hflip": torch.zeros(1, dtype=torch.bool), "vflip": torch.zeros(1, dtype=torch.bool)}
    single = dataset.BaseSingleClassDataset(image_ds.data_path, os.path.join("metadata", "TinySet", "2-shot.jsonl"), S,
                                            "bolt")
    ref = single[0]
    got = image_ds.item(1, off)
    assert torch.equal(got["image"], ref["image"]) and torch.equal(got["mask"], ref["mask"])
    assert got["mask"].sum() > 0


def test_train_stage_raw_items(tiny_set):
    import dataset
    text_ds, image_ds = dataset.get_dataset("TinySet", 28, "few_shot", 2, "train", raw=True)
    it = image_ds[2]
    assert it["image_u8"].dtype == torch.uint8 and it["image_u8"].shape == (33, 47, 3)
    assert it["mask_u8"].dtype == torch.uint8 and it["mask_u8"].shape == (33, 47) and it["mask_u8"].sum() == 0
    assert it["label"].dtype == torch.int64
    assert text_ds[1]["mask_u8"].max() == 255
    b = dataset.collate_raw([image_ds[0], image_ds[1]])
    assert b["image_u8"].shape == (2, 40, 52, 3) and b["mask_u8"].shape == (2, 40, 52)
    b = dataset.collate_raw([image_ds[0], image_ds[2]])
    assert isinstance(b["image_u8"], list)
    with pytest.raises(AssertionError):
        dataset.get_dataset("TinySet", 28, "few_shot", 0, "train")


def test_synthetic_train_stage():
    import dataset
    text_ds, image_ds = dataset.get_dataset("synthetic", 28, "few_shot", 4, "train", synthetic_n=6, raw=True)
    assert len(text_ds) == len(image_ds) == 6
    items = [image_ds[i] for i in range(6)]
    assert items[0]["image_u8"].shape == (96, 80, 3) and items[0]["image_u8"].dtype == torch.uint8
    assert [it["class_name"] for it in items] == dataset.CLASS_NAMES["synthetic_mvtec"][:3] * 2
    assert [int(it["label"]) for it in items] == [0, 1, 0, 1, 0, 1]
    assert all((it["mask_u8"].max() == 255) == bool(it["label"]) for it in items)
    assert torch.equal(image_ds[3]["image_u8"], text_ds[3]["image_u8"])  # seeded
    cpu = dataset.get_dataset("synthetic", 28, "few_shot", 4, "train", synthetic_n=2)[1]
    cpu.generator = torch.Generator().manual_seed(1)
    assert cpu[1]["image"].shape == (3, 28, 28) and set(np.unique(cpu[1]["mask"].numpy())) <= {0.0, 1.0}
    # the test stage is what it was
    assert list(dataset.get_dataset("synthetic", 28, None, stage="test", synthetic_n=2)) == ["bottle"]


def test_parse_args_keeps_the_reference_defaults():
    import train
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "train_args.json")))["defaults"]
    got = vars(train.parse_args([]))
    assert {k: got[k] for k in ref} == ref
    extra = {k: v for k, v in got.items() if k not in ref}
    assert extra == {"allow_random_init": False, "synthetic_n": 16, "gpu_preprocess": True, "max_steps": 0}
    assert train.parse_args(["--no-gpu_preprocess"]).gpu_preprocess is False
    assert "ipdb" not in open(os.path.join(ROOT, "aa-clip_amd", "train.py")).read().replace("ipdb is not imported", "")
