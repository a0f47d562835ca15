"""Host-side checks of the few-shot memory-bank scoring (no GPU): the C ABI (declared, bound, exported,
bad arguments refused without a launch, the ABI version still 9), the wrappers' argument checks, the
numpy statement of tests/fewshot_ref.py held to facts that need no device, the --few_shot flags and
the support stage of get_dataset."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib, ops

import fewshot_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_bank_nn_workspace", "aaclip_bank_nn", "aaclip_bank_distance", "aaclip_fewshot_fuse"]


# ---------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9
    assert "test.py:39-50" in src and "utils.py:86-93" in src
    make = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "Makefile")).read()
    assert "bank.hip" in make and re.search(r"build/bank\.o[^\n]*-fno-honor-nans", make)
    for macro, value in (("AACLIP_BANK_TILE_M", ops.BANK_TM), ("AACLIP_BANK_TILE_N", ops.BANK_TN),
                         ("AACLIP_BANK_MAX_SPLITS", ops.BANK_MAX_SPLITS), ("AACLIP_FEWSHOT_FUSE_HEAD", ops.FUSE_HEAD)):
        assert int(re.search(r"#define " + macro + r" (\d+)", src).group(1)) == value, macro


def test_workspace_plan():
    lib = _lib.lib()
    nbytes, ns = ctypes.c_size_t(0), ctypes.c_int(0)
    ok = lambda M, Nb: lib.aaclip_bank_nn_workspace(M, Nb, ctypes.byref(nbytes), ctypes.byref(ns))  # noqa: E731
    assert lib.aaclip_bank_nn_workspace(4, 4, None, ctypes.byref(ns)) == 1
    assert lib.aaclip_bank_nn_workspace(4, 4, ctypes.byref(nbytes), None) == 1
    assert ok(0, 4) == 1 and ok(4, 0) == 1 and ok(-1, 4) == 1
    for M, Nb in ((1, 1), (576, 2304), (18432, 2304), (43808, 43808), (127, 3 * ops.BANK_TN + 1), (50, 50)):
        assert ok(M, Nb) == 0
        tiles = -(-Nb // ops.BANK_TN)
        assert 1 <= ns.value <= min(tiles, ops.BANK_MAX_SPLITS) and nbytes.value == 4 * M * ns.value
        n_splits, tps = ops.bank_nn_plan(M, Nb)
        assert n_splits == ns.value and (n_splits - 1) * tps < tiles <= n_splits * tps  # no split is empty
    # the block grid runs over row tiles x splits: for one image every bank tile is a block of its
    # own, and a C2 batch's row tiles are multiplied up to one round on more than half of the 256 CUs
    tiles_m = lambda M: -(-M // ops.BANK_TM)  # noqa: E731
    assert ops.bank_nn_plan(576, 2304)[0] == -(-2304 // ops.BANK_TN)
    assert tiles_m(18432) < 128 < tiles_m(18432) * ops.bank_nn_plan(18432, 2304)[0] <= 256
    assert ops.bank_nn_plan(1, 3 * ops.BANK_TN + 1)[0] == 4
    assert tiles_m(43808) * ops.bank_nn_plan(43808, 43808)[0] >= 8 * 256  # many rounds, so the last one weighs little


def test_argument_validation_rejects_without_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)  # non-null and aligned; never dereferenced on the host

    def nn(ptrs=(p,) * 3, dtype=_lib.F16, M=5, Nb=7, K=768, ldq=768, ldr=768, nbytes=4 * 5 * 1):
        return lib.aaclip_bank_nn(dtype, M, Nb, K, ptrs[0], ldq, ptrs[1], ldr, ptrs[2], nbytes, None)
    for bad in range(3):
        assert nn(ptrs=tuple(None if i == bad else p for i in range(3))) == 1, bad
    assert nn(M=0) == 1 and nn(Nb=0) == 1 and nn(K=0) == 1 and nn(M=-3) == 1
    assert nn(dtype=_lib.FP8) == 1 and nn(dtype=7) == 1
    assert nn(K=760, ldq=760, ldr=760) == 1  # K % 64
    assert nn(ldq=704) == 1 and nn(ldr=767) == 1  # below K
    assert nn(ldq=772) == 1  # 1544 bytes: rows not 16-byte aligned
    assert nn(dtype=_lib.F32, ldr=770) == 1
    assert nn(ptrs=(ctypes.c_void_p(264), p, p)) == 1  # a misaligned operand
    assert nn(nbytes=4 * 5 - 1) == 1  # a short workspace
    assert nn(Nb=3 * ops.BANK_TN + 1, nbytes=4 * 5 * 4 - 1) == 1  # four splits need four columns

    def dist(ptrs=(p,) * 2, M=5, ns=2, acc=0):
        return lib.aaclip_bank_distance(ptrs[0], M, ns, acc, ptrs[1], None)
    assert dist(ptrs=(None, p)) == 1 and dist(ptrs=(p, None)) == 1
    assert dist(M=0) == 1 and dist(ns=0) == 1 and dist(ns=ops.BANK_MAX_SPLITS + 1) == 1

    size = ctypes.c_size_t(0)
    assert lib.aaclip_overlay_workspace(3, ctypes.byref(size)) == 0
    need = ops.FUSE_HEAD + size.value

    def fuse(ptrs=(p,) * 7, n=3, pix=100, nbytes=need):
        return lib.aaclip_fewshot_fuse(ptrs[0], ptrs[1], ptrs[2], n, pix, ptrs[3], nbytes, ptrs[4], ptrs[5], ptrs[6],
                                       None)
    for bad in range(7):
        assert fuse(ptrs=tuple(None if i == bad else p for i in range(7))) == 1, bad
    assert fuse(n=0) == 1 and fuse(pix=0) == 1 and fuse(nbytes=need - 1) == 1


def test_wrappers_reject_before_the_library():
    q, bank = torch.zeros(5, 768, dtype=torch.float16), torch.zeros(9, 768, dtype=torch.float16)
    with pytest.raises(TypeError, match="share a dtype"):
        ops.bank_nn(q, bank.to(torch.bfloat16))
    with pytest.raises(TypeError, match="unsupported dtype"):
        ops.bank_nn(q.to(torch.float64), bank.to(torch.float64))
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.bank_nn(q[:, :760].contiguous(), bank[:, :760].contiguous())
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.bank_nn(q, bank[:, :704])
    with pytest.raises(ValueError, match="unit column stride"):
        ops.bank_nn(torch.zeros(768, 5, dtype=torch.float16).t(), bank)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.bank_nn(q, torch.zeros(9, 2 * 768, dtype=torch.float16)[:, ::2])
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.bank_nn(torch.zeros(5, 772, dtype=torch.float16)[:, :768], bank)
    with pytest.raises(ValueError, match="workspace"):  # short: two splits need two columns
        ops.bank_nn(q, torch.zeros(ops.BANK_TN + 1, 768, dtype=torch.float16), torch.zeros(5, 1))
    with pytest.raises(ValueError, match="workspace"):
        ops.bank_nn(q, bank, torch.zeros(5, 1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="device"):  # well-formed operands reach the device check
        ops.bank_nn(q, bank, torch.zeros(5, 1))
    with pytest.raises(ValueError, match="part"):
        ops.bank_distance(torch.zeros(5), torch.zeros(5), accumulate=False)
    with pytest.raises(ValueError, match="grid"):
        ops.bank_distance(torch.zeros(5, 2), torch.zeros(1, 1, 2, 2), accumulate=False)
    with pytest.raises(ValueError, match="one shape"):
        ops.fewshot_fuse(torch.zeros(2, 4, 4), torch.zeros(2, 4, 5), torch.zeros(2))
    with pytest.raises(ValueError, match="one entry per image"):
        ops.fewshot_fuse(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), torch.zeros(3))
    with pytest.raises(TypeError, match="float32"):
        ops.fewshot_fuse(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4).double(), torch.zeros(2))


# ---------------------------------------------------------------------------- the restatement
def _unit(rng, n, k=768):
    x = rng.standard_normal((n, k))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_reference_self_match_permutation_and_splits():
    rng = np.random.default_rng(0)
    bank, q = _unit(rng, 300), _unit(rng, 7)
    q[3] = bank[123]
    sim = FR.bank_nn(q, bank)
    assert sim.dtype == np.float64 and abs(FR.bank_distance([sim])[3]) < 1e-15  # a query equal to a bank row
    assert np.array_equal(FR.bank_nn(q, bank[rng.permutation(300)]), sim)  # the order of the bank is nothing
    parts = FR.bank_nn_parts(q, bank, 3, 128)
    assert parts.shape == (7, 3) and np.array_equal(parts.max(axis=1), sim)
    assert np.allclose(FR.bank_distance([sim, sim]), 2 * (1 - sim), rtol=0, atol=1e-15)
    assert FR.fewshot_grid([q[:4]], [bank], 1, 2).shape == (1, 1, 2, 2)


def test_reference_all_negative_returns_the_largest_not_zero():
    rng = np.random.default_rng(1)
    q = _unit(rng, 1) + 0.5 * _unit(rng, 5)  # rows around one direction: every pair has a positive cosine
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    assert (q @ q.T).min() > 0.5
    bank = -q + 0.01 * rng.standard_normal(q.shape)
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    sim = FR.bank_nn(q, bank)
    assert (sim < -0.5).all() and np.abs(sim - (q @ bank.T).max(axis=1)).max() < 1e-14  # the largest, never 0


def test_reference_fuse_float32_and_constant_input():
    rng = np.random.default_rng(2)
    zs = rng.uniform(0, 1, (3, 6, 6)).astype(np.float32)
    fs = rng.uniform(0, 4, (3, 6, 6)).astype(np.float32)
    score = rng.uniform(0, 1, 3).astype(np.float32)
    fused_map, fs_score, fused_score = FR.fewshot_fuse(zs, fs, score)
    assert fused_map.dtype == fs_score.dtype == fused_score.dtype == np.float32
    assert np.array_equal(fs_score, fs.reshape(3, -1).max(axis=1))
    assert fused_map.min() >= 0 and fused_map.max() <= 2 and fused_score.max() <= 2
    assert fused_map.flat[np.argmax(zs)] >= 1 and fused_map.flat[np.argmin(fs)] <= 1
    flat = np.full((3, 6, 6), 0.3, np.float32)
    const_map, const_fs, const_score = FR.fewshot_fuse(zs, flat, np.full(3, 0.7, np.float32))
    assert np.isfinite(const_map).all() and np.array_equal(const_map, FR.unit_range(zs, zs.min(), zs.max()))
    assert not const_score.any() and (const_fs == np.float32(0.3)).all()  # both inputs constant: 0 + 0
    assert not FR.unit_range(flat, 0.3, 0.3).any()


# ---------------------------------------------------------------------------- flags and data
def test_flags_parse():
    import test as harness
    off = harness.parse_args([])
    assert off.few_shot is False and off.shot == 4 and off.support_meta == ""
    on = harness.parse_args(["--few_shot", "--shot", "2"])
    assert on.few_shot is True and on.shot == 2
    assert harness.parse_args(["--shot", "3"]).few_shot is False  # --shot alone stays accepted and ignored
    assert harness.parse_args(["--few_shot", "--support_meta", "a.jsonl"]).support_meta == "a.jsonl"


def test_synthetic_support_items_are_normal_and_no_test_items():
    from dataset import get_dataset
    support = get_dataset("synthetic", 70, None, 2, "support")
    tests = get_dataset("synthetic", 70, None, 2, "test")
    assert list(support) == list(tests) == ["bottle"]
    many = get_dataset("synthetic_mvtec", 70, None, 2, "support")
    many_tests = get_dataset("synthetic_mvtec", 70, None, 2, "test", synthetic_n=4)
    assert list(many) == list(many_tests) and len(many) == 15
    every_test = [it["image"] for ds in list(tests.values()) + list(many_tests.values())
                  for it in (ds[i] for i in range(len(ds)))]
    seen = []  # ("synthetic" is synthetic_mvtec's first class: the same seed, so it is left out of `many` here)
    for name, ds in list(support.items()) + list(many.items())[1:4]:
        assert len(ds) == 2
        items = [ds[i] for i in range(len(ds))]
        assert len(list(iter(ds))) == 2  # iteration ends
        for it in items:
            assert it["label"] == 0 and not it["mask"].any() and it["class_name"] == name
            assert it["image"].shape == (3, 70, 70) and it["image"].dtype == torch.float32
            assert not any(torch.equal(it["image"], t) for t in every_test + seen)
            seen.append(it["image"])
        assert torch.equal(ds[1]["image"], items[1]["image"])  # seeded
    with pytest.raises(ValueError, match="positive shot"):
        get_dataset("synthetic", 70, None, 0, "support")


def test_real_dataset_needs_support_meta(tmp_path):
    import json

    from dataset import SUPPORT_META_MISSING, get_dataset
    import test as harness
    with pytest.raises(ValueError, match="--support_meta"):
        get_dataset("MVTec", 70, None, 2, "support")
    assert "no default" in SUPPORT_META_MISSING
    # the jsonl: the first `shot` label-0 lines of each class, in file order
    from dataset import CLASS_NAMES
    lines = []
    for c in CLASS_NAMES["MVTec"]:
        lines.append({"image_path": f"{c}/test/broken/000.png", "label": 1, "class_name": c, "mask_path": "m.png"})
        lines += [{"image_path": f"{c}/train/good/{i:03d}.png", "label": 0, "class_name": c, "mask_path": ""}
                  for i in range(3)]
    meta = tmp_path / "support.jsonl"
    meta.write_text("\n".join(json.dumps(m) for m in lines) + "\n")
    sets = get_dataset("MVTec", 70, None, 2, "support", support_meta=str(meta))
    assert list(sets) == CLASS_NAMES["MVTec"]
    assert [m["image_path"] for m in sets["bottle"].meta] == ["bottle/train/good/000.png", "bottle/train/good/001.png"]
    with pytest.raises(ValueError, match="needs 4"):
        get_dataset("MVTec", 70, None, 4, "support", support_meta=str(meta))
    # the harness refuses a sharded few-shot run before it touches a device
    args = harness.parse_args(["--few_shot", "--dataset", "synthetic", "--allow_random_init"])
    old = os.environ.get("WORLD_SIZE")
    os.environ["WORLD_SIZE"] = "2"
    try:
        with pytest.raises(RuntimeError, match="single process"):
            harness.run(args)
    finally:
        if old is None:
            del os.environ["WORLD_SIZE"]
        else:
            os.environ["WORLD_SIZE"] = old
