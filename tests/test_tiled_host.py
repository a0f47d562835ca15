"""Tiled inference, host side (no kernel runs here): aaclip_tile_plan against the numpy statement
of the geometry (tests/tiled_ref.py), the properties the stitch kernel relies on, the argument
checks, the reference's own bilinear against torch, the ABI, and the harness's flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tiled_ref as TR
from aaclip import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(28, 2, 8), (28, 2, 14), (28, 3, 5), (28, 2, 0), (70, 3, 35), (42, 4, 1), (518, 2, 129)]


@pytest.mark.parametrize("S,G,O", SHAPES)
def test_plan_equals_the_reference_tables(S, G, O):
    index, weight = ops.tile_plan(S, G, O)
    ref_index, ref_weight = TR.plan(S, G, O)
    C = TR.canvas_side(S, G, O)
    assert index.shape == (C, 2) and weight.shape == (C, 4) and ops.tile_canvas(S, G, O) == C
    assert np.array_equal(index, ref_index)
    assert np.array_equal(weight.view(np.uint32), ref_weight.view(np.uint32))


@pytest.mark.parametrize("S,G,O", SHAPES)
def test_cover_and_weight_sums(S, G, O):
    """Every canvas coordinate is covered by one or two tiles (the kernel reads no third), the
    second one exactly where the table gives it a weight; the float32 weights of a coordinate sum
    to 1 within 2^-23, the tile pair and the bilinear pair alike; the bilinear cell exists."""
    index, weight = ops.tile_plan(S, G, O)
    C, step = TR.canvas_side(S, G, O), S - O
    for c in range(C):
        cover = [i for i in range(G) if i * step <= c < i * step + S]
        assert 1 <= len(cover) <= 2 and index[c, 0] == cover[0]
        assert (weight[c, 1] != 0) == (len(cover) == 2)
        assert 0 < weight[c, 0] <= 1 and 0 <= weight[c, 1] < 1
    w = weight.astype(np.float64)
    assert np.abs(w[:, 0] + w[:, 1] - 1).max() <= 2.0 ** -23
    assert np.abs(w[:, 2] + w[:, 3] - 1).max() <= 2.0 ** -23
    assert index[:, 1].min() >= 0 and index[:, 1].max() <= S - 1
    assert ops.tile_side(C, G, O) == S


def test_plan_argument_errors():
    lib = _lib.lib()
    idx, wt = np.zeros((4096, 2), np.int32), np.zeros((4096, 4), np.float32)
    pi, pw = idx.ctypes.data_as(ctypes.c_void_p), wt.ctypes.data_as(ctypes.c_void_p)
    assert lib.aaclip_tile_plan(28, 2, 8, pi, pw) == 0
    for S, G, O in ((28, 1, 8), (28, 9, 8), (28, 2, -1), (28, 2, 15), (0, 2, 0)):
        assert lib.aaclip_tile_plan(S, G, O, pi, pw) == 1, (S, G, O)
    assert lib.aaclip_tile_plan(28, 2, 8, None, pw) == 1
    assert lib.aaclip_tile_plan(28, 2, 8, pi, None) == 1
    # the device entries refuse the same geometry, null operands and a bad weight before any launch
    p = ctypes.c_void_p(256)
    assert lib.aaclip_tile_gather(None, 1, 28, 2, 8, 0, 4, p, None) == 1
    assert lib.aaclip_tile_gather(p, 1, 28, 2, 8, 0, 4, None, None) == 1
    for S, G, O in ((28, 1, 8), (28, 9, 8), (28, 2, -1), (28, 2, 15)):
        assert lib.aaclip_tile_gather(p, 1, S, G, O, 0, 1, p, None) == 1
        assert lib.aaclip_tile_stitch(p, p, p, p, 1, S, G, O, 0.5, p, None) == 1
    for t0, nt in ((0, 5), (4, 1), (-1, 2), (0, 0), (3, 2)):  # tile rows outside [0, 4)
        assert lib.aaclip_tile_gather(p, 1, 28, 2, 8, t0, nt, p, None) == 1
    assert lib.aaclip_tile_stitch(None, p, p, p, 1, 28, 2, 8, 0.5, p, None) == 1
    assert lib.aaclip_tile_stitch(p, None, p, p, 1, 28, 2, 8, 0.5, p, None) == 1  # a > 0 needs the global maps
    assert lib.aaclip_tile_stitch(p, p, None, p, 1, 28, 2, 8, 0.5, p, None) == 1
    assert lib.aaclip_tile_stitch(p, p, p, ctypes.c_void_p(260), 1, 28, 2, 8, 0.5, p, None) == 1  # weight alignment
    assert lib.aaclip_tile_stitch(p, p, p, p, 0, 28, 2, 8, 0.5, p, None) == 1
    for a in (-0.1, 1.0, float("nan")):
        assert lib.aaclip_tile_stitch(p, p, p, p, 1, 28, 2, 8, a, p, None) == 1
        assert lib.aaclip_tile_score(p, p, 1, 2, a, p, None) == 1
    assert lib.aaclip_tile_score(p, None, 1, 2, 0.5, p, None) == 1
    assert lib.aaclip_tile_score(None, p, 1, 2, 0.5, p, None) == 1
    assert lib.aaclip_tile_score(p, p, 1, 1, 0.5, p, None) == 1
    assert lib.aaclip_tile_score(p, p, 1, 9, 0.5, p, None) == 1


def test_wrappers_refuse_bad_geometry_on_the_host():
    for S, G, O in ((28, 1, 8), (28, 9, 8), (28, 2, -1), (28, 2, 15)):
        with pytest.raises(ValueError):
            ops.tile_plan(S, G, O)
    with pytest.raises(ValueError, match="not 2 x 2 tiles"):
        ops.tile_side(49, 2, 8)
    with pytest.raises(ValueError):
        ops.tile_side(30, 2, 26)  # S = 28, O > S / 2


@pytest.mark.parametrize("S,G,O", SHAPES + [(32, 2, 0)])
def test_reference_bilinear_is_torch_interpolate(S, G, O):
    """Pins the reference, not the kernel: the reference's cells and weights, taken before the
    table's one rounding to float32 (plan(dtype=float64), the same code), reproduce
    F.interpolate(mode="bilinear", align_corners=False) in float64 on the CPU; the float32 table
    is that, rounded once."""
    index, weight = TR.plan(S, G, O)
    _, exact = TR.plan(S, G, O, dtype=np.float64)
    C = TR.canvas_side(S, G, O)
    assert np.array_equal(exact.astype(np.float32), weight)
    g = np.random.default_rng(S * 100 + G * 10 + O).uniform(0, 4, (2, S, S))
    got = TR.upsample(g, index, exact)
    want = torch.nn.functional.interpolate(torch.from_numpy(g)[:, None], size=(C, C), mode="bilinear",
                                           align_corners=False)[:, 0].numpy()
    assert want.dtype == np.float64
    err = np.abs(got - want).max()
    print(f"S {S} G {G} O {O}: reference bilinear vs F.interpolate float64 max abs {err:.3e}")
    assert err <= 1e-12


def test_reference_stitch_is_slice_multiply_accumulate():
    """The reference's matrix form of the stitch equals the direct statement: every tile times its
    2-D weight window accumulated into a zeroed canvas; a constant comes back as itself."""
    S, G, O = 28, 3, 5
    tables = TR.plan(S, G, O)
    C, step = TR.canvas_side(S, G, O), S - O
    rng = np.random.default_rng(3)
    tiles = rng.uniform(0, 4, (2 * G * G, S, S)).astype(np.float32)
    want = np.zeros((2, C, C))
    w1 = np.array([[TR.ramp(S, G, O, i, u) for u in range(S)] for i in range(G)], np.float32).astype(np.float64)
    for b in range(2):
        for ty in range(G):
            for tx in range(G):
                want[b, ty * step:ty * step + S, tx * step:tx * step + S] += \
                    np.outer(w1[ty], w1[tx]) * tiles[b * G * G + ty * G + tx]
    assert np.abs(TR.stitch(tiles, S, G, O, tables) - want).max() <= 1e-13
    const = TR.stitch(np.full((G * G, S, S), 2.5, np.float32), S, G, O, tables,
                      np.full((1, S, S), 2.5, np.float32), 0.3)
    assert np.abs(const - 2.5).max() <= 2.5 * 2.0 ** -22
    canvas = rng.standard_normal((2, 3, C, C)).astype(np.float32)
    t = TR.gather(canvas, S, G, O)
    assert t.shape == (2 * G * G, 3, S, S) and np.array_equal(t[G * G + G + 2], canvas[1, :, step:step + S, 2 * step:])


def test_header_binding_table_and_library_agree():
    names = ["aaclip_tile_plan", "aaclip_tile_gather", "aaclip_tile_stitch", "aaclip_tile_score"]
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name in names:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name]), name
        for p, ct in zip(params, _lib.SIGNATURES[name]):
            want = ctypes.c_void_p if "*" in p else {"int": ctypes.c_int, "int64_t": ctypes.c_int64,
                                                     "float": ctypes.c_float}[p.split()[0]]
            assert ct is want, (name, p)
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9
    makefile = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "Makefile")).read()
    assert "tiles.hip" in re.search(r"^SRCS := (.*)$", makefile, flags=re.M).group(1).split()


def test_parse_args_tiling_flags(capsys):
    import test as harness
    off = harness.parse_args([])
    assert off.tile_grid == 1 and off.tile_overlap == 518 // 4 and off.tile_global_weight == 0.5
    on = harness.parse_args(["--img_size", "70", "--tile_grid", "2"])
    assert on.tile_grid == 2 and on.tile_overlap == 17 and on.tile_global_weight == 0.5
    assert harness.parse_args(["--img_size", "70", "--tile_grid", "3", "--tile_overlap", "35"]).tile_overlap == 35
    assert harness.parse_args(["--img_size", "70", "--tile_grid", "3", "--tile_overlap", "0"]).tile_overlap == 0
    for bad in (["--tile_grid", "2", "--few_shot"], ["--img_size", "70", "--tile_grid", "2", "--tile_overlap", "36"],
                ["--img_size", "70", "--tile_grid", "2", "--tile_overlap", "-1"], ["--tile_grid", "9"],
                ["--tile_grid", "0"], ["--tile_grid", "2", "--tile_global_weight", "1.0"],
                ["--tile_grid", "2", "--tile_global_weight", "-0.25"]):
        with pytest.raises(SystemExit) as exc:
            harness.parse_args(bad)
        assert exc.value.code == 2, bad
    capsys.readouterr()
    # without the flag --few_shot parses as before, whatever the (unused) overlap
    assert harness.parse_args(["--few_shot"]).tile_grid == 1


def test_get_predictions_empty_loader_gives_canvas_sized_rows():
    """An empty shard still contributes rows of the right shape: C x C with a tiling, img_size
    squared without (CPU stand-in model: nothing is predicted)."""
    import inspect

    import test as harness

    class Model:
        def predict(self, *a, **k):
            raise AssertionError("nothing to predict")
        predict_tiled = predict

    sig = inspect.signature(harness.get_predictions).parameters
    assert sig["tiling"].default is None and sig["global_prep"].default is None
    assert inspect.signature(harness._device_batch).parameters["views"].default is None
    tiling = {"grid": 2, "overlap": 8, "canvas": 48, "global_weight": 0.5}
    masks, labels, preds, scores, names = harness.get_predictions(Model(), None, [], torch.device("cpu"), 28,
                                                                  dataset="synthetic", tiling=tiling)
    assert tuple(masks.shape) == (0, 1, 48, 48) and masks.dtype == torch.uint8
    assert tuple(preds.shape) == (0, 48, 48) and tuple(scores.shape) == (0,) and labels.shape == (0,) and names == []
    masks, _, preds, _, _ = harness.get_predictions(Model(), None, [], torch.device("cpu"), 28, dataset="synthetic")
    assert tuple(masks.shape) == (0, 1, 28, 28) and tuple(preds.shape) == (0, 28, 28)


def test_get_predictions_tiled_batches_on_the_cpu_stand_in():
    """The harness hands predict_tiled the canvas batch, the pooled global view at img_size and the
    tiling's numbers (CPU stand-in; the synthetic items are built at the canvas size)."""
    import test as harness
    from dataset import get_dataset
    seen = []

    class Model:
        def predict_tiled(self, canvas, T, grid, overlap, domain, global_view=None, global_weight=0.5, streams=1,
                          tile_batch=32):
            seen.append((tuple(canvas.shape), tuple(global_view.shape), grid, overlap, global_weight, tile_batch))
            assert torch.equal(global_view, torch.nn.functional.adaptive_avg_pool2d(canvas, 28))
            return canvas.mean(1), canvas.mean((1, 2, 3))

    tiling = {"grid": 2, "overlap": 8, "canvas": 48, "global_weight": 0.25}
    ds = get_dataset("synthetic", 48, None, -1, "test", synthetic_n=5)["bottle"]
    loader = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False)
    masks, labels, preds, scores, names = harness.get_predictions(Model(), None, loader, torch.device("cpu"), 28,
                                                                  dataset="synthetic", tiling=tiling, tile_batch=6)
    assert seen == [((3, 3, 48, 48), (3, 3, 28, 28), 2, 8, 0.25, 6), ((2, 3, 48, 48), (2, 3, 28, 28), 2, 8, 0.25, 6)]
    assert tuple(masks.shape) == (5, 1, 48, 48) and tuple(preds.shape) == (5, 48, 48) and len(names) == 5
