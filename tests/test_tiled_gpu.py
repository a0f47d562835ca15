"""Tiled inference on the device (csrc/tiles.hip, VisualEngine.predict_tiled, test.py --tile_grid)
against tests/tiled_ref.py, the float64 statement of the same tables.

The stitch bound, 16 * 2^-24 * max(|tile|, |global|): two roundings per weighted term and three
additions per four-term sum give 5 u (u = 2^-24) for the tile sum and for the bilinear alike, the
blend adds three roundings, so 8 u * max to first order; the bound doubles that for the second-order
terms and for weight sums an ulp above 1."""
import json
import os

import numpy as np
import pytest
import torch

import tiled_ref as TR
from aaclip import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(28, 2, 8), (28, 2, 14), (28, 3, 5), (28, 2, 0), (70, 3, 35), (42, 4, 1), (518, 2, 129)]


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------- gather
@pytest.mark.parametrize("G,O", [(2, 0), (2, 5), (3, 14)])
def test_gather_is_torch_slicing(dev, G, O):
    B, S = 3, 28
    C, step = TR.canvas_side(S, G, O), S - O
    canvas = torch.randn(B, 3, C, C, device=dev, generator=torch.Generator(dev).manual_seed(G * 100 + O))
    want = torch.stack([canvas[b, :, ty * step:ty * step + S, tx * step:tx * step + S]
                        for b in range(B) for ty in range(G) for tx in range(G)])
    got = ops.tile_gather(canvas, G, O)
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    n = G * G
    assert torch.equal(ops.tile_gather(canvas, G, O, images=(1, 3)), want[n:3 * n])
    assert torch.equal(ops.tile_gather(canvas, G, O, images=(2, 3)), want[2 * n:])
    assert torch.equal(ops.tile_gather(canvas, G, O, tiles=(3, n + 2)), want[3:n + 2])  # a chunk across two images
    assert torch.equal(ops.tile_gather(canvas, G, O, tiles=(3 * n - 1, 3 * n)), want[-1:])
    # an output that is only 4-byte aligned takes the float path, with a guard float on either side
    k = 2 * 3 * S * S
    buf = torch.full((k + 2,), 7.0, device=dev)
    ops.tile_gather(canvas, G, O, tiles=(1, 3), out=buf[1:-1].view(2, 3, S, S))
    assert torch.equal(buf[1:-1].view(2, 3, S, S), want[1:3]) and buf[0] == 7.0 and buf[-1] == 7.0
    with pytest.raises(ValueError, match="lie outside"):
        ops.tile_gather(canvas, G, O, images=(2, 4))
    with pytest.raises(ValueError, match="not 2 x 2 tiles"):
        ops.tile_gather(torch.zeros(1, 3, 49, 49, device=dev), 2, 8)


# ---------------------------------------------------------------------------- stitch
@pytest.fixture(scope="module")
def operands():
    """Per shape the random maps in [0, 4) (tile maps, global maps) and the float32 tables, made once."""
    out = {}
    for S, G, O in SHAPES:
        B = 1 if S == 518 else 2
        rng = np.random.default_rng(S * 1000 + G * 100 + O)
        out[S, G, O] = (rng.uniform(0, 4, (B * G * G, S, S)).astype(np.float32),
                        rng.uniform(0, 4, (B, S, S)).astype(np.float32), TR.plan(S, G, O))
    return out


@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.3])
@pytest.mark.parametrize("S,G,O", SHAPES)
def test_stitch_against_float64(dev, operands, S, G, O, alpha):
    tiles, glob, tables = operands[S, G, O]
    want = TR.stitch(tiles, S, G, O, tables, glob, alpha)
    got = ops.tile_stitch(_dev(tiles, dev), G, O, global_maps=_dev(glob, dev) if alpha else None, global_weight=alpha)
    C = TR.canvas_side(S, G, O)
    assert tuple(got.shape) == (tiles.shape[0] // (G * G), C, C) and got.dtype == torch.float32
    err = np.abs(got.double().cpu().numpy() - want).max()
    top = max(float(tiles.max()), float(glob.max()) if alpha else 0.0)
    print(f"stitch S {S} G {G} O {O} a {alpha}: max abs err {err:.3e} = {err / (U * top):.2f} u max (bound 16)")
    assert err <= 16 * U * top
    again = ops.tile_stitch(_dev(tiles, dev), G, O, global_maps=_dev(glob, dev) if alpha else None,
                            global_weight=alpha)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))  # one writer, one order


@pytest.mark.parametrize("S,G,O", [(28, 3, 5), (42, 4, 1), (28, 2, 0)])
def test_stitch_into_an_output_that_is_only_4_byte_aligned(dev, operands, S, G, O):
    """The row groups follow the output's own address: shifted by one float, every row's head and
    tail change, the values do not, and nothing outside the output is written."""
    tiles, glob, _ = operands[S, G, O]
    t, g = _dev(tiles, dev), _dev(glob, dev)
    want = ops.tile_stitch(t, G, O, global_maps=g, global_weight=0.3)
    for shift in (1, 2, 3):
        buf = torch.full((want.numel() + 8,), -5.0, device=dev)
        out = buf[shift:shift + want.numel()].view(want.shape)
        ops.tile_stitch(t, G, O, global_maps=g, global_weight=0.3, out=out)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), shift
        assert (buf[:shift] == -5.0).all() and (buf[shift + want.numel():] == -5.0).all()


@pytest.mark.parametrize("S,G,O,alpha", [(28, 2, 8, 0.0), (28, 3, 4, 0.0), (32, 2, 0, 0.5)])
def test_stitch_exact_cases(dev, S, G, O, alpha):
    """Integer-valued maps: with dyadic ramps (O a power of two), and with lambda in {0.25, 0.75}
    and a = 0.5 (C = 2 S), every product and sum is exact in fp32, so the bits are float64's."""
    rng = np.random.default_rng(S + G + O)
    B = 2
    tiles = rng.integers(0, 64, (B * G * G, S, S)).astype(np.float32)
    glob = rng.integers(0, 64, (B, S, S)).astype(np.float32)
    tables = TR.plan(S, G, O)
    if alpha:
        assert set(np.unique(tables[1][:, 3])) <= {0.0, 0.25, 0.75}
    want = TR.stitch(tiles, S, G, O, tables, glob, alpha)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    got = ops.tile_stitch(_dev(tiles, dev), G, O, global_maps=_dev(glob, dev) if alpha else None, global_weight=alpha)
    assert np.array_equal(got.double().cpu().numpy(), want)


@pytest.mark.parametrize("S,G,O", [(28, 2, 14), (28, 3, 5), (70, 3, 35)])
def test_stitch_of_constant_maps_is_the_constant(dev, S, G, O):
    for value, alpha in ((2.5, 0.0), (1.7, 0.3), (3.1, 0.5)):
        tiles = torch.full((2 * G * G, S, S), value, device=dev)
        glob = torch.full((2, S, S), value, device=dev)
        got = ops.tile_stitch(tiles, G, O, global_maps=glob if alpha else None, global_weight=alpha)
        err = (got.double() - float(np.float32(value))).abs().max().item()
        assert err <= 16 * U * value, (value, alpha, err)


def test_stitch_and_gather_past_2_to_the_31_bytes(dev):
    """Offsets are 64-bit. With O = 0 and a = 0 the stitch is a pure placement and the gather its
    inverse, so both are checked exactly on the device at sizes whose last image starts beyond
    2^31 bytes: the stitch's output and tile maps (32 images of 4144^2) and the gather's canvas
    and tiles (11 images x 3 channels)."""
    S, G = 518, 8
    C = G * S
    for B, ch in ((32, None), (11, 3)):
        lead = (B,) if ch is None else (B, ch)
        whole = torch.empty(*lead, C, C, device=dev)
        assert whole.numel() * 4 > 2 ** 31
        # distinct over any 2^24 neighbours, and a slip of 2^31 bytes changes the value (2^29 % 16777213 = 96)
        whole.view(-1).copy_(torch.arange(whole.numel(), device=dev, dtype=torch.int32).remainder_(16777213))
        if ch is None:
            tiles = whole.view(B, G, S, G, S).permute(0, 1, 3, 2, 4).contiguous().view(B * G * G, S, S)
            got = ops.tile_stitch(tiles, G, 0)
        else:
            tiles = ops.tile_gather(whole, G, 0)
            got = tiles.view(B, G, G, ch, S, S).permute(0, 3, 1, 4, 2, 5).contiguous().view(B, ch, C, C)
        assert torch.equal(got.view(torch.int32), whole.view(torch.int32))
        del whole, tiles, got
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------- score
@pytest.mark.parametrize("G", [2, 3, 8])
def test_score(dev, G):
    rng = np.random.default_rng(G)
    B = 300  # more than one block
    s = rng.uniform(-1, 3, B * G * G).astype(np.float32)
    g = rng.uniform(-1, 3, B).astype(np.float32)
    got = ops.tile_score(_dev(s, dev), G)
    assert np.array_equal(got.double().cpu().numpy(), TR.score(s, G))
    for alpha in (0.5, 0.3):
        got = ops.tile_score(_dev(s, dev), G, global_scores=_dev(g, dev), global_weight=alpha)
        err = np.abs(got.double().cpu().numpy() - TR.score(s, G, g, alpha)).max()
        assert err <= 4 * U * max(np.abs(s).max(), np.abs(g).max()), (alpha, err)
    with pytest.raises(ValueError, match="needs the global"):
        ops.tile_score(_dev(s, dev), G, global_weight=0.5)


# ---------------------------------------------------------------------------- engine
S_E, G_E, O_E = 70, 2, 14
C_E = TR.canvas_side(S_E, G_E, O_E)


@pytest.fixture(scope="module")
def engine(dev):
    from aaclip.engine import VisualEngine
    from oracle import synth
    sd = synth.clip_state_dict(111, S_E)
    ia, _ = synth.adapter_state_dicts(111)
    vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
    eng = VisualEngine(vp, {k: torch.from_numpy(v).to(dev) for k, v in ia.items()}, dtype=torch.float16)
    T = np.linalg.qr(np.random.default_rng(0).standard_normal((768, 2)))[0].astype(np.float32)
    gen = torch.Generator(dev).manual_seed(5)
    canvas = torch.randn(3, 3, C_E, C_E, device=dev, generator=gen)
    view = torch.nn.functional.adaptive_avg_pool2d(canvas, S_E).contiguous()
    return eng, torch.from_numpy(T).to(dev), canvas, view


def test_engine_equals_the_reference_on_its_own_predictions(dev, engine):
    eng, T, canvas, view = engine
    step = S_E - O_E
    tiles = torch.stack([canvas[b, :, ty * step:ty * step + S_E, tx * step:tx * step + S_E]
                         for b in range(3) for ty in range(G_E) for tx in range(G_E)]).contiguous()
    tm, ts = (t.clone() for t in eng.predict(tiles, T, "Industrial"))
    gm, gs = (t.clone() for t in eng.predict(view, T, "Industrial"))
    tables = TR.plan(S_E, G_E, O_E)
    top = max(tm.abs().max().item(), gm.abs().max().item())
    for alpha in (0.5, 0.3):
        pm, ps = eng.predict_tiled(canvas, T, G_E, O_E, global_view=view, global_weight=alpha)
        assert tuple(pm.shape) == (3, C_E, C_E) and tuple(ps.shape) == (3,)
        want = TR.stitch(tm.cpu().numpy(), S_E, G_E, O_E, tables, gm.cpu().numpy(), alpha)
        err = np.abs(pm.double().cpu().numpy() - want).max()
        print(f"engine a {alpha}: map max abs err {err:.3e} = {err / (U * top):.2f} u max")
        assert err <= 16 * U * top
        serr = np.abs(ps.double().cpu().numpy() - TR.score(ts.cpu().numpy(), G_E, gs.cpu().numpy(), alpha)).max()
        assert serr <= 4 * U * max(ts.abs().max().item(), gs.abs().max().item())
    # global_weight 0: the stitch of the tiles alone, whatever the global view holds (none is needed)
    calls = []
    inner = eng.predict_cached
    eng.predict_cached = lambda x, *a, **k: (calls.append(x.shape[0]), inner(x, *a, **k))[1]
    try:
        pm0, ps0 = eng.predict_tiled(canvas, T, G_E, O_E, global_weight=0.0)
    finally:
        del eng.predict_cached
    assert calls == [12]  # the tiles in one call, no global forward
    assert torch.equal(pm0, ops.tile_stitch(tm, G_E, O_E)) and torch.equal(ps0, ops.tile_score(ts, G_E))
    assert np.array_equal(ps0.double().cpu().numpy(), TR.score(ts.cpu().numpy(), G_E))


def test_engine_bits_do_not_depend_on_batch_chunking_or_streams(dev, engine):
    eng, T, canvas, view = engine
    base_map, base_score = eng.predict_tiled(canvas, T, G_E, O_E, global_view=view)
    variants = [dict(tile_batch=4), dict(tile_batch=5), dict(tile_batch=12), dict(streams=2),
                dict(tile_batch=5, streams=2)]
    for kw in variants:
        m, s = eng.predict_tiled(canvas, T, G_E, O_E, global_view=view, **kw)
        assert m.data_ptr() != base_map.data_ptr()  # fresh tensors
        assert torch.equal(m.view(torch.int32), base_map.view(torch.int32)), kw
        assert torch.equal(s.view(torch.int32), base_score.view(torch.int32)), kw
    for kw in (dict(), dict(tile_batch=4), dict(streams=2)):
        m1, s1 = eng.predict_tiled(canvas[:1], T, G_E, O_E, global_view=view[:1], **kw)
        assert torch.equal(m1.view(torch.int32), base_map[:1].view(torch.int32)), kw
        assert torch.equal(s1.view(torch.int32), base_score[:1].view(torch.int32)), kw


def test_engine_argument_errors(dev, engine):
    eng, T, canvas, view = engine
    with pytest.raises(ValueError, match="positional embedding"):  # 2 x 2 tiles of 84 px: another tower size
        eng.predict_tiled(torch.zeros(1, 3, 154, 154, device=dev), T, G_E, O_E, global_weight=0.0)
    with pytest.raises(ValueError, match="not 2 x 2 tiles"):  # no integer tile side
        eng.predict_tiled(torch.zeros(1, 3, 127, 127, device=dev), T, G_E, O_E, global_weight=0.0)
    with pytest.raises(ValueError, match="no multiple of 14"):
        eng.predict_tiled(torch.zeros(1, 3, 128, 128, device=dev), T, G_E, O_E, global_weight=0.0)
    with pytest.raises(ValueError, match="needs global_view"):
        eng.predict_tiled(canvas, T, G_E, O_E)
    with pytest.raises(ValueError, match="needs global_view"):
        eng.predict_tiled(canvas, T, G_E, O_E, global_view=view[:2])
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        eng.predict_tiled(canvas, T, G_E, O_E, global_view=view, global_weight=1.0)


# ---------------------------------------------------------------------------- CLI
def test_harness_tiled_run(dev, tmp_path):
    import test as harness
    path = tmp_path / "table.json"
    base = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4", "--f1",
            "--regions", "--pro", "--save_path", str(tmp_path), "--results_json", str(path)]
    df, ctx = harness.run(harness.parse_args(base + ["--tile_grid", "2", "--tile_overlap", "14"]))
    tiling = {"grid": 2, "overlap": 14, "canvas": 126, "global_weight": 0.5}
    assert ctx["tiling"] == tiling
    masks, labels, preds, preds_image = ctx["classes"]["bottle"]
    assert tuple(preds.shape) == (4, 126, 126) and tuple(masks.shape) == (4, 1, 126, 126)
    assert tuple(preds_image.shape) == (4,) and torch.isfinite(preds).all() and torch.isfinite(preds_image).all()
    assert "pixel AUPRO" in df.columns and "pixel F1-max" in df.columns
    assert np.isfinite(df.drop(columns=["class name"]).to_numpy(dtype=np.float64)).all()
    table = json.loads(path.read_text())
    assert table["tiling"] == tiling and len(table["rows"]) == 2
    found = ctx["regions"]["bottle"]["images"]
    assert len(found) == 4 and sum(e["n_regions"] for e in found) > 0
    for e in found:
        for r in e["regions"]:
            x0, y0, x1, y1 = r["bbox"]
            assert 0 <= x0 <= x1 < 126 and 0 <= y0 <= y1 < 126
    # the harness's maps are the model's: the same canvas batch and pooled global view through predict_tiled
    from dataset import get_dataset
    ds = get_dataset("synthetic", 126, None, -1, "test", synthetic_n=4)["bottle"]
    canvas = torch.stack([ds[i]["image"] for i in range(4)]).to(dev)
    m, s = ctx["model"].predict_tiled(canvas, ctx["text_embeddings"]["bottle"], 2, 14, "Industrial",
                                      global_view=torch.nn.functional.adaptive_avg_pool2d(canvas, 70),
                                      global_weight=0.5, tile_batch=32)
    assert torch.equal(m, preds) and torch.equal(s, preds_image)
    # without the flag the JSON has no "tiling" and the maps are img_size squared
    df1, ctx1 = harness.run(harness.parse_args(base))
    assert "tiling" not in json.loads(path.read_text()) and "tiling" not in ctx1
    assert tuple(ctx1["classes"]["bottle"][2].shape) == (4, 70, 70)


def test_harness_tiled_visualize_writes_its_files(dev, tmp_path):
    import test as harness
    from PIL import Image
    harness.run(harness.parse_args(["--dataset", "synthetic", "--allow_random_init", "--img_size", "70",
                                    "--synthetic_n", "2", "--tile_grid", "2", "--tile_overlap", "14",
                                    "--tile_global_weight", "0", "--visualize", "--save_path", str(tmp_path)]))
    files = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f.endswith(".png")]
    assert len(files) == 2
    for f in files:
        with Image.open(f) as im:
            assert im.size == (126, 3 * 126)
