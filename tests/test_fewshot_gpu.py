"""Few-shot memory-bank scoring on the MI355X (csrc/bank.hip: aaclip_bank_nn, aaclip_bank_distance,
aaclip_fewshot_fuse; VisualEngine.build_bank / predict_few_shot; test.py --few_shot) against the numpy
statement of tests/fewshot_ref.py.

The bound of the search, BOUND = 768 * 2^-23, is worked out, not measured: products of 16-bit
operands are exact in fp32; the fp32 accumulation of a 768-term dot product errs by at most
768 u sum|a_i b_i| <= 768 u for unit rows, with u = 2^-23 to allow truncating adds inside the MFMA;
a maximum moves by no more than its worst term. (fp32 operands: each product is rounded as part of a
fused multiply-add, which the same count covers.)"""
import functools

import numpy as np
import pytest
import torch

from aaclip import ops

import fewshot_ref as FR

pytestmark = pytest.mark.gpu

K = 768
TM, TN = ops.BANK_TM, ops.BANK_TN
BOUND = K * 2.0 ** -23
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
M_EDGES = (1, TM - 1, TM + 1)
NB_EDGES = (1, TN - 1, TN + 1, 3 * TN + 1)  # the last: four splits, the fourth one ragged row


def _unit(rng, n):
    x = rng.standard_normal((n, K))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _rounded(x, dtype, dev):
    """x on the device in dtype, and the same rounded values back as float64."""
    t = torch.from_numpy(np.asarray(x, np.float32)).to(dev).to(dtype)
    return t, t.double().cpu().numpy()


def _sims(part):
    """The rows' results: the maximum over the splits (exact), as float64 numpy."""
    return part.max(dim=1).values.double().cpu().numpy()


def _split_rows(M, Nb):
    n_splits, tiles_per_split = ops.bank_nn_plan(M, Nb)
    return n_splits, tiles_per_split * TN


@functools.lru_cache(maxsize=None)
def _edge_case(dtype):
    """One Q and one bank of random unit rows per dtype, rounded to it, and their full float64
    similarity matrix, computed once: every edge shape is a corner of it."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    q, q64 = _rounded(_unit(rng, max(M_EDGES)), dtype, dev)
    r, r64 = _rounded(_unit(rng, max(NB_EDGES)), dtype, dev)
    sims = np.stack([(q64[m][None, :] * r64).sum(axis=-1) for m in range(q64.shape[0])])
    return q, r, sims


# ---------------------------------------------------------------------------- 1. designed, exact
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("seed", [0, 1])
def test_designed_operands_are_exact(dev, dtype, seed):
    """Entries 0 or +-2^-k (k <= 3) with at most 8 non-zeros per row: every product and every partial
    sum is a small dyadic number, exact in fp32 in any order, so the device equals float64 bit for bit."""
    rng = np.random.default_rng(seed)
    M, Nb = TM + 1, 2 * TN + 3
    hot = rng.choice(K, 32, replace=False)  # the non-zeros share 32 columns, so rows do meet

    def rows(n):
        x = np.zeros((n, K))
        for i in range(n):
            cols = rng.choice(hot, rng.integers(1, 9), replace=False)
            x[i, cols] = rng.choice([-1.0, 1.0], cols.size) * 2.0 ** -rng.integers(0, 4, cols.size)
        return x
    xq, xr = rows(M), rows(Nb)
    (q, q64), (r, r64) = _rounded(xq, dtype, dev), _rounded(xr, dtype, dev)
    assert np.array_equal(q64, xq) and np.array_equal(r64, xr)  # representable in every dtype
    part = ops.bank_nn(q, r)
    n_splits, rows_per_split = _split_rows(M, Nb)
    assert n_splits == 3 and part.shape == (M, 3) and part.dtype == torch.float32
    want = FR.bank_nn_parts(q64, r64, n_splits, rows_per_split)
    assert len(np.unique(want)) > 8  # not a trivial case
    assert np.array_equal(part.double().cpu().numpy(), want)
    assert np.array_equal(_sims(part), FR.bank_nn(q64, r64))


# ---------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_edges_random_unit_rows(dev, dtype, strided):
    q_all, r_all, sims = _edge_case(dtype)
    worst = 0.0
    for M in M_EDGES:
        for Nb in NB_EDGES:
            q, r = q_all[:M], r_all[:Nb]
            if strided:  # q a level's columns of a [M, 5 * 768] segbuf-like buffer, the bank likewise in 2 * 768
                qb = torch.full((M, 5 * K), 100.0, device=dev, dtype=dtype)
                rb = torch.full((Nb, 2 * K), 100.0, device=dev, dtype=dtype)
                qb[:, K:2 * K], rb[:, K:] = q, r
                q, r = qb[:, K:2 * K], rb[:, K:]
                assert q.stride(0) == 5 * K and r.stride(0) == 2 * K
            part = ops.bank_nn(q, r)
            n_splits, rows_per_split = _split_rows(M, Nb)
            assert part.shape == (M, n_splits) and (Nb != 3 * TN + 1 or n_splits >= 3)
            want = np.stack([sims[:M, s * rows_per_split:min((s + 1) * rows_per_split, Nb)].max(axis=1)
                             for s in range(n_splits)], axis=1)
            err = np.abs(part.double().cpu().numpy() - want).max()
            worst = max(worst, err)
            assert err <= BOUND, (M, Nb, err)
            assert np.abs(_sims(part) - sims[:M, :Nb].max(axis=1)).max() <= BOUND
    print(dtype, "strided" if strided else "dense", "largest |device - float64|", worst, "bound", BOUND)


# ---------------------------------------------------------------------------- 3. the winner in every place
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_winner_in_every_place(dev, dtype):
    rng = np.random.default_rng(11)
    M, Nb = 3, 3 * TN + 1
    n_splits, rows_per_split = _split_rows(M, Nb)
    assert n_splits == 4 and rows_per_split == TN
    q, q64 = _rounded(_unit(rng, M), dtype, dev)
    base = _unit(rng, Nb)
    norm2 = float((q64[1] * q64[1]).sum())
    places = {0: 0, rows_per_split - 1: 0, (n_splits - 1) * rows_per_split: n_splits - 1, Nb - 1: n_splits - 1}
    assert (n_splits - 1) * rows_per_split == Nb - 1  # the last split is the one ragged row
    places[2 * rows_per_split] = 2
    for index, split in places.items():
        r, _ = _rounded(base, dtype, dev)
        r[index] = q[1]
        part = ops.bank_nn(q, r)
        got = part.double().cpu().numpy()
        assert abs(got[1].max() - norm2) <= BOUND, (index, got[1], norm2)
        assert int(got[1].argmax()) == split and got[1].max() > 0.9, (index, got[1])
        others = np.delete(got[1], split)
        assert (others < 0.5).all(), (index, got[1])  # the planted row is seen by its own split alone


# ---------------------------------------------------------------------------- 4. all similarities negative
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_all_negative_similarities(dev, dtype):
    """Bank = -Q plus noise, Q's rows around one direction: every similarity is negative. A kernel
    that padded the ragged tiles with zero rows would return 0 (here: Nb = TN + 1, the second split
    is one row and TN - 1 rows of padding)."""
    rng = np.random.default_rng(13)
    M, Nb = TM + 1, TN + 1
    x = _unit(rng, 1) + 0.5 * _unit(rng, M)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    b = -x[:Nb] + 0.01 * rng.standard_normal((Nb, K))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    (q, q64), (r, r64) = _rounded(x, dtype, dev), _rounded(b, dtype, dev)
    n_splits, rows_per_split = _split_rows(M, Nb)
    assert n_splits == 2
    part = ops.bank_nn(q, r)
    want = FR.bank_nn_parts(q64, r64, n_splits, rows_per_split)
    assert (want < -0.3).all()
    got = part.double().cpu().numpy()
    assert (got < 0).all()
    assert np.abs(got - want).max() <= BOUND


# ---------------------------------------------------------------------------- 5. same bits
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_same_bits(dev, dtype):
    q_all, r_all, _ = _edge_case(dtype)
    q, r = q_all[:TM + 1], r_all[:3 * TN + 1]
    ref = ops.bank_nn(q, r).max(dim=1).values
    for m in (0, 77, TM):  # a row alone against the same row in the batch (TM: the second row tile)
        alone = ops.bank_nn(q[m:m + 1].clone(), r).max(dim=1).values
        assert torch.equal(alone, ref[m:m + 1]), m
    perm = torch.from_numpy(np.random.default_rng(3).permutation(r.shape[0])).to(dev)
    assert torch.equal(ops.bank_nn(q, r[perm].contiguous()).max(dim=1).values, ref)  # any order of the bank
    assert torch.equal(ops.bank_nn(q, r[:TN + 5]).max(dim=1).values,
                       ops.bank_nn(q, r[:TN + 5].flip(0).contiguous()).max(dim=1).values)
    a, b = ops.bank_nn(q, r), ops.bank_nn(q, r)  # back to back
    assert torch.equal(a, b) and torch.equal(a.max(dim=1).values, ref)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = ops.bank_nn(q, r)
    side.synchronize()
    assert torch.equal(c, a)
    part = torch.full_like(a, 7.0)  # a caller-owned workspace is fully overwritten
    assert ops.bank_nn(q, r, part) is part and torch.equal(part, a)


# ---------------------------------------------------------------------------- 6. bank_distance
def test_bank_distance_accumulates_levels_into_the_grid(dev):
    """Two levels, accumulate off then on; part values are multiples of 2^-10 in [-1, 1], so the fp32
    1 - max and the level sum are exact and the grid equals the float64 reference bit for bit."""
    rng = np.random.default_rng(5)
    B, g, n_splits = 3, 5, 3
    M = B * g * g
    parts = [rng.integers(-1024, 1025, (M, n_splits)) / 1024.0 for _ in range(2)]
    grid = torch.full((B, 1, g, g), 1.0e9, device=dev)  # what was there is not read on the first level
    for level, p in enumerate(parts):
        out = ops.bank_distance(torch.from_numpy(p.astype(np.float32)).to(dev), grid, accumulate=level > 0)
        assert out is grid
    want = FR.bank_distance([p.max(axis=1) for p in parts]).reshape(B, 1, g, g)
    assert np.array_equal(grid.double().cpu().numpy(), want)
    for b in range(B):
        for p in (0, 7, g * g - 1):  # row m = b * P + p lands at grid[b][0][p]
            assert grid[b, 0, p // g, p % g].item() == want.reshape(-1)[b * g * g + p]
    one = torch.from_numpy(parts[0][:, :1].astype(np.float32)).contiguous().to(dev)  # a single split
    assert np.array_equal(ops.bank_distance(one, torch.empty(M, device=dev), accumulate=False).double().cpu().numpy(),
                          1.0 - parts[0][:, 0])


# ---------------------------------------------------------------------------- 7. fewshot_fuse
@pytest.mark.parametrize("case", ["random", "constant few-shot", "all constant"])
def test_fuse_equals_the_float32_reference(dev, case):
    rng = np.random.default_rng(17)
    n, S = 3, 70
    zs = rng.uniform(0.02, 0.9, (n, S, S)).astype(np.float32)
    fs = rng.uniform(-1e-4, 3.5, (n, S, S)).astype(np.float32)
    score = rng.uniform(0.1, 0.8, n).astype(np.float32)
    if case != "random":
        fs[:] = np.float32(0.37)
    if case == "all constant":
        zs[:], score[:] = np.float32(0.5), np.float32(0.25)
    got = ops.fewshot_fuse(*(torch.from_numpy(a).to(dev) for a in (zs, fs, score)))
    want = FR.fewshot_fuse(zs, fs, score)
    for g_, w, name in zip(got, want, ("fused_map", "fs_score", "fused_score")):
        g_ = g_.cpu().numpy()
        assert g_.shape == w.shape and g_.dtype == np.float32 and np.isfinite(g_).all(), name
        assert np.array_equal(g_, w), (name, np.abs(g_ - w).max())
    if case == "all constant":
        assert not got[0].any() and not got[2].any()  # constant inputs contribute 0, not NaN
    if case == "random":
        assert float(got[0].max()) > 1.0 and float(got[2].max()) <= 2.0


# ---------------------------------------------------------------------------- 8-10. end to end
ARGS = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4"]


@pytest.fixture(scope="module", params=["fp16", "fp32"])
def harness_runs(request, tmp_path_factory, dev):
    """One --few_shot run and one plain run of the harness per compute dtype, shared by the tests below."""
    import test as harness
    dt = request.param
    save = str(tmp_path_factory.mktemp("fewshot_" + dt))
    few = harness.run(harness.parse_args(ARGS + ["--few_shot", "--shot", "2", "--compute_dtype", dt,
                                                 "--save_path", save]))
    plain = harness.run(harness.parse_args(ARGS + ["--shot", "2", "--compute_dtype", dt, "--save_path", save]))
    return dt, few, plain


def _images(stage, shot=2):
    from dataset import get_dataset
    ds = get_dataset("synthetic", 70, None, shot, stage, synthetic_n=4)["bottle"]
    return torch.stack([ds[i]["image"] for i in range(len(ds))])


def test_harness_few_shot_end_to_end(dev, harness_runs):
    dt, (df, ctx), (plain_df, plain_ctx) = harness_runs
    assert len(df) == 2 and np.isfinite(df.drop(columns=["class name"]).to_numpy(dtype=np.float64)).all()
    model, T = ctx["model"], ctx["text_embeddings"]["bottle"]
    eng = model.visual_engine()
    parts = ctx["few_shot"]["bottle"]
    assert set(parts) >= {"zs_map", "fs_map", "fused_map", "fused_score"}
    x = _images("test").to(dev)
    bank = model.build_memory_bank(_images("support").to(dev))
    L, P = len(eng.levels), 25
    want_dtype = torch.float32 if dt == "fp32" else torch.float16
    assert bank.dtype == want_dtype and bank.img_size == 70 and len(bank.levels) == L
    assert all(tuple(lv.shape) == (2 * P, K) and lv.dtype == want_dtype for lv in bank.levels)
    rows = eng.bank_rows(x)
    assert all(tuple(r.shape) == (4 * P, K) and r.dtype == want_dtype for r in rows)
    norms = torch.stack([r.double().norm(dim=1) for r in rows])
    assert float((norms - 1).abs().max()) < 2.0 ** -10  # unit rows, to the search dtype's rounding
    # the few-shot map: the float64 grid of the same rounded rows through the device blur
    grid = FR.fewshot_grid([r.double().cpu().numpy() for r in rows],
                           [b.double().cpu().numpy() for b in bank.levels], 4, 5)
    want = ops.blur_upsample(torch.from_numpy(grid.astype(np.float32)).to(dev), torch.empty(4, 1, 70, 70, device=dev),
                             ksize=7, sigma=1.0)[:, 0]
    err = float((parts["fs_map"] - want).abs().max())
    print(dt, "fs_map largest |device - reference|", err, "bound", L * BOUND + 1e-5)
    assert parts["fs_map"].shape == (4, 70, 70) and err <= L * BOUND + 1e-5
    # the fusion: bit-equal to the float32 reference on the device's own maps and scores
    fm, fsc, fus = FR.fewshot_fuse(parts["zs_map"].cpu().numpy(), parts["fs_map"].cpu().numpy(),
                                   parts["zs_score"].cpu().numpy())
    assert np.array_equal(parts["fused_map"].cpu().numpy(), fm)
    assert np.array_equal(parts["fs_score"].cpu().numpy(), fsc)
    assert np.array_equal(parts["fused_score"].cpu().numpy(), fus)
    masks, labels, preds, preds_image = ctx["classes"]["bottle"]
    assert torch.equal(preds, parts["fused_map"]) and torch.equal(preds_image, parts["fused_score"])
    # the zero-shot half is predict()'s map and score, from rows instead of partials in the 16-bit modes
    zs_map, zs_score = (t.clone() for t in eng.predict(x, T, "Industrial"))
    # (fp32: the same launches, bit for bit; 16-bit: the bounds test_map_partials_gpu.py holds the two forms to)
    if dt == "fp32":
        assert torch.equal(parts["zs_map"], zs_map) and torch.equal(parts["zs_score"], zs_score)
    else:
        assert float((parts["zs_map"] - zs_map).abs().max()) < 2e-5 * max(1.0, float(zs_map.abs().max()))
        torch.testing.assert_close(parts["zs_score"], zs_score, atol=1e-6, rtol=0)
    # without --few_shot nothing changes: no few-shot context, and the class's maps and scores are
    # exactly what predict() gives (--shot accepted and ignored)
    assert "few_shot" not in plain_ctx
    _, _, plain_preds, plain_scores = plain_ctx["classes"]["bottle"]
    pm, ps = (t.clone() for t in plain_ctx["model"].predict(x, plain_ctx["text_embeddings"]["bottle"], "Industrial"))
    assert torch.equal(plain_preds, pm) and torch.equal(plain_scores, ps)
    assert torch.equal(pm, zs_map) and torch.equal(ps, zs_score)  # two harness runs, one seed: the same model
    assert np.isfinite(plain_df.drop(columns=["class name"]).to_numpy(dtype=np.float64)).all()


def test_self_retrieval_is_zero(dev, harness_runs):
    """A bank built from the test images themselves: every patch finds itself. Per level
    |1 - |fp16(f)|^2| <= 2^-10 plus BOUND, and Cauchy-Schwarz caps any other match at the same value;
    four levels; blur and upsample are convex combinations: |fs_map| <= 5e-3."""
    dt, (_, ctx), _ = harness_runs
    model, T = ctx["model"], ctx["text_embeddings"]["bottle"]
    x = _images("test").to(dev)
    bank = model.build_memory_bank(x)
    zs_map, zs_score, fs_map = model.predict_few_shot(x, T, bank, "Industrial")
    worst = float(fs_map.abs().max())
    print(dt, "self-retrieval largest |fs_map|", worst)
    assert fs_map.shape == (4, 70, 70) and worst <= 5e-3
    assert torch.isfinite(zs_map).all() and zs_score.shape == (4,)


def test_mismatched_bank_raises(dev, harness_runs):
    dt, (_, ctx), _ = harness_runs
    model, T = ctx["model"], ctx["text_embeddings"]["bottle"]
    bank = model.build_memory_bank(_images("support").to(dev))
    with pytest.raises(ValueError, match="built at 70 px"):
        model.predict_few_shot(torch.zeros(1, 3, 84, 84, device=dev), T, bank, "Industrial")
    from aaclip.engine import MemoryBank
    other = torch.float16 if dt == "fp32" else torch.float32
    wrong = MemoryBank([lv.to(other) for lv in bank.levels], 70, other, 2)
    with pytest.raises(ValueError, match="rebuild it"):
        model.predict_few_shot(_images("test").to(dev), T, wrong, "Industrial")
    with pytest.raises(ValueError, match="MemoryBank"):
        model.predict_few_shot(_images("test").to(dev), T, bank.levels, "Industrial")
