"""The MX fp8 few-shot search on the MI355X (csrc/rows.hip aaclip_unit_rows_fp8mx, csrc/bank.hip
aaclip_bank_nn_fp8mx; VisualEngine.build_bank(..., float8_e4m3fn) / predict_few_shot; test.py
--few_shot_search fp8) against the numpy statement of tests/fewshot_fp8_ref.py.

The search returns the cosine between the STORED rows, (q^ . r^) * rr * rq with rr, rq the fp32 reciprocal
norms of the stored rows. Its bound against float64 on the read-back operands, relative to a cosine of
magnitude <= 1, is worked out, not measured:

  * the products e4m3 x e4m3 and the power-of-two block scalings are exact in fp32;
  * the fp32 accumulation of the K-term dot product errs by at most K u sum|a_i b_i| <= K u |q^||r^|
    (Cauchy-Schwarz), u = 2^-23 to allow truncating adds inside the MFMA: K 2^-23 of the cosine's scale;
  * a reciprocal norm: the sum of K exact non-negative squares in fp32 is within K 2^-24 relative, the root
    halves that (K 2^-25) and adds 2^-24, the reciprocal adds 2^-24: K 2^-25 + 2^-23, for each of the two;
  * the two multiplies by the norms round once each: 2 x 2^-24;
  * a maximum moves by no more than its worst term.

Sum: (K + 2 K / 4 + 2 + 1) 2^-23 = (1.5 K + 3) 2^-23 to first order. The issue's count is (1.5 K + 4) 2^-23;
the tests use that, the extra 2^-23 standing for the second-order terms (the factors (1 + e) multiply, and
|q^||r^| rr rq is 1 only to the same order). K = 768: 1.378e-4; K = 128: 2.34e-5."""
import functools

import numpy as np
import pytest
import torch

from aaclip import ops

import fewshot_fp8_ref as F8
import fewshot_ref as FR

pytestmark = pytest.mark.gpu

K = 768
TM, TN = ops.BANK_TM, ops.BANK_TN
M_EDGES = (1, TM - 1, TM + 1)
NB_EDGES = (1, TN - 1, TN + 1, 3 * TN + 1)  # the last: four splits, the fourth one ragged row
KS = (128, 768)
FP8 = torch.float8_e4m3fn


def bound(k):
    return (1.5 * k + 4) * 2.0 ** -23


BOUND = bound(K)


def _unit(rng, n, k=K):
    x = rng.standard_normal((n, k))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _dev_rows(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.asarray(x, np.float32)).to(dev).to(dtype)


def _deq(c):
    """The device's stored rows back as float64 numpy: what the search reads."""
    return F8.dequantise(c.q.cpu().numpy(), c.sc.cpu().numpy())


def _take(c, index):
    """The rows `index` (a slice or an index tensor) of an Fp8MxRows as a container of its own."""
    q, rn = c.q[index].contiguous(), c.rnorm[index].contiguous()
    n = q.shape[0]
    sc = torch.zeros(c.sc.shape[0], (n + 1) // 2 * 2, 2, device=q.device, dtype=torch.uint8)
    sc[:, :n] = c.sc[:, :c.shape[0]][:, index]
    return ops.Fp8MxRows(q, sc, rn)


def _strided(c, fill=0x7E):
    """The same rows inside wider buffers full of large values: q a column band of [n, 3 K] bytes (448s
    around it), the scale buffer with six more rows of 2^100."""
    n, k = c.shape
    qb = torch.full((n, 3 * k), fill, device=c.device, dtype=torch.uint8)
    qb[:, k:2 * k] = c.q
    sc = torch.full((c.sc.shape[0], (n + 1) // 2 * 2 + 6, 2), 227, device=c.device, dtype=torch.uint8)
    sc[:, :n] = c.sc[:, :n]
    out = ops.Fp8MxRows(qb[:, k:2 * k], sc, c.rnorm.clone())
    assert out.q.stride(0) == 3 * k
    return out


def _sims(part):
    return part.max(dim=1).values.double().cpu().numpy()


def _split_rows(M, Nb):
    n_splits, tiles_per_split = ops.bank_nn_plan(M, Nb)
    return n_splits, tiles_per_split * TN


def _designed(rng, n, k, hot=None, zero_row=None):
    """Entries 0 or +-2^-j 2^s: one +-1, four +-2^-1 or sixteen +-2^-2, times a power-of-two row scale
    2^s: the sum of squares is 4^s, the unit row and its e4m3 codes are exact."""
    x = np.zeros((n, k))
    for i in range(n):
        if i == zero_row:
            continue
        kind = int(rng.integers(0, 3))
        cols = rng.choice(hot if hot is not None else k, 4 ** kind, replace=False)
        x[i, cols] = rng.choice([-1.0, 1.0], cols.size) * 2.0 ** (-kind + int(rng.integers(-3, 4)))
    return x


# ---------------------------------------------------------------------------- 1. quantiser, designed rows
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("k", KS + (1024, 384))
def test_quantiser_designed_rows_are_exact(dev, dtype, k):
    """Bytes, scale bytes and rnorm equal the numpy statement bit for bit: fp32, bf16 and fp16 inputs, an
    input row stride above K, an all-zero row, widths with a half chunk (128, 384) and whole ones."""
    rng = np.random.default_rng(k)
    n = 41
    x = _designed(rng, n, k, zero_row=17)
    xb = torch.full((n, 2 * k + 8), 100.0, device=dev, dtype=dtype)
    xb[:, 8:8 + k] = _dev_rows(x, dev, dtype)
    xs = xb[:, 8:8 + k]
    assert xs.stride(0) == 2 * k + 8 and np.array_equal(xs.double().cpu().numpy(), x)  # representable
    for src in (xs, xs.contiguous()):
        c = ops.unit_rows_fp8mx(src)
        assert c.dtype == FP8 and tuple(c.shape) == (n, k) and c.q.dtype == torch.uint8
        assert tuple(c.sc.shape) == (k // 128, 42, 2) and c.rnorm.dtype == torch.float32
        codes, e, rnorm = F8.unit_rows(x)
        assert np.array_equal(c.q.cpu().numpy(), codes)
        assert np.array_equal(F8.exponents_of(c.sc.cpu().numpy(), n), e)
        assert np.array_equal(c.rnorm.cpu().numpy(), rnorm)
        assert not c.q[17].any() and float(c.rnorm[17]) == 0.0 and (np.delete(rnorm, 17) == 1.0).all()
        unit = x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
        assert np.array_equal(_deq(c), unit)


# ---------------------------------------------------------------------------- 2. quantiser, random rows
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("k", KS)
def test_quantiser_random_rows(dev, dtype, k):
    """deq against the float64-normalised row y: the e4m3 rounding is at most 2^-4 |v| for a normal code
    and half a subnormal step, 2^-9 2^e, below (tests/test_fp8_gpu.py::test_quant_fp8_mx), of the device's
    fp32 v = x * inv; v is within d = (K / 2 + 4) 2^-24 relative of y (the fp32 sum of K squares K 2^-24,
    halved by the root; the root, the reciprocal and the multiply one rounding each, and one spare).
    rnorm against float64 1 / |deq| of the read-back rows: K 2^-25 + 2^-23 relative (module docstring)."""
    rng = np.random.default_rng(k + 1)
    n = 301
    x = _dev_rows(rng.standard_normal((n, k)) * np.exp(rng.standard_normal((n, 1))), dev, dtype)
    c = ops.unit_rows_fp8mx(x)
    x64 = x.double().cpu().numpy()
    y = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
    deq = _deq(c)
    e = F8.exponents_of(c.sc.cpu().numpy(), n)
    amax = np.abs(y).reshape(n, k // 64, 64).max(axis=-1)
    d = (k / 2 + 4) * 2.0 ** -24
    assert (amax * 2.0 ** -e <= 448 * (1 + d)).all() and (amax * 2.0 ** -e > 224 * (1 - d)).all()
    step = np.repeat(2.0 ** e, 64, axis=1)
    lim = 2.0 ** -4 * np.abs(y) * (1 + d) + step * 2.0 ** -9 + d * np.abs(y)
    assert (np.abs(deq - y) <= lim).all(), float((np.abs(deq - y) / lim).max())
    want = 1.0 / np.sqrt((deq * deq).sum(axis=1))
    rel = np.abs(c.rnorm.double().cpu().numpy() - want) / want
    print(dtype, k, "rnorm worst relative error", rel.max(), "bound", k * 2.0 ** -25 + 2.0 ** -23,
          "stored norms", (1 / want).min(), (1 / want).max())
    assert (rel <= k * 2.0 ** -25 + 2.0 ** -23).all()


# ---------------------------------------------------------------------------- 3. search, designed operands
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_search_designed_operands_is_exact(dev, seed, k):
    """Rows as in case 1 whose non-zeros share 32 hot columns: every product, partial sum and scaling is a
    small dyadic number and both reciprocal norms are 1, so the device equals float64 bit for bit, per
    split and per row. Within a row every non-zero has one magnitude, so its non-zero blocks share one
    exponent and the all-zero blocks between them carry e = 0: this case catches a scale taken from an
    all-zero block (or the wrong row); a swap between two non-zero blocks of a row is for the random rows
    of the edge and long-bank cases."""
    rng = np.random.default_rng(seed)
    M, Nb = TM + 1, 2 * TN + 3
    hot = rng.choice(k, 32, replace=False)
    q = ops.unit_rows_fp8mx(_dev_rows(_designed(rng, M, k, hot), dev))
    r = ops.unit_rows_fp8mx(_dev_rows(_designed(rng, Nb, k, hot, zero_row=5), dev))
    q64, r64 = _deq(q), _deq(r)
    assert len(np.unique(F8.exponents_of(r.sc.cpu().numpy(), Nb))) >= 3
    part = ops.bank_nn_fp8mx(q, r)
    n_splits, rows_per_split = _split_rows(M, Nb)
    assert n_splits == 3 and part.shape == (M, 3) and part.dtype == torch.float32
    want = F8.bank_nn_parts(q64, r64, n_splits, rows_per_split)
    assert len(np.unique(want)) > 4  # not a trivial case
    assert np.array_equal(part.double().cpu().numpy(), want)
    assert np.array_equal(_sims(part), F8.bank_nn(q64, r64))


# ---------------------------------------------------------------------------- 4. every tile edge
@functools.lru_cache(maxsize=None)
def _edge_case(k):
    """One Q and one bank of random unit rows per K, quantised by the device, and the full float64 cosine
    matrix of the read-back rows, computed once: every edge shape is a corner of it."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7 + k)
    q = ops.unit_rows_fp8mx(_dev_rows(_unit(rng, max(M_EDGES), k), dev))
    r = ops.unit_rows_fp8mx(_dev_rows(_unit(rng, max(NB_EDGES), k), dev))
    return q, r, F8.cosines(_deq(q), _deq(r))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_edges_random_unit_rows(dev, k, strided):
    """Every M in (1, TM - 1, TM + 1) against every Nb in (1, TN - 1, TN + 1, 3 TN + 1), dense and inside
    wider buffers; per split and per row within bound(K) of float64 on the read-back operands."""
    q_all, r_all, cos = _edge_case(k)
    worst = 0.0
    for M in M_EDGES:
        for Nb in NB_EDGES:
            q, r = _take(q_all, slice(0, M)), _take(r_all, slice(0, Nb))
            if strided:
                q, r = _strided(q), _strided(r)
            part = ops.bank_nn_fp8mx(q, r)
            n_splits, rows_per_split = _split_rows(M, Nb)
            assert part.shape == (M, n_splits) and (Nb != 3 * TN + 1 or n_splits >= 3)
            want = np.stack([cos[:M, s * rows_per_split:min((s + 1) * rows_per_split, Nb)].max(axis=1)
                             for s in range(n_splits)], axis=1)
            err = np.abs(part.double().cpu().numpy() - want).max()
            worst = max(worst, err)
            assert err <= bound(k), (M, Nb, err)
            assert np.abs(_sims(part) - cos[:M, :Nb].max(axis=1)).max() <= bound(k)
    print("K", k, "strided" if strided else "dense", "largest |device - float64|", worst, "bound", bound(k),
          "ratio", worst / bound(k))


# ---------------------------------------------------------------------------- 4b. several bank tiles per block
@pytest.mark.parametrize("k", KS)
def test_blocks_that_walk_several_bank_tiles(dev, k):
    """Nb = 2 * 64 * TN + 1 rows: 129 bank tiles, more than twice the 64 splits, so every block walks three
    tiles (the last split: the ragged one-row tile after two full ones) and M = TM + 1 gives two row tiles.
    This is where the code between tiles runs: the next tile's first K-step in flight under this one's
    last, the per-tile scale offsets, and the reciprocal norms' slots (at K = 128, one K-step per tile, a
    tile's norms are fetched while the tile before last may still be folding). Per split and per row
    within bound(K) of float64 on the read-back rows, and the same bits on a second run."""
    rng = np.random.default_rng(29 + k)
    M, Nb = TM + 1, 2 * 64 * TN + 1
    n_splits, rows_per_split = _split_rows(M, Nb)
    assert rows_per_split == 3 * TN and n_splits == 43
    q = ops.unit_rows_fp8mx(_dev_rows(_unit(rng, M, k), dev))
    r = ops.unit_rows_fp8mx(_dev_rows(_unit(rng, Nb, k), dev))
    cos = F8.cosines(_deq(q), _deq(r))
    part = ops.bank_nn_fp8mx(q, r)
    assert part.shape == (M, n_splits)
    want = np.stack([cos[:, s * rows_per_split:min((s + 1) * rows_per_split, Nb)].max(axis=1)
                     for s in range(n_splits)], axis=1)
    err = np.abs(part.double().cpu().numpy() - want).max()
    print("K", k, "three tiles per block: largest |device - float64|", err, "bound", bound(k), "ratio", err / bound(k))
    assert err <= bound(k)
    assert torch.equal(ops.bank_nn_fp8mx(q, r), part)
    # each tile of a split decides some row's maximum: the walk kept every tile's result
    tile_of_winner = np.stack([cos[:, s * rows_per_split:min((s + 1) * rows_per_split, Nb)].argmax(axis=1) // TN
                               for s in range(n_splits - 1)])
    assert set(np.unique(tile_of_winner)) == {0, 1, 2}


# ---------------------------------------------------------------------------- 5. winner in every place, all negative
def test_winner_in_every_place(dev):
    rng = np.random.default_rng(11)
    M, Nb = 3, 3 * TN + 1
    n_splits, rows_per_split = _split_rows(M, Nb)
    assert n_splits == 4 and rows_per_split == TN
    q = ops.unit_rows_fp8mx(_dev_rows(_unit(rng, M), dev))
    base = ops.unit_rows_fp8mx(_dev_rows(_unit(rng, Nb), dev))
    places = {0: 0, rows_per_split - 1: 0, (n_splits - 1) * rows_per_split: n_splits - 1, Nb - 1: n_splits - 1}
    assert (n_splits - 1) * rows_per_split == Nb - 1  # the last split is the one ragged row
    places[2 * rows_per_split] = 2
    for index, split in places.items():
        r = ops.Fp8MxRows(base.q.clone(), base.sc.clone(), base.rnorm.clone())
        r.q[index], r.sc[:, index], r.rnorm[index] = q.q[1], q.sc[:, 1], q.rnorm[1]
        got = ops.bank_nn_fp8mx(q, r).double().cpu().numpy()
        assert abs(got[1].max() - 1.0) <= BOUND, (index, got[1])  # the cosine of a stored row with itself
        assert int(got[1].argmax()) == split, (index, got[1])
        assert (np.delete(got[1], split) < 0.5).all(), (index, got[1])  # seen by its own split alone


def test_all_negative_similarities(dev):
    """Bank = -Q plus noise, Q's rows around one direction: every cosine is negative. A kernel that padded
    the ragged tiles with zero rows would return 0 (Nb = TN + 1: the second split is one row and TN - 1
    rows of padding), one that dropped the bank norm or took it with the wrong sign would leave the bound."""
    rng = np.random.default_rng(13)
    M, Nb = TM + 1, TN + 1
    x = _unit(rng, 1) + 0.5 * _unit(rng, M)
    b = -x[:Nb] + 0.01 * rng.standard_normal((Nb, K))
    q, r = ops.unit_rows_fp8mx(_dev_rows(x, dev)), ops.unit_rows_fp8mx(_dev_rows(b, dev))
    n_splits, rows_per_split = _split_rows(M, Nb)
    assert n_splits == 2
    want = F8.bank_nn_parts(_deq(q), _deq(r), n_splits, rows_per_split)
    assert (want < -0.3).all()
    got = ops.bank_nn_fp8mx(q, r).double().cpu().numpy()
    assert (got < 0).all()
    assert np.abs(got - want).max() <= BOUND


# ---------------------------------------------------------------------------- 6. same bits
def test_same_bits(dev):
    q_all, r_all, _ = _edge_case(K)
    q, r = _take(q_all, slice(0, TM + 1)), _take(r_all, slice(0, 3 * TN + 1))
    ref = ops.bank_nn_fp8mx(q, r).max(dim=1).values
    for m in (0, 77, TM):  # a row alone against the same row in the batch (TM: the second row tile)
        alone = ops.bank_nn_fp8mx(_take(q, slice(m, m + 1)), r).max(dim=1).values
        assert torch.equal(alone, ref[m:m + 1]), m
    perm = torch.from_numpy(np.random.default_rng(3).permutation(r.shape[0])).to(dev)
    assert torch.equal(ops.bank_nn_fp8mx(q, _take(r, perm)).max(dim=1).values, ref)  # any order of the bank
    head = _take(r, slice(0, TN + 5))
    flipped = _take(head, torch.arange(TN + 4, -1, -1, device=dev))
    assert torch.equal(ops.bank_nn_fp8mx(q, head).max(dim=1).values, ops.bank_nn_fp8mx(q, flipped).max(dim=1).values)
    a, b = ops.bank_nn_fp8mx(q, r), ops.bank_nn_fp8mx(q, r)  # back to back
    assert torch.equal(a, b) and torch.equal(a.max(dim=1).values, ref)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = ops.bank_nn_fp8mx(q, r)
    side.synchronize()
    assert torch.equal(c, a)
    part = torch.full_like(a, 7.0)  # a caller-owned workspace is fully overwritten
    assert ops.bank_nn_fp8mx(q, r, part) is part and torch.equal(part, a)
    assert torch.equal(ops.bank_nn_fp8mx(_strided(q), _strided(r)), a)  # wherever the rows lie


# ---------------------------------------------------------------------------- 7-10. end to end
ARGS = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4"]


@pytest.fixture(scope="module", params=["fp16", "fp8"])
def harness_runs(request, tmp_path_factory, dev):
    """One --few_shot --few_shot_search fp8 run and one default --few_shot run per compute dtype."""
    import test as harness
    dt = request.param
    save = str(tmp_path_factory.mktemp("fewshot_fp8_" + dt))
    common = ARGS + ["--few_shot", "--shot", "2", "--compute_dtype", dt, "--save_path", save]
    few8 = harness.run(harness.parse_args(common + ["--few_shot_search", "fp8"]))
    few = harness.run(harness.parse_args(common))
    return dt, few8, few


def _images(stage, shot=2):
    from dataset import get_dataset
    ds = get_dataset("synthetic", 70, None, shot, stage, synthetic_n=4)["bottle"]
    return torch.stack([ds[i]["image"] for i in range(len(ds))])


def _query_rows(eng, x):
    """forward_raw's level rows of x through the row kernel (the rows live in the engine's workspace)."""
    return [ops.unit_rows_fp8mx(s_) for s_ in eng.forward_raw(x)[0]]


def test_harness_fp8_search_end_to_end(dev, harness_runs):
    dt, (df, ctx), (plain_df, plain_ctx) = harness_runs
    assert len(df) == 2 and np.isfinite(df.drop(columns=["class name"]).to_numpy(dtype=np.float64)).all()
    model, T = ctx["model"], ctx["text_embeddings"]["bottle"]
    eng = model.visual_engine()
    parts = ctx["few_shot"]["bottle"]
    x = _images("test").to(dev)
    bank = model.build_memory_bank(_images("support").to(dev), FP8)
    L, P = len(eng.levels), 25
    assert bank.dtype == FP8 and bank.img_size == 70 and len(bank.levels) == L and bank.shots == 2
    assert all(isinstance(lv, ops.Fp8MxRows) and tuple(lv.shape) == (2 * P, K) and lv.dtype == FP8 for lv in bank.levels)
    with torch.cuda.device(dev):
        rows = _query_rows(eng, x)
    assert all(tuple(r.shape) == (4 * P, K) for r in rows)
    # the few-shot map: the float64 grid of the device's own stored rows through the device blur
    grid = F8.fewshot_grid([_deq(r) for r in rows], [_deq(b) for b in bank.levels], 4, 5)
    want = ops.blur_upsample(torch.from_numpy(grid.astype(np.float32)).to(dev), torch.empty(4, 1, 70, 70, device=dev),
                             ksize=7, sigma=1.0)[:, 0]
    err = float((parts["fs_map"] - want).abs().max())
    print(dt, "fp8 fs_map largest |device - reference|", err, "bound", L * BOUND + 1e-5)
    assert parts["fs_map"].shape == (4, 70, 70) and err <= L * BOUND + 1e-5
    # the fusion: bit-equal to the float32 reference on the device's own maps and scores
    fm, fsc, fus = FR.fewshot_fuse(parts["zs_map"].cpu().numpy(), parts["fs_map"].cpu().numpy(),
                                   parts["zs_score"].cpu().numpy())
    assert np.array_equal(parts["fused_map"].cpu().numpy(), fm)
    assert np.array_equal(parts["fs_score"].cpu().numpy(), fsc)
    assert np.array_equal(parts["fused_score"].cpu().numpy(), fus)
    _, _, preds, preds_image = ctx["classes"]["bottle"]
    assert torch.equal(preds, parts["fused_map"]) and torch.equal(preds_image, parts["fused_score"])
    # without the flag the same harness run gives what it gives today: predict_few_shot with a default bank
    plain = plain_ctx["few_shot"]["bottle"]
    pmodel, pT = plain_ctx["model"], plain_ctx["text_embeddings"]["bottle"]
    dbank = pmodel.build_memory_bank(_images("support").to(dev))
    assert dbank.dtype == pmodel.visual_engine().search_dtype == torch.float16
    zs_map, zs_score, fs_map = pmodel.predict_few_shot(x, pT, dbank, "Industrial")
    assert torch.equal(plain["fs_map"], fs_map) and torch.equal(plain["zs_map"], zs_map)
    assert torch.equal(plain["zs_score"], zs_score)
    assert torch.equal(plain["zs_map"], parts["zs_map"])  # the zero-shot half does not see the flag
    assert not torch.equal(plain["fs_map"], parts["fs_map"])
    assert np.isfinite(plain_df.drop(columns=["class name"]).to_numpy(dtype=np.float64)).all()


def test_self_retrieval_is_zero(dev, harness_runs):
    """A bank built from the test images themselves, fp8: every patch finds itself at cosine
    (q^ . q^) rq rq = 1 within BOUND, and Cauchy-Schwarz on the stored rows caps every other match at the
    same value; four levels; blur and upsample are convex combinations: |fs_map| <= L BOUND. Without the
    norm correction (or with one side of it) the same quantity is about 1e-2."""
    dt, (_, ctx), _ = harness_runs
    model, T = ctx["model"], ctx["text_embeddings"]["bottle"]
    x = _images("test").to(dev)
    bank = model.build_memory_bank(x, FP8)
    zs_map, zs_score, fs_map = model.predict_few_shot(x, T, bank, "Industrial")
    L = len(bank.levels)
    worst = float(fs_map.abs().max())
    print(dt, "fp8 self-retrieval largest |fs_map|", worst, "bound", L * BOUND)
    assert fs_map.shape == (4, 70, 70) and worst <= L * BOUND
    assert torch.isfinite(zs_map).all() and zs_score.shape == (4,)


def test_distance_from_the_fp16_search(dev, harness_runs):
    """Per level |cos_fp8 - cos_fp16| < 0.13, a worst-case cap that catches a mis-paired scale: the e4m3
    error is at most 2^-4 per element, so each operand turns by at most asin(2^-4 + eps) = 0.0626 rad and
    the cosine moves by at most the sum of the two angles. Deliberately loose."""
    dt, (_, ctx), _ = harness_runs
    model = ctx["model"]
    eng = model.visual_engine()
    x, support = _images("test").to(dev), _images("support").to(dev)
    bank8, bank16 = model.build_memory_bank(support, FP8), model.build_memory_bank(support)
    with torch.cuda.device(dev):
        rows8 = _query_rows(eng, x)
        rows16 = eng.bank_rows(x)
        worst = 0.0
        for q8, r8, q16, r16 in zip(rows8, bank8.levels, rows16, bank16.levels):
            c8 = ops.bank_nn_fp8mx(q8, r8).max(dim=1).values
            c16 = ops.bank_nn(q16, r16).max(dim=1).values
            worst = max(worst, float((c8 - c16).abs().max()))
    print(dt, "largest per-level |cos_fp8 - cos_fp16|", worst)
    assert worst < 0.13


def test_mismatched_bank_raises(dev, harness_runs):
    dt, (_, ctx), _ = harness_runs
    model, T = ctx["model"], ctx["text_embeddings"]["bottle"]
    bank = model.build_memory_bank(_images("support").to(dev), FP8)
    with pytest.raises(ValueError, match="built at 70 px"):
        model.predict_few_shot(torch.zeros(1, 3, 84, 84, device=dev), T, bank, "Industrial")
    from aaclip.engine import MemoryBank
    d16 = model.build_memory_bank(_images("support").to(dev))
    wrong = MemoryBank([lv.to(torch.bfloat16) for lv in d16.levels], 70, torch.bfloat16, 2)
    with pytest.raises(ValueError, match="rebuild it"):
        model.predict_few_shot(_images("test").to(dev), T, wrong, "Industrial")
    mislabelled = MemoryBank(d16.levels, 70, FP8, 2)  # 16-bit rows under the fp8 label
    with pytest.raises(ValueError, match="rebuild it"):
        model.predict_few_shot(_images("test").to(dev), T, mislabelled, "Industrial")
    with pytest.raises(ValueError, match="search_dtype"):
        model.build_memory_bank(_images("support").to(dev), torch.bfloat16)
