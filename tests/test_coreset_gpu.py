"""Greedy k-centre coreset of the few-shot memory bank on the MI355X (csrc/bank.hip:
aaclip_bank_coreset; VisualEngine.build_bank(coreset=...); test.py --bank_coreset) against the numpy
float64 statement of tests/coreset_ref.py.

Designed rows (integer entries in -8 .. 8): every product and every partial sum of a dot product is
an integer of magnitude at most 64 K <= 49 152 < 2^24, exact in fp32 in any order, so sel, cover and
maxsim equal the float64 reference bit for bit, ties included.

Random unit rows: the device's fp32 dot products err by at most BOUND = K * 2^-23 (the bound worked
out in tests/test_fewshot_gpu.py: K fused multiply-adds on |sum a_i b_i| <= 1), so the pick sequence
may leave the float64 one at a near-tie and is not compared; what is held is that every pick is,
in float64, within 2 BOUND of the best pick given the device's own earlier picks."""
import functools

import numpy as np
import pytest
import torch

from aaclip import ops

import coreset_ref as CR

pytestmark = pytest.mark.gpu

BR, MB = ops.CORESET_BLOCK_ROWS, ops.CORESET_MAX_BLOCKS
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
N_EDGES = (1, BR - 1, BR + 1, 3 * BR + 1)
N_RANDOM, M_RANDOM = 3 * BR + 1, 97


def _bound(k):
    return k * 2.0 ** -23


def _designed(n, k, seed=0):
    """Integer rows in -8 .. 8; two rows are copies of row 3, so equal keys meet at every step."""
    x = np.random.default_rng(seed).integers(-8, 9, (n, k)).astype(np.float64)
    if n > 40:
        x[17], x[40] = x[3], x[3]
    return x


@functools.lru_cache(maxsize=None)
def _designed_reference(n, k, m, start):
    return CR.greedy_kcenter(_designed(n, k), m, start)


def _on_device(x, dtype, dev, strided=False):
    """x on the device in dtype (as a column block of a wider buffer when strided), and the same
    rounded values back as float64."""
    t = torch.from_numpy(np.asarray(x, np.float32)).to(dev).to(dtype)
    back = t.double().cpu().numpy()
    if strided:
        k = t.shape[1]
        wide = torch.full((t.shape[0], 3 * k), 100.0, device=dev, dtype=dtype)
        wide[:, k:2 * k] = t
        t = wide[:, k:2 * k]
        assert t.stride(0) == 3 * k
    return t, back


def _host(*ts):
    return [t.double().cpu().numpy() for t in ts]


# ---------------------------------------------------------------------------- 1. designed, exact
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_designed_rows_are_exact(dev, dtype, strided):
    k = 768
    for n in N_EDGES:
        rows, back = _on_device(_designed(n, k), dtype, dev, strided)
        assert np.array_equal(back, _designed(n, k))  # representable in every dtype
        for m in sorted({1, min(n, 64), n}):
            for start in sorted({0, n - 1}):
                sel, cover, maxsim = ops.bank_coreset(rows, m, start)
                assert sel.dtype == torch.int32 and cover.dtype == torch.float32 and maxsim.dtype == torch.float32
                assert sel.shape == (m,) and cover.shape == (m,) and maxsim.shape == (n,)
                want_sel, want_cover, want_maxsim = _designed_reference(n, k, m, start)
                got_sel, got_cover, got_maxsim = _host(sel, cover, maxsim)
                assert np.array_equal(got_sel, want_sel), (n, m, start)
                assert np.array_equal(got_cover, want_cover), (n, m, start)
                assert np.array_equal(got_maxsim, want_maxsim), (n, m, start)
    sel = ops.bank_coreset(rows, 3 * BR + 1, 0)[0].cpu().tolist()
    assert sorted(sel) == list(range(3 * BR + 1))  # m == N: a permutation
    assert sel.index(3) < sel.index(17) < sel.index(40)  # the copies of row 3 come in index order


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_second_grid_stride_trip(dev, dtype):
    """N = MAX_BLOCKS * BLOCK_ROWS + 1: one slab more than one trip of the most blocks holds, so blocks
    own two slabs; K = 64, where half of a 16-bit row's sixteen lanes have no chunk."""
    n, k, m = MB * BR + 1, 64, 8
    assert ops.coreset_blocks(n) < -(-n // BR)
    rows, back = _on_device(_designed(n, k), dtype, dev)
    assert np.array_equal(back, _designed(n, k))
    for start in (0, n - 1):
        got = _host(*ops.bank_coreset(rows, m, start))
        want = _designed_reference(n, k, m, start)
        for g_, w, name in zip(got, want, ("sel", "cover", "maxsim")):
            assert np.array_equal(g_, w), (name, start)


# ---------------------------------------------------------------------------- 2. random unit rows
@functools.lru_cache(maxsize=None)
def _random_case(dtype, k):
    """Random unit rows rounded to dtype, on the device and as float64, and their float64 similarity
    matrix (every entry its own sum), computed once."""
    dev = torch.device("cuda:0")
    x = np.random.default_rng(k + 1).standard_normal((N_RANDOM, k))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    rows, r64 = _on_device(x, dtype, dev)
    sims = np.stack([CR.row_sims(r64, c) for c in range(N_RANDOM)], axis=1)
    return rows, r64, sims


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("k", [768, 64])
def test_random_unit_rows_every_pick_is_near_optimal(dev, dtype, k):
    rows, r64, sims = _random_case(dtype, k)
    bound = _bound(k)
    sel, cover, maxsim = _host(*ops.bank_coreset(rows, M_RANDOM, 0))
    sel = sel.astype(np.int64)
    assert len(set(sel.tolist())) == M_RANDOM and sel[0] == 0 and cover[0] == -np.inf  # no index is repeated
    taken = np.zeros(N_RANDOM, bool)
    ms64 = np.full(N_RANDOM, -np.inf)
    worst_pick = worst_cover = -np.inf
    for t in range(M_RANDOM):
        if t > 0:  # against the device's own earlier picks, in float64
            best = ms64[~taken].min()
            worst_pick = max(worst_pick, ms64[sel[t]] - best)
            worst_cover = max(worst_cover, abs(cover[t] - ms64[sel[t]]))
        taken[sel[t]] = True
        ms64 = np.maximum(ms64, sims[:, sel[t]])
    worst_maxsim = np.abs(maxsim - ms64).max()
    print(dtype, "K", k, "worst excess of a pick over the float64 best", worst_pick, "bound", 2 * bound,
          "| cover", worst_cover, "maxsim", worst_maxsim, "bound", bound)
    assert worst_pick <= 2 * bound
    assert worst_cover <= bound
    assert worst_maxsim <= bound
    assert np.array_equal(ms64, CR.maxsim_over(r64, sel))


# ---------------------------------------------------------------------------- 3. same bits
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_same_bits(dev, dtype):
    rows, _, _ = _random_case(dtype, 768)
    a = ops.bank_coreset(rows, M_RANDOM, 0)
    b = ops.bank_coreset(rows, M_RANDOM, 0)  # back to back
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = ops.bank_coreset(rows, M_RANDOM, 0)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    head = ops.bank_coreset(rows, 40, 0)  # the prefix property
    assert torch.equal(head[0], a[0][:40]) and torch.equal(head[1], a[1][:40])
    # a row's similarity does not depend on N or on where its block is: n2 rows put row 0 .. n1 - 1
    # into other blocks' company than n1 rows do
    n1, n2 = BR + 1, 3 * BR + 1
    for start in (0, n1 - 1):
        small = ops.bank_coreset(rows[:n1], 1, start)[2]
        large = ops.bank_coreset(rows[:n2], 1, start)[2]
        assert torch.equal(large[:n1], small)
    wide = torch.zeros(N_RANDOM, 2 * 768, device=dev, dtype=dtype)  # and not on the row stride
    wide[:, 768:] = rows
    for x, y in zip(ops.bank_coreset(wide[:, 768:], M_RANDOM, 0), a):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------- 4. with the search
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_coreset_bank_under_the_search(dev, dtype):
    """bank_nn gives a (query, bank row) pair the same bits wherever the bank row sits, so a maximum
    over a subset of the bank is at most the maximum over the whole bank, exactly."""
    k = 768
    rows, _, _ = _random_case(dtype, k)
    x = np.random.default_rng(23).standard_normal((77, k))
    q, _ = _on_device(x / np.linalg.norm(x, axis=1, keepdims=True), dtype, dev)
    full = ops.bank_nn(q, rows).max(dim=1).values
    sel, _, maxsim = ops.bank_coreset(rows, M_RANDOM, 0)
    kept = rows.index_select(0, sel.long())
    part = ops.bank_nn(q, kept)
    sub = part.max(dim=1).values
    assert bool((sub <= full).all()) and bool((sub < full).any())
    grid_full = ops.bank_distance(ops.bank_nn(q, rows), torch.empty(77, device=dev), accumulate=False)
    grid_sub = ops.bank_distance(part, torch.empty(77, device=dev), accumulate=False)
    assert bool((grid_sub >= grid_full).all())
    everything = ops.bank_coreset(rows, N_RANDOM, 0)[0]  # m == N: the bank in another order
    assert sorted(everything.cpu().tolist()) == list(range(N_RANDOM))
    again = ops.bank_nn(q, rows.index_select(0, everything.long())).max(dim=1).values
    assert torch.equal(again, full)
    # the bank's own rows against the coreset: each finds its nearest kept row, as maxsim says
    own = ops.bank_nn(rows, kept).max(dim=1).values
    slack = 2 * _bound(k)
    print(dtype, "coverage", float(maxsim.min()), "smallest self-search result", float(own.min()),
          "largest |search - maxsim|", float((own - maxsim).abs().max()), "slack", slack)
    assert float(own.min()) >= float(maxsim.min()) - slack


# ---------------------------------------------------------------------------- 5. engine and harness
ARGS = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4", "--few_shot",
        "--shot", "2", "--compute_dtype", "fp16"]
FP8 = torch.float8_e4m3fn
P = 25  # patches of a 70 px image


@pytest.fixture(scope="module")
def harness_runs(tmp_path_factory, dev):
    """The harness with --bank_coreset 0.25 (alone; with the fp8 search and the optional columns),
    with --bank_coreset 1.0 and without the flag."""
    import test as harness
    save = str(tmp_path_factory.mktemp("coreset"))

    def run(*extra):
        return harness.run(harness.parse_args(ARGS + ["--save_path", save] + list(extra)))
    return {"quarter": run("--bank_coreset", "0.25"),
            "quarter_fp8": run("--bank_coreset", "0.25", "--few_shot_search", "fp8", "--pro", "--regions",
                               "--visualize"),
            "one": run("--bank_coreset", "1.0"), "none": run()}


def _images(stage, shot=2):
    from dataset import get_dataset
    ds = get_dataset("synthetic", 70, None, shot, stage, synthetic_n=4)["bottle"]
    return torch.stack([ds[i]["image"] for i in range(len(ds))])


def test_build_bank_with_a_coreset(dev, harness_runs):
    _, ctx = harness_runs["none"]
    model, T = ctx["model"], ctx["text_embeddings"]["bottle"]
    eng = model.visual_engine()
    support, x = _images("support").to(dev), _images("test").to(dev)
    n, m = 2 * P, ops.coreset_rows(2 * P, 0.25)
    assert m == 13
    full = eng.build_bank(support)
    assert full.rows == full.source_rows == n and full.coreset_index is None and full.coverage is None
    bank = eng.build_bank(support, coreset=0.25)
    assert bank.rows == m and bank.source_rows == n and bank.dtype == torch.float16 and bank.shots == 2
    assert f"rows={m}/{n}" in repr(bank) and len(bank.levels) == len(full.levels) == len(eng.levels)
    with torch.cuda.device(dev):
        for j, (lv, src) in enumerate(zip(bank.levels, full.levels)):
            sel, cover, maxsim = ops.bank_coreset(src, m, 0)
            assert tuple(lv.shape) == (m, 768) and lv.dtype == torch.float16
            assert torch.equal(bank.coreset_index[j], sel) and torch.equal(bank.cover[j], cover)
            assert torch.equal(lv, src.index_select(0, sel.long()))  # the kept rows, in pick order
            assert float(bank.coverage[j]) == float(maxsim.min()) and -1.0 <= float(bank.coverage[j]) <= 1.001
            assert len(set(sel.cpu().tolist())) == m and int(sel[0]) == 0
    zs_map, zs_score, fs_map = model.predict_few_shot(x, T, bank, "Industrial")
    assert fs_map.shape == (4, 70, 70) and torch.isfinite(fs_map).all() and torch.isfinite(zs_map).all()
    zs_full, _, fs_full = model.predict_few_shot(x, T, full, "Industrial")
    assert torch.equal(zs_map, zs_full) and not torch.equal(fs_map, fs_full)  # the zero-shot half does not see it
    # fp8: the selection is the 16-bit one, and the kept rows are the full fp8 bank's rows at those places
    bank8, full8 = eng.build_bank(support, FP8, 0.25), eng.build_bank(support, FP8)
    assert bank8.dtype == FP8 and bank8.rows == m and bank8.source_rows == n
    for j, (lv, src) in enumerate(zip(bank8.levels, full8.levels)):
        assert isinstance(lv, ops.Fp8MxRows) and tuple(lv.shape) == (m, 768)
        at = bank.coreset_index[j].long()
        assert torch.equal(bank8.coreset_index[j], bank.coreset_index[j])
        assert torch.equal(lv.q, src.q.index_select(0, at)) and torch.equal(lv.rnorm, src.rnorm.index_select(0, at))
    fs8 = model.predict_few_shot(x, T, bank8, "Industrial")[2]
    assert fs8.shape == (4, 70, 70) and torch.isfinite(fs8).all()
    # coreset = 1.0 and None are today's path, bit for bit
    for same in (eng.build_bank(support, coreset=1.0), model.build_memory_bank(support, None, 1.0),
                 model.build_memory_bank(support, None, None)):
        assert same.rows == n and same.coreset_index is None
        assert all(torch.equal(a, b) for a, b in zip(same.levels, full.levels))
    one8 = eng.build_bank(support, FP8, 1.0)
    assert all(torch.equal(a.q, b.q) and torch.equal(a.sc, b.sc) for a, b in zip(one8.levels, full8.levels))
    for bad in (0.0, 1.5, -1):
        with pytest.raises(ValueError, match="coreset"):
            eng.build_bank(support, coreset=bad)


def test_harness_with_a_coreset_bank(dev, harness_runs):
    n, m = 2 * P, 13
    for name in ("quarter", "quarter_fp8"):
        df, ctx = harness_runs[name]
        assert len(df) == 2 and np.isfinite(df.drop(columns=["class name"]).to_numpy(dtype=np.float64)).all()
        parts = ctx["few_shot"]["bottle"]
        for key in ("zs_map", "fs_map", "fused_map", "zs_score", "fs_score", "fused_score"):
            assert torch.isfinite(parts[key]).all(), (name, key)
        info = parts["bank"]
        assert info["rows"] == m and info["source_rows"] == n and len(info["coverage"]) == 4
        assert all(isinstance(c, float) and -1.0 <= c <= 1.001 for c in info["coverage"])
    assert "pixel AUPRO" in harness_runs["quarter_fp8"][0].columns and "regions" in harness_runs["quarter_fp8"][1]
    # the coverage the harness reports is the bank's
    _, ctx = harness_runs["quarter"]
    bank = ctx["model"].build_memory_bank(_images("support").to(dev), None, 0.25)
    assert ctx["few_shot"]["bottle"]["bank"]["coverage"] == [float(c) for c in bank.coverage]
    fs_q, fs_none = ctx["few_shot"]["bottle"]["fs_map"], harness_runs["none"][1]["few_shot"]["bottle"]["fs_map"]
    assert not torch.equal(fs_q, fs_none)
    # --bank_coreset 1.0 is no flag at all
    (df1, ctx1), (df0, ctx0) = harness_runs["one"], harness_runs["none"]
    assert df1.equals(df0)
    for key in ("zs_map", "fs_map", "fused_map", "zs_score", "fs_score", "fused_score"):
        assert torch.equal(ctx1["few_shot"]["bottle"][key], ctx0["few_shot"]["bottle"][key]), key
    assert ctx1["few_shot"]["bottle"]["bank"] == ctx0["few_shot"]["bottle"]["bank"] == {
        "rows": n, "source_rows": n, "coverage": None}
