"""Greedy k-centre coreset of the few-shot memory bank, the parts that need no GPU: the numpy
statement (tests/coreset_ref.py) against a brute-force restatement and its own properties, the C
entries' declarations and argument rejections (the library loads on a CPU host; nothing is
launched), the wrappers' checks and the harness flag."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib, ops

import coreset_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_bank_coreset_workspace", "aaclip_bank_coreset"]


def _unit(rng, n, k=64):
    x = rng.standard_normal((n, k))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ---------------------------------------------------------------------------- the restatement
def _brute_force(rows, m, start):
    """The same selection with nothing carried from step to step: at every step all pairwise
    similarities to the rows picked so far are recomputed."""
    r = np.asarray(rows, np.float64)
    n = r.shape[0]
    sel, cover = [start], [-np.inf]
    while len(sel) < m:
        best, best_key = None, None
        for i in range(n):
            if i in sel:
                continue
            key = max(CR.row_sims(r[[i, s]], 1)[0] for s in sel)
            if best is None or key < best_key:  # strict: the lowest index keeps a tie
                best, best_key = i, key
        sel.append(best)
        cover.append(best_key)
    maxsim = np.array([max(CR.row_sims(r[[i, s]], 1)[0] for s in sel) for i in range(n)])
    return np.array(sel), np.array(cover), maxsim


@pytest.mark.parametrize("start", [0, 36])
def test_reference_equals_brute_force(start):
    rows = _unit(np.random.default_rng(1), 37)
    for m in (1, 2, 11, 37):
        sel, cover, maxsim = CR.greedy_kcenter(rows, m, start)
        bsel, bcover, bmaxsim = _brute_force(rows, m, start)
        assert sel.dtype == np.int64 and sel.shape == (m,) and cover.shape == (m,) and maxsim.shape == (37,)
        assert np.array_equal(sel, bsel) and np.array_equal(cover, bcover) and np.array_equal(maxsim, bmaxsim)
        assert np.array_equal(CR.maxsim_over(rows, sel), maxsim)


def test_reference_prefix_monotone_and_permutation():
    rows = _unit(np.random.default_rng(2), 61)
    sel, cover, maxsim = CR.greedy_kcenter(rows, 61, 5)
    assert sorted(sel.tolist()) == list(range(61))  # m == N: a permutation
    assert sel[0] == 5 and cover[0] == -np.inf
    assert (np.diff(cover[1:]) >= 0).all()  # each pick is at least as close to the picks so far as the one before
    norms2 = (rows * rows).sum(axis=1)
    assert np.allclose(maxsim, norms2, atol=1e-12)  # every row is picked: it is its own nearest
    for m in (1, 2, 17, 60):
        s2, c2, ms2 = CR.greedy_kcenter(rows, m, 5)
        assert np.array_equal(s2, sel[:m]) and np.array_equal(c2, cover[:m])  # the prefix property
        assert (ms2 <= maxsim).all()
        if m > 1:  # what the next pick would cover is what the rows not taken still lack
            rest = np.setdiff1d(np.arange(61), s2)
            assert ms2[rest].min() == cover[m]


def test_reference_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(3)
    rows = rng.integers(-8, 9, (23, 64)).astype(np.float64)
    rows[11] = rows[3]
    rows[19] = rows[3]
    sel, cover, _ = CR.greedy_kcenter(rows, 23, 0)
    where = {int(s): t for t, s in enumerate(sel)}
    assert where[3] < where[11] < where[19]  # equal keys at every step: the copies come in index order
    # two rows equally far from the start, and a third that is nearer
    e = np.zeros((4, 64))
    e[0, 0], e[1, 1], e[2, 2], e[3, 0] = 1, 1, 1, 1
    sel, cover, maxsim = CR.greedy_kcenter(e, 4, 0)
    assert sel.tolist() == [0, 1, 2, 3] and cover.tolist() == [-np.inf, 0.0, 0.0, 1.0]
    assert CR.greedy_kcenter(e, 2, 2)[0].tolist() == [2, 0]
    with pytest.raises(ValueError):
        CR.greedy_kcenter(e, 0)
    with pytest.raises(ValueError):
        CR.greedy_kcenter(e, 5)
    with pytest.raises(ValueError):
        CR.greedy_kcenter(e, 2, 4)


# ---------------------------------------------------------------------------- sizes
def test_coreset_rows_edges():
    assert ops.coreset_rows(43808, 0.1) == 4381 and ops.coreset_rows(2304, 0.1) == 231
    assert ops.coreset_rows(273800, 0.01) == 2738
    assert ops.coreset_rows(50, 0.25) == 13 and ops.coreset_rows(50, 1.0) == 50 and ops.coreset_rows(1, 0.5) == 1
    assert ops.coreset_rows(50, 1e-9) == 1 and ops.coreset_rows(7, 0.999) == 7
    for n, ratio in ((97, 0.3), (1000, 0.001), (3, 1 / 3)):
        assert ops.coreset_rows(n, ratio) == max(1, math.ceil(ratio * n))
    for bad in (0.0, -0.1, 1.0000001, 2, float("nan")):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            ops.coreset_rows(10, bad)
    with pytest.raises(ValueError, match="at least one row"):
        ops.coreset_rows(0, 0.5)


def test_block_plan_is_a_function_of_n():
    br, mb = ops.CORESET_BLOCK_ROWS, ops.CORESET_MAX_BLOCKS
    assert ops.coreset_blocks(1) == 1 and ops.coreset_blocks(br) == 1 and ops.coreset_blocks(br + 1) == 2
    assert ops.coreset_blocks(mb * br) == mb
    assert ops.coreset_blocks(mb * br + 1) == (mb + 2) // 2  # a second grid-stride trip, dealt evenly
    for n in (43808, 273800, 1 << 30):
        slabs = -(-n // br)
        blocks = ops.coreset_blocks(n)
        trips = -(-slabs // blocks)
        assert blocks <= mb and trips == -(-slabs // mb) and blocks * trips >= slabs > blocks * (trips - 1)
    assert 8 * ops.coreset_blocks(43808) ** 2 < 2 ** 20  # the redundant candidate reduction: under 1 MiB a step


# ---------------------------------------------------------------------------- C ABI
def test_entry_points_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9
    for macro, value in (("AACLIP_CORESET_MAX_K", ops.CORESET_MAX_K),
                         ("AACLIP_CORESET_BLOCK_ROWS", ops.CORESET_BLOCK_ROWS),
                         ("AACLIP_CORESET_MAX_BLOCKS", ops.CORESET_MAX_BLOCKS)):
        assert int(re.search(r"#define " + macro + r" (\d+)", src).group(1)) == value, macro
    assert ops.CORESET_MAX_K >= 768 and ops.CORESET_MAX_K * 4 <= 64 * 1024  # the centre row fits in LDS as fp32


def test_argument_validation_rejects_without_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)  # non-null and aligned; never dereferenced on the host
    size = ctypes.c_size_t(0)
    assert lib.aaclip_bank_coreset_workspace(100, None) == 1
    assert lib.aaclip_bank_coreset_workspace(0, ctypes.byref(size)) == 1
    assert lib.aaclip_bank_coreset_workspace(-4, ctypes.byref(size)) == 1
    assert lib.aaclip_bank_coreset_workspace((1 << 30) + 1, ctypes.byref(size)) == 1
    assert lib.aaclip_bank_coreset_workspace(1 << 30, ctypes.byref(size)) == 0 and size.value >= 1 << 30
    assert lib.aaclip_bank_coreset_workspace(100, ctypes.byref(size)) == 0
    need = size.value
    assert need >= 2 * ops.CORESET_MAX_BLOCKS * 8 + 100 and need % 16 == 0

    def cs(ptrs=(p,) * 5, dtype=_lib.F16, N=100, K=768, ldr=768, m=10, start=0, nbytes=need):
        return lib.aaclip_bank_coreset(dtype, N, K, ptrs[0], ldr, m, start, ptrs[1], ptrs[2], ptrs[3], ptrs[4], nbytes,
                                       None)
    for bad in range(5):
        assert cs(ptrs=tuple(None if i == bad else p for i in range(5))) == 1, bad
    assert cs(N=0) == 1 and cs(N=-1) == 1 and cs(K=0) == 1
    assert cs(m=0) == 1 and cs(m=-1) == 1 and cs(m=101) == 1
    assert cs(start=-1) == 1 and cs(start=100) == 1
    assert cs(dtype=_lib.FP8) == 1 and cs(dtype=7) == 1
    assert cs(K=760, ldr=760) == 1  # K % 64
    k_big = ops.CORESET_MAX_K + 64
    assert cs(K=k_big, ldr=k_big) == 1  # the centre row would not fit
    assert cs(ldr=704) == 1  # below K
    assert cs(ldr=772) == 1  # 1544 bytes: rows not 16-byte aligned
    assert cs(dtype=_lib.F32, ldr=770) == 1
    assert cs(ptrs=(ctypes.c_void_p(264), p, p, p, p)) == 1  # a misaligned bank
    assert cs(ptrs=(p, ctypes.c_void_p(258), p, p, p)) == 1  # misaligned sel
    assert cs(ptrs=(p, p, p, p, ctypes.c_void_p(264))) == 1  # a misaligned workspace
    assert cs(nbytes=need - 1) == 1 and cs(nbytes=0) == 1  # a short workspace


def test_wrappers_reject_before_the_library():
    rows = torch.zeros(9, 768, dtype=torch.float16)
    with pytest.raises(TypeError, match="unsupported dtype"):
        ops.bank_coreset(rows.to(torch.float64), 3)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.bank_coreset(rows[:, :760].contiguous(), 3)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.bank_coreset(torch.zeros(3, ops.CORESET_MAX_K + 64, dtype=torch.float16), 3)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.bank_coreset(torch.zeros(768, 9, dtype=torch.float16).t(), 3)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.bank_coreset(torch.zeros(9, 772, dtype=torch.float16)[:, :768], 3)
    with pytest.raises(ValueError, match="no rows"):
        ops.bank_coreset(rows[:0], 1)
    for m, start in ((0, 0), (10, 0), (-1, 0), (3, 9), (3, -1)):
        with pytest.raises(ValueError, match="1 <= m <= N"):
            ops.bank_coreset(rows, m, start)
    with pytest.raises(RuntimeError, match="device"):  # well-formed operands reach the device check
        ops.bank_coreset(rows, 3)


# ---------------------------------------------------------------------------- the harness flag
def test_flag_parses_and_rejects_ratios_outside_the_interval(capsys):
    import test as harness
    assert harness.parse_args([]).bank_coreset == 1.0
    assert harness.parse_args(["--few_shot", "--bank_coreset", "0.25"]).bank_coreset == 0.25
    assert harness.parse_args(["--bank_coreset", "1"]).bank_coreset == 1.0  # accepted and ignored without --few_shot
    both = harness.parse_args(["--few_shot", "--bank_coreset", "0.1", "--few_shot_search", "fp8", "--pro", "--regions",
                               "--visualize"])
    assert both.bank_coreset == 0.1 and both.few_shot_search == "fp8" and both.f1 and both.pro and both.visualize
    for bad in ("0", "1.5", "-0.2", "nan", "half"):
        with pytest.raises(SystemExit):
            harness.parse_args(["--few_shot", "--bank_coreset", bad])
        assert "--bank_coreset" in capsys.readouterr().err


def test_memory_bank_constructor_stays_call_compatible():
    from aaclip.engine import MemoryBank
    levels = [torch.zeros(50, 768, dtype=torch.float16) for _ in range(4)]
    full = MemoryBank(levels, 70, torch.float16, 2)
    assert full.rows == full.source_rows == 50 and full.coreset_index is None and full.cover is None
    assert full.coverage is None and "rows=50/50" in repr(full)
    kept = MemoryBank([lv[:13] for lv in levels], 70, torch.float16, 2, source_rows=50,
                      coreset_index=[torch.arange(13, dtype=torch.int32)] * 4, cover=[torch.zeros(13)] * 4,
                      coverage=[torch.tensor(0.5)] * 4)
    assert kept.rows == 13 and kept.source_rows == 50 and "rows=13/50" in repr(kept)
