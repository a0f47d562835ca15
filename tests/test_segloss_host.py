"""Host-side checks of the stage-1 loss head (no GPU): the six entry points are declared,
bound and exported under ABI 8 and reject bad arguments without a launch; the reference API
surface exists; and tests/segloss_ref.py, the fp64 restatement the GPU tests compare with,
reproduces the real reference's golden_segloss.npz (tests/golden/make_golden_segloss.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib

import segloss_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_patch_logits_per_image", "aaclip_seg_loss", "aaclip_seg_loss_bwd", "aaclip_upsample_softmax_bwd",
       "aaclip_patch_logits_bwd", "aaclip_patch_logits_bwd_workspace"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_segloss.npz"))


# ---------------------------------------------------------------------------- C ABI
def test_abi_8_declares_binds_and_exports_the_six_entry_points():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9
    for cite in ("forward_utils.py:21-126", "199-202", "211-215", "forward_utils.py:219-227", "train.py:86-100"):
        assert cite in src, cite
    # argument counts follow the header
    for name in NEW:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name


def test_reference_api_surface():
    import forward_utils as fu
    assert list(inspect.signature(fu.calculate_seg_loss).parameters) == ["patch_preds", "mask"]
    assert list(inspect.signature(fu.calculate_similarity_map).parameters)[:4] == [
        "patch_features", "epoch_text_feature", "img_size", "test"]
    with pytest.raises(RuntimeError, match="device"):
        fu.calculate_seg_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError, match="patch_preds"):
        fu.calculate_seg_loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4))
    # three anchors with a grad-requiring input: refused before any launch (CPU tensors never get that far)
    T3 = torch.zeros(768, 3, requires_grad=True)
    with pytest.raises(NotImplementedError, match="2 anchors"):
        fu.calculate_similarity_map(torch.zeros(1, 4, 768), T3, 8)
    with pytest.raises(ValueError, match="per image"):
        fu.calculate_similarity_map(torch.zeros(2, 4, 768), torch.zeros(3, 768, 2), 8)


P, Q, R_, W = (ctypes.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 4 << 20))


def test_patch_logits_per_image_rejects_bad_arguments_without_a_launch():
    fn = _lib.lib().aaclip_patch_logits_per_image
    good = [_lib.F32, P, 768, Q, 1536, 2, 50, 768, 25, R_, None]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    assert bad(a1=None) == 1 and bad(a3=None) == 1 and bad(a9=None) == 1  # null f / T / out
    assert bad(a0=_lib.F16) == 1 and bad(a0=_lib.FP8) == 1               # dtype
    assert bad(a4=-1536) == 1 and bad(a4=1535) == 1                      # negative / overlapping t_stride
    assert bad(a5=0) == 1 and bad(a5=9) == 1                             # n_anchor outside 1..8
    assert bad(a7=512) == 1 and bad(a2=764) == 1 and bad(a2=770) == 1    # channels != 768, ld
    assert bad(a8=0) == 1 and bad(a8=7) == 1 and bad(a6=-25) == 1        # group


def test_seg_loss_rejects_bad_arguments_without_a_launch():
    lib = _lib.lib()
    fwd, bwd = lib.aaclip_seg_loss, lib.aaclip_seg_loss_bwd
    ws = 3 * 1 * 8 * 8  # B=3, S=23: one chunk
    assert fwd(None, Q, 3, 23, W, ws, R_, P, None) == 1      # null probs
    assert fwd(P, None, 3, 23, W, ws, R_, Q, None) == 1      # null mask
    assert fwd(P, Q, 3, 23, None, ws, R_, W, None) == 1      # null workspace
    assert fwd(P, Q, 3, 23, W, ws, None, R_, None) == 1      # null sums
    assert fwd(P, Q, 3, 23, W, ws, R_, None, None) == 1      # null loss
    assert fwd(P, Q, 0, 23, W, ws, R_, P, None) == 1         # batch 0
    assert fwd(P, Q, -1, 23, W, ws, R_, P, None) == 1
    assert fwd(P, Q, 3, 1, W, ws, R_, P, None) == 1          # out_size < 2
    assert fwd(P, Q, 3, 23, W, ws - 1, R_, P, None) == 1     # workspace too small
    assert fwd(P, Q, 3, 65, W, 3 * 8 * 8, R_, P, None) == 1  # 65^2 = 4225 pixels need 2 chunks per image
    assert fwd(ctypes.c_void_p((1 << 20) + 2), Q, 3, 23, W, ws, R_, P, None) == 1  # misaligned
    d = ctypes.c_void_p(5 << 20)
    assert bwd(None, Q, R_, W, 3, 23, d, None) == 1
    assert bwd(P, None, R_, W, 3, 23, d, None) == 1
    assert bwd(P, Q, None, W, 3, 23, d, None) == 1           # null sums
    assert bwd(P, Q, R_, None, 3, 23, d, None) == 1          # null dloss (a device scalar, not a value)
    assert bwd(P, Q, R_, W, 3, 23, None, None) == 1
    assert bwd(P, Q, R_, W, 0, 23, d, None) == 1             # batch 0
    assert bwd(P, Q, R_, W, 3, 1, d, None) == 1              # out_size < 2
    assert bwd(P, Q, R_, W, 3, 23, P, None) == 1             # in place


def test_upsample_softmax_bwd_rejects_bad_arguments_without_a_launch():
    fn = _lib.lib().aaclip_upsample_softmax_bwd
    assert fn(None, Q, 3, 2, 5, 23, R_, None) == 1 and fn(P, None, 3, 2, 5, 23, R_, None) == 1
    assert fn(P, Q, 3, 2, 5, 23, None, None) == 1
    assert fn(P, Q, 0, 2, 5, 23, R_, None) == 1              # batch 0
    assert fn(P, Q, 3, 1, 5, 23, R_, None) == 1 and fn(P, Q, 3, 3, 5, 23, R_, None) == 1  # channels != 2
    assert fn(P, Q, 3, 2, 1, 23, R_, None) == 1 and fn(P, Q, 3, 2, 65, 23, R_, None) == 1  # g < 2, g > 64
    assert fn(P, Q, 3, 2, 5, 1, R_, None) == 1               # out_size < 2
    assert fn(P, Q, 3, 2, 5, 23, P, None) == 1               # in place


def test_patch_logits_bwd_rejects_bad_arguments_without_a_launch():
    lib = _lib.lib()
    fn, wsq = lib.aaclip_patch_logits_bwd, lib.aaclip_patch_logits_bwd_workspace
    nbytes = ctypes.c_size_t(0)
    assert wsq(75, 25, ctypes.byref(nbytes)) == 0 and nbytes.value == 3 * 2 * 1536 * 4  # 25 rows = 2 chunks of 16
    assert wsq(2738, 1369, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 86 * 1536 * 4
    assert wsq(75, 25, None) == 1 and wsq(0, 25, ctypes.byref(nbytes)) == 1 and wsq(75, 0, ctypes.byref(nbytes)) == 1
    assert wsq(75, 20, ctypes.byref(nbytes)) == 1
    need = 3 * 2 * 1536 * 4
    dT, df = ctypes.c_void_p(5 << 20), ctypes.c_void_p(6 << 20)
    good = [_lib.F32, P, 768, Q, 1536, 2, R_, 75, 768, 25, W, need, dT, df, None]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    assert bad(a1=None) == 1 and bad(a3=None) == 1 and bad(a6=None) == 1   # null f / T / dgrid
    assert bad(a12=None, a13=None) == 1                                  # neither output
    assert bad(a10=None) == 1 and bad(a11=need - 1) == 1                 # dT without / with too small a workspace
    assert bad(a5=1) == 1 and bad(a5=3) == 1                             # n_anchor != 2
    assert bad(a8=512) == 1 and bad(a2=764) == 1                         # channels != 768, ld
    assert bad(a4=-1536) == 1 and bad(a4=1532) == 1                      # negative / overlapping t_stride
    assert bad(a7=0) == 1 and bad(a9=0) == 1 and bad(a9=20) == 1         # no rows, group
    assert bad(a0=_lib.F16) == 1                                         # dtype
    assert bad(a13=P) == 1                                               # df over f


# ---------------------------------------------------------------------------- the restatement is the reference
def _case(gold, tag):
    B, g, S = (int(v) for v in gold[tag + "_shape"])
    f, T, mask = SR.inputs(int(gold[tag + "_seed"]), B, g, S, per_image=(tag == "a"))
    assert np.array_equal(T, gold[tag + "_T"]) and np.array_equal(mask.astype(np.uint8), gold[tag + "_mask"])
    flat = f.reshape(B * g * g, 768)
    if tag == "a":
        assert np.array_equal(f, gold["a_f"])
    else:
        assert np.array_equal(flat[gold["b_rows"]], gold["b_f_rows"])
        assert float(flat.astype(np.float64).sum()) == float(gold["b_f_sum"])
    return (B, g, S), f, T, mask


def test_golden_fixture_is_what_the_issue_describes(gold):
    assert list(gold["a_shape"]) == [3, 5, 23] and list(gold["b_shape"]) == [2, 24, 336]
    assert gold["a_T"].shape == (3, 768, 2) and gold["b_T"].shape == (768, 2)
    m = gold["a_mask"].reshape(3, -1)
    assert 0 < m[0].sum() < m.shape[1] and m[1].sum() == 0 and m[2].sum() == m.shape[1]
    assert gold["a_mid_share"] > 0.6 and gold["b_mid_share"] > 0.6       # the softmax gradient is alive
    al = gold["a_adam_losses"]
    assert al.shape == (4,) and np.all(np.diff(al) < 0) and al[0] == gold["a_loss32"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_segloss.npz")) < 1 << 20


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_the_reference_fp64(gold, tag):
    """Loss terms within 1e-12, gradients and sums rel-L2 within 1e-10."""
    (B, g, S), f, T, mask = _case(gold, tag)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    r = SR.run(f, T, mask, S, torch.float64)
    for k in ("loss", "focal", "dice0", "dice1"):
        d = abs(float(r[k]) - float(gold[f"{tag}_{k}64"]))
        print(f"case {tag} {k}: |restated - reference| = {d:.2e}")
        assert d <= 1e-12
    rows = gold[tag + "_rows"]
    dprobs = r["dprobs"] if tag == "a" else r["dprobs"].ravel()[::int(gold["b_pix_step"])]
    for name, got, want in (("sums", r["sums"], gold[tag + "_sums64"]), ("dT", r["dT"], gold[tag + "_dT64"]),
                            ("dgrid", r["dgrid"], gold[tag + "_dgrid64"]),
                            ("df", r["df"].reshape(-1, 768)[rows], gold[tag + "_df64"]),
                            ("dprobs", dprobs, gold[tag + "_dprobs64"])):
        e = SR.rel_l2(got, want)
        print(f"case {tag} {name}: rel-L2 {e:.2e}")
        assert np.shape(got) == np.shape(want) and e <= 1e-10
    # the fp32 restatement lands where the reference's fp32 run does (the yardstick is the same arithmetic)
    r32 = SR.run(f, T, mask, S, torch.float32)
    assert abs(float(r32["loss"]) - float(gold[tag + "_loss32"])) <= 4 * np.spacing(np.float32(gold[tag + "_loss32"]))
    assert SR.rel_l2(r32["dT"], gold[tag + "_dT32"]) <= 1e-5
