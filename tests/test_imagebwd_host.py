"""Host-side checks of the visual-tower backward (no GPU): the four entry points are declared, bound
and exported and reject bad arguments without a launch; the ops wrappers refuse bad shapes, dtypes
and CPU tensors; the API surface exists; and tests/imagebwd_ref.py, the fp64 restatement the GPU
tests compare with, reproduces the real reference's golden_imagebwd.npz
(tests/golden/make_golden_imagebwd.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib
from oracle import synth

import imagebwd_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_attention_bwd_tiled_workspace", "aaclip_attention_bwd_tiled", "aaclip_tap_ln_bwd",
       "aaclip_l2_normalize_bwd"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_imagebwd.npz"))


# ---------------------------------------------------------------------------- C ABI
def test_header_declares_loader_binds_and_library_exports_the_visual_backward():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert lib.aaclip_abi_version() == _lib.ABI_VERSION
    for cite in ("model/adapter.py:90-91", "model/adapter.py:100-105", "model/adapter.py:109", "train.py:156",
                 "train.py:117-174"):
        assert cite in src, cite
    assert "visual_bwd.hip" in open(os.path.join(ROOT, "aa-clip_amd", "csrc", "Makefile")).read()
    # aaclip_attention_bwd keeps its LDS-resident form and its limit
    text = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "text_bwd.hip")).read()
    assert "AB_MAX_SEQ = 77" in text


def test_loader_refuses_a_library_without_the_new_entries(tmp_path):
    """A library of the same ABI version that lacks aaclip_attention_bwd_tiled is refused by name."""
    import subprocess
    names = [s for s in _lib.SIGNATURES if s not in ("aaclip_abi_version", "aaclip_attention_bwd_tiled")]
    body = f"int aaclip_abi_version(void) {{ return {_lib.ABI_VERSION}; }}\n" + "".join(f"int {n}(void) {{ return 0; }}\n" for n in names)
    c, so = tmp_path / "stale.c", tmp_path / "libstale.so"
    c.write_text(body)
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(c)], check=True)
    with pytest.raises(RuntimeError, match=r"lacks aaclip_attention_bwd_tiled"):
        _lib.load(str(so))


P, Q, R_, W, S5, S6 = (ctypes.c_void_p(a << 20) for a in (1, 2, 3, 4, 5, 6))


def _bad(fn, good):
    """Call fn with one or more of the well-formed arguments replaced (`good` itself never runs)."""
    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    return bad


def test_attention_bwd_tiled_rejects_bad_arguments_without_a_launch():
    lib = _lib.lib()
    nbytes = ctypes.c_size_t(0)
    wsq = lib.aaclip_attention_bwd_tiled_workspace
    assert wsq(2, 1370, 16, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 2 * 16 * 1370 * 4
    assert wsq(0, 5, 1, ctypes.byref(nbytes)) == 1 and wsq(1, 0, 1, ctypes.byref(nbytes)) == 1
    assert wsq(1, 5, 0, ctypes.byref(nbytes)) == 1 and wsq(1, 5, 1, None) == 1
    need = 2 * 2 * 16 * 577 * 4
    bad = _bad(lib.aaclip_attention_bwd_tiled, [P, Q, R_, W, 2, 577, 16, 64, S5, need, None])
    assert all(bad(**{f"a{i}": None}) == 1 for i in (0, 1, 2, 3, 8))
    assert bad(a7=32) == 1 and bad(a7=128) == 1                           # head_dim
    assert bad(a5=0) == 1 and bad(a4=0) == 1 and bad(a6=0) == 1           # seq, batch, heads
    assert bad(a3=P) == 1 and bad(a3=Q) == 1 and bad(a3=R_) == 1          # dqkv over an input
    assert bad(a8=W) == 1 and bad(a8=P) == 1                              # the workspace over an operand
    assert bad(a9=need - 1) == 1 and bad(a9=0) == 1                       # short workspace
    assert bad(a4=4096, a6=16) == 1                                       # batch * heads > 65535
    assert bad(a0=ctypes.c_void_p((1 << 20) + 4)) == 1                    # misaligned


def test_row_kernels_reject_bad_arguments_without_a_launch():
    lib = _lib.lib()
    bad = _bad(lib.aaclip_tap_ln_bwd, [P, Q, R_, W, 2, 17, 1024, None])
    assert all(bad(**{f"a{i}": None}) == 1 for i in range(4))
    assert bad(a4=0) == 1 and bad(a5=1) == 1 and bad(a6=512) == 1         # batch, n_tok (no patch row), width
    assert bad(a3=Q) == 1 and bad(a3=P) == 1                              # g over x / dtap
    assert bad(a4=1 << 20, a5=1 << 11) == 1
    assert bad(a1=ctypes.c_void_p((2 << 20) + 8)) == 1
    bad = _bad(lib.aaclip_l2_normalize_bwd, [P, 768, 0, 1.0, Q, 768, R_, 768, 10, 768, None])
    assert bad(a0=None) == 1 and bad(a4=None) == 1 and bad(a6=None) == 1
    assert bad(a9=512) == 1 and bad(a1=764) == 1 and bad(a5=770) == 1 and bad(a7=767) == 1 and bad(a8=-1) == 1
    assert bad(a2=-1) == 1 and bad(a6=Q) == 1                             # group < 0, dx over x
    assert bad(a6=P, a2=5) == 1 and bad(a6=P, a7=1536) == 1               # dx over dy: row for row only
    assert bad(a6=ctypes.c_void_p((3 << 20) + 4)) == 1


# ---------------------------------------------------------------------------- ops wrappers, API surface
def test_ops_wrappers_reject_cpu_tensors_and_bad_shapes():
    from aaclip import ops
    z = torch.zeros
    for call in (lambda: ops.attention_bwd_tiled(z(10, 384), z(10, 128), z(10, 128), 2, 5, 2, workspace=z(40)),
                 lambda: ops.tap_ln_bwd(z(8, 1024), z(10, 1024), z(1024), z(10, 1024), 2, 5),
                 lambda: ops.l2_normalize_bwd(z(3, 768), z(3, 768)),
                 lambda: ops.l2_normalize_bwd(z(1, 768), z(3, 768), group=3, scale=1 / 3)):
        with pytest.raises(RuntimeError, match="device"):
            call()
    # shapes and dtypes are checked before the device is (and so before any launch)
    for call in (lambda: ops.attention_bwd_tiled(z(10, 384), z(10, 64), z(10, 128), 2, 5, 2),
                 lambda: ops.attention_bwd_tiled(z(10, 384), z(10, 128), z(10, 128).double(), 2, 5, 2),
                 lambda: ops.attention_bwd_tiled(z(10, 384), z(10, 128), z(10, 128), 2, 0, 2),
                 lambda: ops.attention_bwd_tiled(z(10, 384), z(10, 128), z(10, 128), 2, 5, 2, dqkv=z(10, 128)),
                 lambda: ops.tap_ln_bwd(z(10, 1024), z(10, 1024), z(1024), z(10, 1024), 2, 5),
                 lambda: ops.tap_ln_bwd(z(8, 640), z(10, 640), z(640), z(10, 640), 2, 5),
                 lambda: ops.tap_ln_bwd(z(8, 1024), z(10, 1024), z(768), z(10, 1024), 2, 5),
                 lambda: ops.l2_normalize_bwd(z(3, 768), z(4, 768)),
                 lambda: ops.l2_normalize_bwd(z(3, 512), z(3, 512)),
                 lambda: ops.l2_normalize_bwd(z(2, 768), z(5, 768), group=2),
                 lambda: ops.l2_normalize_bwd(z(3, 768).double(), z(3, 768))):
        with pytest.raises(ValueError):
            call()
    for name in ("attention_bwd_tiled", "attention_bwd_tiled_workspace", "tap_ln_bwd", "l2_normalize_bwd"):
        assert callable(getattr(ops, name)), name
    assert ops.ATTN_BWD_MAX_SEQ == 77  # the LDS-resident kernel keeps its limit


def test_training_api_surface():
    from aaclip.engine import VisualEngine
    from model.adapter import AdaptedCLIP
    assert list(inspect.signature(VisualEngine.forward_train).parameters)[:3] == ["self", "x", "adapter_weights"]
    assert callable(VisualEngine.set_adapter)
    src = inspect.getsource(AdaptedCLIP.forward)
    assert "is_grad_enabled" in src and "forward_train" in src and "float32" in src
    # the frozen tower's signature no longer holds the adapter tensors' versions
    src = inspect.getsource(AdaptedCLIP.visual_engine)
    assert "set_adapter" in src
    assert "once_differentiable" in inspect.getsource(__import__("aaclip.engine", fromlist=["_VisualTrain"])._VisualTrain)


# ---------------------------------------------------------------------------- the restatement is the reference
def test_golden_fixture_is_what_the_issue_describes(gold):
    assert list(gold["taps"]) == [23, 18, 12, 6, 5, 0] and list(gold["rows"]) == IR.ROWS and len(IR.ROWS) == 16
    names = IR.weight_names()
    assert len(names) == 11
    for i in range(11):
        assert gold[f"g{i}_rows64"].shape == (16, 1024 // IR.COL_STEP) and gold[f"g{i}_rows64"].dtype == np.float64
        assert float(gold[f"g{i}_norm64"]) > 0 and 0 < float(gold[f"g{i}_rel32"]) < 1e-4
    for b in IR.TAPS:
        assert gold[f"tap{b}_64"].shape == (len(IR.TAP_TOKENS), 1024) and 0 < float(gold[f"tap{b}_rel32"]) < 1e-4
    al = gold["adam_losses32"]
    # the reference's own run: Adam's first step overshoots on the synthetic tower, then the loss falls
    assert al.shape == (4,) and al[3] < al[2] < al[1] and al[3] < al[0] and gold["adam_losses64"].shape == (4,)
    assert float(gold["relu_g_norm64"]) > 0 and float(gold["relu_loss64"]) != float(gold["loss64"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_imagebwd.npz")) < 1 << 20
    mask, label = IR.adam_inputs()
    assert mask.shape == (2, 1, 112, 112) and 0 < mask.mean() < 1 and list(label) == [0, 1]


def test_restatement_reproduces_the_reference_fp64(gold):
    """Outputs, loss, the stored gradient rows and norms and the block taps: rel-L2 within 1e-10."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = synth.clip_state_dict(111, img_size=IR.IMG)
    ia, _ = synth.adapter_state_dicts(111)
    x = synth.images(IR.X_SEED, IR.BATCH, IR.IMG)
    r = IR.run(sd, ia, x, IR.loss_weights((IR.IMG // 14) ** 2), torch.float64)
    figures = [("loss", abs(r["loss"] - float(gold["loss64"])) / abs(float(gold["loss64"]))),
               ("det", IR.rel_l2(r["det"], gold["det64"])),
               ("seg", IR.rel_l2(np.stack([s[:, ::21, ::IR.COL_STEP] for s in r["seg"]]), gold["seg_rows64"]))]
    for i, n in enumerate(IR.weight_names()):
        figures.append((f"d {n} rows", IR.rel_l2(r["grads"][i][IR.ROWS][:, ::IR.COL_STEP], gold[f"g{i}_rows64"])))
        figures.append((f"d {n} norm", abs(np.linalg.norm(r["grads"][i]) / float(gold[f"g{i}_norm64"]) - 1)))
    for b in IR.TAPS:
        figures.append((f"tap {b}", IR.rel_l2(r["taps"][b][list(IR.TAP_TOKENS)], gold[f"tap{b}_64"])))
    for name, e in figures:
        print(f"{name}: |restated - reference| {e:.2e}")
    assert all(e <= 1e-10 for _, e in figures)
