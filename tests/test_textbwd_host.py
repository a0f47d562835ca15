"""Host-side checks of the text-tower backward (no GPU): the nine entry points are declared, bound
and exported under ABI 8 and reject bad arguments without a launch; the ops wrappers refuse bad
shapes, dtypes and CPU tensors; the API surface exists; and tests/textbwd_ref.py, the fp64
restatement the GPU tests compare with, reproduces the real reference's golden_textbwd.npz
(tests/golden/make_golden_textbwd.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib
from oracle import synth

import textbwd_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_attention_bwd", "aaclip_layernorm_bwd", "aaclip_eot_ln_bwd", "aaclip_act", "aaclip_act_bwd",
       "aaclip_adapter_blend_bwd", "aaclip_anchor_reduce_bwd", "aaclip_linear_wgrad_workspace", "aaclip_linear_wgrad"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_textbwd.npz"))


# ---------------------------------------------------------------------------- C ABI
def test_abi_8_declares_binds_and_exports_the_text_backward():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9
    for cite in ("model/adapter.py:125-128", "model/adapter.py:130-136", "model/adapter.py:138-140",
                 "forward_utils.py:155-159", "transformer.py:46-49", "model/adapter_modules.py:6-47", "train.py:99"):
        assert cite in src, cite
    mk = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "Makefile")).read()
    assert "text_bwd.hip" in mk
    # the activation the training forward applies is the GEMM epilogue's own device function
    common = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "common.h")).read()
    gemm = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "gemm.hip")).read()
    for fn in ("gelu_erf", "qgelu_exact"):
        assert re.search(r"float " + fn + r"\(float", common) and not re.search(r"float " + fn + r"\(float", gemm)
        assert fn + "(v)" in gemm


P, Q, R_, W, S5, S6 = (ctypes.c_void_p(a << 20) for a in (1, 2, 3, 4, 5, 6))


def _bad(fn, good):
    """Call fn with one or more of the well-formed arguments replaced (`good` itself never runs)."""
    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    return bad


def test_attention_bwd_rejects_bad_arguments_without_a_launch():
    bad = _bad(_lib.lib().aaclip_attention_bwd, [P, Q, R_, 2, 77, 12, 64, 1, None])
    assert bad(a0=None) == 1 and bad(a1=None) == 1 and bad(a2=None) == 1
    assert bad(a4=78) == 1 and bad(a4=0) == 1 and bad(a4=1000) == 1      # seq outside 1..77
    assert bad(a6=32) == 1 and bad(a3=0) == 1 and bad(a5=0) == 1          # head_dim, batch, heads
    assert bad(a7=2) == 1 and bad(a7=4) == 1                              # flags other than CAUSAL
    assert bad(a2=P) == 1                                                 # in place
    assert bad(a3=1 << 20, a5=1 << 11) == 1                               # batch * heads >= 2^31


def test_row_kernels_reject_bad_arguments_without_a_launch():
    lib = _lib.lib()
    bad = _bad(lib.aaclip_layernorm_bwd, [P, 768, Q, 768, R_, W, 768, S5, 768, 10, 768, None])
    assert bad(a0=None) == 1 and bad(a2=None) == 1 and bad(a4=None) == 1 and bad(a7=None) == 1
    assert bad(a10=512) == 1 and bad(a1=764) == 1 and bad(a3=770) == 1 and bad(a8=767) == 1 and bad(a6=766) == 1
    assert bad(a9=-1) == 1 and bad(a7=Q) == 1                             # rows < 0, dx over x
    assert bad(a7=W, a8=1536) == 1                                        # dx aliases the residual at another stride
    assert bad(a0=ctypes.c_void_p((1 << 20) + 4)) == 1                    # misaligned
    bad = _bad(lib.aaclip_eot_ln_bwd, [P, Q, R_, W, S5, 3, 9, 768, None])
    assert all(bad(**{f"a{i}": None}) == 1 for i in range(5))
    assert bad(a5=0) == 1 and bad(a6=0) == 1 and bad(a7=512) == 1 and bad(a4=Q) == 1 and bad(a4=P) == 1
    assert bad(a5=1 << 20, a6=1 << 11) == 1
    bad = _bad(lib.aaclip_adapter_blend_bwd, [P, Q, R_, 0.1, W, S5, 10, 768, None])
    assert all(bad(**{f"a{i}": None}) == 1 for i in (0, 1, 2, 4, 5))
    assert bad(a7=512) == 1 and bad(a6=-1) == 1
    assert bad(a4=Q) == 1 and bad(a5=P) == 1 and bad(a5=W) == 1 and bad(a5=R_) == 1  # only dx may alias (dy)
    bad = _bad(lib.aaclip_anchor_reduce_bwd, [P, 6, 768, Q, 0, 2, R_, None])
    assert bad(a0=None) == 1 and bad(a3=None) == 1 and bad(a6=None) == 1 and bad(a6=P) == 1
    assert bad(a1=0) == 1 and bad(a1=257) == 1 and bad(a2=1025) == 1 and bad(a4=2) == 1 and bad(a4=-1) == 1
    for fn, good in ((lib.aaclip_act, [_lib.EPI_GELU, P, Q, 100, None]),
                     (lib.aaclip_act_bwd, [_lib.EPI_LEAKY, P, Q, R_, 100, None])):
        bad = _bad(fn, good)
        assert bad(a0=0) == 1 and bad(a0=_lib.EPI_BIAS) == 1 and bad(a0=_lib.EPI_GELU | _lib.EPI_LEAKY) == 1
        assert bad(a1=None) == 1 and bad(a2=None) == 1 and bad(**{f"a{len(good) - 2}": -1}) == 1


def test_linear_wgrad_rejects_bad_arguments_without_a_launch():
    lib = _lib.lib()
    nbytes = ctypes.c_size_t(0)
    wsq = lib.aaclip_linear_wgrad_workspace
    assert wsq(170, 768, 768, ctypes.byref(nbytes)) == 0 and nbytes.value == 3 * 768 * 768 * 4  # 170 rows: 3 chunks
    assert wsq(64, 64, 128, ctypes.byref(nbytes)) == 0 and nbytes.value == 64 * 128 * 4
    assert wsq(65, 1024, 1024, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 1024 * 1024 * 4  # not tied to 768
    assert wsq(0, 768, 768, ctypes.byref(nbytes)) == 1 and wsq(1, 100, 768, ctypes.byref(nbytes)) == 1
    assert wsq(1, 768, 32, ctypes.byref(nbytes)) == 1 and wsq(1, 768, 768, None) == 1
    need = 3 * 768 * 768 * 4
    bad = _bad(lib.aaclip_linear_wgrad, [P, 768, Q, 768, 170, 768, 768, S6, need, R_, 768, None])
    assert bad(a0=None) == 1 and bad(a2=None) == 1 and bad(a7=None) == 1 and bad(a9=None) == 1
    assert bad(a8=need - 1) == 1 and bad(a4=0) == 1 and bad(a5=100) == 1 and bad(a6=96) == 1
    assert bad(a1=704) == 1 and bad(a3=704) == 1 and bad(a10=704) == 1   # leading dimensions
    assert bad(a9=P) == 1 and bad(a9=Q) == 1 and bad(a9=S6) == 1         # dW over an input / the workspace


# ---------------------------------------------------------------------------- ops wrappers, API surface
def test_ops_wrappers_reject_cpu_tensors_and_bad_shapes():
    from aaclip import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="device"):
        ops.attention_bwd(z(10, 384), z(10, 128), 2, 5, 2)
    with pytest.raises(ValueError, match="1..77"):
        ops.attention_bwd(z(156, 384), z(156, 128), 2, 78, 2)
    for call in (lambda: ops.layernorm_bwd(z(3, 768), z(3, 768), z(768)),
                 lambda: ops.eot_ln_bwd(z(2, 768), z(18, 768), z(2, 9, dtype=torch.int32), z(768)),
                 lambda: ops.act(z(8), "gelu"), lambda: ops.act_bwd(z(8), z(8), "leaky"),
                 lambda: ops.adapter_blend_bwd(z(3, 768), z(3, 768), z(3, 768), 0.1),
                 lambda: ops.anchor_reduce_bwd(z(6, 768), z(768, 2), 0), lambda: ops.anchor_column(z(6, 768)),
                 lambda: ops.linear_wgrad(z(5, 64), z(5, 128))):
        with pytest.raises(RuntimeError, match="device"):
            call()
    # shapes and dtypes are checked before the device is (and so before any launch)
    for call in (lambda: ops.attention_bwd(z(10, 384), z(10, 64), 2, 5, 2),
                 lambda: ops.attention_bwd(z(10, 384).double(), z(10, 128), 2, 5, 2),
                 lambda: ops.layernorm_bwd(z(3, 768), z(3, 512), z(512)),
                 lambda: ops.layernorm_bwd(z(3, 768), z(4, 768), z(768)),
                 lambda: ops.layernorm_bwd(z(3, 768).half(), z(3, 768), z(768)),
                 lambda: ops.eot_ln_bwd(z(2, 768), z(18, 768), z(2, 9, dtype=torch.int64), z(768)),
                 lambda: ops.eot_ln_bwd(z(3, 768), z(18, 768), z(2, 9, dtype=torch.int32), z(768)),
                 lambda: ops.act(z(8).double(), "gelu"), lambda: ops.act_bwd(z(8), z(9), "gelu"),
                 lambda: ops.adapter_blend_bwd(z(3, 768), z(3, 768), z(2, 768), 0.1),
                 lambda: ops.adapter_blend_bwd(z(3, 640), z(3, 640), z(3, 640), 0.1),
                 lambda: ops.anchor_reduce_bwd(z(6, 768), z(768, 2), 2),
                 lambda: ops.anchor_reduce_bwd(z(300, 768), z(768, 2), 0),
                 lambda: ops.linear_wgrad(z(5, 64), z(4, 128)), lambda: ops.linear_wgrad(z(5, 100), z(5, 128)),
                 lambda: ops.linear_wgrad(z(5, 64).double(), z(5, 128))):
        with pytest.raises(ValueError):
            call()
    for name in ("attention_bwd", "layernorm_bwd", "eot_ln_bwd", "act", "act_bwd", "adapter_blend_bwd",
                 "anchor_reduce_bwd", "linear_wgrad", "linear_wgrad_workspace", "anchor_column"):
        assert callable(getattr(ops, name)), name
    assert ops.WGRAD_ROWS == 64 and ops.ATTN_BWD_MAX_SEQ == 77
    with pytest.raises(ValueError, match="mode"):
        ops._act_mode("relu")


def test_training_api_surface():
    from aaclip.engine import TextEngine
    from model.adapter import AdaptedCLIP
    from model.clip import CLIP
    assert list(inspect.signature(TextEngine.encode_train).parameters)[:3] == ["self", "tokens", "adapter_weights"]
    assert callable(TextEngine.set_adapter)
    src = inspect.getsource(AdaptedCLIP.encode_text)
    assert "is_grad_enabled" in src and "encode_train" in src and "adapt_text" in src
    # the frozen tower's signature no longer holds the adapter tensors' versions
    src = inspect.getsource(CLIP.text_engine)
    assert "set_adapter" in src


# ---------------------------------------------------------------------------- the restatement is the reference
def test_golden_fixture_is_what_the_issue_describes(gold):
    assert gold["G"].shape == (768, 2) and np.array_equal(gold["G"], TR.loss_weights())
    assert gold["tok_normal"].shape == (6, 77) and gold["tok_abnormal"].shape == (10, 77)
    assert list(gold["taps"]) == [11, 6, 2, 0] and list(gold["rows"]) == TR.ROWS and len(TR.ROWS) == 16
    for i in range(4):
        assert gold[f"g{i}_rows64"].shape == (16, 768) and gold[f"g{i}_rows64"].dtype == np.float64
        assert float(gold[f"g{i}_norm64"]) > 0 and 0 < float(gold[f"g{i}_rel32"]) < 1e-5
    for b in (11, 6, 2, 0):
        assert gold[f"tap{b}_64"].shape == (int(gold["n_eot"]), 768)
    al = gold["adam_losses32"]
    assert al.shape == (4,) and np.all(np.diff(al) < 0) and gold["adam_losses64"].shape == (4,)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_textbwd.npz")) < 1 << 20


def test_restatement_reproduces_the_reference_fp64(gold):
    """T, loss, the stored gradient rows and norms and the block taps: rel-L2 within 1e-10."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = synth.clip_state_dict(111)
    _, ta = synth.adapter_state_dicts(111)
    r = TR.run(sd, ta, gold["tok_normal"], gold["tok_abnormal"], gold["G"], torch.float64)
    figures = [("T", TR.rel_l2(r["T"], gold["T64"])), ("loss", abs(r["loss"] - float(gold["loss64"])))]
    for i in range(4):
        figures.append((f"dW{i} rows", TR.rel_l2(r["grads"][i][TR.ROWS], gold[f"g{i}_rows64"])))
        figures.append((f"dW{i} norm", abs(np.linalg.norm(r["grads"][i]) / float(gold[f"g{i}_norm64"]) - 1)))
    for b in TR.TAPS:
        figures.append((f"tap {b}", TR.rel_l2(r["taps"][b], gold[f"tap{b}_64"])))
    for name, e in figures:
        print(f"{name}: |restated - reference| {e:.2e}")
    assert all(e <= 1e-10 for _, e in figures)
