"""Host-side checks of stage-2 training in bf16 mixed precision (no GPU): the new entry points are
declared, bound and exported under the unchanged ABI version and reject bad arguments without a
launch; the ops wrappers refuse bad shapes, dtypes and CPU tensors; train_dtype and
AACLIP_TRAIN_DTYPE are validated and train.py's arguments are unchanged; and
tests/imagebwd_bf16_ref.py, the yardstick of the GPU tests, keeps the error against fp64 it was
measured with."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib
from oracle import synth

import imagebwd_bf16_ref as E
import imagebwd_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aaclip_attention_bwd16_workspace", "aaclip_attention_bwd16", "aaclip_act_to16", "aaclip_act_bwd16",
       "aaclip_cast_rows"]


# ---------------------------------------------------------------------------- C ABI
def test_header_declares_loader_binds_and_library_exports_the_bf16_backward():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9  # additions only
    mk = open(os.path.join(ROOT, "aa-clip_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvisual_bwd16\.hip\b", mk, re.M)


def test_loader_refuses_a_library_without_the_new_entries(tmp_path):
    """A library of the same ABI version that lacks aaclip_attention_bwd16 is refused by name."""
    import subprocess
    names = [s for s in _lib.SIGNATURES if s not in ("aaclip_abi_version", "aaclip_attention_bwd16")]
    body = f"int aaclip_abi_version(void) {{ return {_lib.ABI_VERSION}; }}\n" + "".join(
        f"int {n}(void) {{ return 0; }}\n" for n in names)
    c, so = tmp_path / "stale.c", tmp_path / "libstale.so"
    c.write_text(body)
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(c)], check=True)
    with pytest.raises(RuntimeError, match=r"lacks aaclip_attention_bwd16\b.*stale"):
        _lib.load(str(so))


P, Q, R_, W, S5 = (ctypes.c_void_p(a << 20) for a in (1, 2, 3, 4, 5))
ODD = ctypes.c_void_p((1 << 20) + 4)


def _bad(fn, good):
    """Call fn with one or more of the well-formed arguments replaced (`good` itself never runs)."""
    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    return bad


def test_attention_bwd16_rejects_bad_arguments_without_a_launch():
    lib = _lib.lib()
    nbytes = ctypes.c_size_t(0)
    wsq = lib.aaclip_attention_bwd16_workspace
    assert wsq(2, 1370, 16, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 2 * 16 * 1370 * 4
    assert wsq(0, 5, 1, ctypes.byref(nbytes)) == 1 and wsq(1, 0, 1, ctypes.byref(nbytes)) == 1
    assert wsq(1, 5, 0, ctypes.byref(nbytes)) == 1 and wsq(1, 5, 1, None) == 1
    need = 2 * 2 * 16 * 577 * 4
    bad = _bad(lib.aaclip_attention_bwd16, [_lib.BF16, P, Q, R_, W, 2, 577, 16, 64, 0, S5, need, None])
    assert bad(a0=_lib.F32) == 1 and bad(a0=_lib.F16) == 1 and bad(a0=_lib.FP8) == 1  # bf16 only
    assert all(bad(**{f"a{i}": None}) == 1 for i in (1, 2, 3, 4, 10))
    assert bad(a8=32) == 1 and bad(a8=128) == 1                           # head_dim
    assert bad(a6=0) == 1 and bad(a5=0) == 1 and bad(a7=0) == 1           # seq, batch, heads
    assert bad(a4=P) == 1 and bad(a4=Q) == 1 and bad(a4=R_) == 1          # dqkv over an input
    assert bad(a10=W) == 1 and bad(a10=P) == 1                            # the workspace over an operand
    assert bad(a11=need - 1) == 1 and bad(a11=0) == 1                     # short workspace
    assert bad(a9=_lib.ATTN_CAUSAL) == 1 and bad(a9=4) == 1               # non-causal only, unknown flag
    assert bad(a5=4096, a7=16) == 1                                       # batch * heads > 65535
    assert bad(a1=ODD) == 1                                               # misaligned


def test_row_kernels_reject_bad_arguments_without_a_launch():
    lib = _lib.lib()
    G = _lib.EPI_GELU
    bad = _bad(lib.aaclip_act_to16, [G, P, Q, _lib.BF16, 4096, None])
    assert bad(a1=None) == 1 and bad(a2=None) == 1 and bad(a4=-1) == 1
    assert bad(a0=_lib.EPI_BIAS) == 1 and bad(a0=0) == 1                  # not an activation
    assert bad(a3=_lib.F32) == 1 and bad(a3=_lib.FP8) == 1                # 16-bit outputs only
    assert bad(a2=P) == 1 and bad(a1=ODD) == 1                            # in place, misaligned
    bad = _bad(lib.aaclip_act_bwd16, [G, P, Q, R_, _lib.BF16, 4096, None])
    assert all(bad(**{f"a{i}": None}) == 1 for i in (1, 2, 3))
    assert bad(a0=7) == 1 and bad(a4=_lib.F32) == 1 and bad(a5=-1) == 1
    assert bad(a3=Q) == 1 and bad(a2=ODD) == 1                            # dx over ref, misaligned
    bad = _bad(lib.aaclip_cast_rows, [_lib.F32, _lib.BF16, P, 1024, Q, 1024, 10, 1024, None])
    assert bad(a2=None) == 1 and bad(a4=None) == 1 and bad(a4=P) == 1
    assert bad(a1=_lib.F32) == 1 and bad(a0=_lib.BF16) == 1 and bad(a1=_lib.FP8) == 1  # one side fp32, the other 16-bit
    assert bad(a7=1020) == 1 and bad(a7=0) == 1 and bad(a6=-1) == 1       # columns in 8s
    assert bad(a3=1000) == 1 and bad(a3=1026) == 1 and bad(a5=1028) == 1  # ld < cols, rows off 16 bytes
    assert bad(a2=ODD) == 1


# ---------------------------------------------------------------------------- ops wrappers
def test_ops_wrappers_reject_cpu_tensors_and_bad_shapes():
    from aaclip import ops
    z = torch.zeros
    b = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
    for call in (lambda: ops.attention_bwd16(b(10, 384), b(10, 128), b(10, 128), 2, 5, 2, workspace=z(40)),
                 lambda: ops.act_to16(z(16), "gelu", out=b(16)),
                 lambda: ops.act_bwd16(b(16), z(16), "quick"),
                 lambda: ops.cast_rows(z(4, 16), dtype=torch.bfloat16),
                 lambda: ops.cast_rows(b(4, 16), dtype=torch.float32)):
        with pytest.raises(RuntimeError, match="device"):
            call()
    # shapes and dtypes are checked before the device is (and so before any launch)
    for call in (lambda: ops.attention_bwd16(z(10, 384), z(10, 128), z(10, 128), 2, 5, 2),          # fp32
                 lambda: ops.attention_bwd16(b(10, 384).half(), b(10, 128).half(), b(10, 128).half(), 2, 5, 2),
                 lambda: ops.attention_bwd16(b(10, 384), b(10, 64), b(10, 128), 2, 5, 2),
                 lambda: ops.attention_bwd16(b(10, 384), b(10, 128), b(10, 128), 2, 0, 2),
                 lambda: ops.attention_bwd16(b(10, 384), b(10, 128), b(10, 128), 2, 5, 2, dqkv=b(10, 128)),
                 lambda: ops.act_to16(z(16), "gelu", out=z(16)),
                 lambda: ops.act_to16(z(16), "tanh", out=b(16)),
                 lambda: ops.act_to16(z(16), "gelu", out=b(8)),
                 lambda: ops.act_bwd16(z(16), z(16), "gelu"),
                 lambda: ops.act_bwd16(b(16), b(16), "gelu"),
                 lambda: ops.cast_rows(z(4, 16)),
                 lambda: ops.cast_rows(z(4, 16), dtype=torch.float32),
                 lambda: ops.cast_rows(z(4, 12), dtype=torch.bfloat16),
                 lambda: ops.cast_rows(z(4, 16), b(4, 8))):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------- public interface
def test_train_dtype_is_validated():
    from model import adapter
    assert adapter.check_train_dtype(None) is None and adapter.check_train_dtype(torch.bfloat16) == torch.bfloat16
    for bad in (torch.float16, torch.float32, torch.float8_e4m3fn, "bf16"):
        with pytest.raises(ValueError, match="train_dtype"):
            adapter.check_train_dtype(bad)
    sig = inspect.signature(adapter.AdaptedCLIP.__init__)
    assert sig.parameters["train_dtype"].default is None
    assert "check_train_dtype(train_dtype)" in inspect.getsource(adapter.AdaptedCLIP.__init__)
    src = inspect.getsource(adapter.AdaptedCLIP.forward)
    assert "train_dtype" in src and "float32" in src and "forward_train" in src


def test_train_dtype_environment_variable(monkeypatch):
    import train
    assert train.train_dtype_from_env({}) == torch.float32
    for v, want in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("BF16", torch.bfloat16)):
        assert train.train_dtype_from_env({"AACLIP_TRAIN_DTYPE": v}) == want
    for v in ("fp16", "fp8", "", "half"):
        with pytest.raises(ValueError, match="AACLIP_TRAIN_DTYPE"):
            train.train_dtype_from_env({"AACLIP_TRAIN_DTYPE": v})
    monkeypatch.setenv("AACLIP_TRAIN_DTYPE", "bf16")
    assert train.train_dtype_from_env() == torch.bfloat16
    monkeypatch.delenv("AACLIP_TRAIN_DTYPE")
    assert train.train_dtype_from_env() == torch.float32


def test_train_arguments_are_unchanged():
    import train
    a = vars(train.parse_args([]))
    assert sorted(a) == sorted([
        "model_name", "img_size", "surgery_until_layer", "relu", "dataset", "training_mode", "shot",
        "text_batch_size", "image_batch_size", "text_epoch", "image_epoch", "text_lr", "image_lr", "criterion",
        "seed", "save_path", "text_norm_weight", "text_adapt_weight", "image_adapt_weight", "text_adapt_until",
        "image_adapt_until", "allow_random_init", "synthetic_n", "gpu_preprocess", "max_steps"])
    assert (a["img_size"], a["image_epoch"], a["text_epoch"], a["image_batch_size"], a["image_lr"]) == (518, 20, 5, 2, 5e-4)
    with pytest.raises(SystemExit):
        train.parse_args(["--train_dtype", "bf16"])  # the dtype is not a flag


def test_engine_refuses_only_what_does_not_train():
    from aaclip import engine
    src = inspect.getsource(engine.VisualEngine.forward_train)
    assert "fp32 only" in src and "torch.bfloat16" in src


# ---------------------------------------------------------------------------- the yardstick
def test_rnd_rounds_forward_and_backward():
    x = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -9, -3.0], requires_grad=True)
    y = E.rnd(x)
    assert y.tolist() == [1.0, 1.0 + 2.0 ** -7, -3.0]  # ties to even
    y.backward(torch.tensor([1.0 + 2.0 ** -10, 2.0, 0.5 + 2.0 ** -12]))
    assert x.grad.tolist() == [1.0, 2.0, 0.5]
    x.grad = None
    E.rnd(x, bwd=False).backward(torch.tensor([1.0 + 2.0 ** -10, 2.0, 0.5]))
    assert x.grad.tolist() == [1.0 + 2.0 ** -10, 2.0, 0.5]
    assert E.rnd(x, fwd=False).tolist() == x.tolist()


def test_attention_restatement_follows_autograd():
    """The hand-written backward of the attention restatement against fp64 autograd on the same
    bf16-rounded inputs: within bf16 rounding, with and without the folded Q scale."""
    B, N, H = 2, 37, 2
    rng = np.random.default_rng(5)
    qkv = E.r(torch.from_numpy(rng.standard_normal((B * N, 3 * H * 64)).astype(np.float32)))
    dout = E.r(torch.from_numpy(rng.standard_normal((B * N, H * 64)).astype(np.float32)))
    for pre in (False, True):
        q = qkv.clone()
        if pre:
            q[:, :H * 64] = E.r(q[:, :H * 64] * E.Q_SCALE)
        a = q.clone().requires_grad_()
        E.attention16(a, B, N, H, pre).backward(dout)
        t = q.double().requires_grad_()
        E.attention_truth(t, B, N, H, pre).backward(dout.double())
        e = IR.rel_l2(a.grad.numpy(), t.grad.numpy())
        print(f"attention restatement, prescaled {pre}: rel-L2 {e:.3e}")
        assert e <= 4 * E.BF16_EPS


def test_restatement_keeps_its_error_against_fp64():
    """On the fixture (112 px, B = 2, synthetic weights) the restatement stood at 3.3e-2 .. 4.3e-2 (the
    six layer_adapters gradients), 5.7e-3 .. 6.8e-3 (the projections) and 5.6e-3 .. 6.8e-3 (the level
    features) against fp64, and moved by 12 % with the thread count: it stays within 1.5 x those."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = synth.clip_state_dict(111, img_size=IR.IMG)
    ia, _ = synth.adapter_state_dicts(111)
    x = synth.images(IR.X_SEED, IR.BATCH, IR.IMG)
    G = IR.loss_weights((IR.IMG // 14) ** 2)
    r64 = IR.run(sd, ia, x, G, torch.float64)
    e = E.run16(sd, ia, x, G)
    names = IR.weight_names()
    errs = [IR.rel_l2(e["grads"][i], r64["grads"][i]) for i in range(11)]
    feats = [IR.rel_l2(a, b) for a, b in zip(e["seg"] + [e["det"]], r64["seg"] + [r64["det"]])]
    for n, v in zip(names, errs):
        print(f"d {n}: restatement vs fp64 {v:.3e}")
    print("level features, det:", " ".join(f"{v:.3e}" for v in feats))
    assert all(1e-3 < v <= 1.5 * 4.3e-2 for v in errs[:6])
    assert all(1e-4 < v <= 1.5 * 6.8e-3 for v in errs[6:])
    assert all(1e-4 < v <= 1.5 * 6.8e-3 for v in feats)
