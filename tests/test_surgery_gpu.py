"""Frozen CLIP image paths on the MI355X: aaclip_vv_attention against a float64 reference,
its addressing and exact properties, FrozenVisualEngine / CLIP.encode_image /
AdaptedCLIP.forward_original against the REAL reference's outputs
(tests/golden/golden_surgery.npz) and, at a second shape, against the torch-CPU
restatement (tests/surgery_ref.py, itself pinned to the goldens by test_surgery_host.py).

The reference's surgery attention mixes the IMAGES of a batch (model/transformer.py:125-152
on the tower's [L, N, D] layout), so batch semantics are the contract: the golden yardstick
rel_drop_one (image 0 with and without image 1 beside it, 1.4 - 3.8 % on the stored rows)
is what a wrong batch coupling would cost, and the engine's error has to stay well inside it.
"""
import functools
import os

import numpy as np
import pytest
import torch

from aaclip import ops
from aaclip.engine import FrozenVisualEngine
from oracle import synth

import surgery_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# ---- kernel bounds: the ones tests/test_kernels_gpu.py holds aaclip_attention to (max abs);
# fp32 arithmetic with one final rounding gave 2.2e-6 / 1.9e-3 / 1.6e-2 on these inputs on the CPU
KERNEL_TOL = {"fp32": 1e-5, "fp16": 4e-3, "bf16": 3e-2}

# ---- engine against the goldens: rel-L2 per level (6, 12, 18, 24) over the stored rows, the
# larger of the batch-of-3 and batch-of-1 fixtures and of the row-norm metric. MEASURED on the
# MI355X; the asserted bound is twice the measured value, and never above the hard cap
# (fp32: rel_drop_one / 10, fp16: rel_drop_one / 2, bf16: rel_plain / 10, from the fixture).
MEASURED_TOKENS = {
    "fp32": (1.29e-6, 1.62e-6, 1.80e-6, 1.91e-6),   # caps 1.35e-3, 2.67e-3, 3.28e-3, 3.79e-3
    "fp16": (3.55e-4, 4.80e-4, 5.43e-4, 5.79e-4),   # caps 6.77e-3, 1.33e-2, 1.64e-2, 1.89e-2
    "bf16": (4.22e-3, 5.58e-3, 6.20e-3, 6.56e-3),   # caps 4.37e-2, 7.06e-2, 7.69e-2, 8.09e-2
}
# surgery pooled, plain pooled, plain level-24 tokens, forward_original patches / cls, teacher
# feature (train.py:74-85, level 24): rel-L2, MEASURED; bound = twice, capped by the level-24 cap
MEASURED_OUTPUTS = {
    "fp32": dict(surg_pooled=2.24e-6, plain_pooled=1.34e-6, plain_tok24=1.12e-6, fo_patch=1.30e-6, fo_cls=1.34e-6,
                 teacher=1.40e-6),
    "fp16": dict(surg_pooled=6.21e-4, plain_pooled=3.51e-4, plain_tok24=2.85e-4, fo_patch=3.55e-4, fo_cls=3.51e-4,
                 teacher=3.98e-4),
    "bf16": dict(surg_pooled=7.39e-3, plain_pooled=5.93e-3, plain_tok24=5.10e-3, fo_patch=5.64e-3, fo_cls=5.93e-3,
                 teacher=5.92e-3),
}

# ---- second shape (70 px, B = 16 / 17) against the fp32 CPU restatement, rel-L2 per level.
# Reasoned, not cut from a measurement (measured: fp32 1.4 - 1.9e-6, fp16 4.4 - 6.4e-4):
# an fp32 GEMM output carries ~sqrt(K) u = 4e-6 (K = 4096, u = 6e-8) relative error, ~4 GEMMs in each of 24 blocks add like a random walk to ~4e-5, and the CPU
# side carries as much: 1e-4. fp16 operands (u = 4.9e-4, rms u / sqrt(3)) through ~5 rounded
# tensors per block and 24 blocks: sqrt(120) * 2.8e-4 = 3e-3 -> 5e-3 (the reference run
# entirely in half precision sits at 1.0 - 1.7e-3). A wrong lane / padding path at these
# batch sizes is an O(1) error.
SECOND_SHAPE_TOL = {"fp32": 1e-4, "fp16": 5e-3}


def _bound(measured, cap):
    return min(2.0 * measured, cap)


def _caps(gold, name):
    if name == "fp32":
        return gold["rel_drop_one"] / 10
    if name == "fp16":
        return gold["rel_drop_one"] / 2
    return gold["rel_plain"] / 10


# =============================================================================== kernel
@functools.lru_cache(maxsize=None)
def _case(name, batch, n_tok, heads):
    """Inputs rounded to the storage type, and the float64 reference on those values."""
    v = torch.from_numpy(SR.vv_inputs(1000 + batch * 31 + n_tok, batch, n_tok, heads)).to(DT[name])
    ref, diag = SR.vv_attention_ref(v.double().numpy(), batch, n_tok, heads)
    return v, ref, diag


def _run(v, batch, n_tok, heads, dev):
    vd = v.to(dev)
    out = torch.empty_like(vd)
    ops.vv_attention(vd, out, batch, n_tok, heads)
    return out


SHAPES = [(1, 3, 16), (2, 1, 16), (5, 7, 16), (5, 7, 2), (16, 7, 16), (17, 4, 16), (33, 3, 16), (64, 2, 16),
          (3, 577, 16)]


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("batch,n_tok,heads", SHAPES)
def test_vv_attention_against_float64(dev, name, batch, n_tok, heads):
    v, ref, diag = _case(name, batch, n_tok, heads)
    if batch >= 5:  # the softmax really mixes images (a kernel ignoring the batch must fail)
        assert diag <= 0.7, diag
    out = _run(v, batch, n_tok, heads, dev).double().cpu().numpy()
    err = float(np.abs(out - ref).max())
    print(f"vv {name} B={batch} n_tok={n_tok} heads={heads}: max abs err {err:.2e}, mean diag p {diag:.2f}")
    assert np.isfinite(out).all()
    assert err <= KERNEL_TOL[name], err


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
def test_vv_attention_addressing(dev, name):
    """v as the V third of a packed [R, 3W] buffer whose q / k thirds are NaN, against v
    as its own buffer; out with a wider row stride and guard rows, whose sentinel
    (columns past W, rows before and after) comes back untouched."""
    batch, n_tok, heads = 5, 7, 16
    W, R = heads * 64, batch * n_tok
    v, _, _ = _case(name, batch, n_tok, heads)
    own = _run(v, batch, n_tok, heads, dev)
    qkv = torch.full((R, 3 * W), float("nan"), device=dev, dtype=DT[name])
    qkv[:, 2 * W:] = v.to(dev)
    ld_out, guard, sentinel = W + 64, 3, -7.25
    buf = torch.full((R + 2 * guard, ld_out), sentinel, device=dev, dtype=DT[name])
    out = buf[guard:guard + R, :W]
    ops.vv_attention(qkv[:, 2 * W:], out, batch, n_tok, heads)
    assert torch.equal(out, own)
    assert torch.isfinite(out).all()
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + R:] == sentinel).all())
    assert bool((buf[:, W:] == sentinel).all())
    assert bool(torch.isnan(qkv[:, :2 * W]).all()) and torch.equal(qkv[:, 2 * W:], v.to(dev))
    with pytest.raises(ValueError, match="overlap"):
        ops.vv_attention(qkv[:, 2 * W:], qkv[:, :W], batch, n_tok, heads)
    with pytest.raises(ValueError, match="1..64"):
        ops.vv_attention(torch.empty(65, W, device=dev, dtype=DT[name]),
                         torch.empty(65, W, device=dev, dtype=DT[name]), 65, 1, heads)


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
def test_vv_attention_exact_properties(dev, name):
    # a batch of one returns v bit for bit
    v1, _, _ = _case(name, 1, 3, 16)
    assert torch.equal(_run(v1, 1, 3, 16, dev).cpu(), v1)
    # two launches are bit-identical
    batch, n_tok, heads = 5, 7, 16
    v, ref, _ = _case(name, batch, n_tok, heads)
    a, b = _run(v, batch, n_tok, heads, dev), _run(v, batch, n_tok, heads, dev)
    assert torch.equal(a, b)
    # token 3 of the n_tok = 7 call == a call on that token alone
    W = heads * 64
    tok3 = v.view(batch, n_tok, W)[:, 3].contiguous()
    alone = _run(tok3, batch, 1, heads, dev)
    assert torch.equal(a.view(batch, n_tok, W)[:, 3], alone)
    # permuting the images permutes the outputs (the sums run in another order: dtype bound)
    perm = torch.tensor([3, 0, 4, 1, 2])
    vp = v.view(batch, n_tok, W)[perm].reshape(batch * n_tok, W).contiguous()
    ap = _run(vp, batch, n_tok, heads, dev).view(batch, n_tok, W)
    err = float((ap.double() - a.view(batch, n_tok, W)[perm.to(dev)].double()).abs().max())
    print(f"vv {name} permutation: max abs diff {err:.2e}")
    assert err <= KERNEL_TOL[name]


# =============================================================================== engine
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_surgery.npz"))


@pytest.fixture(scope="module")
def models(dev):
    """create_model objects on the synthetic weights, as train.py:235-262 sets them up: a
    surgery tower (DAPM_replace(20)) and an AdaptedCLIP around a plain one."""
    from model.adapter import AdaptedCLIP
    from model.clip import create_model
    sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(111).items()}
    out = []
    for _ in range(2):
        m = create_model("ViT-L-14-336", 336, pretrained=None, device="cpu")
        m.load_state_dict(sd, strict=True)
        out.append(m.to(dev).eval())
    clip_surgery, clip = out
    clip_surgery.visual.DAPM_replace(DPAM_layer=20)
    x = torch.from_numpy(synth.images(111, 3, 336)).to(dev)
    return clip_surgery, AdaptedCLIP(clip).to(dev).eval(), x


def _teacher(clip_surgery, adapted_model, image):
    """reference train.py:74-85, copied unchanged."""
    with torch.no_grad():
        _, patch_features = clip_surgery.encode_image(image, [6, 12, 18, 24])
        cls_token, _ = adapted_model.clipmodel.encode_image(image, [])
        cls_token = cls_token / cls_token.norm(dim=-1, keepdim=True)
        patch_features = [
            clip_surgery.visual.ln_post(t[:, 1:, :]) for t in patch_features
        ]
        patch_features = [t @ clip_surgery.visual.proj for t in patch_features]
        patch_features = [
            t / t.norm(dim=-1, keepdim=True) for t in patch_features
        ]
        patch_features = [t + cls_token.unsqueeze(1) for t in patch_features]
    return patch_features


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
def test_engine_against_reference_goldens(dev, gold, models, name, monkeypatch):
    clip_surgery, adapted, x = models
    monkeypatch.setenv("AACLIP_DTYPE", name)
    adapted.compute_dtype = DT[name]
    caps = _caps(gold, name)
    rows = list(gold["rows"])
    prow = list(gold["patch_rows"])
    eng = clip_surgery.visual.frozen_engine(DT[name])
    assert isinstance(eng, FrozenVisualEngine) and eng.surgery_from == 5 and eng.dtype == DT[name]
    assert clip_surgery.visual.frozen_engine(DT[name]) is eng  # cached on signature + DPAM layer

    # ---- surgery tokens, batch of 3 and batch of 1: rel-L2 on the stored rows + every row norm
    level_err = np.zeros(4)
    pooled_err = 0.0
    for key, xb in (("3", x), ("1", x[:1])):
        pooled, toks = clip_surgery.encode_image(xb, [6, 12, 18, 24])
        assert len(toks) == 4 and toks[0].shape == (xb.shape[0], 577, 1024) and toks[0].dtype == torch.float32
        assert pooled.shape == (xb.shape[0], 768) and pooled.dtype == torch.float32
        for j, tk in enumerate(toks):
            tk = tk.cpu().numpy()
            assert np.isfinite(tk).all()
            r = SR.rel_l2(tk[:, rows], gold["surg_tok" + key][j])
            rn = SR.rel_l2(np.linalg.norm(tk, axis=-1), gold["surg_norm" + key][j])
            level_err[j] = max(level_err[j], r, rn)
        pooled_err = max(pooled_err, SR.rel_l2(pooled.cpu().numpy(), gold["surg_pooled" + key]))
    print(f"engine {name} surgery tokens rel-L2 per level: {[f'{e:.3e}' for e in level_err]} "
          f"(caps {[f'{c:.3e}' for c in caps]}), pooled {pooled_err:.3e}")

    # ---- plain tower, forward_original, teacher feature
    plain_pooled, none = adapted.clipmodel.encode_image(x, [])
    assert none == []
    _, (tok24,) = adapted.clipmodel.encode_image(x, [24])
    fo_patch, fo_cls = adapted.forward_original(x)
    assert len(fo_patch) == 1 and fo_patch[0].shape == (3, 576, 768) and fo_cls.shape == (3, 768)
    teacher = _teacher(clip_surgery, adapted, x)
    errs = dict(
        surg_pooled=pooled_err,
        plain_pooled=SR.rel_l2(plain_pooled.cpu().numpy(), gold["plain_pooled"]),
        plain_tok24=SR.rel_l2(tok24.cpu().numpy()[:, rows], gold["plain_tok24"]),
        fo_patch=SR.rel_l2(fo_patch[0].cpu().numpy()[:, prow], gold["fo_patch"]),
        fo_cls=SR.rel_l2(fo_cls.cpu().numpy(), gold["fo_cls"]),
        teacher=SR.rel_l2(teacher[-1].cpu().numpy()[:, prow], gold["teacher24"]),
    )
    print(f"engine {name} outputs rel-L2: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))

    for j in range(4):
        assert level_err[j] <= _bound(MEASURED_TOKENS[name][j], caps[j]), (j, level_err[j])
    for k, v in errs.items():
        assert v <= _bound(MEASURED_OUTPUTS[name][k], caps[3]), (k, v)


@pytest.mark.parametrize("name", ["fp32", "fp16"])
def test_copied_train_block_equals_golden_teacher(dev, gold, models, name, monkeypatch):
    """reference train.py:74-85, unchanged, on create_model objects; the compute dtype comes
    from AACLIP_DTYPE as for every other entry point (default fp16)."""
    clip_surgery, adapted, x = models
    if name == "fp16":
        monkeypatch.delenv("AACLIP_DTYPE", raising=False)
    else:
        monkeypatch.setenv("AACLIP_DTYPE", name)
    feats = _teacher(clip_surgery, adapted, x)
    assert len(feats) == 4 and all(f.shape == (3, 576, 768) and f.is_cuda for f in feats)
    err = SR.rel_l2(feats[-1].cpu().numpy()[:, list(gold["patch_rows"])], gold["teacher24"])
    print(f"train.py block {name}: teacher rel-L2 {err:.3e}")
    assert err <= _bound(MEASURED_OUTPUTS[name]["teacher"], _caps(gold, name)[3])
    assert clip_surgery.visual.ln_post.weight.is_cuda and clip_surgery.visual.proj.is_cuda


@pytest.fixture(scope="module")
def small(dev):
    """70 px tower (5 x 5 patches + CLS = 26 tokens), surgery from block 5; the fp32 CPU
    restatement for B = 17 and B = 16 (the batches differ: the images are coupled)."""
    sd = synth.clip_state_dict(111, img_size=70)
    w = SR.prepare(sd)
    x = synth.images(112, 17, 70)
    ref = {B: SR.frozen_forward(w, x[:B], SR.LEVELS, surgery_from=5) for B in (16, 17)}
    vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
    return vp, torch.from_numpy(x).to(dev), ref


@pytest.mark.parametrize("name", ["fp32", "fp16"])
@pytest.mark.parametrize("B", [16, 17])
def test_engine_second_shape_against_restatement(dev, small, name, B):
    vp, x, ref = small
    eng = FrozenVisualEngine(vp, dtype=DT[name], surgery_from=5)
    eng.poison = True  # new workspaces start as NaN: a read-before-write shows
    pooled, toks = eng.encode(x[:B], SR.LEVELS)
    rp, rt = ref[B]
    errs = [SR.rel_l2(t.cpu().numpy(), r.numpy()) for t, r in zip(toks, rt)]
    ep = SR.rel_l2(pooled.cpu().numpy(), rp.numpy())
    print(f"70 px {name} B={B}: tokens rel-L2 {[f'{e:.3e}' for e in errs]}, pooled {ep:.3e}")
    assert all(np.isfinite(t.cpu().numpy()).all() for t in toks)
    assert max(errs) <= SECOND_SHAPE_TOL[name] and ep <= SECOND_SHAPE_TOL[name]
    # a second call reuses the workspace and gives the same bits
    pooled2, toks2 = eng.encode(x[:B], SR.LEVELS)
    assert torch.equal(pooled, pooled2) and all(torch.equal(a, b) for a, b in zip(toks, toks2))


def test_engine_errors(dev, small):
    vp, x, _ = small
    eng = FrozenVisualEngine(vp, dtype=torch.float16, surgery_from=5)
    with pytest.raises(ValueError, match="at most 64"):
        eng.encode(torch.zeros(65, 3, 70, 70, device=dev), [])
    with pytest.raises(ValueError, match="multiple of 14"):
        eng.encode(torch.zeros(1, 3, 72, 72, device=dev), [])
    with pytest.raises(RuntimeError, match="patch_features"):
        eng.patch_features()
    # a plain tower takes any batch: above max_chunk it runs as chunks (arithmetic checked on
    # the host, tests/test_surgery_host.py; not run here)
    assert not FrozenVisualEngine(vp, dtype=torch.float16).surgery
