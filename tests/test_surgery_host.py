"""Host-side checks of the frozen CLIP image paths (no GPU): the torch-CPU restatement
the GPU tests lean on is pinned to the reference's goldens (golden_surgery.npz, made by
tests/golden/make_golden_surgery.py from the real reference), and the C ABI / reference
API surface of the feature exists and validates its arguments without a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from aaclip import _lib
from oracle import synth

import surgery_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_surgery.npz"))


@pytest.fixture(scope="module")
def restated():
    """One fp32 run of the restatement per fixture batch, shared by the tests below (the
    plain tower is per-image, so image 0 alone stands for its batch of 3)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    w = SR.prepare(synth.clip_state_dict(111))
    x = synth.images(111, 3, 336)
    return dict(w=w, surg3=SR.frozen_forward(w, x, SR.LEVELS, surgery_from=5),
                surg1=SR.frozen_forward(w, x[:1], SR.LEVELS, surgery_from=5),
                plain=SR.frozen_forward(w, x[:1], [24]))


def test_golden_fixture_is_what_the_issue_describes(gold):
    assert list(gold["rows"]) == SR.ROWS and list(gold["levels"]) == SR.LEVELS
    assert list(gold["replaced_blocks"]) == list(range(5, 24))  # DAPM_replace(20): blocks 5..23
    assert gold["clip_sha"] == synth.state_checksum(synth.clip_state_dict(111))
    assert gold["surg_tok3"].shape == (4, 3, 8, 1024) and gold["surg_norm3"].shape == (4, 3, 577)
    # the batch really matters (the yardsticks the GPU caps are cut from), and grows with depth
    assert np.all(gold["rel_drop_one"] > 5e-3) and np.all(gold["rel_plain"] > 0.3)
    assert np.all(np.diff(gold["rel_drop_one_full"]) > 0)


def test_restatement_matches_reference_surgery_tower(gold, restated):
    """fp32 restatement against the reference's fp32 run: <= 1e-5 rel-L2 per level (the
    reference block restated alone gave 9.5e-7), batch of 3 and batch of 1."""
    for tag, key in (("surg3", "3"), ("surg1", "1")):
        pooled, toks = restated[tag]
        for j, tk in enumerate(toks):
            tk = tk.numpy()
            r = SR.rel_l2(tk[:, SR.ROWS], gold["surg_tok" + key][j])
            rn = SR.rel_l2(np.linalg.norm(tk, axis=-1), gold["surg_norm" + key][j])
            print(f"batch {key} level {SR.LEVELS[j]}: rel-L2 {r:.2e}, row norms {rn:.2e}")
            assert r <= 1e-5 and rn <= 1e-5
        assert SR.rel_l2(pooled.numpy(), gold["surg_pooled" + key]) <= 1e-5


def test_restatement_matches_reference_plain_tower_and_teacher(gold, restated):
    w = restated["w"]
    pooled, (tok24,) = restated["plain"]
    assert SR.rel_l2(pooled.numpy(), gold["plain_pooled"][:1]) <= 1e-5
    assert SR.rel_l2(pooled.numpy(), gold["fo_cls"][:1]) <= 1e-5
    assert SR.rel_l2(tok24.numpy()[:, SR.ROWS], gold["plain_tok24"][:1]) <= 1e-5
    prow = list(gold["patch_rows"])
    assert SR.rel_l2(SR.patch_project(w, tok24).numpy()[:, prow], gold["fo_patch"][:1]) <= 1e-5
    # train.py:74-85 at level 24: unit surgery patch features + the unit plain CLS (image 0)
    f = SR.patch_project(w, restated["surg3"][1][-1][:1])
    f = f / f.norm(dim=-1, keepdim=True) + (pooled / pooled.norm(dim=-1, keepdim=True)).unsqueeze(1)
    assert SR.rel_l2(f.numpy()[:, prow], gold["teacher24"][:1]) <= 1e-5


def test_vv_reference_properties():
    """The float64 kernel reference: identity at batch 1, and on the GPU tests' inputs the
    softmax really mixes images (mean diagonal probability 0.61 / 0.31 / 0.10 at B = 5 /
    16 / 64; plain randn would give 0.998 and hide a kernel that ignores the batch)."""
    v = SR.vv_inputs(3, 1, 3, 16)
    out, diag = SR.vv_attention_ref(v, 1, 3, 16)
    assert np.array_equal(out, v.astype(np.float64)) and diag == 1.0
    for B, want in ((5, 0.61), (16, 0.31), (64, 0.10)):
        _, diag = SR.vv_attention_ref(SR.vv_inputs(3, B, 4, 16), B, 4, 16)
        assert abs(diag - want) < 0.08, (B, diag)


# ---------------------------------------------------------------------------- C ABI
def test_abi_8_declares_binds_and_exports_vv_attention():
    src = open(os.path.join(ROOT, "include", "aaclip.h")).read()
    assert re.search(r"int aaclip_vv_attention\(int dtype, const void\* v, int64_t ld_v, void\* out, int64_t ld_out,"
                     r"\s+int batch, int n_tok, int heads, int head_dim, void\* stream\);", src)
    assert re.search(r"#define AACLIP_VV_MAX_BATCH 64\b", src)
    assert "transformer.py:125-152" in src and "407-425" in src
    assert "aaclip_vv_attention" in _lib.SIGNATURES and len(_lib.SIGNATURES["aaclip_vv_attention"]) == 10
    assert _lib.ABI_VERSION == 9 and _lib.VV_MAX_BATCH == 64
    lib = _lib.lib()
    assert lib.aaclip_abi_version() == 9 and hasattr(lib, "aaclip_vv_attention")


def test_vv_attention_rejects_bad_arguments_without_a_launch():
    vv = _lib.lib().aaclip_vv_attention
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        assert vv(dt, p, 1024, q, 1024, 3, 7, 16, 128, None) == 1      # head_dim
        assert vv(dt, p, 1024, q, 1024, 0, 7, 16, 64, None) == 1       # batch 0
        assert vv(dt, p, 1024, q, 1024, 65, 7, 16, 64, None) == 1      # batch 65
        assert vv(dt, None, 1024, q, 1024, 3, 7, 16, 64, None) == 1    # null v
        assert vv(dt, p, 1024, None, 1024, 3, 7, 16, 64, None) == 1    # null out
        assert vv(dt, p, 1016, q, 1024, 3, 7, 16, 64, None) == 1       # ld_v < heads*64
        assert vv(dt, p, 3072, q, 960, 3, 7, 16, 64, None) == 1        # ld_out < heads*64
        assert vv(dt, p, 1024, p, 1024, 3, 7, 16, 64, None) == 1       # out aliases v
        assert vv(dt, p, 1024, q, 1024, 3, 0, 16, 64, None) == 1       # no tokens
        assert vv(dt, p, 1024, q, 1024, 64, 1 << 26, 16, 64, None) == 1  # batch*n_tok past an int
    assert vv(_lib.FP8, p, 1024, q, 1024, 3, 7, 16, 64, None) == 1     # no fp8 form
    # 16-bit strides / starts that break the 8-element (128-bit) vector; fp32: 4 elements
    assert vv(_lib.F16, p, 1028, q, 1024, 3, 7, 16, 64, None) == 1
    assert vv(_lib.BF16, p, 1024, q, 1036, 3, 7, 16, 64, None) == 1
    assert vv(_lib.F16, ctypes.c_void_p(4096 + 8), 1024, q, 1024, 3, 7, 16, 64, None) == 1
    assert vv(_lib.F32, p, 1026, q, 1024, 3, 7, 16, 64, None) == 1


# ---------------------------------------------------------------------------- reference API
def _model():
    from model.clip import create_model
    return create_model("ViT-L-14-336", 336, pretrained=None, device="cpu")


def test_dapm_replace_bookkeeping():
    m = _model()
    v = m.visual
    assert list(v.surgery_blocks) == []
    v.DAPM_replace(DPAM_layer=None)
    v.DAPM_replace(1)
    assert list(v.surgery_blocks) == [] and v.DPAM_layer is None
    v.DAPM_replace(DPAM_layer=20)
    assert list(v.surgery_blocks) == list(range(5, 24))
    with pytest.raises(ValueError, match="24"):
        v.DAPM_replace(26)
    assert list(v.surgery_blocks) == list(range(5, 24))
    v.DAPM_replace(25)
    assert list(v.surgery_blocks) == list(range(24))
    # the parameters keep their nn.MultiheadAttention names
    assert "transformer.resblocks.23.attn.in_proj_weight" in v.state_dict()
    cls, patches = v._global_pool(torch.zeros(2, 5, 8))
    assert cls.shape == (2, 8) and patches.shape == (2, 4, 8)


def test_frozen_paths_exist_and_need_device_tensors():
    """On CPU tensors the three entry points stop at the engine's "needs device tensors",
    no longer at NotImplementedError."""
    from model.adapter import AdaptedCLIP
    m = _model()
    x = torch.zeros(1, 3, 336, 336)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        m.encode_image(x, [6, 12, 18, 24])
    m.visual.DAPM_replace(DPAM_layer=20)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        m.encode_image(x, [])
    with pytest.raises(ValueError, match="normalize"):
        m.encode_image(x, [], normalize=True)
    a = AdaptedCLIP(_model(), compute_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        a.forward_original(x)
    with pytest.raises(ValueError, match="modality"):
        a.forward_original(x, modality="text")


def test_frozen_engine_host_checks():
    """dtype / surgery_from validation comes before any device work; the plain tower's
    chunk arithmetic (batches above max_chunk) is host logic."""
    from aaclip.engine import FrozenVisualEngine, VisualEngine
    with pytest.raises(ValueError, match="fp8"):
        FrozenVisualEngine({}, dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="surgery_from"):
        FrozenVisualEngine({}, dtype=torch.float16, surgery_from=24)
    mc = FrozenVisualEngine.max_chunk(336)
    assert mc == VisualEngine.max_chunk(336) and mc * 577 * 3072 * 2 < 2 ** 31 <= (mc + 1) * 577 * 3072 * 2
    b = FrozenVisualEngine.chunk_bounds(2 * mc + 5, mc)
    assert b == [(0, mc), (mc, 2 * mc), (2 * mc, 2 * mc + 5)]
    assert FrozenVisualEngine.chunk_bounds(mc, mc) == [(0, mc)] and FrozenVisualEngine.chunk_bounds(1, mc) == [(0, 1)]
