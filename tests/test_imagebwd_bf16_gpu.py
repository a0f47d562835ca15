"""Stage-2 training in bf16 mixed precision on the MI355X (csrc/visual_bwd16.hip,
VisualEngine.forward_train on a bf16 engine, AdaptedCLIP(train_dtype=bfloat16), AACLIP_TRAIN_DTYPE).

Bound: the device's error against fp64 is at most 2 x the error of tests/imagebwd_bf16_ref.py, the
recipe restated in fp32 torch on the CPU with a rounding at every tensor the recipe stores in bf16,
against the same fp64 (rel-L2). bf16 rounding and LeakyReLU's kink make the step chaotic at the
level of a few per cent, so the device is never compared with the restatement directly. Every
figure is printed before it is asserted.

Measured on an MI355X (device error / restatement error, both against fp64): see DESIGN.md
section 5, "Stage-2 in bf16"."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth

import imagebwd_bf16_ref as E
import imagebwd_ref as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _np(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def within(name, got, truth, yard, rows=False):
    """err(got vs fp64) <= 2 x err(restatement vs fp64); rows: the worst single row's too."""
    got, truth, yard = _np(got), _np(truth), _np(yard)
    assert got.shape == truth.shape == yard.shape, (name, got.shape, truth.shape, yard.shape)
    e, y = IR.rel_l2(got, truth), IR.rel_l2(yard, truth)
    print(f"{name}: err {e:.3e}  restatement {y:.3e}  ratio {e / max(y, 1e-300):.2f}  bound {2 * y:.3e}")
    ok = e <= 2 * y
    if rows:
        er, yr = E.worst_row(got, truth), E.worst_row(yard, truth)
        print(f"{name}, worst row: err {er:.3e}  restatement {yr:.3e}  ratio {er / max(yr, 1e-300):.2f}  bound {2 * yr:.3e}")
        ok = ok and er <= 2 * yr
    assert ok, name


def rnd(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def bf(a):
    """A float32 array rounded to bf16, as a float32 CPU tensor."""
    return E.r(torch.from_numpy(np.ascontiguousarray(a)))


# ---------------------------------------------------------------------------- the attention kernel
def _attn_case(dev, B, N, H, pre, seed=0):
    """The fp32 test's draws rounded to bf16 (with the folded scale on the q columns when pre), the
    forward's bf16 output from ops.attention."""
    from aaclip import ops
    qkv = torch.from_numpy(rnd(N * 31 + H + seed, B * N, 3 * H * 64))
    if pre:
        qkv[:, :H * 64] *= E.Q_SCALE
    qkv, dout = E.r(qkv), bf(rnd(N * 37 + H + seed, B * N, H * 64))
    qd, dd = qkv.to(dev, BF), dout.to(dev, BF)
    out = torch.empty(B * N, H * 64, device=dev, dtype=BF)
    ops.attention(qd, out, B, N, H, q_prescaled=pre)
    return qkv, dout, qd, dd, out


@pytest.mark.parametrize("pre", [False, True], ids=["scaled_at_load", "q_prescaled"])
@pytest.mark.parametrize("seq", [1, 5, 63, 64, 65, 130, 577])
def test_attention_bwd16(dev, seq, pre):
    from aaclip import ops
    B, H = 2, 3
    qkv, dout, qd, dd, out = _attn_case(dev, B, seq, H, pre)
    t = qkv.double().requires_grad_()
    E.attention_truth(t, B, seq, H, pre).backward(dout.double())  # fp64 autograd on the bf16-rounded inputs
    a = qkv.clone().requires_grad_()
    E.attention16(a, B, seq, H, pre).backward(dout)              # the kernel's roundings, by hand
    got = torch.full_like(qd, float("nan"))  # every element is written
    ops.attention_bwd16(qd, out, dd, B, seq, H, q_prescaled=pre, dqkv=got)
    assert bool(torch.isfinite(got).all())
    again = ops.attention_bwd16(qd, out, dd, B, seq, H, q_prescaled=pre)
    assert torch.equal(got, again)  # two launches, the same bits
    if seq == 1:  # softmax over one key: P = 1, dS = 0; dq = dk = 0 has no relative error
        d = got.view(B, 3, H * 64)
        assert torch.count_nonzero(d[:, :2]) == 0 and torch.equal(d[:, 2], dd)
        return
    within(f"attention_bwd16 seq {seq} prescaled {pre}", got, t.grad, a.grad, rows=True)
    for j, n in enumerate("qkv"):  # each of dq, dk, dv on its own: a wrong factor on one shows here
        c = slice(j * H * 64, (j + 1) * H * 64)
        within(f"attention_bwd16 seq {seq} prescaled {pre} d{n}", got[:, c], t.grad[:, c], a.grad[:, c])


def test_attention_bwd16_is_image_local(dev):
    """Image 1 of a batch of 3 gets the bits it gets when launched alone."""
    from aaclip import ops
    B, N, H = 3, 130, 2
    _, _, qd, dd, out = _attn_case(dev, B, N, H, True, seed=5)
    full = ops.attention_bwd16(qd, out, dd, B, N, H, q_prescaled=True)
    one = slice(N, 2 * N)
    alone = ops.attention_bwd16(qd[one].contiguous(), out[one].contiguous(), dd[one].contiguous(), 1, N, H,
                                q_prescaled=True)
    assert torch.equal(full[one], alone)


def test_attention_bwd16_rejects_bad_arguments(dev):
    from aaclip import _lib, ops
    B, N, H = 1, 70, 2
    _, _, qd, dd, out = _attn_case(dev, B, N, H, False)
    ws = ops.attention_bwd16_workspace(B, N, H, dev)
    assert ws.numel() == 2 * B * H * N
    dq = torch.empty_like(qd)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    fn = _lib.lib().aaclip_attention_bwd16
    args = lambda dt, dqkv, hd, nbytes: (dt, p(qd), p(out), p(dd), p(dqkv), B, N, H, hd, 0, p(ws), nbytes, None)  # noqa: E731
    full = ws.numel() * 4
    assert fn(*args(_lib.F16, dq, 64, full)) == 1 and fn(*args(_lib.F32, dq, 64, full)) == 1  # bf16 only
    assert fn(*args(_lib.BF16, dq, 32, full)) == 1           # head_dim != 64
    for alias in (qd, out, dd):
        assert fn(*args(_lib.BF16, alias, 64, full)) == 1    # dqkv aliases an input
    assert fn(*args(_lib.BF16, dq, 64, full - 4)) == 1       # short workspace
    with pytest.raises(ValueError, match="alias"):
        ops.attention_bwd16(qd, out, dd, B, N, H, dqkv=qd)
    with pytest.raises(ValueError, match="bfloat16"):
        ops.attention_bwd16(qd.half(), out.half(), dd.half(), B, N, H)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.attention_bwd16(qd, out, dd, B, N, H, workspace=ws[:-1])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- the row kernels
N_ACT = 4096 * 3 + 8  # whole 2048-element workgroups and a tail


@pytest.mark.parametrize("mode", ["gelu", "quick", "leaky"])
def test_act_to16_has_the_epilogue_bits(dev, mode):
    """A bias-only GEMM with fp32 output + act_to16 = the fused bf16 epilogue, bit for bit."""
    from aaclip import ops
    M, N, K = 13, 1024, 128
    a, w = bf(rnd(21, M, K)).to(dev, BF), bf(rnd(22, N, K, scale=0.2)).to(dev, BF)
    bias = torch.from_numpy(rnd(23, N)).to(dev) if mode != "leaky" else None
    pre = ops.gemm(a, w, torch.empty(M, N, device=dev), bias=bias)
    kw = dict(leaky=True) if mode == "leaky" else dict(gelu=True if mode == "gelu" else "quick")
    fused = ops.gemm(a, w, torch.empty(M, N, device=dev, dtype=BF), bias=bias, **kw)
    x = pre.flatten()[:N_ACT].contiguous()
    got = torch.full((N_ACT + 8,), float("nan"), device=dev, dtype=BF)
    ops.act_to16(x, mode, out=got[:N_ACT])
    assert torch.equal(got[:N_ACT], fused.flatten()[:N_ACT])
    assert bool(torch.isnan(got[N_ACT:]).all())  # nothing past the end
    assert float(got[:N_ACT].float().abs().max()) > 0.5


def _slope(v, mode):
    if mode == "gelu":
        return 0.5 * (1 + torch.erf(v * 2 ** -0.5)) + v * torch.exp(-0.5 * v * v) * (2 * np.pi) ** -0.5
    if mode == "quick":
        s = torch.sigmoid(1.702 * v)
        return s + 1.702 * v * s * (1 - s)
    return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, 0.01))


@pytest.mark.parametrize("mode", ["gelu", "quick", "leaky"])
def test_act_bwd16(dev, mode):
    from aaclip import ops
    dy, ref = bf(rnd(31, N_ACT)), torch.from_numpy(rnd(32, N_ACT, scale=2.0))
    truth = dy.double() * _slope(ref.double(), mode)
    yard = E.r(dy * _slope(ref, mode))  # the formula in fp32, rounded
    got = torch.full((N_ACT + 8,), float("nan"), device=dev, dtype=BF)
    ops.act_bwd16(dy.to(dev, BF), ref.to(dev), mode, out=got[:N_ACT])
    assert bool(torch.isnan(got[N_ACT:]).all())
    within(f"act_bwd16 {mode}", got[:N_ACT], truth, yard)
    inplace = dy.to(dev, BF)
    assert ops.act_bwd16(inplace, ref.to(dev), mode, out=inplace) is inplace and torch.equal(inplace, got[:N_ACT])


def test_cast_rows_is_torch_to(dev):
    """Both directions, rows a padded leading dimension apart: the bits of torch's .to()."""
    from aaclip import ops
    rows, cols = 37, 1024
    x32 = torch.from_numpy(rnd(41, rows, cols + 8, scale=3.0)).to(dev)
    x32[0, :4] = torch.tensor([1 + 2.0 ** -9, 1 + 3 * 2.0 ** -9, -0.0, 3.3e38], device=dev)  # ties to even, -0, overflow
    src = x32[:, :cols]
    dst = torch.full((rows, cols + 16), 7.0, device=dev, dtype=BF)
    assert ops.cast_rows(src, dst[:, :cols]) is not None
    assert torch.equal(dst[:, :cols], src.to(BF)) and bool((dst[:, cols:] == 7).all())
    up = torch.full((rows, cols + 4), 7.0, device=dev)
    ops.cast_rows(dst[:, :cols], up[:, :cols])
    assert torch.equal(up[:, :cols], dst[:, :cols].float()) and bool((up[:, cols:] == 7).all())
    fresh = ops.cast_rows(src, dtype=BF)
    assert fresh.is_contiguous() and torch.equal(fresh, src.to(BF))
    assert torch.equal(ops.cast_rows(src, dtype=torch.float16), src.to(torch.float16))


# ---------------------------------------------------------------------------- the tower
NAMES = IR.weight_names()


@pytest.fixture(scope="module")
def sd():
    return synth.clip_state_dict(111, img_size=IR.IMG)


def _engine(dev, sd, img, dtype=BF, quick=False, relu=False):
    from aaclip.engine import VisualEngine
    vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
    n_tok = (img // 14) ** 2 + 1
    vp["visual.positional_embedding"] = vp["visual.positional_embedding"][:n_tok].contiguous()
    ia, _ = synth.adapter_state_dicts(111, relu=relu)
    ad = {k: torch.from_numpy(v).to(dev) for k, v in ia.items()}
    return VisualEngine(vp, ad, dtype=dtype, quick_gelu=quick), ad


@pytest.mark.parametrize("img", [70, 112])  # 26 and 65 tokens: under one tile, one tile and a tail of 1
def test_one_frozen_block(dev, sd, img):
    """dL/dx_in through _train_block_fwd / _block_bwd of a bf16 engine against fp64 imagebwd_ref.block on
    the weights the engine packed (bf16-rounded, the Q fold undone). No LeakyReLU: the tight check."""
    from aaclip import engine, ops
    i, B, W = 7, 2, IR.WIDTH
    eng, _ = _engine(dev, sd, img)
    assert eng.q_prescaled
    N = (img // 14) ** 2 + 1
    R = B * N
    x, dy = rnd(51, B, N, W), rnd(52, B, N, W)
    P16 = E.params16(sd)
    t = torch.from_numpy(x).double().requires_grad_()
    IR.block(E.unscaled(P16), i, t).backward(torch.from_numpy(dy).double())
    a = torch.from_numpy(x).requires_grad_()
    E.block16(P16, i, a).backward(torch.from_numpy(dy))
    blk = eng.blocks[i]
    c = lambda *s: torch.empty(*s, device=dev, dtype=BF)  # noqa: E731
    e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    X, H, saved = torch.from_numpy(x).to(dev).view(R, W), c(R, W), {}
    with torch.cuda.device(dev):
        ops.layernorm(X, blk["ln1"][0], blk["ln1"][1], H)
        attend = lambda qkv, att: ops.attention(qkv, att, B, N, engine.HEADS, q_prescaled=True)  # noqa: E731
        Y, u = engine._train_block_fwd(blk, X, H, (c(R, 3 * W), c(R, W), c(R, 4 * W), e(R, W), c(R, W)), attend,
                                       keep=True, keep_blend=False, keep_att=True, act=eng.act, w_adapt=None,
                                       saved=saved, i=i, dtype=BF)
        assert u is None and set(saved[i]) == {"x_in", "qkv", "x_mid", "fc_pre", "att"}
        sv = saved[i]
        assert sv["x_in"].dtype == sv["x_mid"].dtype == sv["fc_pre"].dtype == torch.float32
        assert sv["qkv"].dtype == sv["att"].dtype == BF
        bt = engine._bwd_weights(eng.blocks, i + 1)[i]
        assert bt["w_qkv"].dtype == BF and bt["w_qkv"].shape == (W, 3 * W)
        ws = ops.attention_bwd16_workspace(B, N, engine.HEADS, dev)
        attend_bwd = lambda s, d_att, dqkv: ops.attention_bwd16(  # noqa: E731
            s["qkv"], s["att"], d_att, B, N, engine.HEADS, q_prescaled=True, dqkv=dqkv, workspace=ws)
        g = torch.from_numpy(dy).to(dev).view(R, W).clone()
        engine._block_bwd(g, blk, bt, sv, attend_bwd, "gelu", c(R, 3 * W), c(R, 4 * W), e(R, W), lo=(c(R, W), c(R, W)))
    within(f"one frozen block at {N} tokens, dL/dx_in", g.view(B, N, W), t.grad, a.grad, rows=True)


@pytest.mark.parametrize("img,batch", [(112, 2), (70, 3)])
@pytest.mark.parametrize("quick", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_training_forward_has_forward_bits(dev, sd, img, batch, quick, relu):
    eng, ad = _engine(dev, sd, img, quick=quick, relu=relu)
    x = torch.from_numpy(synth.images(7, batch, img)).to(dev)
    seg0, det0 = eng.forward(x)
    ws = [ad[n].clone().requires_grad_() for n in IR.weight_names(relu=relu)]

    def same():
        seg, det = eng.forward_train(x, ws)
        assert seg[0].grad_fn is not None and det.grad_fn is not None
        assert all(torch.equal(a.detach(), b) for a, b in zip(seg, seg0)) and torch.equal(det.detach(), det0)
    same()                       # the whole tower above block 0 keeps its activations
    for w in ws[:3]:
        w.requires_grad_(False)  # lowest trainable adapter 3
    same()
    for w in ws[:6]:
        w.requires_grad_(False)  # only the projections train
    same()
    if img == 70 and not quick and not relu:  # fp16 (no loss scaling here) and fp8 engines still refuse
        for dt in (torch.float16, torch.float8_e4m3fn):
            with pytest.raises(RuntimeError, match="fp32 only"):
                _engine(dev, sd, img, dtype=dt)[0].forward_train(x, ws)


@pytest.fixture(scope="module")
def clip(dev, sd):
    from model.clip import create_model
    c = create_model("ViT-L-14-336", IR.IMG, pretrained=None, device=dev, force_image_size=IR.IMG)
    c.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return c


@pytest.fixture(scope="module")
def model(dev, clip):
    from model.adapter import AdaptedCLIP
    m = AdaptedCLIP(clip, relu=False, compute_dtype=BF, train_dtype=BF).to(dev).eval()
    ia, _ = synth.adapter_state_dicts(111)
    m.image_adapter.load_state_dict({k: torch.from_numpy(v) for k, v in ia.items()})
    for p in m.parameters():
        p.requires_grad_(False)
    for p in m.image_adapter.parameters():
        p.requires_grad_(True)
    return m


@pytest.fixture(scope="module")
def x_np():
    return synth.images(IR.X_SEED, IR.BATCH, IR.IMG)


def _clear(m):
    for w in m._adapter_weights():
        w.grad = None


@pytest.fixture(scope="module")
def fixture_run(dev, model, sd, x_np):
    """The fixture's "grad" case once: on the device through the public API (gradients and dL/dx after
    the tapped blocks kept), then fp64 (truth) and the bf16 restatement (yardstick) on the CPU."""
    G = IR.loss_weights((IR.IMG // 14) ** 2)
    eng = model.visual_engine()
    assert eng.dtype == BF
    eng.tap_blocks, eng.tap_records = tuple(IR.TAPS), []
    _clear(model)
    try:
        seg, det = model(torch.from_numpy(x_np).to(dev))
        loss = IR.fixture_loss(seg, det, [torch.from_numpy(g).to(dev) for g in G])
        loss.backward()
        records = list(eng.tap_records)
    finally:
        eng.tap_blocks, eng.tap_records = (), []
    ws = model._adapter_weights()
    assert all(w.grad.dtype == torch.float32 and w.dtype == torch.float32 for w in ws)
    grads = [w.grad.detach().clone() for w in ws]
    _clear(model)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ia, _ = synth.adapter_state_dicts(111)
    r64 = IR.run(sd, ia, x_np, G, torch.float64)
    r16 = E.run16(sd, ia, x_np, G)
    return dict(seg=[s.detach() for s in seg], det=det.detach(), loss=float(loss.detach()), grads=grads,
                records=records, r64=r64, r16=r16, G=G)


def test_outputs_and_loss_on_the_fixture(fixture_run):
    f = fixture_run
    for j in range(4):
        within(f"seg {j}", f["seg"][j], f["r64"]["seg"][j], f["r16"]["seg"][j])
    within("det", f["det"], f["r64"]["det"], f["r16"]["det"])
    e, y = abs(f["loss"] - f["r64"]["loss"]), abs(f["r16"]["loss"] - f["r64"]["loss"])
    bound = max(2 * y, 8 * E.BF16_EPS * abs(f["r64"]["loss"]))  # floor: 8 bf16 ulps of the loss
    print(f"loss: {f['loss']:.6f} fp64 {f['r64']['loss']:.6f}  err {e:.3e}  restatement {y:.3e}  bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("i", range(11), ids=NAMES)
def test_gradients_on_the_fixture(fixture_run, i):
    """Each of the 11 .grads of L = sum_j sum(G_j seg_j) + sum(G_d det) against fp64 imagebwd_ref.run."""
    f = fixture_run
    assert torch.count_nonzero(f["grads"][i]) > 0 and bool(torch.isfinite(f["grads"][i]).all())
    within(f"d {NAMES[i]}", f["grads"][i], f["r64"]["grads"][i], f["r16"]["grads"][i])


@pytest.mark.parametrize("b", IR.TAPS)
def test_block_output_gradients_on_the_fixture(fixture_run, b):
    """dL/dx after blocks 23, 18, 12, 6, 5 and 0 (image 0): the tap_blocks diagnostic in bf16."""
    f = fixture_run
    assert len(f["records"]) == 1
    rec = f["records"][0]
    tap = rec["taps"][b].view(IR.BATCH, rec["n_tok"], -1)[0]
    assert tap.dtype == torch.float32  # the gradient stream stays fp32
    within(f"dL/dx after block {b}", tap, f["r64"]["taps"][b], f["r16"]["taps"][b])


def test_without_train_dtype_bf16_under_grad_is_the_forward_only_path(dev, clip, x_np):
    from model.adapter import AdaptedCLIP
    m = AdaptedCLIP(clip, relu=False, compute_dtype=BF).to(dev).eval()
    assert m.train_dtype is None
    ia, _ = synth.adapter_state_dicts(111)
    m.image_adapter.load_state_dict({k: torch.from_numpy(v) for k, v in ia.items()})
    x = torch.from_numpy(x_np).to(dev)
    assert torch.is_grad_enabled() and all(w.requires_grad for w in m._adapter_weights())
    seg, det = m(x)
    assert all(s.grad_fn is None and not s.requires_grad for s in seg) and det.grad_fn is None
    with torch.no_grad():
        seg0, det0 = m(x)
    assert all(torch.equal(a, b) for a, b in zip(seg, seg0)) and torch.equal(det, det0)
    with pytest.raises(ValueError, match="train_dtype"):
        AdaptedCLIP(clip, relu=False, compute_dtype=torch.float16, train_dtype=torch.float16)


def test_three_adam_steps_of_the_stage2_loop(dev, model, x_np):
    """train.py:134-159 through the public API on the fp32 test's inputs: finite losses, the last below
    the first, the frozen packing stays put. The distances from the reference's fp32 / fp64 losses
    (tests/golden/golden_imagebwd.npz) are printed, not asserted."""
    from forward_utils import calculate_seg_loss, calculate_similarity_map
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_imagebwd.npz"))
    gt = np.load(os.path.join(ROOT, "tests", "golden", "golden_text.npz"))
    mask_np, label_np = IR.adam_inputs()
    image, mask, label = (torch.from_numpy(a).to(dev) for a in (x_np, mask_np, label_np))
    epoch_text_feature = torch.from_numpy(np.stack([gt[k] for k in IR.ADAM_ANCHORS])).float().to(dev)
    keep = {k: v.detach().clone() for k, v in model.image_adapter.state_dict().items()}
    optimizer = torch.optim.Adam(model.image_adapter.parameters(), lr=IR.ADAM_LR, betas=IR.ADAM_BETAS)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(IR.ADAM_MILESTONES), gamma=0.5)

    def step_loss():
        patch_features, det_feature = model(image)
        loss = 0.0
        det_feature = det_feature.unsqueeze(1)
        cls_preds = torch.matmul(det_feature, epoch_text_feature)[:, 0]
        loss += F.cross_entropy(cls_preds, label)
        for f in patch_features:
            patch_preds = calculate_similarity_map(f, epoch_text_feature, IR.IMG)
            loss += calculate_seg_loss(patch_preds, mask)
        return loss

    losses = []
    try:
        eng, frozen = model.visual_engine(), None
        for _ in range(3):
            loss = step_loss()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
            scheduler.step()
            e2 = model.visual_engine()
            ptrs = (e2.conv.data_ptr(), e2.blocks[7]["w_fc"].data_ptr(), e2._bwd[7]["w_fc"].data_ptr(),
                    e2.blocks[23]["w_qkv"].data_ptr(), e2._bwd[23]["w_qkv"].data_ptr())
            assert e2 is eng and (frozen is None or frozen == ptrs)  # an optimizer step repacks nothing frozen
            frozen = ptrs
        with torch.no_grad():
            losses.append(float(step_loss()))
        assert all(p.dtype == torch.float32 for p in model.image_adapter.parameters())
    finally:
        model.image_adapter.load_state_dict(keep)
        _clear(model)
    l32, l64 = gold["adam_losses32"], gold["adam_losses64"]
    print("losses", losses, "reference fp32", l32.tolist(), "fp64", l64.tolist())
    print("distance from the reference's fp64 losses:", [f"{abs(a - b) / abs(b):.2e}" for a, b in zip(losses, l64)])
    assert np.all(np.isfinite(losses))
    assert losses[3] < losses[0]


def test_projection_only_training_keeps_no_tower_state(dev, model, fixture_run, x_np):
    """Only seg_proj.1 requires grad: nothing of the tower is saved, and its gradient meets the bound."""
    r64, r16, G = fixture_run["r64"], fixture_run["r16"], fixture_run["G"]
    ws = model._adapter_weights()
    _clear(model)
    try:
        for w in ws:
            w.requires_grad_(False)
        ws[7].requires_grad_(True)
        seg, det = model(torch.from_numpy(x_np).to(dev))
        st = seg[1].grad_fn.st
        assert st["lowest"] is None and st["blocks"] == {} and st["x_tap"] == {}
        IR.fixture_loss(seg, det, [torch.from_numpy(g).to(dev) for g in G]).backward()
        assert all((w.grad is not None) == (i == 7) for i, w in enumerate(ws))
        within("d seg_proj.1 alone", ws[7].grad, r64["grads"][7], r16["grads"][7])
    finally:
        for w in ws:
            w.requires_grad_(True)
        _clear(model)


# ---------------------------------------------------------------------------- train.py
TRAIN_ARGS = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4",
              "--text_epoch", "1", "--image_epoch", "1", "--max_steps", "2"]


def test_train_py_in_bf16_end_to_end(dev, tmp_path, monkeypatch):
    import test as harness
    import train
    monkeypatch.setenv("AACLIP_TRAIN_DTYPE", "bf16")
    save = str(tmp_path)
    ctx = train.run(train.parse_args(TRAIN_ARGS + ["--save_path", save]))
    m = ctx["model"]
    assert ctx["train_dtype"] == BF and m.compute_dtype == BF and m.train_dtype == BF
    assert m.visual_engine().dtype == BF and m.visual_engine()._bwd is not None  # stage 2 ran its backward in bf16
    assert len(ctx["image_losses"]) >= 1 and np.all(np.isfinite(ctx["image_losses"]))
    assert len(ctx["text_losses"]) >= 1 and np.all(np.isfinite(ctx["text_losses"]))
    files = sorted(os.path.basename(f) for f in glob.glob(save + "/*.pth"))
    assert files == ["image_adapter.pth", "image_adapter_1.pth", "text_adapter.pth"]
    t = torch.load(os.path.join(save, "text_adapter.pth"), map_location="cpu", weights_only=True)
    assert set(t) == {"epoch", "text_adapter", "text_optimizer"}
    c = torch.load(os.path.join(save, "image_adapter_1.pth"), map_location="cpu", weights_only=True)
    assert set(c) == {"epoch", "image_adapter", "image_optimizer"} and c["epoch"] == 1
    assert set(c["image_adapter"]) == set(m.image_adapter.state_dict())
    for sdict in (c["image_adapter"], t["text_adapter"]):
        assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in sdict.values())
    monkeypatch.delenv("AACLIP_TRAIN_DTYPE")
    df, tctx = harness.run(harness.parse_args(["--dataset", "synthetic", "--allow_random_init", "--img_size", "70",
                                               "--synthetic_n", "4", "--batch_size", "4", "--save_path", save,
                                               "--compute_dtype", "fp32"]))
    assert list(df["class name"]) == ["bottle", "Average"]
    assert np.all(np.isfinite(df.drop(columns=["class name"]).to_numpy(dtype=np.float64)))
    for k, v in tctx["model"].image_adapter.state_dict().items():
        assert torch.equal(v.cpu(), c["image_adapter"][k]), k


def test_train_py_without_the_variable_is_the_fp32_run(dev, tmp_path, monkeypatch):
    """AACLIP_TRAIN_DTYPE unset: the fp32 path, the same stage-2 losses on the same seed, run twice."""
    import train
    monkeypatch.delenv("AACLIP_TRAIN_DTYPE", raising=False)
    runs = []
    for n in ("a", "b"):
        ctx = train.run(train.parse_args(TRAIN_ARGS + ["--save_path", str(tmp_path / n)]))
        assert ctx["train_dtype"] == torch.float32
        assert ctx["model"].compute_dtype == torch.float32 and ctx["model"].train_dtype is None
        assert ctx["model"].visual_engine().dtype == torch.float32
        runs.append(ctx["image_losses"])
    print("stage-2 losses, fp32, twice:", runs)
    assert len(runs[0]) >= 1 and runs[0] == runs[1]
