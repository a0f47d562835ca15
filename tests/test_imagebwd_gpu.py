"""The backward through the adapted visual tower on the MI355X (csrc/visual_bwd.hip,
VisualEngine.forward_train): each new kernel against fp64 torch autograd of the same formula, the
training forward's bits against forward()'s, the 11 image_adapter gradients on the fixture of the
real reference (tests/golden/golden_imagebwd.npz, tests/imagebwd_ref.py), and three Adam steps of
the reference's stage-2 loop body through the public API.

Bound (the project's rule): the error against fp64 stays within 8x the error the same formula has
in fp32 torch on the CPU (rel-L2 for tensors); scalars get a floor of 8 fp32 ulps. Every figure is
printed before it is asserted."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth

import imagebwd_ref as IR

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def within(name, got, r64, r32, scalar=False):
    """err(got vs fp64) <= 8 x err(fp32 CPU vs fp64) (+ 8 ulps of the value for a scalar)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    r64 = r64.detach().numpy() if isinstance(r64, torch.Tensor) else np.asarray(r64)
    r32 = r32.detach().numpy() if isinstance(r32, torch.Tensor) else np.asarray(r32)
    if scalar:
        e, y = abs(float(got) - float(r64)), abs(float(r32) - float(r64))
        bound = max(8 * y, 8 * EPS * abs(float(r64)))
    else:
        assert got.shape == r64.shape, (name, got.shape, r64.shape)
        e, y = IR.rel_l2(got, r64), IR.rel_l2(r32, r64)
        bound = 8 * y
    print(f"{name}: err {e:.3e}  fp32-CPU yardstick {y:.3e}  bound {bound:.3e}")
    assert e <= bound, name


def both(fn, *arrays):
    """fn on fp64 and on fp32 CPU leaves built from the fp32 arrays: ((out64, grads64), (out32, grads32))."""
    res = []
    for dt in (torch.float64, torch.float32):
        leaves = [torch.from_numpy(a).to(dt).requires_grad_() for a in arrays]
        out, dout = fn(*leaves)
        out.backward(dout.to(dt))
        res.append((out.detach(), [t.grad for t in leaves]))
    return res


def rnd(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


# ---------------------------------------------------------------------------- kernels
def _attn_ref(qkv, dout, B, N, H):
    q, k, v = (t.reshape(B, N, H, 64).transpose(1, 2) for t in qkv.split(H * 64, dim=-1))
    s = (q @ k.transpose(-1, -2)) / 8.0
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * N, H * 64)
    return o, dout


def _attn_case(dev, B, N, H, seed=0):
    from aaclip import ops
    qkv, dout = rnd(N * 31 + H + seed, B * N, 3 * H * 64), rnd(N * 37 + H + seed, B * N, H * 64)
    qd, dd = torch.from_numpy(qkv).to(dev), torch.from_numpy(dout).to(dev)
    out = torch.empty(B * N, H * 64, device=dev)
    ops.attention(qd, out, B, N, H)
    return qkv, dout, qd, dd, out


@pytest.mark.parametrize("seq,batch,heads", [(s, 2, 3) for s in (1, 5, 63, 64, 65, 130, 577)] + [(1370, 1, 2)])
def test_attention_bwd_tiled(dev, seq, batch, heads):
    from aaclip import ops
    qkv, dout, qd, dd, out = _attn_case(dev, batch, seq, heads)
    (_, (g64, _)), (_, (g32, _)) = both(lambda a, d: _attn_ref(a, d.detach(), batch, seq, heads), qkv, dout)
    got = torch.full_like(qd, float("nan"))  # every element is written
    ops.attention_bwd_tiled(qd, out, dd, batch, seq, heads, dqkv=got)
    assert bool(torch.isfinite(got).all())
    again = ops.attention_bwd_tiled(qd, out, dd, batch, seq, heads)
    assert torch.equal(got, again)  # two launches, the same bits
    within(f"attention_bwd_tiled seq {seq} batch {batch} heads {heads}", got, g64, g32)
    if seq == 1:  # softmax over one key: P = 1, dS = 0
        d = got.view(batch, 3, heads * 64)
        assert torch.count_nonzero(d[:, :2]) == 0 and torch.equal(d[:, 2], dd)


def test_attention_bwd_tiled_agrees_with_the_lds_kernel(dev):
    from aaclip import ops
    B, N, H = 2, 77, 3
    qkv, dout, qd, dd, out = _attn_case(dev, B, N, H)
    (_, (g64, _)), (_, (g32, _)) = both(lambda a, d: _attn_ref(a, d.detach(), B, N, H), qkv, dout)
    got, old = ops.attention_bwd_tiled(qd, out, dd, B, N, H), ops.attention_bwd(qd, dd, B, N, H, causal=False)
    within("attention_bwd_tiled seq 77", got, g64, g32)
    e, y = IR.rel_l2(got.cpu().numpy(), old.cpu().numpy()), IR.rel_l2(g32.numpy(), g64.numpy())
    print(f"tiled vs attention_bwd at seq 77: rel-L2 {e:.3e}  bound {8 * y:.3e}")
    assert e <= 8 * y


def test_attention_bwd_tiled_is_image_local(dev):
    """Image 1 of a batch of 3 gets the bits it gets when launched alone."""
    from aaclip import ops
    B, N, H = 3, 130, 2
    _, _, qd, dd, out = _attn_case(dev, B, N, H, seed=5)
    full = ops.attention_bwd_tiled(qd, out, dd, B, N, H)
    one = slice(N, 2 * N)
    alone = ops.attention_bwd_tiled(qd[one].contiguous(), out[one].contiguous(), dd[one].contiguous(), 1, N, H)
    assert torch.equal(full[one], alone)


def test_attention_bwd_tiled_rejects_bad_arguments(dev):
    from aaclip import _lib, ops
    B, N, H = 1, 70, 2
    _, _, qd, dd, out = _attn_case(dev, B, N, H)
    ws = ops.attention_bwd_tiled_workspace(B, N, H, dev)
    assert ws.numel() == 2 * B * H * N
    dq = torch.empty_like(qd)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    fn = _lib.lib().aaclip_attention_bwd_tiled
    args = lambda dqkv, hd, nbytes: (p(qd), p(out), p(dd), p(dqkv), B, N, H, hd, p(ws), nbytes, None)  # noqa: E731
    assert fn(*args(dq, 32, ws.numel() * 4)) == 1           # head_dim != 64
    assert fn(*args(qd, 64, ws.numel() * 4)) == 1           # dqkv aliases qkv
    assert fn(*args(dq, 64, ws.numel() * 4 - 4)) == 1       # short workspace
    with pytest.raises(ValueError, match="alias"):
        ops.attention_bwd_tiled(qd, out, dd, B, N, H, dqkv=qd)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.attention_bwd_tiled(qd, out, dd, B, N, H, workspace=ws[:-1])
    torch.cuda.synchronize()


def _ln(x, w, b=None):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def test_tap_ln_bwd(dev):
    """2 images x 17 tokens: the token rows accumulate onto a non-zero g, the CLS rows keep their bits."""
    from aaclip import ops
    B, n_tok, W = 2, 17, 1024
    x, dtap, w, g0 = rnd(3, B * n_tok, W, scale=2.0) + 0.3, rnd(4, B * (n_tok - 1), W), rnd(5, W) * 0.2 + 1, rnd(6, B * n_tok, W)
    tok = np.array([b * n_tok + t for b in range(B) for t in range(1, n_tok)])

    def ref(a, ww):
        return _ln(a[tok], ww.detach()), torch.from_numpy(dtap)
    (_, (g64, _)), (_, (g32, _)) = both(ref, x, w)
    g64, g32 = g64 + torch.from_numpy(g0).double(), g32 + torch.from_numpy(g0)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    g = t(g0)
    assert ops.tap_ln_bwd(t(dtap), t(x), t(w), g, B, n_tok) is g
    cls = [b * n_tok for b in range(B)]
    assert torch.equal(g[cls].cpu(), torch.from_numpy(g0[cls]))
    assert not torch.equal(g[tok[0]].cpu(), torch.from_numpy(g0[tok[0]]))
    within("tap_ln_bwd", g, g64, g32)
    z = torch.zeros_like(g)  # from zero: the plain ln_post backward of the token rows
    ops.tap_ln_bwd(t(dtap), t(x), t(w), z, B, n_tok)
    within("tap_ln_bwd onto zeros", z, g64 - torch.from_numpy(g0).double(), g32 - torch.from_numpy(g0))


@pytest.mark.parametrize("width", [768, 1024])
def test_l2_normalize_bwd(dev, width):
    from aaclip import ops
    rows = 77
    x, dy = rnd(7, rows, width, scale=3.0), rnd(8, rows, width)
    x[5] = 0.0  # the clamp branch: y = x / 1e-12, dx = dy / 1e-12
    (_, (g64,)), (_, (g32,)) = both(lambda a: (F.normalize(a, dim=-1), torch.from_numpy(dy)), x)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    got = ops.l2_normalize_bwd(t(dy), t(x))
    assert torch.equal(got, ops.l2_normalize_bwd(t(dy), t(x)))
    keep = np.arange(rows) != 5
    within(f"l2_normalize_bwd width {width}", got[torch.from_numpy(keep).to(dev)], g64[keep], g32[keep])
    within(f"l2_normalize_bwd width {width}, the zero row", got[5], g64[5], g32[5])
    assert bool(torch.isfinite(got).all())
    inplace = t(dy)
    assert ops.l2_normalize_bwd(inplace, t(x), out=inplace) is inplace and torch.equal(inplace, got)


def test_l2_normalize_bwd_det_broadcast(dev):
    """det = mean_p normalize(d_p): one launch with the per-image gradient broadcast and scaled."""
    from aaclip import ops
    B, P = 3, 25
    x, dd = rnd(9, B * P, 768, scale=2.0), rnd(10, B, 768)
    (_, (g64,)), (_, (g32,)) = both(lambda a: (F.normalize(a, dim=-1).view(B, P, 768).mean(1), torch.from_numpy(dd)), x)
    got = ops.l2_normalize_bwd(torch.from_numpy(dd).to(dev), torch.from_numpy(x).to(dev), group=P, scale=1.0 / P)
    within("l2_normalize_bwd det broadcast", got, g64, g32)
    with pytest.raises(ValueError):
        ops.l2_normalize_bwd(torch.from_numpy(dd).to(dev), torch.from_numpy(x).to(dev), group=P + 1)


# ---------------------------------------------------------------------------- the tower
NAMES = IR.weight_names()


@pytest.fixture(scope="module")
def sd():
    return synth.clip_state_dict(111, img_size=IR.IMG)


@pytest.fixture(scope="module")
def clip(dev, sd):
    from model.clip import create_model
    c = create_model("ViT-L-14-336", IR.IMG, pretrained=None, device=dev, force_image_size=IR.IMG)
    c.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return c


def _load_adapter(m, relu=False):
    ia, _ = synth.adapter_state_dicts(111, relu=relu)
    m.image_adapter.load_state_dict({k: torch.from_numpy(v) for k, v in ia.items()})
    return ia


@pytest.fixture(scope="module")
def model(dev, clip):
    from model.adapter import AdaptedCLIP
    m = AdaptedCLIP(clip, relu=False, compute_dtype=torch.float32).to(dev).eval()
    _load_adapter(m)
    for p in m.parameters():
        p.requires_grad_(False)
    for p in m.image_adapter.parameters():
        p.requires_grad_(True)
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_imagebwd.npz"))


@pytest.fixture(scope="module")
def x_np():
    return synth.images(IR.X_SEED, IR.BATCH, IR.IMG)


def _weights(m):
    return m._adapter_weights()


def _clear(m):
    for w in _weights(m):
        w.grad = None


def _sides(seg, batch):
    """{block: u > 0 [B, n_tok, 1024]} of the adapter outputs the training forward kept: the side of
    LeakyReLU's kink each element took on the device (imagebwd_ref._adapter_act)."""
    st = seg[0].grad_fn.st
    return {i: (sv["u"] > 0).view(batch, st["n_tok"], -1).cpu() for i, sv in st["blocks"].items() if "u" in sv}


def _restate(sd, ia, x_np, G, sides, **kw):
    """The restatement in fp64 (truth) and fp32 (yardstick) on the device's side of the kinks, and the
    fp64 run on its own side where that differs (what the real reference's stored rows are)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P64 = IR.params(sd, torch.float64)
    r64 = IR.run(sd, ia, x_np, G, torch.float64, P=P64, sides=sides, **kw)
    print("adapter pre-activations inside the kink window that took the device's branch, per block:", r64["moved"])
    assert sum(r64["moved"]) <= 16  # a handful among ~800 k: the window decides nothing else
    plain = IR.run(sd, ia, x_np, G, torch.float64, P=P64, **kw) if sum(r64["moved"]) else r64
    P32 = {k: v.float() for k, v in P64.items()}
    del P64
    r32 = IR.run(sd, ia, x_np, G, torch.float32, P=P32, sides=sides, **kw)
    return r64, r32, plain


@pytest.fixture(scope="module")
def fixture_run(dev, model, sd, x_np):
    """The fixture's "grad" case once: on the device through the public API (gradients and dL/dx after
    the tapped blocks kept), then the restatement."""
    G = IR.loss_weights((IR.IMG // 14) ** 2)
    eng = model.visual_engine()
    eng.tap_blocks, eng.tap_records = tuple(IR.TAPS), []
    _clear(model)
    try:
        seg, det = model(torch.from_numpy(x_np).to(dev))
        sides = _sides(seg, IR.BATCH)
        loss = IR.fixture_loss(seg, det, [torch.from_numpy(g).to(dev) for g in G])
        loss.backward()
        records = list(eng.tap_records)
    finally:
        eng.tap_blocks, eng.tap_records = (), []
    grads = [w.grad.detach().clone() for w in _weights(model)]
    _clear(model)
    ia, _ = synth.adapter_state_dicts(111)
    r64, r32, plain = _restate(sd, ia, x_np, G, sides)
    return dict(seg=[s.detach() for s in seg], det=det.detach(), loss=loss.detach(), grads=grads, records=records,
                r64=r64, r32=r32, plain=plain, G=G)


def test_forward_has_a_grad_fn_and_backward_fills_the_adapter(dev, model, x_np):
    """The stage-2 contract (train.py:145-156): model(x) is differentiable into image_adapter."""
    x = torch.from_numpy(x_np).to(dev)
    _clear(model)
    seg, det = model(x)
    assert seg[0].requires_grad and det.requires_grad and seg[0].shape == (IR.BATCH, 64, 768)
    loss = sum(s.square().sum() * (j + 1) for j, s in enumerate(seg)) + det.sum()
    loss.backward()
    for n, w in zip(NAMES, _weights(model)):
        assert w.grad is not None and bool(torch.isfinite(w.grad).all()) and torch.count_nonzero(w.grad) > 0, n
    for p in model.image_encoder.parameters():
        assert p.grad is None
    with torch.no_grad():
        seg0, det0 = model(x)
    assert seg0[0].grad_fn is None and all(torch.equal(a.detach(), b) for a, b in zip(seg, seg0))
    assert torch.equal(det.detach(), det0)
    _clear(model)


@pytest.mark.parametrize("img,batch", [(112, 2), (70, 3)])
@pytest.mark.parametrize("quick", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_training_forward_has_forward_bits(dev, sd, img, batch, quick, relu):
    from aaclip.engine import VisualEngine
    vp = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k.startswith("visual.")}
    n_tok = (img // 14) ** 2 + 1
    vp["visual.positional_embedding"] = vp["visual.positional_embedding"][:n_tok].contiguous()
    ia, _ = synth.adapter_state_dicts(111, relu=relu)
    ad = {k: torch.from_numpy(v).to(dev) for k, v in ia.items()}
    eng = VisualEngine(vp, ad, dtype=torch.float32, quick_gelu=quick)
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
    with pytest.raises(ValueError, match="one chunk"):
        eng.forward_train(x[:1].expand(eng.max_chunk(img) + 1, -1, -1, -1), ws)  # a view: refused before any copy
    with pytest.raises(RuntimeError, match="fp32 only"):
        VisualEngine(vp, ad, dtype=torch.float16, quick_gelu=quick).forward_train(x, ws)


def test_outputs_and_loss_on_the_fixture(fixture_run):
    f = fixture_run
    for j in range(4):
        within(f"seg {j}", f["seg"][j], f["r64"]["seg"][j], f["r32"]["seg"][j])
    within("det", f["det"], f["r64"]["det"], f["r32"]["det"])
    # the loss is a sum of ~4e5 terms G * seg of either sign that cancels from ~1e4 down to ~32: its
    # rounding is that of the terms, so the floor is 8 ulps of sum |G * seg|, not of the cancelled value
    mag = sum(float(np.abs(g * s).sum()) for g, s in zip(f["G"], f["r64"]["seg"] + [f["r64"]["det"]]))
    e, y = abs(float(f["loss"]) - f["r64"]["loss"]), abs(f["r32"]["loss"] - f["r64"]["loss"])
    print(f"loss: err {e:.3e}  fp32-CPU yardstick {y:.3e}  sum |terms| {mag:.3e}  bound {max(8 * y, 8 * EPS * mag):.3e}")
    assert e <= max(8 * y, 8 * EPS * mag)


@pytest.mark.parametrize("i", range(11), ids=NAMES)
def test_gradients_on_the_fixture(gold, fixture_run, i):
    """Each of the 11 .grads of L = sum_j sum(G_j seg_j) + sum(G_d det) against the fp64 restatement in
    full (bound: 8x the fp32 restatement's error) and against the real reference's stored rows and norm
    (bound: 8x the reference's own fp32-vs-fp64 rel-L2).

    Truth and yardstick are evaluated on the device's side of LeakyReLU's kink for the adapter
    pre-activations within 1e-5 rms of 0 (imagebwd_ref._adapter_act; a handful of ~800 k, printed):
    the slope jumps from 0.01 to 1 there and an fp32 forward cannot tell the sides apart. Measured
    without that, plain fp64 truth: the device's d layer_adapters.0..4 stand at 6.5e-5, 6.5e-5,
    6.4e-5, 6.1e-5, 5.3e-4 (yardstick 6e-7 .. 7e-7) with every dL/dx tap, layer_adapters.5 and the
    projections at 1.1e-6 .. 1.9e-6; fp32 torch on a CPU with 16 threads instead of 8 stands at
    8.6e-5, 8.4e-5, 7.5e-4 for layer_adapters.0..2 for the same reason. The reference's stored rows
    are on fp64's own side: the device's rows are compared after the fp64 difference between the
    two sides is taken off."""
    f, n = fixture_run, NAMES[i]
    g, r64, r32, plain = f["grads"][i], f["r64"], f["r32"], f["plain"]
    assert torch.count_nonzero(g) > 0
    within(f"d {n} vs the restatement", g, r64["grads"][i], r32["grads"][i])
    g0 = g.double().cpu().numpy() - (r64["grads"][i] - plain["grads"][i])
    yard, rows = float(gold[f"g{i}_rel32"]), gold["rows"]
    e_rows = IR.rel_l2(g0[rows][:, ::IR.COL_STEP], gold[f"g{i}_rows64"])
    e_norm = abs(float(np.linalg.norm(g0)) - float(gold[f"g{i}_norm64"])) / float(gold[f"g{i}_norm64"])
    print(f"d {n} vs the reference: rows rel-L2 {e_rows:.3e}  norm rel {e_norm:.3e}  reference fp32 yardstick {yard:.3e}")
    assert e_rows <= 8 * yard and e_norm <= 8 * yard


@pytest.mark.parametrize("b", IR.TAPS)
def test_block_output_gradients_on_the_fixture(gold, fixture_run, b):
    """dL/dx after blocks 23, 18, 12, 6, 5 and 0 (image 0), against the restatement and the reference."""
    f = fixture_run
    assert len(f["records"]) == 1
    rec = f["records"][0]
    tap = rec["taps"][b].view(IR.BATCH, rec["n_tok"], -1)[0]
    within(f"dL/dx after block {b} vs the restatement", tap, f["r64"]["taps"][b], f["r32"]["taps"][b])
    t0 = tap.double().cpu().numpy() - (f["r64"]["taps"][b] - f["plain"]["taps"][b])
    e = IR.rel_l2(t0[list(IR.TAP_TOKENS)], gold[f"tap{b}_64"])
    print(f"dL/dx after block {b} vs the reference: rel-L2 {e:.3e}  reference fp32 yardstick {float(gold[f'tap{b}_rel32']):.3e}")
    assert e <= 8 * float(gold[f"tap{b}_rel32"])


def test_relu_projections_on_the_fixture(dev, clip, sd, gold, x_np):
    """relu=True (LeakyReLU in seg_proj / det_proj): the loss and one gradient norm of the reference."""
    from model.adapter import AdaptedCLIP
    m = AdaptedCLIP(clip, relu=True, compute_dtype=torch.float32).to(dev).eval()
    _load_adapter(m, relu=True)
    G = IR.loss_weights((IR.IMG // 14) ** 2)
    seg, det = m(torch.from_numpy(x_np).to(dev))
    loss = IR.fixture_loss(seg, det, [torch.from_numpy(g).to(dev) for g in G])
    loss.backward()
    within("relu loss", loss, gold["relu_loss64"], gold["relu_loss32"], scalar=True)
    g = m.image_adapter["seg_proj"][1].weight.grad
    e, yard = abs(float(g.double().norm()) - float(gold["relu_g_norm64"])) / float(gold["relu_g_norm64"]), float(gold["relu_g_rel32"])
    print(f"relu d seg_proj.1 norm rel {e:.3e}  reference fp32 yardstick {yard:.3e}")
    assert e <= 8 * yard


def test_three_adam_steps_of_the_stage2_loop(dev, model, gold, x_np):
    """train.py:134-159 through the public API; losses against the reference's fp64 run within 8x the
    error of the reference's own fp32 run (floor 8 ulps); the frozen packing stays put."""
    from forward_utils import calculate_seg_loss, calculate_similarity_map
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
    finally:
        model.image_adapter.load_state_dict(keep)
        _clear(model)
    l32, l64 = gold["adam_losses32"], gold["adam_losses64"]
    print("losses", losses, "reference fp32", l32.tolist(), "fp64", l64.tolist())
    for k in range(4):
        within(f"adam loss {k}", losses[k], l64[k], l32[k], scalar=True)
    # as the reference's own run: Adam's first step (lr 5e-4 on every weight) overshoots on the synthetic
    # tower, then the loss falls to below its start
    assert losses[2] < losses[1] and losses[3] < losses[2] and losses[3] < losses[0]


@pytest.mark.parametrize("until", [0, 2])
def test_image_adapt_until(dev, clip, sd, x_np, until):
    from model.adapter import AdaptedCLIP
    m = AdaptedCLIP(clip, image_adapt_until=until, relu=False, compute_dtype=torch.float32).to(dev).eval()
    ia, _ = synth.adapter_state_dicts(111)
    m.image_adapter.load_state_dict({k: torch.from_numpy(v) for k, v in ia.items() if k in m.image_adapter.state_dict()})
    assert len(m.image_adapter["layer_adapters"]) == until
    G = IR.loss_weights((IR.IMG // 14) ** 2)
    seg, det = m(torch.from_numpy(x_np).to(dev))
    sides = _sides(seg, IR.BATCH)
    assert sorted(sides) == list(range(until))
    IR.fixture_loss(seg, det, [torch.from_numpy(g).to(dev) for g in G]).backward()
    r64, r32, _ = _restate(sd, ia, x_np, G, sides, adapt_until=until)
    for i, (n, w) in enumerate(zip(IR.weight_names(until), m._adapter_weights())):
        within(f"image_adapt_until {until}: d {n}", w.grad, r64["grads"][i], r32["grads"][i])
    assert (m.visual_engine()._bwd is None) == (until == 0)  # no adapter: the backward ends at the taps


def test_projection_only_training_keeps_no_tower_state(dev, model, fixture_run, x_np):
    """Only seg_proj.1 requires grad: nothing of the tower is saved, and its gradient is the same."""
    r64, r32, G = fixture_run["r64"], fixture_run["r32"], fixture_run["G"]
    ws = _weights(model)
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
        within("d seg_proj.1 alone", ws[7].grad, r64["grads"][7], r32["grads"][7])
    finally:
        for w in ws:
            w.requires_grad_(True)
        _clear(model)
