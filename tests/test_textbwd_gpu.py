"""The backward through the adapted text tower on the MI355X (csrc/text_bwd.hip, TextEngine.encode_train):
each kernel against fp64 torch autograd of the same formula, the training forward's bits against
encode()'s, the four text_adapter gradients on the fixture of the real reference
(tests/golden/golden_textbwd.npz, tests/textbwd_ref.py), and three Adam steps of the reference's
stage-1 loop body through the public API.

Bound (the project's rule): the error against fp64 stays within 8x the error the same formula has
in fp32 torch on the CPU (rel-L2 for tensors); scalars get a floor of 8 fp32 ulps. Every figure is
printed before it is asserted."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth

import segloss_ref as SR
import textbwd_ref as TR

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
        e, y = TR.rel_l2(got, r64), TR.rel_l2(r32, r64)
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
def _attn_ref(qkv, dout, B, N, H, causal):
    q, k, v = (t.reshape(B, N, H, 64).transpose(1, 2) for t in qkv.split(H * 64, dim=-1))
    s = (q @ k.transpose(-1, -2)) / 8.0
    if causal:
        s = s + torch.full((N, N), float("-inf"), dtype=qkv.dtype).triu_(1)
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * N, H * 64)
    return o, dout


@pytest.mark.parametrize("seq,heads,causal", [(s, 2, c) for s in (1, 5, 64, 65, 77) for c in (True, False)]
                         + [(77, 12, True)])
def test_attention_bwd(dev, seq, heads, causal):
    from aaclip import ops
    B = 2
    qkv, dout = rnd(seq * 31 + heads, B * seq, 3 * heads * 64), rnd(seq * 37 + heads, B * seq, heads * 64)
    (_, (g64, _)), (_, (g32, _)) = both(lambda a, d: _attn_ref(a, d.detach(), B, seq, heads, causal), qkv, dout)
    got = ops.attention_bwd(torch.from_numpy(qkv).to(dev), torch.from_numpy(dout).to(dev), B, seq, heads,
                            causal=causal)
    again = ops.attention_bwd(torch.from_numpy(qkv).to(dev), torch.from_numpy(dout).to(dev), B, seq, heads,
                              causal=causal)
    assert torch.equal(got, again)
    within(f"attention_bwd seq {seq} heads {heads} causal {causal}", got, g64, g32)


def test_attention_bwd_causal_last_token_and_limits(dev):
    """Causal: only the last query sees the last key, so with that query's dout zero the last
    token's dK and dV are exactly zero. seq 78 is refused before any launch."""
    from aaclip import ops
    B, N, H = 2, 77, 2
    qkv, dout = torch.from_numpy(rnd(1, B * N, 3 * H * 64)).to(dev), torch.from_numpy(rnd(2, B * N, H * 64)).to(dev)
    dout.view(B, N, H * 64)[:, N - 1] = 0
    d = ops.attention_bwd(qkv, dout, B, N, H, causal=True).view(B, N, 3, H * 64)
    assert torch.count_nonzero(d[:, N - 1, 1:]) == 0 and torch.count_nonzero(d[:, N - 2, 1:]) > 0
    with pytest.raises(ValueError, match="1..77"):
        ops.attention_bwd(torch.zeros(2 * 78, 3 * 128, device=dev), torch.zeros(2 * 78, 128, device=dev), 2, 78, 2)


def _ln(x, w, b=None):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("resid", [False, True])
def test_layernorm_bwd(dev, rows, resid):
    from aaclip import ops
    x, dy, w, r = rnd(3, rows, 768, scale=2.0) + 0.3, rnd(4, rows, 768), rnd(5, 768) * 0.2 + 1, rnd(6, rows, 768)
    (_, (g64, _)), (_, (g32, _)) = both(lambda a, ww: (_ln(a, ww.detach()), torch.from_numpy(dy)), x, w)
    if resid:
        g64, g32 = g64 + torch.from_numpy(r).double(), g32 + torch.from_numpy(r)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    out = t(r) if resid else None
    got = ops.layernorm_bwd(t(dy), t(x), t(w), residual=out, out=out)  # the residual aliases the output
    assert not resid or got.data_ptr() == out.data_ptr()
    within(f"layernorm_bwd rows {rows} residual {resid}", got, g64, g32)


def test_eot_ln_bwd(dev):
    from aaclip import ops
    ctx, eots = 9, [0, 4, 8]
    tokens = np.tile(np.arange(1, ctx + 1, dtype=np.int32) * 3, (3, 1))
    for s, p in enumerate(eots):
        tokens[s, p] = 49407
    x, dy, w = rnd(7, 3 * ctx, 768), rnd(8, 3, 768), rnd(9, 768) * 0.2 + 1
    rows = [s * ctx + p for s, p in enumerate(eots)]

    def ref(a, ww):
        return _ln(a[rows], ww.detach()), torch.from_numpy(dy)
    (_, (g64, _)), (_, (g32, _)) = both(ref, x, w)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    got = ops.eot_ln_bwd(t(dy), t(x), t(tokens), t(w))
    keep = torch.ones(3 * ctx, dtype=torch.bool)
    keep[rows] = False
    assert torch.count_nonzero(got[keep.to(dev)]) == 0 and torch.count_nonzero(got[rows[2]]) > 0
    within("eot_ln_bwd", got, g64, g32)


@pytest.mark.parametrize("mode", ["gelu", "quick", "leaky"])
def test_act_and_act_bwd(dev, mode):
    from aaclip import ops
    fn = {"gelu": F.gelu, "quick": lambda v: v * torch.sigmoid(1.702 * v), "leaky": lambda v: F.leaky_relu(v, 0.01)}[mode]
    special = np.array([0.0, -0.0, 1e-30, -1e-30, 10.0, -10.0, 1e-3, -1e-3], np.float32)
    x = np.concatenate([special, rnd(10, 1003, scale=2.0)])
    dy = rnd(11, x.size) + 2.0
    ((y64, (g64,)), (y32, (g32,))) = both(lambda a: (fn(a), torch.from_numpy(dy)), x)
    xd, dyd = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
    y = ops.act(xd, mode)
    within(f"act {mode}", y, y64, y32)
    got = ops.act_bwd(dyd, y if mode == "leaky" else xd, mode)
    within(f"act_bwd {mode}", got, g64, g32)
    if mode == "leaky":  # slope 0.01 at exactly 0, as torch
        assert torch.equal(got[:2].cpu(), torch.from_numpy(dy[:2] * np.float32(0.01))) and torch.equal(got[:2].cpu(), g32[:2])
        assert torch.equal(got[4:5].cpu(), torch.from_numpy(dy[4:5]))
    # the epilogue's own function: bias-only GEMM + act == GEMM with the fused activation, bit for bit
    a, w, b = (torch.from_numpy(v).to(dev) for v in (rnd(12, 37, 768), rnd(13, 256, 768, scale=0.05), rnd(14, 256)))
    pre, fused = torch.empty(37, 256, device=dev), torch.empty(37, 256, device=dev)
    kw = dict(leaky=True) if mode == "leaky" else dict(gelu=True if mode == "gelu" else "quick")
    ops.gemm(a, w, pre, bias=b)
    ops.gemm(a, w, fused, bias=b, **kw)
    assert torch.equal(ops.act(pre, mode), fused)


@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("aw", [0.1, 1.0])
def test_adapter_blend_bwd(dev, rows, aw):
    from aaclip import ops
    x, u, dy = rnd(15, rows, 768, scale=1.5), rnd(16, rows, 768), rnd(17, rows, 768)

    def ref(a, b):
        y = aw * (b * a.norm(dim=-1, keepdim=True) / b.norm(dim=-1, keepdim=True)) + (1 - aw) * a
        return y, torch.from_numpy(dy)
    (_, (gx64, gu64)), (_, (gx32, gu32)) = both(ref, x, u)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    g = t(dy)
    dx, du = ops.adapter_blend_bwd(g, t(x), t(u), aw, dx=g)  # dx over dy
    assert dx.data_ptr() == g.data_ptr()
    within(f"adapter_blend_bwd du rows {rows} w {aw}", du, gu64, gu32)
    within(f"adapter_blend_bwd dx rows {rows} w {aw}", dx, gx64, gx32)


@pytest.mark.parametrize("n", [1, 6, 10])
def test_anchor_reduce_bwd(dev, n):
    from aaclip import ops
    emb, dT = rnd(18 + n, n, 768, scale=3.0), rnd(30 + n, 768, 2)
    (t64, (g64,)), (t32, (g32,)) = both(lambda e: (TR.anchor(e), torch.from_numpy(dT[:, 1].copy())), emb)
    ed = torch.from_numpy(emb).to(dev)
    got = ops.anchor_reduce_bwd(ed, torch.from_numpy(dT).to(dev), 1)
    within(f"anchor_reduce_bwd n {n}", got, g64, g32)
    # the gradient of a normalised vector is orthogonal to it: |cos(demb_s, emb_s)|, a scalar against 1
    cos = lambda g, e: float((np.abs((g * e).sum(-1)) / (np.linalg.norm(g, axis=-1) * np.linalg.norm(e, axis=-1))).max())  # noqa: E731
    c_gpu, c_32 = cos(got.cpu().numpy().astype(np.float64), emb.astype(np.float64)), cos(g32.numpy().astype(np.float64), emb.astype(np.float64))
    print(f"anchor_reduce_bwd n {n}: max |cos(demb, emb)| {c_gpu:.2e} (fp32 CPU {c_32:.2e})")
    assert c_gpu <= max(8 * c_32, 8 * EPS)
    # through autograd: the column op gives anchor_reduce's bits and a grad_fn
    e2 = ed.clone().requires_grad_()
    col = ops.anchor_column(e2)
    T = torch.empty(768, 2, device=dev)
    ops.anchor_reduce(ed, T, 1)
    assert col.grad_fn is not None and torch.equal(col.detach(), T[:, 1])
    col.backward(torch.from_numpy(dT[:, 1].copy()).to(dev))
    assert torch.equal(e2.grad, got)


@pytest.mark.parametrize("M", [1, 17, 170, 1000])
@pytest.mark.parametrize("N,K", [(768, 768), (64, 128)])
def test_linear_wgrad(dev, M, N, K):
    from aaclip import ops
    dy, x = rnd(40 + M, M, N), rnd(41 + M, M, K)
    r64 = torch.from_numpy(dy).double().T @ torch.from_numpy(x).double()
    r32 = torch.from_numpy(dy).T @ torch.from_numpy(x)
    dyd, xd = torch.from_numpy(dy).to(dev), torch.from_numpy(x).to(dev)
    got = ops.linear_wgrad(dyd, xd)
    assert torch.equal(got, ops.linear_wgrad(dyd, xd))  # two launches, the same bits
    within(f"linear_wgrad M {M} N {N} K {K}", got, r64, r32)
    # rows of X set to zero contribute nothing, whatever their dY
    zero = torch.arange(M, device=dev) % 3 == 1
    x0 = xd.clone()
    x0[zero] = 0
    dy2 = dyd.clone()
    dy2[zero] = 1e30
    assert torch.equal(ops.linear_wgrad(dyd, x0), ops.linear_wgrad(dy2, x0))
    if M > 1:
        keep = ~zero
        within(f"linear_wgrad M {M} zeroed rows vs dropped rows", ops.linear_wgrad(dyd, x0),
               torch.from_numpy(dy).double()[keep.cpu()].T @ torch.from_numpy(x).double()[keep.cpu()],
               torch.from_numpy(dy)[keep.cpu()].T @ torch.from_numpy(x)[keep.cpu()])


# ---------------------------------------------------------------------------- the tower
@pytest.fixture(scope="module")
def sd():
    return synth.clip_state_dict(111)


@pytest.fixture(scope="module")
def clip(dev, sd):
    from model.clip import create_model
    c = create_model("ViT-L-14-336", 336, pretrained=None, device=dev)
    c.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return c


@pytest.fixture(scope="module")
def model(dev, clip):
    """The full-size synthetic model, as tests/test_api_gpu.py builds it."""
    from model.adapter import AdaptedCLIP
    m = AdaptedCLIP(clip, relu=False, compute_dtype=torch.float32).to(dev).eval()
    _, ta = synth.adapter_state_dicts(111)
    m.text_adapter.load_state_dict({k: torch.from_numpy(v) for k, v in ta.items()})
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_textbwd.npz"))


def _weights(model):
    return [m.fc[0].weight for m in model.text_adapter]


@pytest.mark.parametrize("quick", [False, True])
def test_training_forward_has_encode_bits(dev, model, gold, quick):
    from aaclip.engine import TextEngine
    tok = torch.from_numpy(gold["tok_abnormal"]).to(dev)
    ws = [w.detach().clone().requires_grad_() for w in _weights(model)]
    eng = TextEngine(model.clipmodel.text_params(), model.text_adapter.state_dict(), quick_gelu=quick)
    emb = eng.encode_train(tok, ws)
    assert emb.grad_fn is not None and torch.equal(emb.detach(), eng.encode(tok))
    ws[0].requires_grad_(False)  # lowest trainable adapter 1: block 0 and 1 keep nothing
    assert torch.equal(eng.encode_train(tok, ws).detach(), eng.encode(tok))
    for w in ws[:3]:
        w.requires_grad_(False)  # only the output projection trains
    assert torch.equal(eng.encode_train(tok, ws).detach(), eng.encode(tok))


def test_anchors_with_grad_equal_anchors_without(dev, model):
    from forward_utils import get_adapted_single_class_text_embedding as anchors
    T = anchors(model, "MVTec", "bottle", dev)
    with torch.no_grad():
        T0 = anchors(model, "MVTec", "bottle", dev)
    assert T.grad_fn is not None and T0.grad_fn is None and torch.equal(T.detach(), T0)


def test_end_to_end_on_the_fixture(dev, model, sd, gold):
    """The four .grads of L = sum G * T + 0.1 (T0 . T1)^2 on "bottle" against the fp64 restatement in
    full (bound: 8x the fp32 restatement's error) and against the real reference's stored rows and
    norms (bound: 8x the reference's own fp32-vs-fp64 rel-L2); the block taps likewise."""
    from forward_utils import get_adapted_single_class_text_embedding as anchors
    G = gold["G"]
    _, ta = synth.adapter_state_dicts(111)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P64 = TR.params(sd, torch.float64)
    r64 = TR.run(sd, ta, gold["tok_normal"], gold["tok_abnormal"], G, torch.float64, P=P64)
    P32 = {k: v.float() for k, v in P64.items()}
    del P64
    r32 = TR.run(sd, ta, gold["tok_normal"], gold["tok_abnormal"], G, torch.float32, P=P32)
    del P32
    eng = model.clipmodel.text_engine(model.text_adapter.state_dict(), model.text_adapt_until, model.t_w)
    eng.tap_blocks, eng.tap_records = tuple(TR.TAPS), []
    for w in _weights(model):
        w.grad = None
    try:
        T = anchors(model, "MVTec", "bottle", dev)
        assert T.grad_fn is not None  # the parent commit stops here: no grad_fn
        loss = TR.fixture_loss(T, torch.from_numpy(G).to(dev))
        loss.backward()
        records = list(eng.tap_records)
    finally:
        eng.tap_blocks, eng.tap_records = (), []
    within("T", T, r64["T"], r32["T"])
    within("loss", loss, r64["loss"], r32["loss"], scalar=True)
    rows = gold["rows"]
    for i, w in enumerate(_weights(model)):
        g = w.grad
        assert g is not None and torch.count_nonzero(g) > 0
        within(f"dW{i} vs the restatement", g, r64["grads"][i], r32["grads"][i])
        yard = float(gold[f"g{i}_rel32"])
        e_rows = TR.rel_l2(g[rows].cpu().numpy(), gold[f"g{i}_rows64"])
        e_norm = abs(float(g.double().norm()) - float(gold[f"g{i}_norm64"])) / float(gold[f"g{i}_norm64"])
        print(f"dW{i} vs the reference: rows rel-L2 {e_rows:.3e}  norm rel {e_norm:.3e}  reference fp32 yardstick {yard:.3e}")
        assert e_rows <= 8 * yard and e_norm <= 8 * yard
    n_normal, n_eot = gold["tok_normal"].shape[0], int(gold["n_eot"])
    rec = [r for r in records if r["n"] == n_normal]
    assert len(rec) == 1 and len(records) == 2
    for b in TR.TAPS:
        tap = rec[0]["taps"][b].view(n_normal, rec[0]["ctx"], -1)[0, :n_eot]
        within(f"tap after block {b} vs the restatement", tap, r64["taps"][b], r32["taps"][b])
        e = TR.rel_l2(tap.cpu().numpy(), gold[f"tap{b}_64"])
        print(f"tap after block {b} vs the reference: rel-L2 {e:.3e}  reference fp32 yardstick {float(gold[f'tap{b}_rel32']):.3e}")
        assert e <= 8 * float(gold[f"tap{b}_rel32"])
    for w in _weights(model):
        w.grad = None


def test_three_adam_steps_of_the_stage1_loop(dev, model, gold):
    """train.py:62-72, :87-100 through the public API; losses against the reference's fp64 run within
    8x the error of the reference's own fp32 run (floor 8 ulps); falling; frozen buffers stay."""
    from forward_utils import (calculate_seg_loss, calculate_similarity_map,
                               get_adapted_single_class_text_embedding)
    f, _, mask = SR.inputs(int(gold["adam_seed"]), 3, 5, 23)
    f, mask = torch.from_numpy(f).to(dev), torch.from_numpy(mask).to(dev)
    class_names = TR.ADAM_CLASSES
    keep = {k: v.detach().clone() for k, v in model.text_adapter.state_dict().items()}
    optimizer = torch.optim.Adam(model.text_adapter.parameters(), lr=1e-3, betas=(0.5, 0.999))

    def step_loss():
        d = {c: get_adapted_single_class_text_embedding(model, "MVTec", c, dev) for c in set(class_names)}
        epoch_text_feature = torch.stack([d[c] for c in class_names], dim=0)
        patch_preds = calculate_similarity_map(f, epoch_text_feature, 23)
        loss = calculate_seg_loss(patch_preds, mask)
        orthogonal_loss = ((epoch_text_feature[:, :, 0] * epoch_text_feature[:, :, 1]).sum(1).mean()) ** 2
        loss += orthogonal_loss * 0.1
        return loss

    losses = []
    try:
        eng = model.clipmodel.text_engine(model.text_adapter.state_dict(), model.text_adapt_until, model.t_w)
        frozen = None
        for _ in range(3):
            loss = step_loss()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
            e2 = model.clipmodel.text_engine(model.text_adapter.state_dict(), model.text_adapt_until, model.t_w)
            ptrs = (e2.tok_emb.data_ptr(), e2.blocks[5]["w_fc"].data_ptr(), e2._bwd[5]["w_fc"].data_ptr())
            assert e2 is eng and (frozen is None or frozen == ptrs)
            frozen = ptrs
        with torch.no_grad():
            losses.append(float(step_loss()))
    finally:
        model.text_adapter.load_state_dict(keep)
        for w in _weights(model):
            w.grad = None
    l32, l64 = gold["adam_losses32"], gold["adam_losses64"]
    print("losses", losses, "reference fp32", l32.tolist(), "fp64", l64.tolist())
    assert all(b < a for a, b in zip(losses, losses[1:]))
    for k in range(4):
        within(f"adam loss {k}", losses[k], l64[k], l32[k], scalar=True)


def test_text_adapt_until(dev, clip, model, gold):
    from model.adapter import AdaptedCLIP
    tok = torch.from_numpy(gold["tok_normal"]).to(dev)
    m0 = AdaptedCLIP(clip, text_adapt_until=0, relu=False, compute_dtype=torch.float32).to(dev).eval()
    assert len(m0.text_adapter) == 1
    emb = m0.encode_text(tok)
    emb.square().sum().backward()
    g = m0.text_adapter[0].fc[0].weight.grad
    assert g is not None and torch.count_nonzero(g) > 0
    assert m0.clipmodel.text_engine(m0.text_adapter.state_dict(), 0, m0.t_w)._bwd is None  # ends at the EOT rows
    for w in _weights(model):
        w.grad = None
    model.encode_text(tok).square().sum().backward()
    for w in _weights(model):
        assert w.grad is not None and torch.count_nonzero(w.grad) > 0
        w.grad = None
