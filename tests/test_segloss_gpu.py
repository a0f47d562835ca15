"""The stage-1 loss head on the GPU (train.py:86-100): every kernel against the fp64
restatement tests/segloss_ref.py (pinned to the real reference by tests/test_segloss_host.py)
on the same inputs, then the reference's lines as written, on the golden's inputs.

Bounds. The yardstick is the error of the same formula evaluated in fp32 torch on the CPU
against the same fp64 values (computed here, or loss32 / dT32 of golden_segloss.npz). The
kernels get 8x that: they sum S^2 terms in another order than torch and recompute the fp32
coordinates and softmax in the backward. Scalars (the loss terms, the per-image sums) have a
floor of 8 fp32 ulps at the value, since a scalar's yardstick can be zero by luck. Gradient
bounds are rel-L2 over the whole tensor. Every measured error is printed.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aaclip import ops

import segloss_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = SR.SHAPES
IDS = [f"B{b}g{g}S{s}" for b, g, s in SHAPES]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_segloss.npz"))


@functools.lru_cache(maxsize=None)
def case(B, g, S, per_image=True):
    """Inputs of one shape and the fp64 / fp32 CPU runs of the whole head on them, computed once
    and shared (read-only) by the tests below."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    f, T, mask = SR.inputs(1000 + 7 * g + S, B, g, S, per_image=per_image)
    r64 = SR.run(f, T, mask, S, torch.float64)
    return dict(f=f, T=T, mask=mask, r64=r64)


def scalar_bound(yard, ref):
    ref = np.asarray(ref, np.float64)
    floor = 8 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.maximum(8 * np.abs(np.asarray(yard, np.float64) - ref), floor)


def check_scalars(name, got, yard, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, bound = np.abs(got - ref), scalar_bound(yard, ref)
    print(f"{name}: max |err| / bound = {np.max(err / bound):.3f}  (max |err| {err.max():.3e}, "
          f"yardstick max {np.abs(np.asarray(yard, np.float64) - ref).max():.3e})")
    assert np.all(err <= bound), (name, err, bound)


def check_rel(name, got, yard, ref):
    e, y = SR.rel_l2(got, ref), SR.rel_l2(yard, ref)
    print(f"{name}: rel-L2 {e:.3e}, fp32-torch yardstick {y:.3e}, bound {8 * y:.3e}")
    assert np.shape(got) == np.shape(ref) and e <= 8 * y, (name, e, y)


def cuda(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev, dtype).contiguous()


# ---------------------------------------------------------------------------- 1. patch_logits_per_image
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_patch_logits_per_image(dev, shape, dtype):
    B, g, S = shape
    c = case(*shape)
    L = g * g
    fh = torch.from_numpy(c["f"]).to(dtype)           # the (bf16-rounded) features the kernel sees
    f = fh.to(dev).reshape(B * L, 768).contiguous()
    T = cuda(c["T"], dev)
    shared = T[0].contiguous()
    a = ops.patch_logits(f, shared, torch.empty(B, 2, L, device=dev), group=L)
    b = ops.patch_logits_per_image(f, shared, torch.empty(B, 2, L, device=dev), group=L)
    assert torch.equal(a, b)                          # t_stride = 0: the same bits as patch_logits
    got = ops.patch_logits_per_image(f, T, torch.empty(B, 2, L, device=dev), group=L).cpu().numpy()
    ref = SR.logits(fh.double(), torch.from_numpy(c["T"]).double()).reshape(B, 2, L).numpy()
    yard = SR.logits(fh.float(), torch.from_numpy(c["T"])).reshape(B, 2, L).numpy()
    check_rel(f"per-image logits {shape} {dtype}", got, yard, ref)
    # three anchors per image go through the same kernel
    T3 = torch.cat([T, T[:, :, :1] * 0.5], dim=2).contiguous()
    got3 = ops.patch_logits_per_image(f, T3, torch.empty(B, 3, L, device=dev), group=L).cpu().numpy()
    check_rel(f"per-image logits, 3 anchors {shape} {dtype}", got3[:, :2], yard, ref)


# ---------------------------------------------------------------------------- 2. / 3. seg_loss and its backward
def _loss_io(c, S):
    """fp32 probabilities (the fp64 run's, rounded) and the mask: what the loss kernels read."""
    probs = c["r64"]["probs"].astype(np.float32)
    mask = c["mask"].reshape(-1, S, S)
    return probs, mask


def _loss_ref(probs, mask, dtype):
    p = torch.from_numpy(probs).to(dtype).requires_grad_()
    total, focal, d0, d1, sums = SR.seg_loss(p, torch.from_numpy(mask).to(dtype))
    total.backward()
    terms = np.array([float(t.detach()) for t in (focal, d0, d1, total)])
    return terms, sums.detach().numpy(), p.grad.numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_seg_loss_forward_and_backward(dev, shape):
    B, g, S = shape
    probs, mask = _loss_io(case(*shape), S)
    l64, s64, g64 = _loss_ref(probs, mask, torch.float64)
    l32, s32, g32 = _loss_ref(probs, mask, torch.float32)
    p, m = cuda(probs, dev), cuda(mask, dev)
    sums, loss = ops.seg_loss(p, m)
    check_scalars(f"loss terms {shape}", loss.cpu().numpy(), l32, l64)
    check_scalars(f"per-image sums {shape}", sums.cpu().numpy()[:, :7], s32, s64)
    assert torch.all(sums[:, 7] == 0)
    one = torch.ones(1, device=dev)
    d1 = ops.seg_loss_bwd(p, m, sums, one)
    check_rel(f"dprobs {shape}", d1.cpu().numpy(), g32, g64)
    # dloss is a device scalar and scales the result linearly
    s = torch.full((1,), 0.37, device=dev)
    ds = ops.seg_loss_bwd(p, m, sums, s).cpu().numpy()
    want = (d1 * s).cpu().numpy()
    ulps = np.abs(ds.astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"dloss = 0.37 against 0.37 * (dloss = 1): max {ulps.max():.2f} ulp")
    assert ulps.max() <= 2


# ---------------------------------------------------------------------------- 4. upsample_softmax_bwd
def _up_ref(grid, dprobs, S, dtype):
    z = torch.from_numpy(grid).to(dtype).requires_grad_()
    SR.upsample_softmax(z, S).backward(torch.from_numpy(dprobs).to(dtype))
    return z.grad.numpy()


@pytest.mark.parametrize("kind", ["dense", "corner", "last"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_upsample_softmax_bwd(dev, shape, kind):
    B, g, S = shape
    grid = case(*shape)["r64"]["grid"].astype(np.float32)
    rng = np.random.default_rng(5 + S)
    if kind == "dense":
        dprobs = rng.standard_normal((B, 2, S, S)).astype(np.float32)
    else:  # one pixel: the first corner, or the last row and column (where the taps clamp)
        dprobs = np.zeros((B, 2, S, S), np.float32)
        y = x = 0 if kind == "corner" else S - 1
        dprobs[:, 0, y, x], dprobs[:, 1, y, x] = 1.3, -0.7
    got = ops.upsample_softmax_bwd(cuda(grid, dev), cuda(dprobs, dev)).cpu().numpy()
    ref, yard = _up_ref(grid, dprobs, S, torch.float64), _up_ref(grid, dprobs, S, torch.float32)
    if kind == "corner":  # src = 0 exactly: only cell (0, 0) receives anything
        assert np.count_nonzero(got[:, :, 1:, :]) == 0 and np.count_nonzero(got[:, :, :, 1:]) == 0
    if kind == "last":    # at most the last two rows / columns (fp32 scale * (S - 1) may fall short of g - 1)
        assert np.count_nonzero(got[:, :, :max(g - 2, 0), :]) == 0 and np.count_nonzero(got[:, :, :, :max(g - 2, 0)]) == 0
    check_rel(f"dgrid {kind} {shape}", got, yard, ref)


# ---------------------------------------------------------------------------- 5. patch_logits_bwd
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_patch_logits_bwd(dev, shape, dtype):
    B, g, S = shape
    c = case(*shape)
    L = g * g
    fh = torch.from_numpy(c["f"]).to(dtype)
    f = fh.to(dev).reshape(B * L, 768).contiguous()
    dg = np.random.default_rng(9 + g).standard_normal((B, 2, L)).astype(np.float32)
    dgrid = cuda(dg, dev)

    def ref(dt, T):
        ff, d, T = fh.to(dt), torch.from_numpy(dg).to(dt), T.to(dt)
        dT = 100.0 * torch.einsum("bpc,bap->bca", ff, d)
        if T.dim() == 2:
            return dT.sum(0).numpy(), (100.0 * torch.einsum("bap,ca->bpc", d, T)).numpy()
        return dT.numpy(), (100.0 * torch.einsum("bap,bca->bpc", d, T)).numpy()

    for Th in (torch.from_numpy(c["T"]), torch.from_numpy(c["T"][0].copy())):
        tag = "per-image" if Th.dim() == 3 else "shared"
        T = Th.to(dev).contiguous()
        dT, df = ops.patch_logits_bwd(f, T, dgrid, group=L)
        dT_only, none = ops.patch_logits_bwd(f, T, dgrid, group=L, need_df=False)
        none2, df_only = ops.patch_logits_bwd(f, T, dgrid, group=L, need_dT=False)
        assert none is None and none2 is None and dT.shape == T.shape and df.shape == (B * L, 768)
        assert torch.equal(dT, dT_only) and torch.equal(df, df_only)  # each alone gives the bits of both
        (dT64, df64), (dT32, df32) = ref(torch.float64, Th), ref(torch.float32, Th)
        check_rel(f"dT {tag} {shape} {dtype}", dT.cpu().numpy(), dT32, dT64)
        check_rel(f"df {tag} {shape} {dtype}", df.cpu().numpy().reshape(B, L, 768), df32, df64)


# ---------------------------------------------------------------------------- 6. / 7. train.py:86-100 as written
def _gold_case(gold, tag):
    B, g, S = (int(v) for v in gold[tag + "_shape"])
    f, T, mask = SR.inputs(int(gold[tag + "_seed"]), B, g, S, per_image=(tag == "a"))
    assert np.array_equal(T, gold[tag + "_T"])
    return (B, g, S), f, T, mask


@pytest.mark.parametrize("tag", ["a", "b"])
def test_train_lines_end_to_end_against_the_reference(dev, gold, tag):
    from forward_utils import calculate_seg_loss, calculate_similarity_map
    (B, g, img_size), f_np, T_np, mask_np = _gold_case(gold, tag)
    mask = cuda(mask_np, dev)
    f = cuda(f_np, dev)
    epoch_text_feature = cuda(T_np, dev).requires_grad_()
    patch_preds = calculate_similarity_map(f, epoch_text_feature, img_size)
    loss = calculate_seg_loss(patch_preds, mask)
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and f.grad is None
    check_scalars(f"case {tag} loss", float(loss.detach()), gold[tag + "_loss32"], gold[tag + "_loss64"])
    check_rel(f"case {tag} T.grad", epoch_text_feature.grad.cpu().numpy(), gold[tag + "_dT32"], gold[tag + "_dT64"])
    # the same with the features as the leaf
    f2 = cuda(f_np, dev).requires_grad_()
    T2 = cuda(T_np, dev)
    loss2 = calculate_seg_loss(calculate_similarity_map(f2, T2, img_size), mask)
    loss2.backward()
    assert torch.equal(loss2, loss) and T2.grad is None
    rows = gold[tag + "_rows"]
    got, want = f2.grad.cpu().numpy().reshape(-1, 768)[rows], gold[tag + "_df64"]
    e, y = SR.rel_l2(got, want), float(gold[tag + "_df32_rel"])
    print(f"case {tag} f.grad: rel-L2 {e:.3e}, the reference's fp32 run {y:.3e}, bound {8 * y:.3e}")
    assert f2.grad.shape == f2.shape and e <= 8 * y
    # both leaves in one backward give the same gradients
    f3, T3 = cuda(f_np, dev).requires_grad_(), cuda(T_np, dev).requires_grad_()
    calculate_seg_loss(calculate_similarity_map(f3, T3, img_size), mask[:, 0]).backward()
    assert torch.equal(f3.grad, f2.grad) and torch.equal(T3.grad, epoch_text_feature.grad)


def test_three_adam_steps_on_the_anchors(dev, gold):
    from forward_utils import calculate_seg_loss, calculate_similarity_map
    (B, g, S), f_np, T_np, mask_np = _gold_case(gold, "a")
    f, mask = cuda(f_np, dev), cuda(mask_np, dev)
    T = cuda(T_np, dev).requires_grad_()
    opt = torch.optim.Adam([T], lr=1e-3, betas=(0.5, 0.999))
    losses = []
    for _ in range(3):
        loss = calculate_seg_loss(calculate_similarity_map(f, T, S), mask)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(calculate_seg_loss(calculate_similarity_map(f, T, S), mask)))
    print("losses", losses, "reference", gold["a_adam_losses"])
    assert all(b < a for a, b in zip(losses, losses[1:]))
    check_scalars("step-0 loss", losses[0], gold["a_loss32"], gold["a_loss64"])


# ---------------------------------------------------------------------------- 8. determinism, batch invariance
def _all_kernels(dev, f_np, T_np, mask_np, S):
    B, L, _ = f_np.shape
    g = int(round(L ** 0.5))
    f, T, m = cuda(f_np, dev).reshape(B * L, 768), cuda(T_np, dev), cuda(mask_np, dev).reshape(B, S, S)
    grid = ops.patch_logits_per_image(f, T, torch.empty(B, 2, g, g, device=dev), group=L)
    probs = ops.blur_upsample(grid, torch.empty(B, 2, S, S, device=dev), ksize=0, sigma=0.0, softmax=True)
    sums, loss = ops.seg_loss(probs, m)
    dprobs = ops.seg_loss_bwd(probs, m, sums, torch.ones(1, device=dev))
    dgrid = ops.upsample_softmax_bwd(grid, dprobs)
    dT, df = ops.patch_logits_bwd(f, T, dgrid, group=L)
    return dict(grid=grid, sums=sums, loss=loss, dprobs=dprobs, dgrid=dgrid, dT=dT, df=df.reshape(B, L, 768))


@pytest.mark.parametrize("shape", [(3, 5, 23), (2, 37, 518)], ids=["B3g5S23", "B2g37S518"])
def test_determinism_and_batch_invariance(dev, shape):
    B, g, S = shape
    c = case(*shape)
    a = _all_kernels(dev, c["f"], c["T"], c["mask"], S)
    b = _all_kernels(dev, c["f"], c["T"], c["mask"], S)
    for k in a:
        assert torch.equal(a[k], b[k]), k                      # two launches, the same bits
    # image 0 alone, on its own slices of the batch's tensors (the loss carries 1 / B, so the
    # end-to-end gradients of a batch of 1 differ by that factor; the kernels' rows do not)
    L = g * g
    f0, T0 = cuda(c["f"][:1], dev).reshape(L, 768), cuda(c["T"][:1], dev)
    grid0 = ops.patch_logits_per_image(f0, T0, torch.empty(1, 2, g, g, device=dev), group=L)
    probs0 = ops.blur_upsample(grid0, torch.empty(1, 2, S, S, device=dev), ksize=0, sigma=0.0, softmax=True)
    sums0, _ = ops.seg_loss(probs0, cuda(c["mask"][:1], dev).reshape(1, S, S))
    dgrid0 = ops.upsample_softmax_bwd(grid0, a["dprobs"][:1].contiguous())
    dT0, df0 = ops.patch_logits_bwd(f0, T0, a["dgrid"][:1].contiguous(), group=L)
    assert torch.equal(grid0[0], a["grid"][0]) and torch.equal(sums0[0], a["sums"][0])
    assert torch.equal(dgrid0[0], a["dgrid"][0])
    assert torch.equal(dT0[0], a["dT"][0]) and torch.equal(df0, a["df"][0])


# ---------------------------------------------------------------------------- 9. / 10. the API keeps its behaviour
def test_shared_anchors_without_grad_are_todays_launches(dev):
    from forward_utils import calculate_similarity_map
    B, g, S = 2, 24, 336
    c = case(B, g, S)
    L = g * g
    f, T = cuda(c["f"], dev), cuda(c["T"][0], dev)
    grid = torch.empty(B, 2, g, g, device=dev)
    ops.patch_scores([f.reshape(B * L, 768)], T, grid, normalize=False, mode=1, group=L)
    today = ops.blur_upsample(grid, torch.empty(B, 2, S, S, device=dev), ksize=0, sigma=0.0, softmax=True)
    out = calculate_similarity_map(f, T, S, test=False)
    assert out.grad_fn is None and torch.equal(out, today)
    Tg = T.clone().requires_grad_()
    outg = calculate_similarity_map(f, Tg, S, test=False)
    assert outg.grad_fn is not None and torch.equal(outg.detach(), today)
    with torch.no_grad():
        assert calculate_similarity_map(f, Tg, S, test=False).grad_fn is None


def test_three_anchors_need_no_grad(dev):
    from forward_utils import calculate_similarity_map
    B, g, S = 3, 5, 23
    c = case(B, g, S)
    f = cuda(c["f"], dev)
    T3 = torch.cat([cuda(c["T"], dev), cuda(c["T"], dev)[:, :, :1] * 0.5], dim=2).contiguous()
    for T in (T3, T3[0].contiguous()):
        with pytest.raises(NotImplementedError, match="2 anchors"):
            calculate_similarity_map(f, T.clone().requires_grad_(), S)
        out = calculate_similarity_map(f, T, S).cpu()
        z = 100.0 * torch.matmul(torch.from_numpy(c["f"]).double(), T.cpu().double())
        ref = torch.softmax(F.interpolate(z.permute(0, 2, 1).reshape(B, 3, g, g), size=S, mode="bilinear",
                                          align_corners=True), dim=1)
        assert out.shape == (B, 3, S, S) and torch.allclose(out.double(), ref, atol=2e-5)
