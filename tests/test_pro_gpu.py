"""Pixel AUPRO on the MI355X: the component labelling kernel (aaclip_label_components) against
scipy.ndimage.label with exact integer equality, and aaclip_metrics_eval_pro against the
curve-walking float64 reference (tests/pro_ref.py) within 1e-9, the bound
tests/test_metrics_gpu.py holds AUROC / AP to; its first four numbers bit-identical to
aaclip_metrics_eval; the drop-in API and the harness's --pro column."""
import json

import numpy as np
import pytest
import torch
from scipy import ndimage

from aaclip import ops

import pro_ref as PR

pytestmark = pytest.mark.gpu

LIMITS = (0.05, 0.3, 1.0)


# ---------------------------------------------------------------------------- labelling
def _serpentine(H, W):
    """A one-pixel-wide path over the whole image: full even rows, joined at alternating ends."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def _patterns(H, W, seed):
    r = np.random.default_rng(seed)
    z = lambda: np.zeros((H, W), dtype=np.uint8)  # noqa: E731
    yy, xx = np.mgrid[0:H, 0:W]
    out = {"empty": z(), "full": z() + 1}
    m = z()
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = 1
    out["corners"] = m
    out["checkerboard"] = ((yy + xx) % 2 == 0).astype(np.uint8)
    out["diagonal"] = (yy == xx).astype(np.uint8)
    out["antidiagonal"] = (yy == (W - 1 - xx)).astype(np.uint8)
    out["alternate rows"] = (yy % 2 == 0).astype(np.uint8)
    out["alternate columns"] = (xx % 2 == 0).astype(np.uint8)
    if H > 1:
        m = z()
        m[H // 2 - 1, W - 1] = m[H // 2, 0] = 1
        out["row end and next row start"] = m
    m = ((xx % 2 == 0) | (yy == H - 1)).astype(np.uint8)
    out["comb"] = m
    out["serpentine"] = _serpentine(H, W)
    for p in (0.1, 0.4, 0.6):
        out[f"bernoulli {p}"] = (r.random((H, W)) < p).astype(np.uint8)
    return out


def _check_labelling(dev, masks, what):
    masks = np.ascontiguousarray(masks)
    labels, areas, counts = ops.label_components(torch.from_numpy(masks).to(dev))
    rl, ra, rc = PR.label_ref(masks)
    counts = counts.cpu().numpy()
    assert not (counts == 0xFFFFFFFF).any(), (what, counts)  # a loop cap was hit
    assert np.array_equal(counts, rc), (what, counts, rc)
    assert np.array_equal(labels.cpu().numpy(), rl), what
    assert np.array_equal(areas.cpu().numpy(), ra), what


@pytest.mark.parametrize("S", [1, 7, 37, 64, 65, 130])
def test_label_components_patterns(dev, S):
    pats = _patterns(S, S, S)
    names, imgs = list(pats), list(pats.values())
    at, k = 0, 0
    while at < len(imgs):  # calls of 1, 2, 3, 4, 5, 1, ... images
        n = min(1 + k % 5, len(imgs) - at)
        _check_labelling(dev, np.stack(imgs[at:at + n]), (S, names[at:at + n]))
        at, k = at + n, k + 1
    if S > 1:
        # last row of image k and first row of image k + 1 full: consecutive images never merge
        m = np.zeros((3, S, S), dtype=np.uint8)
        m[0, S - 1], m[1, 0], m[1, S - 1], m[2, 0] = 1, 1, 1, 1
        _check_labelling(dev, m, (S, "image seams"))
        labels, _, counts = ops.label_components(torch.from_numpy(m).to(dev))
        assert counts.tolist() == [1, 2, 1]


def test_label_components_expected_counts(dev):
    """The patterns' component counts by construction, so that the reference is checked too."""
    S = 37
    pats = _patterns(S, S, 0)
    want = {"empty": 0, "full": 1, "corners": 4, "checkerboard": 1, "diagonal": 1, "antidiagonal": 1,
            "alternate rows": (S + 1) // 2, "alternate columns": (S + 1) // 2, "row end and next row start": 2,
            "comb": 1, "serpentine": 1}
    m = np.stack([pats[k] for k in want])
    _, areas, counts = ops.label_components(torch.from_numpy(m).to(dev))
    assert counts.tolist() == list(want.values())
    assert int(areas[list(want).index("serpentine")].max()) == int(pats["serpentine"].sum())


def test_label_components_non_square_and_dtypes(dev):
    pats = _patterns(37, 70, 3)
    _check_labelling(dev, np.stack(list(pats.values())[:5]), "37x70 a")
    _check_labelling(dev, np.stack(list(pats.values())[5:]), "37x70 b")
    m = torch.from_numpy(pats["bernoulli 0.4"]).to(dev)
    want = ops.label_components(m[None])
    for t in (m[None, None].float() * 0.25, m[None].bool(), m[None].to(torch.int64) * -3):  # binarised with != 0
        got = ops.label_components(t)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        ops.label_components(m)


def test_label_components_serpentine_518(dev):
    """One component of 134 k pixels along a path: the deepest parent chains."""
    _check_labelling(dev, _serpentine(518, 518)[None], "serpentine 518")


# ---------------------------------------------------------------------------- AUPRO
def _blobs(seed, N, S, sigma=2.5, q=0.9):
    """Smooth random blobs (a thresholded blurred noise field); the last image is defect-free."""
    r = np.random.default_rng(seed)
    field = np.stack([ndimage.gaussian_filter(r.standard_normal((S, S)), sigma) for _ in range(N)])
    masks = (field > np.quantile(field, q)).astype(np.uint8)
    masks[-1] = 0
    scores = (field / field.std() + 0.8 * r.standard_normal((N, S, S))).astype(np.float32)
    return masks, scores


def _with_images(masks, scores, seed=0):
    N = masks.shape[0]
    ip = np.random.default_rng(seed).random(N).astype(np.float32)
    il = (masks.reshape(N, -1).max(1) > 0).astype(np.int64)
    return masks, scores, ip, il


def _quantise(scores, levels):
    lo, hi = scores.min(), scores.max()
    return (np.floor((scores - lo) / (hi - lo) * levels).clip(0, levels - 1) / levels).astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    masks, scores = _blobs(11, 4, 37)
    out = {"continuous": _with_images(masks, scores)}
    for lv in (2, 4, 8):
        out[f"{lv} levels"] = _with_images(masks, _quantise(scores, lv))
    out["all equal 1.0"] = _with_images(masks, np.ones_like(scores))
    out["all equal 0.5"] = _with_images(masks, np.full_like(scores, 0.5))
    out["separated"] = _with_images(masks, (np.random.default_rng(2).random(scores.shape) + 2.0 * masks)
                                    .astype(np.float32))
    return out


def _device(dev, case, L, medical=False):
    masks, scores, ip, il = case
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (scores, masks, ip, il)]
    out5 = ops.metrics_eval_device(*t, medical=medical, pro=True, fpr_limit=L)
    again = ops.metrics_eval_device(*t, medical=medical, pro=True, fpr_limit=L)
    out4 = ops.metrics_eval_device(t[0].reshape(t[0].shape[0], -1), t[1].reshape(t[1].shape[0], -1), t[2], t[3],
                                   medical=medical)
    assert out5.shape == (5,) and out5.dtype == torch.float64 and out4.shape == (4,)
    assert torch.equal(out5[:4].view(torch.int64), out4.view(torch.int64))  # the bits of aaclip_metrics_eval
    assert torch.equal(out5.view(torch.int64), again.view(torch.int64))  # two launches, the same bits
    return out5.tolist()


@pytest.mark.parametrize("L", LIMITS)
@pytest.mark.parametrize("name", ["continuous", "2 levels", "4 levels", "8 levels", "all equal 1.0", "all equal 0.5",
                                  "separated"])
def test_aupro_vs_reference(dev, cases, name, L):
    case = cases[name]
    got = _device(dev, case, L)[4]
    want = PR.aupro_ref(case[0], case[1], L)
    print(name, L, got, want, abs(got - want))
    assert abs(got - want) <= 1e-9, (name, L, got, want)
    if name.startswith("all equal"):
        assert abs(got - L / 2) <= 1e-9  # 0.15 at L = 0.3
    if name == "separated":
        assert abs(got - 1.0) <= 1e-9


def test_aupro_single_component_full_range_is_auroc(dev):
    """One component and L = 1: PRO is the true-positive rate, so AUPRO is the pixel AUROC."""
    r = np.random.default_rng(4)
    masks = np.zeros((2, 37, 37), dtype=np.uint8)
    masks[0, 5:16, 9:20] = 1
    for lv in (None, 4):
        scores = (r.standard_normal(masks.shape) + masks).astype(np.float32)
        if lv:
            scores = _quantise(scores, lv)
        out = _device(dev, _with_images(masks, scores), 1.0)
        assert abs(out[4] - out[0]) <= 1e-12, out
        assert abs(out[4] - PR.aupro_ref(masks, scores, 1.0)) <= 1e-9


def test_aupro_weights_regions_equally(dev):
    """A large and a one-pixel component, scores that find only the large one: the pixel AUROC
    is near 1, AUPRO is one half."""
    masks = np.zeros((1, 24, 24), dtype=np.uint8)
    masks[0, 2:12, 2:12] = 1
    masks[0, 20, 20] = 1
    scores = np.random.default_rng(6).random(masks.shape).astype(np.float32)
    scores += 2.0 * masks
    scores[0, 20, 20] = -1.0  # below every ok pixel
    case = (masks, scores, np.array([0.5], np.float32), np.array([1]))
    out = _device(dev, case, 0.3)
    assert out[0] > 0.98 and abs(out[4] - 0.5) <= 1e-9, out
    assert abs(out[4] - PR.aupro_ref(masks, scores, 0.3)) <= 1e-9


def test_aupro_518(dev):
    """8 maps of 518 x 518 (4-byte arrays that are no multiple of 256 B), 512 score levels."""
    masks, scores = _blobs(12, 8, 518, sigma=9.0, q=0.97)
    scores = _quantise(scores, 512)
    case = _with_images(masks, scores)
    for medical in (False, True):
        out = _device(dev, case, 0.3, medical)
    want = PR.aupro_ref(masks, scores, 0.3)
    print("518", out[4], want, abs(out[4] - want))
    assert abs(out[4] - want) <= 1e-9, (out[4], want)


@pytest.mark.parametrize("fill", [0, 1])
def test_aupro_no_component_or_no_ok_pixel(dev, cases, fill):
    from forward_utils import metrics_eval
    masks, scores, ip, il = cases["continuous"]
    masks = np.full_like(masks, fill)
    out = _device(dev, (masks, scores, ip, il), 0.3)
    assert np.isnan(out[4]) and np.isnan(out[0])
    with pytest.raises(ValueError, match="Only one class present"):
        metrics_eval(masks[:, None], il, scores, ip, "c", "Industrial", pro=True)


def test_ops_pro_arguments(dev, cases):
    masks, scores, ip, il = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in cases["continuous"])
    with pytest.raises(ValueError, match="H, W"):  # flattened maps carry no image shape
        ops.metrics_eval_device(scores.reshape(4, -1), masks.reshape(4, -1), ip, il, medical=False, pro=True)
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="fpr_limit"):
            ops.metrics_eval_device(scores, masks, ip, il, medical=False, pro=True, fpr_limit=bad)
    five = ops.metrics_eval(scores, masks[:, None], ip, il, medical=False, pro=True, fpr_limit=0.05)
    four = ops.metrics_eval(scores, masks, ip, il, medical=False)
    assert len(five) == 5 and five[:4] == four
    assert abs(five[4] - PR.aupro_ref(cases["continuous"][0], cases["continuous"][1], 0.05)) <= 1e-9


# ---------------------------------------------------------------------------- public API, harness
def test_forward_utils_pro_dict(dev, cases):
    from forward_utils import metrics_eval
    masks, scores, ip, il = cases["8 levels"]
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (masks[:, None], il, scores, ip)]
    plain = metrics_eval(*t, "cls", "Industrial")
    assert list(plain) == ["class name", "pixel AUC", "pixel AP", "image AUC", "image AP"]
    r = metrics_eval(*t, "cls", "Industrial", pro=True)
    assert list(r) == list(plain) + ["pixel AUPRO"]
    assert all(r[k] == plain[k] for k in plain)
    assert r["pixel AUPRO"] == pytest.approx(round(PR.aupro_ref(masks, scores, 0.3), 4) * 100, abs=1e-9)
    # numpy inputs, as the reference passes them
    rn = metrics_eval(masks[:, None], il, scores, ip, "cls", "Industrial", pro=True)
    assert rn == r


def test_harness_pro_column(dev, tmp_path):
    import test as harness
    from dataset import DOMAINS
    path = tmp_path / "table.json"
    args = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4", "--pro",
            "--save_path", str(tmp_path), "--results_json", str(path)]
    df, ctx = harness.run(harness.parse_args(args))
    assert list(df.columns) == ["class name", "pixel AUC", "pixel AP", "image AUC", "image AP", "pixel AUPRO"]
    assert df.iloc[-1]["class name"] == "Average" and len(df) == len(ctx["classes"]) + 1
    col = []
    for cls, (masks, labels, preds, preds_image) in ctx["classes"].items():
        want = PR.aupro_ref(masks.cpu().numpy(), preds.cpu().numpy(), 0.3)
        raw = ops.metrics_eval_device(preds, masks, preds_image, torch.from_numpy(np.asarray(labels)).to(preds.device),
                                      medical=DOMAINS["synthetic"] == "Medical", pro=True).tolist()[4]
        row = df[df["class name"] == cls].iloc[0]
        print(cls, row["pixel AUPRO"], raw, want)
        assert abs(raw - want) <= 1e-9
        assert abs(float(row["pixel AUPRO"]) - round(want, 4) * 100) <= 1e-9 * 100
        col.append(float(row["pixel AUPRO"]))
        # a random-init model can rank every defect below the FPR limit (AUPRO 0): the same class
        # with the maps negated goes through the deferred entry point the harness uses
        from forward_utils import metrics_eval_deferred
        flipped = metrics_eval_deferred(masks, labels, -preds, preds_image, cls, DOMAINS["synthetic"], pro=True)()
        want = PR.aupro_ref(masks.cpu().numpy(), -preds.cpu().numpy(), 0.3)
        print(cls, "negated", flipped["pixel AUPRO"], want)
        assert max(want, PR.aupro_ref(masks.cpu().numpy(), preds.cpu().numpy(), 0.3)) > 0.05
        assert abs(flipped["pixel AUPRO"] - round(want, 4) * 100) <= 1e-9 * 100
    assert abs(float(df.iloc[-1]["pixel AUPRO"]) - np.mean(col)) <= 1e-9
    rows = json.loads(path.read_text())["rows"]
    assert [abs(r["pixel AUPRO"] - c) <= 1e-9 for r, c in zip(rows, col)] == [True] * len(col)
