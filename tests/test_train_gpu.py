"""train.py end to end on the synthetic train set: both stages, the reference's checkpoint files
and keys, resume, and test.py loading what train.py wrote. One module-scoped training run (random
init, 70 px, 4 images, batches of 2, one epoch per stage) is shared by the checks."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4",
        "--text_batch_size", "2", "--image_batch_size", "2", "--text_epoch", "1"]


def _visual_ptrs(model):
    """Where the frozen visual packing lives (forward and backward copies), and which engine."""
    v = model.visual_engine()
    return (id(v), v.conv.data_ptr(), v.blocks[7]["w_fc"].data_ptr(), v._bwd[7]["w_fc"].data_ptr(),
            v.blocks[23]["w_qkv"].data_ptr(), v._bwd[23]["w_qkv"].data_ptr())


def _text_ptrs(model):
    t = model.clipmodel.text_engine(model.text_adapter.state_dict(), model.text_adapt_until, model.t_w)
    return (id(t), t.tok_emb.data_ptr(), t.blocks[5]["w_fc"].data_ptr(), t._bwd[5]["w_fc"].data_ptr())


def _spy_steps(optimizer, record, probe):
    """optimizer.step that appends probe() to `record` after every step."""
    real = optimizer.step

    def step(*a, **k):
        r = real(*a, **k)
        record.append(probe())
        return r
    optimizer.step = step


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    import train
    save = str(tmp_path_factory.mktemp("train_run"))
    args = train.parse_args(ARGS + ["--image_epoch", "1", "--save_path", save])
    seen = {"text_steps": [], "image_steps": []}
    real_text, real_image = train.train_text_adapter, train.train_image_adapter

    def spy_text(adapted_model, optimizer, **kw):
        # the initial adapter weights: what train.run built after its own seeding
        seen["text0"] = {k: v.detach().clone() for k, v in adapted_model.text_adapter.state_dict().items()}
        seen["image0"] = {k: v.detach().clone() for k, v in adapted_model.image_adapter.state_dict().items()}
        _spy_steps(optimizer, seen["text_steps"], lambda: _text_ptrs(adapted_model))
        return real_text(adapted_model=adapted_model, optimizer=optimizer, **kw)

    def spy_image(model, optimizer, **kw):
        _spy_steps(optimizer, seen["image_steps"], lambda: _visual_ptrs(model))
        return real_image(model=model, optimizer=optimizer, **kw)

    train.train_text_adapter, train.train_image_adapter = spy_text, spy_image
    try:
        ctx = train.run(args)
    finally:
        train.train_text_adapter, train.train_image_adapter = real_text, real_image
    return dict(save=save, ctx=ctx, **seen)


def test_checkpoints_have_the_reference_keys(trained):
    save = trained["save"]
    files = sorted(os.path.basename(f) for f in glob.glob(save + "/*.pth"))
    assert files == ["image_adapter.pth", "image_adapter_1.pth", "text_adapter.pth"]
    t = torch.load(os.path.join(save, "text_adapter.pth"), map_location="cpu", weights_only=True)
    assert set(t) == {"epoch", "text_adapter", "text_optimizer"} and t["epoch"] == 1
    for name in ("image_adapter.pth", "image_adapter_1.pth"):
        c = torch.load(os.path.join(save, name), map_location="cpu", weights_only=True)
        assert set(c) == {"epoch", "image_adapter", "image_optimizer"} and c["epoch"] == 1
        assert tuple(c["image_optimizer"]["param_groups"][0]["betas"]) == (0.5, 0.999)
    model = trained["ctx"]["model"]
    assert set(t["text_adapter"]) == set(model.text_adapter.state_dict())
    assert set(c["image_adapter"]) == set(model.image_adapter.state_dict())
    assert model.compute_dtype == torch.float32


def test_every_adapter_weight_moved_and_losses_are_finite(trained):
    ctx, save = trained["ctx"], trained["save"]
    assert ctx["adapt_text"] and ctx["text_start_epoch"] == 0 and ctx["image_start_epoch"] == 0
    assert len(ctx["text_losses"]) == 2 and len(ctx["image_losses"]) == 2  # 4 images, batches of 2
    assert np.all(np.isfinite(ctx["text_losses"])) and np.all(np.isfinite(ctx["image_losses"]))
    t = torch.load(os.path.join(save, "text_adapter.pth"), map_location="cpu", weights_only=True)["text_adapter"]
    c = torch.load(os.path.join(save, "image_adapter_1.pth"), map_location="cpu", weights_only=True)["image_adapter"]
    for k, v in trained["text0"].items():
        assert not torch.equal(v.cpu(), t[k]), k
        assert torch.isfinite(t[k]).all(), k
    for k, v in trained["image0"].items():
        assert not torch.equal(v.cpu(), c[k]), k
        assert torch.isfinite(c[k]).all(), k


def test_frozen_packing_stays_put_across_steps(trained):
    for steps in (trained["text_steps"], trained["image_steps"]):
        assert len(steps) == 2 and steps[0] == steps[1]  # an optimizer step repacks nothing frozen


def test_test_py_loads_the_checkpoints(trained):
    import test as harness
    args = harness.parse_args(["--dataset", "synthetic", "--allow_random_init", "--img_size", "70", "--synthetic_n", "4",
                               "--batch_size", "4", "--save_path", trained["save"], "--compute_dtype", "fp32"])
    df, ctx = harness.run(args)
    assert list(df["class name"]) == ["bottle", "Average"]
    assert np.all(np.isfinite(df.drop(columns=["class name"]).to_numpy(dtype=np.float64)))
    # the adapters test.py evaluated are the trained ones
    c = torch.load(os.path.join(trained["save"], "image_adapter_1.pth"), map_location="cpu", weights_only=True)
    for k, v in ctx["model"].image_adapter.state_dict().items():
        assert torch.equal(v.cpu(), c["image_adapter"][k]), k
    t = torch.load(os.path.join(trained["save"], "text_adapter.pth"), map_location="cpu", weights_only=True)
    for k, v in ctx["model"].text_adapter.state_dict().items():
        assert torch.equal(v.cpu(), t["text_adapter"][k]), k


def test_resume_runs_only_the_missing_epoch(trained):
    import train
    save = trained["save"]
    read = lambda n: open(os.path.join(save, n), "rb").read()  # noqa: E731
    before = {n: read(n) for n in ("image_adapter_1.pth", "text_adapter.pth")}
    ctx = train.run(train.parse_args(ARGS + ["--image_epoch", "2", "--save_path", save]))
    assert ctx["image_start_epoch"] == 1 and ctx["text_start_epoch"] == 1
    # the reference's expression: adapt_text = not (1 == text_epoch - 1) is True, and range(1, 1) is empty
    assert ctx["adapt_text"] and ctx["text_losses"] == []
    assert len(ctx["image_losses"]) == 2 and np.all(np.isfinite(ctx["image_losses"]))
    assert read("image_adapter_1.pth") == before["image_adapter_1.pth"]
    assert read("text_adapter.pth") == before["text_adapter.pth"]
    c2 = torch.load(os.path.join(save, "image_adapter_2.pth"), map_location="cpu", weights_only=True)
    c = torch.load(os.path.join(save, "image_adapter.pth"), map_location="cpu", weights_only=True)
    assert c2["epoch"] == 2 and c["epoch"] == 2
    c1 = torch.load(os.path.join(save, "image_adapter_1.pth"), map_location="cpu", weights_only=True)
    assert any(not torch.equal(c1["image_adapter"][k], c2["image_adapter"][k]) for k in c1["image_adapter"])
    assert float(c2["image_optimizer"]["state"][0]["step"]) == 4  # Adam's state came back from the checkpoint


def test_cpu_preprocess_path_runs_one_step_of_each_stage(dev, tmp_path):
    import train
    ctx = train.run(train.parse_args(ARGS + ["--image_epoch", "1", "--no-gpu_preprocess", "--max_steps", "1",
                                             "--save_path", str(tmp_path)]))
    assert len(ctx["text_losses"]) == 1 and len(ctx["image_losses"]) == 1
    assert np.isfinite(ctx["text_losses"][0]) and np.isfinite(ctx["image_losses"][0])
    assert os.path.exists(tmp_path / "text_adapter.pth") and os.path.exists(tmp_path / "image_adapter_1.pth")
