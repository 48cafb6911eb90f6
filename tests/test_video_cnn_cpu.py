"""CPU tests of eav_amd.cnn_vision: state_dict keys and shapes, seeded initialisation against an independent restatement
of torchvision's ResNet-50 construction, backbone_weights loading, the constructor refusals, the C ABI's argument
refusals (nothing is launched) and the float64 restatement of tests/video_cnn_ref.py against torch.nn modules."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import video_cnn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_keys_shapes_and_seeded_init(capsys):
    from eav_amd.cnn_vision import VideoModel
    torch.manual_seed(1234)
    m = VideoModel()
    assert "backbone is not pretrained" in capsys.readouterr().out
    torch.manual_seed(1234)
    r = ref.TvVideoModel()
    a, b = m.state_dict(), r.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    for k in ("feature_extractor.0.weight", "feature_extractor.1.running_var", "feature_extractor.4.0.conv1.weight",
              "feature_extractor.7.2.bn3.num_batches_tracked", "feature_extractor.5.0.downsample.0.weight",
              "feature_extractor.5.0.downsample.1.bias", "attn_fc1.weight", "attn_fc2.bias", "classifier.1.weight",
              "classifier.3.bias"):
        assert k in a, k
    assert len([k for k in a if k.endswith(".weight") and a[k].dim() == 4]) == 53


def test_backbone_weights_from_torchvision_keys(tmp_path):
    from eav_amd.cnn_vision import VideoModel
    torch.manual_seed(5)
    tv = ref.TvResNet50().state_dict()
    path = str(tmp_path / "r50.pth")
    torch.save(tv, path)
    torch.manual_seed(6)
    for src in (tv, path):
        m = VideoModel(backbone_weights=src)
        fe = m.feature_extractor.state_dict()
        assert torch.equal(fe["0.weight"], tv["conv1.weight"])
        assert torch.equal(fe["4.0.downsample.0.weight"], tv["layer1.0.downsample.0.weight"])
        assert torch.equal(fe["7.2.bn3.running_var"], tv["layer4.2.bn3.running_var"])
    bad = dict(tv)
    del bad["layer2.1.conv2.weight"]
    with pytest.raises(KeyError):
        VideoModel(backbone_weights=bad)
    bad = dict(tv)
    bad["conv1.weight"] = torch.zeros(64, 3, 3, 3)
    with pytest.raises(ValueError):
        VideoModel(backbone_weights=bad)


def test_constructor_refusals():
    from eav_amd.cnn_vision import VideoModel
    with pytest.raises(ValueError, match="ratio"):
        VideoModel(ratio=2)
    with pytest.raises(ValueError):
        VideoModel(num_labels=0)


def test_batchnorm_forms_without_kernels_are_refused():
    from eav_amd.cnn_vision import VideoModel
    m = VideoModel()
    m.feature_extractor[5][1].bn2.momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        m(torch.zeros(1, 3, 64, 64))


def test_no_cpu_fallback():
    from eav_amd._lib import EavError
    from eav_amd.cnn_vision import VideoModel
    m = VideoModel()
    with pytest.raises(EavError):
        m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 64, 64))


def test_abi_argument_validation_without_gpu():
    """Bad shapes, strides and channel counts return a status with a message before anything is launched (run in a
    child process: with no device present the calls must fail in validation, never in a launch)."""
    code = r'''
from eav_amd import _lib
_lib.load()
L = _lib.load()
def rc(name, *a):
    r = getattr(L, name)(*a)
    return r, L.eav_last_error().decode()
p = 16
cases = [
    ("eav_video_conv_fwd", (p, p, p, 1, 3, 8, 8, 64, 3, 3, 2, 1, 5, 4, 0, None), "output map"),
    ("eav_video_conv_fwd", (p, p, p, 1, 5000, 8, 8, 64, 3, 3, 1, 1, 8, 8, 0, None), "bad geometry"),
    ("eav_video_conv_fwd", (p, p, p, 1, 3, 8, 8, 64, 3, 3, 0, 1, 8, 8, 0, None), "bad geometry"),
    ("eav_video_conv_fwd", (p, p, None, 1, 3, 8, 8, 64, 3, 3, 1, 1, 8, 8, 0, None), "null"),
    ("eav_video_conv_fwd", (p + 4, p, p, 1, 8, 8, 8, 64, 3, 3, 1, 1, 8, 8, 0, None), "aligned"),
    ("eav_video_conv_fwd", (p, p + 4, p, 1, 8, 8, 8, 64, 3, 3, 1, 1, 8, 8, 1, None), "aligned"),
    ("eav_video_conv_dgrad", (p + 4, p, None, p, 1, 64, 8, 8, 64, 3, 3, 1, 1, 8, 8, None), "aligned"),
    ("eav_video_conv_dgrad", (p, p, None, p, 1, 64, 8, 8, 64, 3, 3, 2, 3, 4, 4, None), "bad geometry"),
    ("eav_video_conv_wgrad", (p, p, p, 1, 64, 8, 8, 64, 3, 3, 1, 1, 8, 8, 0, 999, None), "nparts"),
    ("eav_video_bn_stats", (p, p, 100, 5000, None), "bad sizes"),
    ("eav_video_bn_apply", (p, p, p, None, p, p, p, 100, 64, 1, None), "residual"),
    ("eav_video_bn_bwd", (p, p, p, p, None, p, 100, 64, None), "gated"),
    ("eav_video_maxpool_fwd", (p, p, p, 1, 8, 8, 64, 3, 4, 3, 2, 1, None), "output map"),
    ("eav_video_head_pool", (p, p, p, 2, 300, 64, None), "HW <= 256"),
    ("eav_video_conv_relayout", (p, None, None, 4, 4, 9, None), "null"),
]
for name, args, msg in cases:
    r, m = rc(name, *args)
    assert r != 0 and msg in m, (name, r, m)
print("ok", len(cases))
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr


def test_kernels_compile_for_gfx950_without_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "eav_amd", "csrc", "video_cnn.hip")], capture_output=True, text=True)
    rows = [ln.split() for ln in out.stdout.splitlines()[1:] if ln.strip()]
    assert len(rows) >= 14, out.stdout + out.stderr
    for r in rows:
        assert r[2] == "0", f"scratch in {' '.join(r[5:])}"


@pytest.mark.parametrize("training,freeze", [(True, False), (True, True), (False, False)])
def test_reference_restatement_equals_torch_modules(training, freeze):
    torch.manual_seed(3)
    r = ref.TvVideoModel().double()
    with torch.no_grad():
        for k, v in r.state_dict().items():
            if k.endswith("running_var"):
                v.uniform_(0.5, 1.5)
            elif k.endswith("running_mean") or (k.endswith("bias") and k.startswith("feature")):
                v.uniform_(-0.1, 0.1)
    sd = {k: v.clone() for k, v in r.state_dict().items()}
    x = torch.randn(2, 3, 48, 40, dtype=torch.float64)
    y = torch.tensor([1, 3])
    r.train(training)
    if freeze:
        for p in r.feature_extractor.parameters():
            p.requires_grad_(False)
    out = r(x)
    torch.nn.functional.cross_entropy(out, y).backward()
    logits, loss, grads, sd1 = ref.step(sd, x, y, training=training, freeze=freeze)
    assert torch.allclose(logits, out.detach(), rtol=1e-12, atol=1e-12)
    for k, p in r.named_parameters():
        if p.grad is None:
            assert grads[k] is None, k
        else:
            assert torch.allclose(grads[k], p.grad, rtol=1e-10, atol=1e-13), k
    for k, v in r.state_dict().items():
        assert torch.allclose(sd1[k].double(), v.double(), rtol=1e-12, atol=1e-14), k


# ---------------------------------------------------------------------------------------------- golden fixtures
GOLDEN_STEPS = ["unfrozen_b4", "frozen_b4", "eval_b3", "adamw2_b4"]


def _golden(golden_dir, name):
    return ref.load_golden(os.path.join(golden_dir, f"video_cnn_{name}.npz"))


@pytest.mark.parametrize("name", GOLDEN_STEPS)
def test_seeded_state_dict_equals_golden(name, golden_dir):
    """torch.manual_seed(s); VideoModel() draws the numbers the imported reference (over the restated torchvision
    resnet50) drew: every floating state_dict tensor's sample and its sum |.| / max |.|."""
    from eav_amd.cnn_vision import VideoModel
    g, pins = _golden(golden_dir, name)
    torch.manual_seed(int(g["wseed"]))
    sd = VideoModel().state_dict()
    keys = [k for k, v in sd.items() if v.is_floating_point()]
    assert sorted("init." + k for k in keys) == sorted(k for k in pins if k.startswith("init."))
    for k in keys:
        smp, ab = pins["init." + k]
        assert np.array_equal(ref.sample_of(sd[k]), smp), k
        assert float(sd[k].double().abs().sum()) == pytest.approx(ab[0], rel=1e-12) and float(sd[k].abs().max()) == ab[1]


@pytest.mark.parametrize("name", GOLDEN_STEPS)
def test_reference_restatement_pinned_to_golden(name, golden_dir):
    """tests/video_cnn_ref.py in fp32 on the CPU reproduces the imported reference's step bit for bit: logits, loss,
    every gradient and (after torch.optim.AdamW) every post-step parameter and BatchNorm buffer sample."""
    from eav_amd.cnn_vision import VideoModel
    g, pins = _golden(golden_dir, name)
    torch.manual_seed(int(g["wseed"]))
    sd = {k: v.clone() for k, v in VideoModel().state_dict().items()}
    train, freeze, steps, lr = bool(g["train"]), bool(g["freeze"]), int(g["steps"]), float(g["lr"])
    state = {}
    for s in range(steps):
        x, y = ref.golden_inputs(g, s)
        if not train:
            with torch.no_grad():
                logits = ref.head(ref.trunk(x, sd, False), sd)
            assert np.array_equal(logits.numpy(), g[f"logits{s}"])
            continue
        logits, loss, grads, sd = ref.step(sd, x, y, training=True, freeze=freeze, dtype=torch.float32)
        assert np.array_equal(logits.numpy(), g[f"logits{s}"]), f"logits of step {s}"
        assert loss.item() == float(g[f"loss{s}"])
        for k, gr in grads.items():
            assert (gr is None) == (f"grad{s}." + k not in pins), k
            if gr is not None:
                assert np.array_equal(ref.sample_of(gr), pins[f"grad{s}." + k][0]), f"grad {k} of step {s}"
        # the reference's torch.optim.AdamW(model.parameters(), lr), one state per parameter across the steps
        for k, gr in grads.items():
            if gr is None:
                continue
            if k not in state:
                leaf = sd[k].clone().requires_grad_(True)
                state[k] = (leaf, torch.optim.AdamW([leaf], lr=lr))
            leaf, opt = state[k]
            leaf.grad = gr.clone()
            opt.step()
            sd[k] = leaf.detach().clone()
    nbt = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")]
    assert nbt == list(g["post.num_batches_tracked"])
    for k, v in sd.items():
        if v.is_floating_point():
            assert np.array_equal(ref.sample_of(v), pins["post." + k][0]), f"post-step {k}"


def test_golden_trainer_lines_are_the_reference_run(golden_dir):
    """The trainer fixture: the imported reference's printed lines, one logit row per argmax behind them (with the margin
    the generator required) and outputs_test [N_test * F, C] - read by the GPU trainer test."""
    g = np.load(os.path.join(golden_dir, "video_cnn_trainer.npz"))
    lines = [str(s) for s in g["lines"]]
    assert lines[:3] == ["Preprocessing images...", "Done.", "Training (frozen) | lr=0.0005"]
    assert sum(ln.startswith("Epoch ") for ln in lines) == 3
    F_, ntr, nte, _ = (int(v) for v in g["frames"])
    assert g["outputs_test"].shape == (nte * F_, 5)
    rows = np.sort(g["rows"], axis=1)
    assert float((rows[:, -1] - rows[:, -2]).min()) >= float(g["margin"])
