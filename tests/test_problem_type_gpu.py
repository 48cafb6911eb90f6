"""config.problem_type through the encoder and the trainers on the GPU: labelled forwards of the three problem types against
oracle.vit_oracle.forward + tests/problem_type_ref.loss (pinned to the Hugging Face classes by
tests/test_problem_type_cpu.py), the unchanged single-label route, the two fine-tuning trainers with float labels, and
save_pretrained after training.

Bounds: those of tests/test_wide_head_gpu.py::test_wide_head_model_steps_match_oracle (logits and loss 1e-4 relative +
1e-4, gradients 1e-3 of the tensor's maximum) and the 1e-3 on outputs_test of tests/test_transformer_trainers_gpu.py."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import problem_type_ref as ptr
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu

REDUCED = dict(hidden=64, layers=2, heads=4, ff=128)          # at the canonical token counts: 1214 (AST), 197 (ViT)
CASES = {
    "ast-multi-label-527": ("ast", 527, None, "multi_label_classification"),
    "vit-regression-2": ("vit", 2, "regression", "regression"),
    "vit-unset-1": ("vit", 1, None, "regression"),
}


def _model(kind, num_labels, seed, problem_type=None):
    from eav_amd import transformer as T
    from oracle import vit_oracle as vo
    ocfg = (vo.cfg_ast if kind == "ast" else vo.cfg_vit)(num_labels=num_labels, **REDUCED)
    assert ocfg["ntok"] == (1214 if kind == "ast" else 197)
    W = tf_weights(seed, vo.param_shapes(ocfg), std=0.05)
    model = T.Encoder(T.make_config(kind, num_labels=num_labels, problem_type=problem_type, **REDUCED), W).cuda().train()
    return model, ocfg, W


def _batch(kind, seed, B):
    return (synth.mel_batch(seed, B, 1024, 128) if kind == "ast" else synth.frame_batch(seed, B, 224))[0]


def _labels(problem_type, seed, B, num_labels):
    if problem_type == "multi_label_classification":
        return (synth.uniform(seed, (B, num_labels)) < 0.1).astype(np.float32)
    return synth.normal(seed, (B, num_labels)).astype(np.float32)


def _close(got, ref, rtol, atol, what):
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    print(f"{what}: max error {err.max():.3e}, reference max {np.abs(ref).max():.3e}")
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("precision", ["fp32", "split"])
@pytest.mark.parametrize("case", list(CASES))
def test_labelled_steps_match_oracle(case, precision):
    """One unfrozen and one frozen step through forward(labels=...): logits, loss and every gradient against the oracle;
    the same step through Encoder.head on the cached features gives the same bits; the type is resolved once and stays."""
    kind, NC, given, resolved = CASES[case]
    model, ocfg, W = _model(kind, NC, 61, given)
    model.precision = precision
    assert model.cfg.problem_type == given
    for s, freeze in enumerate((False, True)):
        x = _batch(kind, 63 + s, 3)
        y = _labels(resolved, 65 + s, 3, NC)
        for k, p in model.named_parameters():
            p.requires_grad = (not freeze) or k.startswith("classifier.")
            p.grad = None
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        out = model(xd, labels=yd)
        assert model.cfg.problem_type == resolved
        crit = model.criterion()
        assert type(crit).__name__ == {"regression": "MSELoss", "multi_label_classification": "BCEWithLogitsLoss"}[resolved]
        out.loss.backward()
        named = dict(model.named_parameters())
        grads = {k: p.grad.clone() for k, p in named.items() if p.grad is not None}
        torch.cuda.synchronize()
        lref, lossref, gref = ptr.step_reference(W, ocfg, x, y, resolved, freeze)
        _close(out.logits, lref, 1e-4, 1e-4, f"{case} {precision} logits{s}")
        _close(out.loss, lossref, 1e-4, 1e-4, f"{case} {precision} loss{s}")
        assert sorted(grads) == sorted(gref)
        for k, g in gref.items():
            g = g.numpy()
            _close(grads[k], g, 1e-3, max(1e-3 * np.abs(g).max(), 1e-6), f"{case} {precision} grad{s}.{k}")
        if NC == 1:         # HF's squeeze(): [B] and [B, 1] targets are one thing
            flat = model(xd, labels=yd[:, 0])
            assert torch.equal(_bits(flat.loss), _bits(out.loss)) and torch.equal(_bits(flat.logits), _bits(out.logits))
        # the head alone on the cached features: the same kernels on the same values
        for p in model.parameters():
            p.grad = None
        again = model.head(model.last_features()).logits
        assert torch.equal(_bits(again), _bits(out.logits))
        loss2 = crit(again, yd)
        assert torch.equal(_bits(loss2), _bits(out.loss))
        loss2.backward()
        for k in grads:
            if k.startswith("classifier."):
                assert torch.equal(_bits(named[k].grad), _bits(grads[k])), k
        assert model.criterion() is crit                  # held on the encoder, not rebuilt per call


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_single_label_route_is_unchanged(precision):
    """Integer labels, five classes: forward(labels=y).loss is CrossEntropyLoss()(forward(x).logits, y) - loss, logits
    and every gradient bit for bit."""
    from eav_amd.optim import CrossEntropyLoss
    model, _, _ = _model("vit", 5, 71)
    model.precision = precision
    x = torch.from_numpy(_batch("vit", 72, 3)).cuda()
    y = torch.from_numpy(synth.labels(73, 3)).cuda()

    def step(labelled):
        for p in model.parameters():
            p.grad = None
        if labelled:
            out = model(x, labels=y)
            loss, logits = out.loss, out.logits
        else:
            logits = model(x).logits
            loss = CrossEntropyLoss()(logits, y)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}

    la, ga, da = step(True)
    assert model.cfg.problem_type == "single_label_classification"
    assert type(model.criterion()).__name__ == "CrossEntropyLoss"
    lb, gb, db = step(False)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ga), _bits(gb))
    assert sorted(da) == sorted(db)
    for k in da:
        assert torch.equal(_bits(da[k]), _bits(db[k])), k


# ------------------------------------------------------------------------------------------------------------ trainers
TRAINERS = {"ast": ("multi_label_classification", 20), "vit": ("regression", 2)}
ORDERS = [[3, 0, 5, 1, 4, 2], [2, 4, 1, 5, 0, 3], [5, 3, 0, 2, 1, 4]]
_RUNS = {}


def _save_model_dir(path, kind, seed):
    """HF-format directory of the reduced model (five labels, as the stock fine-tuning checkpoints are laid out)."""
    from safetensors.numpy import save_file
    from oracle import vit_oracle as vo
    path.mkdir()
    ocfg = (vo.cfg_ast if kind == "ast" else vo.cfg_vit)(**REDUCED)
    W = tf_weights(seed, vo.param_shapes(ocfg), std=0.08)
    save_file({k: np.ascontiguousarray(v) for k, v in W.items()}, str(path / "model.safetensors"))
    common = {"hidden_size": 64, "num_hidden_layers": 2, "num_attention_heads": 4, "intermediate_size": 128,
              "patch_size": 16, "layer_norm_eps": 1e-12, "hidden_act": "gelu",
              "id2label": {str(i): f"LABEL_{i}" for i in range(5)}}
    if kind == "ast":
        cfg = dict(common, model_type="audio-spectrogram-transformer", num_mel_bins=128, max_length=1024,
                   frequency_stride=10, time_stride=10)
    else:
        cfg = dict(common, model_type="vit", image_size=224, num_channels=3)
        json.dump({"do_normalize": True, "do_rescale": True, "do_resize": True, "image_mean": [0.5, 0.5, 0.5],
                   "image_std": [0.5, 0.5, 0.5], "image_processor_type": "ViTImageProcessor", "resample": 2,
                   "rescale_factor": 1 / 255, "size": {"height": 224, "width": 224}},
                  open(path / "preprocessor_config.json", "w"))
    json.dump(cfg, open(path / "config.json", "w"))
    return str(path), W


def _trained(kind, precision, frozen_epochs, cache, base, monkeypatch):
    """The trainer after `frozen_epochs` frozen epochs and one unfrozen epoch on 6 train / 4 test items in batches of 4
    (ragged last batches), with everything the comparisons need; one run per configuration and module."""
    key = (kind, precision, frozen_epochs, cache)
    if key in _RUNS:
        return _RUNS[key]
    from eav_amd.audio import AudioModelTrainer
    from eav_amd.vision import ImageClassifierTrainer
    problem_type, NC = TRAINERS[kind]
    path, W = _save_model_dir(base / f"{kind}-{precision}-{frozen_epochs}-{int(cache)}", kind, 9)
    monkeypatch.chdir(base)
    y = _labels(problem_type, 81, 10, NC)
    head_w, head_b = synth.normal(82, (NC, 64), 0.0, 0.05), synth.normal(83, (NC,), 0.0, 0.02)
    buf = io.StringIO()
    with redirect_stdout(buf):
        if kind == "ast":
            x = torch.from_numpy(synth.mel_batch(84, 10, 1024, 128)[0])
            tr = AudioModelTrainer([x[:6], y[:6], x[6:], y[6:]], path, sub="s", num_classes=NC, batch_size=4,
                                   problem_type=problem_type)
        else:
            x = (synth.uniform(85, (10, 3, 56, 56, 3)) * 255).astype(np.uint8)     # three frames per item
            tr = ImageClassifierTrainer([x[:6], y[:6], x[6:], y[6:]], path, sub="s", num_labels=NC, batch_size=4,
                                        problem_type=problem_type)
        tr.model.precision = precision
        tr.cache_frozen_features = cache
        tr.model.reset_head(head_w, head_b)
        tr.optimizer = type(tr.optimizer)(tr.model.parameters(), lr=tr.initial_lr, weight_decay=0.01, decoupled=True)
        n = len(tr.train_dataloader.dataset)
        per = n // 6                                            # vision: three frames per item, 18 = 4 x 4 + 2
        assert torch.equal(tr.train_dataloader.y.cpu(), torch.from_numpy(np.repeat(y[:6], per, axis=0)))   # a row per frame
        assert n % 4 != 0                                       # a ragged last batch
        orders = [[per * i + f for i in o for f in range(per)] for o in ORDERS[:frozen_epochs + 1]]
        tr.train_dataloader.order_override = [list(o) for o in orders]
        tr.train(epochs=frozen_epochs, lr=5e-4, freeze=True)
        assert not hasattr(tr, "outputs_test")
        tr.train(epochs=1, lr=5e-6, freeze=False)
    key_w = "classifier.dense" if kind == "ast" else "classifier"
    W0 = dict(W)
    W0[key_w + ".weight"], W0[key_w + ".bias"] = head_w, head_b
    _RUNS[key] = dict(tr=tr, W0=W0, orders=orders, stdout=buf.getvalue(), path=path, NC=NC, problem_type=problem_type)
    return _RUNS[key]


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    yield tmp_path_factory.mktemp("problem_type")
    _RUNS.clear()


@pytest.mark.parametrize("precision", ["fp32", "split"])
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_trainers_with_float_labels_match_the_reference_stepper(kind, precision, base, monkeypatch):
    from oracle import vit_oracle as vo
    r = _trained(kind, precision, 1, True, base, monkeypatch)
    tr, NC = r["tr"], r["NC"]
    assert tr.model.cfg.problem_type == r["problem_type"] and tr.train_dataloader.y.dtype == torch.float32
    assert tuple(tr.train_dataloader.y.shape) == (len(tr.train_dataloader.dataset), NC)
    ocfg = (vo.cfg_ast if kind == "ast" else vo.cfg_vit)(num_labels=NC, **REDUCED)
    dl, te = tr.train_dataloader, tr.test_dataloader
    ref, _ = ptr.train_reference(r["W0"], ocfg, r["problem_type"], dl.x.cpu(), dl.y.cpu(), te.x.cpu(),
                                 [(5e-4, True, r["orders"][:1]), (5e-6, False, r["orders"][1:])], 4)
    assert tr.outputs_test.shape == ref.shape == (len(te.dataset), NC) and tr.outputs_test.dtype == np.float32
    err = float(np.abs(tr.outputs_test - ref).max())
    print(f"{kind} {precision}: max |outputs_test - reference stepper| = {err:.3e} (max |reference| {np.abs(ref).max():.3e})")
    assert err < 1e-3, err
    # the epoch lines of the new modes (finetune.FineTuneBase's docstring), their value from the device-side counts
    lines = [l for l in r["stdout"].splitlines() if l.startswith("Epoch")]
    assert len(lines) == 2
    ty = te.y.cpu().numpy()
    if kind == "ast":
        acc = float(((tr.outputs_test > 0) == (ty > 0.5)).mean())
        assert lines[1].startswith("Epoch 1/1, Training Label Accuracy: ") and lines[1].endswith(f"Test Label Accuracy: {acc * 100:.2f}%")
        assert open(base / "training_performance_audio.txt").read().count("Test Label Accuracy") >= 2
    else:
        mse = float(((tr.outputs_test.astype(np.float64) - ty) ** 2).mean())
        assert lines[1].startswith("Epoch 1, Test MSE: ")
        assert abs(float(lines[1].split("MSE: ")[1]) - mse) <= 1e-5 * mse + 1e-6


@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_feature_cache_changes_nothing_with_float_labels(kind, base, monkeypatch):
    """Two frozen epochs (the second runs on the cached features) and one unfrozen epoch, cache on and off, exact-fp32
    arithmetic: outputs_test and the head are bit-equal."""
    a = _trained(kind, "fp32", 2, True, base, monkeypatch)["tr"]
    b = _trained(kind, "fp32", 2, False, base, monkeypatch)["tr"]
    assert np.array_equal(a.outputs_test, b.outputs_test)
    ha, hb = a.model.classifier.state_dict(), b.model.classifier.state_dict()
    assert all(torch.equal(ha[k], hb[k]) for k in ha)


@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_save_pretrained_after_training(kind, base, monkeypatch, tmp_path):
    """trainer.save_pretrained after the unfrozen epoch: the directory reloads into a model with the same logits bit for
    bit, config.json carries the problem type, the vision directory its preprocessor_config.json, and the oracle agrees on
    the saved weights.  (No Hugging Face import here: the CPU tests load such directories into its classes.)"""
    import os
    from eav_amd import transformer as T
    from oracle import vit_oracle as vo
    from safetensors.numpy import load_file
    r = _trained(kind, "split", 1, True, base, monkeypatch)
    tr, NC = r["tr"], r["NC"]
    d = str(tmp_path / "saved")
    tr.save_pretrained(d)
    cj = json.load(open(os.path.join(d, "config.json")))
    assert cj["problem_type"] == r["problem_type"] and len(cj["id2label"]) == NC
    assert os.path.exists(os.path.join(d, "preprocessor_config.json")) == (kind == "vit")
    if kind == "vit":
        assert json.load(open(os.path.join(d, "preprocessor_config.json"))) == \
            json.load(open(os.path.join(r["path"], "preprocessor_config.json")))
    x = tr.test_dataloader.x[:3]
    tr.model.eval()
    with torch.no_grad():
        live = tr.model(x).logits
    back = T.Encoder.from_pretrained(d).to(tr.device).eval()
    back.precision = tr.model.precision
    assert back.cfg.problem_type == r["problem_type"] and back.cfg.num_labels == NC
    with torch.no_grad():
        again = back(x).logits
    assert torch.equal(_bits(again), _bits(live))
    saved = load_file(os.path.join(d, "model.safetensors"))
    moved = max(float(np.abs(saved[k] - r["W0"][k]).max()) for k in saved)
    assert moved > 0                                            # the trained weights, not the ones that were loaded
    ocfg = (vo.cfg_ast if kind == "ast" else vo.cfg_vit)(num_labels=NC, **REDUCED)
    with torch.no_grad():
        ref = vo.forward({k: torch.from_numpy(v) for k, v in saved.items()}, x.cpu(), ocfg)
    _close(live, ref, 1e-4, 1e-4, f"{kind}: logits of the saved weights")
