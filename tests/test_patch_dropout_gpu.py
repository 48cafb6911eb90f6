"""Patch dropout of the AST / ViT encoders on the MI355X: the identity table against a plain forward, Hugging Face goldens
(tests/golden/patch_dropout*.npz) under explicit keep tables, generated plans against the numpy restatement
(tests/patch_keep_ref.py) eagerly and in a captured step, off-means-off by launch lists, the extra outputs, the refusals
and the trainer."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import patch_keep_ref as R
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "split"]
KEEP_LAUNCHES = ("eav_patch_keep_plan", "eav_patch_keep_invert", "eav_im2col_keep", "eav_embed_finish_keep",
                 "eav_embed_bwd_keep")


def close(got, ref, rtol, atol, what):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}"


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32)


def _weights(name):
    from oracle import vit_oracle as vo
    c = R.MODEL_CASES[name]
    ocfg = vo.cfg_ast(**c["kw"], frames=c["native"]) if c["kind"] == "ast" else vo.cfg_vit(**c["kw"], image=c["native"])
    return tf_weights(R.MODEL_WSEED, vo.param_shapes(ocfg), std=R.MODEL_STD)


def _model(name, precision, W=None, **kw):
    from eav_amd import transformer as T
    c = R.MODEL_CASES[name]
    size = dict(frames=c["native"]) if c["kind"] == "ast" else dict(image=c["native"])
    model = T.Encoder(T.make_config(c["kind"], **c["kw"], **size, **kw), _weights(name) if W is None else W).cuda().train()
    model.precision = precision
    model.variable_length = c["kind"] == "ast" and c["size"] != c["native"]
    return model


def _data(name):
    x, y = R.model_batch(name)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def _step(model, x, y, **kw):
    from eav_amd.optim import CrossEntropyLoss
    for p in model.parameters():
        p.grad = None
    out = model(x, **kw)
    loss = CrossEntropyLoss()(out.logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return out.logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def _log_calls(monkeypatch):
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


def _table(keep):
    return torch.from_numpy(np.ascontiguousarray(keep, np.int32)).cuda()


# ============================================================================================ identity
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["vit64", "ast96"])
def test_the_identity_table_is_a_plain_forward(name, precision):
    """keep = arange(P) under a rate just above 0 (K = P) takes the _keep launches and gives the plain forward's bits."""
    c = R.MODEL_CASES[name]
    x, y = _data(name)
    plain = _step(_model(name, precision), x, y)
    model = _model(name, precision)
    model.patch_dropout = 1e-17
    model.set_patch_keep(_table(np.tile(np.arange(c["P"]), (R.MODEL_B, 1))))
    got = _step(model, x, y)
    assert getattr(model._active_geo, "grid_npatch", None) == c["P"] == model._active_geo.npatch
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    for k in plain[2]:
        assert np.array_equal(bits(got[2][k]), bits(plain[2][k])), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_identity_table_on_a_resampled_grid(precision):
    """The third geometry: a ViT with interpolate_pos_encoding on 32 x 48 frames (2 x 3 patches, the 4 x 4 table resampled).
    The identity table gives the plain forward's bits; a generated plan at p = 0.5 keeps 3 of 6 and its table gradient has
    the stored shape."""
    x = torch.from_numpy(synth.uniform(321, (R.MODEL_B, 3, 32, 48), -1.0, 1.0)).cuda()
    y = torch.from_numpy(synth.labels(322, R.MODEL_B)).cuda()
    models = [_model("vit64", precision) for _ in range(2)]
    for m in models:
        m.interpolate_pos_encoding = True
    plain = _step(models[0], x, y)
    model = models[1]
    model.patch_dropout = 1e-17
    model.set_patch_keep(_table(np.tile(np.arange(6), (R.MODEL_B, 1))))
    got = _step(model, x, y)
    assert (model._active_geo.grid_npatch, model._active_geo.npatch, model._active_geo.pos_grid) == (6, 6, 4)
    assert torch.equal(got[0], plain[0])
    for k in plain[2]:
        assert np.array_equal(bits(got[2][k]), bits(plain[2][k])), k
    model.set_patch_keep(None)
    model.patch_dropout = 0.5
    model.dropout_seed = 5
    logits, _, grads = _step(model, x, y)
    keep = model.last_patch_keep().cpu().numpy()
    assert np.array_equal(keep, R.plan(R.MODEL_B, 6, 3, R.plan_seed(5), 1)[0]) and model._active_geo.ntok == 4
    gpos = grads["vit.embeddings.position_embeddings"]
    assert tuple(gpos.shape) == (1, 17, 64) and torch.isfinite(gpos).all() and torch.isfinite(logits).all()


# ============================================================================================ Hugging Face
def _unkept_rows(name, keep):
    """Rows of the STORED position table no sample's kept patch reads (ast96: the fit is a centre cut of the time axis)."""
    c = R.MODEL_CASES[name]
    nextra = 2 if c["kind"] == "ast" else 1
    used = np.zeros(c["P"], bool)
    used[np.unique(keep)] = True
    if name == "ast96":
        from tests.ast_length_ref import cut_window
        a, b = cut_window(25, 9)
        stored = np.zeros((12, 25), bool)
        stored[:, a:b] = used.reshape(12, 9)
        used = stored.reshape(-1)
    return nextra + np.flatnonzero(~used)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_kept_subsets_match_hf(golden_dir, name, precision):
    """HF's embeddings, the kept rows gathered, HF's encoder / LayerNorm / head.  Bounds of
    test_ast_length_gpu.test_other_lengths_match_hf: logits and loss 1e-4 relative + 1e-4 absolute, gradients 1e-3 relative +
    1e-3 of the reference's maximum."""
    c = R.MODEL_CASES[name]
    g = np.load(os.path.join(golden_dir, c["file"]))
    keep = g[f"{name}.keep"]
    assert np.array_equal(keep, R.model_keep(name)) and keep.shape == (R.MODEL_B, c["K"])
    model = _model(name, precision)
    assert model._fused_attention() == (name == "ast256w")
    model.patch_dropout = c["p"]
    model.set_patch_keep(_table(keep))
    logits, loss, grads = _step(model, *_data(name))
    assert torch.equal(model.last_patch_keep().cpu(), torch.from_numpy(keep))
    close(logits, g[f"{name}.logits"], 1e-4, 1e-4, "logits")
    close(loss, g[f"{name}.loss"], 1e-4, 1e-4, "loss")
    pre = f"{name}.grad."
    gkeys = sorted(k[len(pre):] for k in g.files if k.startswith(pre))
    assert gkeys == (sorted(grads) if c["grads"] == "all" else sorted(k for k in grads if ".embeddings." in k))
    for k in gkeys:
        ref = g[pre + k]
        assert tuple(grads[k].shape) == tuple(ref.shape), k
        close(grads[k], ref, 1e-3, max(1e-3 * np.abs(ref).max(), 1e-6), f"grad.{k}")
    key = f"{model.cfg.prefix}.embeddings.position_embeddings"
    assert tuple(grads[key].shape) == tuple(model.state_dict()[key].shape) == (1, model.cfg.ntok, c["kw"]["hidden"])
    rows = _unkept_rows(name, keep)
    gpos = bits(grads[key][0])
    assert len(rows) and not gpos[rows].any()
    kept_rows = np.setdiff1d(np.arange(model.cfg.ntok), rows)
    assert all(gpos[r].any() for r in kept_rows)
    # cfg is the checkpoint's: the geometry belonged to the forward
    assert model.cfg.npatch == (300 if c["kind"] == "ast" else 16) and not hasattr(model.cfg, "grid_npatch")


# ============================================================================================ generated plans
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["vit64", "ast256w"])
def test_generated_plans_are_the_restatements(name, precision):
    c = R.MODEL_CASES[name]
    model = _model(name, precision)
    model.patch_dropout = c["p"]
    model.dropout_seed = 987654321
    x, y = _data(name)
    seen = []
    for step in (1, 2):
        _step(model, x, y)
        assert model.forward_counter() == step
        last = model.last_patch_keep().cpu().numpy()
        want = R.plan(R.MODEL_B, c["P"], c["K"], R.plan_seed(987654321), step)[0]
        assert np.array_equal(last, want)
        assert np.array_equal(model.generated_patch_keep(R.MODEL_B, step).cpu().numpy(), want)
        seen.append(last)
    assert not np.array_equal(seen[0], seen[1])
    model.mix_dropout_rank(3)                                   # another replica, another subset
    other = model.generated_patch_keep(R.MODEL_B, 1).cpu().numpy()
    assert not np.array_equal(other, seen[0])
    assert np.array_equal(other, R.plan(R.MODEL_B, c["P"], c["K"], R.plan_seed(model.dropout_seed), 1)[0])
    model.eval()                                                # evaluation sees every token and draws nothing
    with torch.no_grad():
        model(x)
    assert model.forward_counter() == 2 and model._active_geo is None


# ============================================================================================ captured step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_step_draws_a_fresh_subset_per_replay(precision):
    """GraphStep over a head_dim-64 AST at 96 frames of a 256-frame checkpoint under patch_dropout 0.5 (54 of 108 patches):
    two eager steps, the capture, three replays.  Every step's table is the restatement's at its counter, the replays'
    differ, and the losses are those of a twin stepped eagerly under the same tables, bit for bit."""
    import copy
    from eav_amd import transformer as T
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    from eav_amd.runtime import GraphStep, eager_step, gather_batch
    from tests.ast_length_ref import clips
    torch.manual_seed(11)
    model = T.Encoder(T.make_config("ast", hidden=128, heads=2, ff=256, layers=2, frames=256))
    model.precision, model.overlap_wgrad, model.variable_length = precision, False, True
    with torch.no_grad():
        model.audio_spectrogram_transformer.embeddings.position_embeddings.normal_(0.0, 0.02)
    twin = copy.deepcopy(model)
    model, twin = model.cuda().train(), twin.cuda().train()
    model.patch_dropout = twin.patch_dropout = 0.5
    model.dropout_seed = 2468
    x, y = clips(281, 6, 96)
    xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    crit = CrossEntropyLoss()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=0.01, decoupled=True, capturable=True)
    topt = FusedAdam(twin.parameters(), lr=1e-3, weight_decay=0.01, decoupled=True, capturable=True)
    gs = GraphStep(model, opt, crit, xs, ys, 2)
    steps = [[0, 1], [2, 3], [4, 5], [1, 4], [5, 0]]
    got, tables = [], []
    for s, idx in enumerate(steps, start=1):
        got.append(gs.run(idx)[1].clone())
        assert model.forward_counter() == s
        tables.append(model.last_patch_keep())
        assert np.array_equal(tables[-1].cpu().numpy(), R.plan(2, 108, 54, R.plan_seed(2468), s)[0]), s
    assert gs.graph is not None
    replays = [t.cpu().numpy() for t in tables[2:]]
    assert len(replays) == 3 and all(not np.array_equal(a, b) for i, a in enumerate(replays) for b in replays[i + 1:])
    for s, idx in enumerate(steps):
        twin.set_patch_keep(tables[s])
        data, targets = gather_batch(xs, ys, torch.as_tensor(idx, dtype=torch.long, device=xs.device))
        want = eager_step(lambda d: twin(d).logits, topt, crit, data, targets)[1]
        torch.cuda.synchronize()
        assert torch.equal(got[s], want), (s, float(got[s]), float(want))
    assert torch.equal(model._flat[0], twin._flat[0])


# ============================================================================================ off means off
@pytest.mark.parametrize("precision", PRECISIONS)
def test_off_means_off(precision, monkeypatch):
    """patch_dropout = 0 in training mode, 0.5 in eval mode and a model that never set the attribute launch the same list
    and give the same logits, bit for bit."""
    name = "ast96"
    x, y = _data(name)
    runs = []
    for setup in ("zero", "eval", "untouched"):
        model = _model(name, precision)
        if setup == "zero":
            model.patch_dropout = 0.0
        elif setup == "eval":
            model.patch_dropout = 0.5
            model.eval()
        names = _log_calls(monkeypatch)
        logits = _step(model, x, y)[0]
        monkeypatch.undo()
        runs.append((list(names), logits))
    assert runs[0][0] and not set(runs[0][0]) & set(KEEP_LAUNCHES)
    assert runs[0][0] == runs[1][0] == runs[2][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])
    # ... and on: the three embedding launches are their _keep forms, one counter step and one plan per forward
    model = _model(name, precision)
    model.patch_dropout = 0.5
    names = _log_calls(monkeypatch)
    _step(model, x, y)
    monkeypatch.undo()
    for launch in ("eav_patch_keep_plan", "eav_im2col_keep", "eav_embed_finish_keep", "eav_embed_bwd_keep"):
        assert names.count(launch) == 1, launch
    assert not {"eav_im2col", "eav_embed_finish", "eav_embed_bwd", "eav_patch_keep_invert"} & set(names)
    assert names.count("eav_counter_inc") == 1
    assert len(names) == len(runs[0][0]) + 2


# ============================================================================================ extra outputs
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["vit64", "ast256w"])
def test_extra_outputs_have_the_forwards_token_count(name, precision):
    """p = 0.5: 8 of the ViT's 16 patches (9 tokens, the GEMM + softmax attention), 150 of the AST's 300 (152 tokens, the fused
    kernels and csrc/attn_probs.hip)."""
    c = R.MODEL_CASES[name]
    K = R.keep_count(c["P"], 0.5)
    model = _model(name, precision)
    model.patch_dropout = 0.5
    model.set_patch_keep(_table(R.plan(R.MODEL_B, c["P"], K, R.plan_seed(3), 1)[0]))
    x, y = _data(name)
    plain = _step(model, x, y)
    out = model(x, output_hidden_states=True, output_attentions=True)
    torch.cuda.synchronize()
    N, D, H = model.cfg.nextra + K, c["kw"]["hidden"], c["kw"]["heads"]
    assert len(out.hidden_states) == 3 and all(tuple(h.shape) == (R.MODEL_B, N, D) for h in out.hidden_states)
    assert len(out.attentions) == 2 and all(tuple(a.shape) == (R.MODEL_B, H, N, N) for a in out.attentions)
    for a in out.attentions:
        close(a.sum(-1), np.ones((R.MODEL_B, H, N)), 0.0, 1e-5, "attention rows")
    assert torch.equal(out.logits, plain[0])
    flagged = _step(model, x, y, output_hidden_states=True, output_attentions=True)
    for k in plain[2]:
        assert torch.equal(flagged[2][k], plain[2][k]), k


# ============================================================================================ refusals
def test_refusals_on_the_device():
    name = "vit64"
    c = R.MODEL_CASES[name]
    model = _model(name, "split")
    x, y = _data(name)
    for bad in (1.0, -0.1, 1.5):
        model.patch_dropout = bad
        with pytest.raises(ValueError, match="patch_dropout"):
            model(x)
    model.patch_dropout = c["p"]
    keep = R.model_keep(name)
    unsorted, repeated, outside = keep.copy(), keep.copy(), keep.copy()
    unsorted[1, [0, 1]] = unsorted[1, [1, 0]]
    repeated[2, 1] = repeated[2, 0]
    outside[0, -1] = c["P"]
    for bad in (unsorted, repeated, outside, keep[:, :-1], keep[:-1]):          # (the last two: another K, another B)
        with pytest.raises(ValueError):
            model.set_patch_keep(_table(bad))
            model(x)
        model.set_patch_keep(None)
    model.set_patch_keep(_table(keep))
    assert model(x).logits.shape == (R.MODEL_B, 5)
    model.set_patch_keep(None)                                  # back to generated plans
    model(x)
    assert model.forward_counter() == 1
    dropping = _model(name, "split", hidden_dropout=0.1)
    dropping.patch_dropout = 0.5
    with pytest.raises(NotImplementedError, match="dropout"):
        dropping(x)
    dropping.eval()                                             # nothing drops in eval mode
    with torch.no_grad():
        assert dropping(x).logits.shape == (R.MODEL_B, 5)


# ============================================================================================ trainer
def _save_model_dir(path):
    """HF-format directory of the reduced AST, 256 frames (config.json, model.safetensors, preprocessor_config.json)."""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    save_file({k: np.ascontiguousarray(v) for k, v in _weights("ast256").items()}, os.path.join(path, "model.safetensors"))
    json.dump({"model_type": "audio-spectrogram-transformer", "hidden_size": 64, "num_hidden_layers": 2,
               "num_attention_heads": 4, "intermediate_size": 128, "patch_size": 16, "layer_norm_eps": 1e-12,
               "hidden_act": "gelu", "num_mel_bins": 128, "max_length": 256, "frequency_stride": 10, "time_stride": 10,
               "id2label": {str(i): f"LABEL_{i}" for i in range(5)}}, open(os.path.join(path, "config.json"), "w"))
    json.dump({"feature_extractor_type": "ASTFeatureExtractor", "max_length": 256, "num_mel_bins": 128,
               "sampling_rate": 16000, "do_normalize": True, "mean": -4.2677393, "std": 4.5689974},
              open(os.path.join(path, "preprocessor_config.json"), "w"))
    return str(path)


def test_trainer_drops_patches_in_unfrozen_epochs_only(tmp_path, monkeypatch):
    from eav_amd.audio import AudioModelTrainer
    path = _save_model_dir(tmp_path / "model")
    monkeypatch.chdir(tmp_path)
    wav = synth.normal(295, (12, 8000), 0.0, 0.1)                   # 0.5 s: 56 frames, 12 x 5 = 60 patches, 30 kept
    y = synth.labels(296, 12)
    data = [wav[:8], y[:8], wav[8:], y[8:]]
    frozen = []
    with redirect_stdout(io.StringIO()):
        for p in (0.5, None):
            torch.manual_seed(0)
            tr = AudioModelTrainer(data, path, sub="s", num_classes=5, batch_size=4, max_length="auto")
            if p is not None:
                tr.patch_dropout = p
            names = _log_calls(monkeypatch)
            tr.train(epochs=1, lr=5e-4, freeze=True)
            monkeypatch.undo()
            monkeypatch.chdir(tmp_path)
            frozen.append(list(names))
            if p is not None:
                kept = tr
    assert frozen[0] and frozen[0] == frozen[1] and not set(frozen[0]) & set(KEEP_LAUNCHES)
    tr = kept
    with redirect_stdout(io.StringIO()):
        names = _log_calls(monkeypatch)
        tr.train(epochs=1, lr=5e-6, freeze=False)
        monkeypatch.undo()
        monkeypatch.chdir(tmp_path)
        unfrozen = list(names)
        names = _log_calls(monkeypatch)
        rows = tr._evaluate()
        monkeypatch.undo()
        monkeypatch.chdir(tmp_path)
        evaluate = list(names)
    # two training batches drop (plan, im2col, finish, backward each), the test batch of the epoch runs the plain launches
    for launch in ("eav_patch_keep_plan", "eav_im2col_keep", "eav_embed_finish_keep", "eav_embed_bwd_keep"):
        assert unfrozen.count(launch) == 2, launch
    assert unfrozen.count("eav_im2col") == 1 and unfrozen.count("eav_embed_bwd") == 0
    assert tr.model.forward_counter() == 2 and tr.model.patch_dropout == 0.5
    assert evaluate and "eav_im2col" in evaluate and not set(evaluate) & set(KEEP_LAUNCHES)
    assert len(rows) == 1
    assert tr.outputs_test.shape == (4, 5) and np.isfinite(tr.outputs_test).all()
