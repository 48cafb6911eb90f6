"""AST clips at their own length on the MI355X: the two fitting kernels against the float64 restatement
(tests/ast_length_ref.py), the encoder at 96 and 336 frames of a 256-frame checkpoint against Hugging Face
(tests/golden/ast_length.npz) and against the CPU oracle, the native length with the flag on, alternating lengths, the
refusals, a captured step, and the trainer."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import ast_length_ref as R
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "split"]
REDUCED = dict(hidden=64, layers=2, heads=4, ff=128)
NATIVE = 256                                     # frames of the reduced checkpoint: a stored grid of 12 x 25
KEY = "audio_spectrogram_transformer.embeddings.position_embeddings"


def close(got, ref, rtol, atol, what):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}"


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32)


# ============================================================================================ kernels
@pytest.mark.parametrize("D", [64, 772])
@pytest.mark.parametrize("ny,nx0,nx", R.GRIDS)
def test_kernels_against_float64(ny, nx0, nx, D):
    """Element-wise within ast_length_ref.error_bounds (0 for a cut); D = 772 is 193 float4 lanes - no multiple of the block."""
    from eav_amd import pos_time as pt
    pos = synth.normal(3000 + D + nx, (2 + ny * nx0, D))
    dout = synth.normal(4000 + D + nx, (2 + ny * nx, D))
    pos[2 + nx0 // 2, 3] = dout[2 + nx // 2, 7] = -0.0              # (the centre column lies inside every cut's window)
    pos_d, dout_d = torch.from_numpy(pos).cuda(), torch.from_numpy(dout).cuda()
    out = torch.full((2 + ny * nx, D), float("nan"), device="cuda")
    pt.pos_time_fwd(pos_d, out, ny, nx0, nx, 2)
    dpos = [torch.full((2 + ny * nx0, D), float("nan"), device="cuda") for _ in range(2)]
    for d in dpos:
        pt.pos_time_bwd(dout_d, d, ny, nx0, nx, 2)
    torch.cuda.synchronize()
    what = f"{ny}x{nx0}->{nx} D={D}"
    got = out.cpu().double().numpy()
    err = np.abs(got - R.fit(pos, ny, nx0, nx))
    assert np.isfinite(got).all() and (err <= R.error_bounds(pos, ny, nx0, nx)).all(), (what, err.max())
    assert np.array_equal(bits(out[:2]), bits(pos[:2]))
    gotb = dpos[0].cpu().double().numpy()
    assert np.isfinite(gotb).all(), what + ": an element of dpos was not written"
    errb = np.abs(gotb - R.fit_adjoint(dout, ny, nx0, nx))
    assert (errb <= R.error_bounds(dout, ny, nx0, nx, adjoint=True)).all(), (what, errb.max())
    assert np.array_equal(bits(dpos[0][:2]), bits(dout[:2]))
    assert torch.equal(dpos[0], dpos[1]), what + ": the backward is not deterministic"
    if nx < nx0:            # a cut: the window's rows bit for bit (-0 included) in both directions, exact zeros outside it
        a, b = R.cut_window(nx0, nx)
        grid = bits(pos[2:]).reshape(ny, nx0, D)
        assert np.array_equal(bits(out[2:]).reshape(ny, nx, D), grid[:, a:b])
        back = bits(dpos[0][2:]).reshape(ny, nx0, D)
        assert np.array_equal(back[:, a:b], bits(dout[2:]).reshape(ny, nx, D))
        assert not back[:, :a].any() and not back[:, b:].any()


# ============================================================================================ model
def _weights(seed, std=0.08, **kw):
    from oracle import vit_oracle as vo
    return tf_weights(seed, vo.param_shapes(vo.cfg_ast(**{**REDUCED, **kw}, frames=NATIVE)), std=std)


def _model(W, precision, **kw):
    from eav_amd import transformer as T
    model = T.Encoder(T.make_config("ast", **{**REDUCED, **kw}, frames=NATIVE), W).cuda().train()
    model.precision = precision
    model.variable_length = True
    return model


def _step(model, x, y):
    from eav_amd.optim import CrossEntropyLoss
    for p in model.parameters():
        p.grad = None
    out = model(x)
    loss = CrossEntropyLoss()(out.logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return out.logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_other_lengths_match_hf(golden_dir, precision):
    """HF's ASTForAudioClassification at max_length 96 / 336 with the fitted table: bounds of test_vit_interp_gpu's
    test_other_sizes_match_hf."""
    g = np.load(os.path.join(golden_dir, "ast_length.npz"))
    assert int(g["native"]) == NATIVE
    model = _model(_weights(int(g["wseed"]), float(g["std"])), precision)
    x, y = R.clips(int(g["xseed"]) + 96, int(g["B"]), 96)
    logits, loss, grads = _step(model, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    close(logits, g["logits96"], 1e-4, 1e-4, "logits 96")
    close(loss, g["loss96"], 1e-4, 1e-4, "loss 96")
    gkeys = sorted(k[len("grad96."):] for k in g.files if k.startswith("grad96."))
    assert sorted(grads) == gkeys
    for k in gkeys:
        ref = g[f"grad96.{k}"]
        assert tuple(grads[k].shape) == tuple(ref.shape), k               # the table's: the stored 302 rows
        close(grads[k], ref, 1e-3, max(1e-3 * np.abs(ref).max(), 1e-6), f"grad96.{k}")
    a, b = R.cut_window(25, 9)
    gpos = bits(grads[KEY][0, 2:]).reshape(12, 25, 64)
    assert not gpos[:, :a].any() and not gpos[:, b:].any() and gpos[:, a:b].any()
    x, y = R.clips(int(g["xseed"]) + 336, int(g["B"]), 336)
    with torch.no_grad():
        out = model(input_values=torch.from_numpy(x).cuda(), labels=torch.from_numpy(y).cuda())
    close(out.logits, g["logits336"], 1e-4, 1e-4, "logits 336")
    close(out.loss, g["loss336"], 1e-4, 1e-4, "loss 336")
    # cfg, the parameters' shapes and the state dict are those of the checkpoint: the geometry belonged to the forward
    assert (model.cfg.W, model.cfg.nx, model.cfg.ntok) == (NATIVE, 25, 302)
    assert tuple(model.state_dict()[KEY].shape) == (1, 302, 64)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_attention_path_at_another_length(precision):
    """head_dim 64 takes the fused attention kernels (the reduced model's head_dim 16 the GEMM + softmax path), here at 110
    tokens, against the CPU oracle fed the fitted table.  Bounds: those of test_vit_interp_gpu's twin."""
    from oracle import vit_oracle as vo
    kw = dict(hidden=128, layers=2, heads=2, ff=256)
    ocfg = vo.cfg_ast(**kw, frames=NATIVE)
    W = tf_weights(24, vo.param_shapes(ocfg), std=0.08)
    x, y = R.clips(241, 3, 96)
    P = {k: torch.from_numpy(v.copy()) for k, v in W.items()}
    P[KEY] = torch.from_numpy(R.fit(W[KEY][0], 12, 25, 9).astype(np.float32))[None]
    logits, lref, grads = vo.Stepper(P, ocfg, lr=1e-3).step(torch.from_numpy(x), torch.from_numpy(y), False)
    grads = {k: v.numpy() for k, v in grads.items()}
    grads[KEY] = R.fit_adjoint(grads[KEY][0], 12, 25, 9)[None]
    model = _model(W, precision, **kw)
    assert model._fused_attention()
    got, loss, ggot = _step(model, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    close(got, logits.numpy(), 1e-4, 1e-4, "logits")
    close(loss, lref.numpy(), 1e-4, 1e-4, "loss")
    for k in ggot:
        close(ggot[k], grads[k], 2e-3, max(2e-3 * np.abs(grads[k]).max(), 1e-7), f"grad.{k}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_native_length_with_the_flag_on_is_bit_equal(precision):
    """At the checkpoint's length the stored table is used - the same launches, the same bits."""
    W = _weights(25)
    x, y = R.clips(250, 2, NATIVE)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = []
    for flag in (False, True):
        model = _model(W, precision)
        model.variable_length = flag
        res.append(_step(model, xd, yd))
        assert model._active_geo is None
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lengths_alternate_on_one_model(precision):
    """The geometry travels with the forward's token: forwards of 96, 256 and 336 frames interleaved with their backwards
    give the gradients of separate runs, bit for bit."""
    W = _weights(27)
    data = {t: tuple(torch.from_numpy(a).cuda() for a in R.clips(270 + t, 2, t)) for t in (96, NATIVE, 336)}
    one = _model(W, precision)
    for t in (96, NATIVE, 336, 96):
        got, fresh = _step(one, *data[t]), _step(_model(W, precision), *data[t])
        assert torch.equal(got[0], fresh[0]), t
        for k in got[2]:
            assert torch.equal(got[2][k], fresh[2][k]), (t, k)


def test_refusals_on_the_device():
    from eav_amd import transformer as T
    W = _weights(26)
    model = _model(W, "split")
    x = torch.from_numpy(R.clips(260, 2, 96)[0]).cuda()
    model.variable_length = False
    with pytest.raises(ValueError, match="expected input"):
        model(x)                                                    # flag off: the same error as ever
    model.variable_length = True
    with pytest.raises(ValueError):
        model(x[:, :, :64])                                         # mel bins are the checkpoint's, flag on ...
    model.variable_length = False
    with pytest.raises(ValueError):
        model(torch.zeros(2, NATIVE, 64, device="cuda"))            # ... or off
    model.variable_length = True
    with pytest.raises(ValueError):
        model(x[:, :8])                                             # shorter than a patch
    with pytest.raises(NotImplementedError):
        model(x, interpolate_pos_encoding=True)                     # that argument stays ViT's
    vit = T.Encoder(T.make_config("vit", hidden=64, layers=1, heads=4, ff=128, image=32)).cuda()
    vit.variable_length = True
    with pytest.raises(NotImplementedError):
        vit(torch.zeros(1, 3, 32, 32, device="cuda"))
    dropping = _model(W, "split", hidden_dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        dropping(x)
    dropping.eval()                                                 # nothing drops in eval mode
    with torch.no_grad():
        assert dropping(x).logits.shape == (2, 5)


# ============================================================================================ captured step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_step_at_another_length(precision):
    """GraphStep over an Encoder whose attribute is on and whose data set is 96 frames long: eager, captured and replayed
    steps (3 replays) equal a twin stepped eagerly, bit for bit (the tables are on the device before the capture)."""
    import copy
    from eav_amd import transformer as T
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    from eav_amd.runtime import GraphStep, eager_step, gather_batch
    torch.manual_seed(11)
    model = T.Encoder(T.make_config("ast", hidden=128, heads=2, ff=256, layers=2, frames=NATIVE))
    model.precision, model.overlap_wgrad, model.variable_length = precision, False, True
    with torch.no_grad():
        model.audio_spectrogram_transformer.embeddings.position_embeddings.normal_(0.0, 0.02)
    pos_init = model.audio_spectrogram_transformer.embeddings.position_embeddings.detach().clone()
    twin = copy.deepcopy(model)
    model, twin = model.cuda().train(), twin.cuda().train()
    x, y = R.clips(280, 6, 96)
    xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    crit = CrossEntropyLoss()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=0.01, decoupled=True, capturable=True)
    topt = FusedAdam(twin.parameters(), lr=1e-3, weight_decay=0.01, decoupled=True, capturable=True)
    gs = GraphStep(model, opt, crit, xs, ys, 2)
    steps = [[0, 1], [2, 3], [4, 5], [1, 4], [5, 0]]
    got = [gs.run(idx)[1].clone() for idx in steps]
    want = []
    for idx in steps:
        data, targets = gather_batch(xs, ys, torch.as_tensor(idx, dtype=torch.long, device=xs.device))
        want.append(eager_step(lambda d: twin(d).logits, topt, crit, data, targets)[1].clone())
    torch.cuda.synchronize()
    assert gs.graph is not None
    for s, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (s, float(a), float(b))
    assert torch.equal(model._flat[0], twin._flat[0])
    pos = model.audio_spectrogram_transformer.embeddings.position_embeddings.detach().cpu()
    a, b = R.cut_window(25, 9)
    grid, grid0 = pos[0, 2:].reshape(12, 25, 128), pos_init[0, 2:].reshape(12, 25, 128)
    assert not torch.equal(grid[:, a:b], grid0[:, a:b])            # the table itself trained, inside the window


# ============================================================================================ trainer
def _save_model_dir(path, seed):
    """HF-format directory of the reduced AST, 256 frames (config.json, model.safetensors, preprocessor_config.json)."""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    save_file({k: np.ascontiguousarray(v) for k, v in _weights(seed).items()}, os.path.join(path, "model.safetensors"))
    json.dump({"model_type": "audio-spectrogram-transformer", "hidden_size": 64, "num_hidden_layers": 2,
               "num_attention_heads": 4, "intermediate_size": 128, "patch_size": 16, "layer_norm_eps": 1e-12,
               "hidden_act": "gelu", "num_mel_bins": 128, "max_length": NATIVE, "frequency_stride": 10, "time_stride": 10,
               "id2label": {str(i): f"LABEL_{i}" for i in range(5)}}, open(os.path.join(path, "config.json"), "w"))
    json.dump({"feature_extractor_type": "ASTFeatureExtractor", "max_length": NATIVE, "num_mel_bins": 128,
               "sampling_rate": 16000, "do_normalize": True, "mean": -4.2677393, "std": 4.5689974},
              open(os.path.join(path, "preprocessor_config.json"), "w"))
    return str(path)


def test_trainer_with_max_length_auto(tmp_path, monkeypatch):
    from safetensors.numpy import load_file
    from eav_amd import transformer as T
    from eav_amd.audio import AudioModelTrainer
    from eav_amd.preprocess import waveforms_to_input_values
    path = _save_model_dir(tmp_path / "model", 28)
    monkeypatch.chdir(tmp_path)
    wav = synth.normal(290, (12, 8000), 0.0, 0.1)                   # 0.5 s: 48 frames -> T' = 56, 5 time patches
    y = synth.labels(291, 12)
    data = [wav[:8], y[:8], wav[8:], y[8:]]
    with pytest.raises(ValueError):
        AudioModelTrainer(data, path, batch_size=4, max_length=8)   # refused before any feature is extracted
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        tr = AudioModelTrainer(data, path, sub="s", num_classes=5, batch_size=4, max_length="auto")
        assert tr.max_length == 56 and tr.model.variable_length is True
        assert tuple(tr.tr_x.shape) == (8, 56, 128) and tuple(tr.te_x.shape) == (4, 56, 128)
        tr.train(epochs=1, lr=5e-4, freeze=True)
        tr.train(epochs=1, lr=5e-6, freeze=False)
    assert tr.outputs_test.shape == (4, 5)
    want = waveforms_to_input_values(wav[8:], max_length=56)
    assert torch.equal(tr.te_x, want.cpu())
    tr.model.eval()
    with torch.no_grad():
        logits = tr.model(want).logits
    close(logits, tr.outputs_test, 1e-4, 1e-4, "outputs_test")
    out = tmp_path / "saved"
    tr.save_pretrained(str(out))
    assert json.load(open(out / "config.json"))["max_length"] == 56
    assert json.load(open(out / "preprocessor_config.json"))["max_length"] == 56
    table = load_file(str(out / "model.safetensors"))[KEY]
    assert table.shape == (1, 2 + 12 * 5, 64)
    stored = tr.model.state_dict()[KEY].cpu().numpy()
    assert stored.shape == (1, 302, 64)                                            # the model keeps the checkpoint's table
    a, b = R.cut_window(25, 5)
    assert np.array_equal(table[0, 2:].reshape(12, 5, 64), stored[0, 2:].reshape(12, 25, 64)[:, a:b])
    # the table trained through the adjoint kernel inside the window
    before = _weights(28)[KEY][0, 2:].reshape(12, 25, 64)
    after = stored[0, 2:].reshape(12, 25, 64)
    assert not np.array_equal(after[:, a:b], before[:, a:b])
    # the saved directory is a model of 56 frames that runs with the flag off
    again = T.Encoder.from_pretrained(str(out)).cuda().eval()
    assert again.cfg.W == 56 and again.variable_length is False
    with torch.no_grad():
        close(again(want).logits, tr.outputs_test, 1e-4, 1e-4, "saved model")
