"""ViT interpolate_pos_encoding on the MI355X: the two resampling kernels against the float64 reference
(tests/vit_interp_ref.py), the encoder at 112 x 112, 56 x 56 and 64 x 144 against the CPU oracle and against Hugging Face
(tests/golden/vit_interp.npz), the native size with the flag on, the refusals, a captured step, and the trainer."""
import functools
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import vit_interp_ref as R
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "split"]
REDUCED = dict(hidden=64, layers=2, heads=4, ff=128)
SIZES = [(112, 112), (56, 56), (64, 144)]       # 56: the dataset's own crop size (remainder 8 pixels per axis)


def close(got, ref, rtol, atol, what):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}"


# ============================================================================================ kernels
@pytest.mark.parametrize("g,ny,nx", R.GRIDS)
def test_kernels_against_float64(g, ny, nx):
    from eav_amd import pos_interp as pi
    for D in (4, 64, 768):
        for nextra in (1, 2):
            pos = synth.normal(1000 + D + nextra, (nextra + g * g, D))
            dout = synth.normal(2000 + D + nextra, (nextra + ny * nx, D))
            pos_d, dout_d = torch.from_numpy(pos).cuda(), torch.from_numpy(dout).cuda()
            out = torch.full((nextra + ny * nx, D), float("nan"), device="cuda")
            pi.pos_bicubic_fwd(pos_d, out, g, ny, nx, nextra)
            dpos = [torch.full((nextra + g * g, D), float("nan"), device="cuda") for _ in range(2)]
            for d in dpos:
                pi.pos_bicubic_bwd(dout_d, d, g, ny, nx, nextra)
            torch.cuda.synchronize()
            what = f"{g}->{ny}x{nx} D={D} nextra={nextra}"
            got = out.cpu().double().numpy()
            err = np.abs(got - R.resample(pos, g, ny, nx, nextra))
            assert np.isfinite(got).all() and (err <= R.error_bounds(pos, g, ny, nx, nextra)).all(), (what, err.max())
            assert np.array_equal(got[:nextra], pos[:nextra])
            gotb = dpos[0].cpu().double().numpy()
            assert np.isfinite(gotb).all(), what + ": an element of dpos was not written"
            errb = np.abs(gotb - R.resample_adjoint(dout, g, ny, nx, nextra))
            assert (errb <= R.error_bounds(dout, g, ny, nx, nextra, adjoint=True)).all(), (what, errb.max())
            assert np.array_equal(gotb[:nextra], dout[:nextra])
            assert torch.equal(dpos[0], dpos[1]), what + ": the backward is not deterministic"


@pytest.mark.parametrize("n", [1, 2, 14])
def test_equal_sizes_copy_bit_for_bit(n):
    """n_out == n_in: t = 0, the coefficients are 0, 1, 0, 0 - forward and backward are copies."""
    from eav_amd import pos_interp as pi
    x = synth.normal(77 + n, (1 + n * n, 64))
    x[3 % len(x), 5] = -0.0
    xd = torch.from_numpy(x).cuda()
    out, back = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    pi.pos_bicubic_fwd(xd, out, n, n, n, 1)
    pi.pos_bicubic_bwd(xd, back, n, n, n, 1)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32))
    assert np.array_equal(back.cpu().numpy().view(np.uint32), x.view(np.uint32))


# ============================================================================================ model
def _weights(seed, std=0.08):
    from oracle import vit_oracle as vo
    return tf_weights(seed, vo.param_shapes(vo.cfg_vit(**REDUCED)), std=std)


def _model(W, precision, **kw):
    from eav_amd import transformer as T
    model = T.Encoder(T.make_config("vit", **REDUCED, **kw), W).cuda().train()
    model.precision = precision
    return model


@functools.lru_cache(maxsize=None)
def _oracle_case(H, W_):
    """(weights, x, y, logits, loss, gradients) of the CPU oracle on B = 3 frames of H x W_: the oracle's forward is
    size-agnostic, its position table is the float64-resampled one (cast to fp32), and the gradient of the STORED table is
    row 0 of the oracle's table gradient plus (Wy (x) Wx)^T of its patch rows."""
    from oracle import vit_oracle as vo
    ocfg = vo.cfg_vit(**REDUCED)
    W = _weights(13)
    x, y = R.frames(130 + H, 3, H, W_)
    key = "vit.embeddings.position_embeddings"
    ny, nx = H // 16, W_ // 16
    P = {k: torch.from_numpy(v.copy()) for k, v in W.items()}
    P[key] = torch.from_numpy(R.resample(W[key][0], 14, ny, nx).astype(np.float32))[None]
    st = vo.Stepper(P, ocfg, lr=1e-3)
    logits, loss, grads = st.step(torch.from_numpy(x), torch.from_numpy(y), False)
    grads = {k: v.numpy() for k, v in grads.items()}
    grads[key] = R.resample_adjoint(grads[key][0], 14, ny, nx)[None]
    return W, x, y, logits.numpy(), loss.numpy(), grads


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_other_sizes_match_the_oracle(size, precision):
    """Bounds: those of test_full_size_gradients_match_oracle."""
    from eav_amd.optim import CrossEntropyLoss
    W, x, y, logits, lref, grads = _oracle_case(*size)
    model = _model(W, precision)
    out = model(torch.from_numpy(x).cuda(), interpolate_pos_encoding=True)
    loss = CrossEntropyLoss()(out.logits, torch.from_numpy(y).cuda())
    loss.backward()
    torch.cuda.synchronize()
    close(out.logits, logits, 1e-4, 1e-4, "logits")
    close(loss, lref, 1e-4, 1e-4, "loss")
    for k, p in model.named_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(W[k].shape), k
        close(p.grad, grads[k], 2e-3, max(2e-3 * np.abs(grads[k]).max(), 1e-7), f"grad.{k}")
    # cfg, the parameters' shapes and the state dict are those of the checkpoint: the geometry belonged to the forward
    assert (model.cfg.H, model.cfg.W, model.cfg.ntok) == (224, 224, 197)
    assert tuple(model.state_dict()["vit.embeddings.position_embeddings"].shape) == (1, 197, 64)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_attention_path_at_another_size(precision):
    """head_dim 64 takes the fused attention kernels (the reduced model's head_dim 16 the GEMM + softmax path): 7 x 7 patches,
    the flag given as the model's attribute.  Bounds: those of test_full_size_gradients_match_oracle."""
    from eav_amd import transformer as T
    from eav_amd.optim import CrossEntropyLoss
    from oracle import vit_oracle as vo
    kw = dict(hidden=128, layers=2, heads=2, ff=256)
    ocfg = vo.cfg_vit(**kw)
    W = tf_weights(14, vo.param_shapes(ocfg), std=0.08)
    x, y = R.frames(141, 3, 112, 112)
    key = "vit.embeddings.position_embeddings"
    P = {k: torch.from_numpy(v.copy()) for k, v in W.items()}
    P[key] = torch.from_numpy(R.resample(W[key][0], 14, 7, 7).astype(np.float32))[None]
    logits, lref, grads = vo.Stepper(P, ocfg, lr=1e-3).step(torch.from_numpy(x), torch.from_numpy(y), False)
    grads = {k: v.numpy() for k, v in grads.items()}
    grads[key] = R.resample_adjoint(grads[key][0], 14, 7, 7)[None]
    model = T.Encoder(T.make_config("vit", **kw), W).cuda().train()
    model.precision = precision
    assert model._fused_attention()
    model.interpolate_pos_encoding = True           # the attribute: what forward_batch and the trainers run with
    out = model(torch.from_numpy(x).cuda())
    loss = CrossEntropyLoss()(out.logits, torch.from_numpy(y).cuda())
    loss.backward()
    torch.cuda.synchronize()
    close(out.logits, logits.numpy(), 1e-4, 1e-4, "logits")
    close(loss, lref.numpy(), 1e-4, 1e-4, "loss")
    for k, p in model.named_parameters():
        close(p.grad, grads[k], 2e-3, max(2e-3 * np.abs(grads[k]).max(), 1e-7), f"grad.{k}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_other_sizes_match_hf(golden_dir, precision):
    """HF's ViTForImageClassification(..., interpolate_pos_encoding=True): bounds of
    test_reduced_model_training_steps_match_hf (its unfrozen step)."""
    from eav_amd.optim import CrossEntropyLoss
    g = np.load(os.path.join(golden_dir, "vit_interp.npz"))
    model = _model(_weights(int(g["wseed"]), float(g["std"])), precision)
    crit = CrossEntropyLoss()
    x, y = R.frames(int(g["xseed"]), int(g["B"]), 112, 112)
    out = model(torch.from_numpy(x).cuda(), interpolate_pos_encoding=True)
    loss = crit(out.logits, torch.from_numpy(y).cuda())
    loss.backward()
    close(out.logits, g["logits112"], 1e-4, 1e-4, "logits 112")
    close(loss, g["loss112"], 1e-4, 1e-4, "loss 112")
    named = dict(model.named_parameters())
    gkeys = sorted(k[len("grad112."):] for k in g.files if k.startswith("grad112."))
    assert sorted(named) == gkeys
    for k in gkeys:
        ref = g[f"grad112.{k}"]
        close(named[k].grad, ref, 1e-3, max(1e-3 * np.abs(ref).max(), 1e-6), f"grad112.{k}")
    x, y = R.frames(int(g["xseed"]) + 1, int(g["B"]), 64, 144)
    with torch.no_grad():
        out = model(pixel_values=torch.from_numpy(x).cuda(), labels=torch.from_numpy(y).cuda(), interpolate_pos_encoding=True)
    close(out.logits, g["logits64x144"], 1e-4, 1e-4, "logits 64x144")
    close(out.loss, g["loss64x144"], 1e-4, 1e-4, "loss 64x144")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_native_size_with_the_flag_on_is_bit_equal(precision):
    """HF's shortcut: at the native size the stored table is used - the same launches, the same bits."""
    from eav_amd.optim import CrossEntropyLoss
    W = _weights(15)
    x, y = R.frames(150, 2, 224, 224)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = []
    for flag in (False, True):
        model = _model(W, precision)
        out = model(xd, interpolate_pos_encoding=flag)
        CrossEntropyLoss()(out.logits, yd).backward()
        torch.cuda.synchronize()
        assert model._active_geo is None
        res.append((out.logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_refusals_on_the_device():
    from eav_amd import transformer as T
    W = _weights(16)
    model = _model(W, "split")
    x = torch.from_numpy(R.frames(160, 2, 112, 112)[0]).cuda()
    with pytest.raises(ValueError, match="expected input"):
        model(x)                                                    # flag off: the same error as ever
    with pytest.raises(ValueError):
        model(x[:, :2], interpolate_pos_encoding=True)              # channels
    with pytest.raises(ValueError):
        model(x[:, :, :8], interpolate_pos_encoding=True)           # smaller than a patch
    dropping = _model(W, "split", hidden_dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        dropping(x, interpolate_pos_encoding=True)
    dropping.eval()                                                 # nothing drops in eval mode
    with torch.no_grad():
        assert dropping(x, interpolate_pos_encoding=True).logits.shape == (2, 5)
    ast = T.Encoder(T.make_config("ast", hidden=64, layers=1, heads=4, ff=128, frames=64)).cuda()
    with pytest.raises(NotImplementedError):
        ast(torch.zeros(1, 64, 128, device="cuda"), interpolate_pos_encoding=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sizes_alternate_on_one_model(precision):
    """The geometry travels with the forward's token: forwards of two sizes interleaved with their backwards give the
    gradients of separate runs, bit for bit."""
    from eav_amd.optim import CrossEntropyLoss
    W = _weights(17)
    crit = CrossEntropyLoss()
    data = {s: tuple(torch.from_numpy(a).cuda() for a in R.frames(170 + s, 2, s, s)) for s in (112, 224, 56)}

    def step(model, s):
        for p in model.parameters():
            p.grad = None
        out = model(data[s][0], interpolate_pos_encoding=True)
        crit(out.logits, data[s][1]).backward()
        torch.cuda.synchronize()
        return out.logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}

    one = _model(W, precision)
    for s in (112, 224, 56, 112):
        got, fresh = step(one, s), step(_model(W, precision), s)
        assert torch.equal(got[0], fresh[0]), s
        for k in got[1]:
            assert torch.equal(got[1][k], fresh[1][k]), (s, k)


# ============================================================================================ captured step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_step_at_another_size(precision):
    """GraphStep over an Encoder whose attribute is on and whose data set is not of the native size: eager, captured and
    replayed steps equal a twin stepped eagerly, bit for bit (the tables are on the device before the capture)."""
    import copy
    from eav_amd import transformer as T
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    from eav_amd.runtime import GraphStep, eager_step, gather_batch
    torch.manual_seed(11)
    model = T.Encoder(T.make_config("vit", hidden=128, heads=2, ff=256, layers=2, image=64))
    model.precision, model.overlap_wgrad, model.interpolate_pos_encoding = precision, False, True
    with torch.no_grad():
        model.vit.embeddings.position_embeddings.normal_(0.0, 0.02)
    pos_init = model.vit.embeddings.position_embeddings.detach().clone()
    twin = copy.deepcopy(model)
    model, twin = model.cuda().train(), twin.cuda().train()
    x, y = R.frames(180, 6, 32, 48)                      # 2 x 3 patches of a 4 x 4 table
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
    assert not torch.equal(model.vit.embeddings.position_embeddings.detach().cpu(), pos_init)     # the table itself trained


# ============================================================================================ trainer
def _save_model_dir(tmp_path, seed):
    """HF-format directory of the reduced ViT (config.json, model.safetensors, preprocessor_config.json)."""
    from safetensors.numpy import save_file
    os.makedirs(tmp_path, exist_ok=True)
    save_file({k: np.ascontiguousarray(v) for k, v in _weights(seed).items()}, os.path.join(tmp_path, "model.safetensors"))
    json.dump({"model_type": "vit", "hidden_size": 64, "num_hidden_layers": 2, "num_attention_heads": 4,
               "intermediate_size": 128, "patch_size": 16, "layer_norm_eps": 1e-12, "hidden_act": "gelu",
               "image_size": 224, "num_channels": 3, "id2label": {str(i): f"LABEL_{i}" for i in range(5)}},
              open(os.path.join(tmp_path, "config.json"), "w"))
    json.dump({"do_normalize": True, "do_rescale": True, "do_resize": True, "image_mean": [0.5, 0.5, 0.5],
               "image_std": [0.5, 0.5, 0.5], "image_processor_type": "ViTImageProcessor", "resample": 2,
               "rescale_factor": 1 / 255, "size": {"height": 224, "width": 224}},
              open(os.path.join(tmp_path, "preprocessor_config.json"), "w"))
    return str(tmp_path)


def test_trainer_with_image_size(tmp_path, monkeypatch):
    from eav_amd import transformer as T
    from eav_amd.preprocess import frames_to_pixel_values
    from eav_amd.vision import ImageClassifierTrainer
    path = _save_model_dir(tmp_path / "model", 18)
    monkeypatch.chdir(tmp_path)
    frames = (synth.uniform(190, (12, 2, 56, 56, 3)) * 255).astype(np.uint8)
    y = synth.labels(191, 12)
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        tr = ImageClassifierTrainer([frames[:8], y[:8], frames[8:], y[8:]], path, sub="s", num_labels=5, batch_size=4,
                                    image_size=112)
        assert tr.model.interpolate_pos_encoding is True
        assert tuple(tr.train_dataloader.x.shape) == (16, 3, 112, 112)
        assert tuple(tr.test_dataloader.x.shape) == (8, 3, 112, 112)
        # the frames were resized to 112 x 112 by the same kernel, not to the processor's 224
        want = frames_to_pixel_values(frames[8:].reshape(-1, 56, 56, 3), (112, 112))
        assert torch.equal(tr.test_dataloader.x, want)
        tr.train(epochs=1, lr=5e-4, freeze=True)
        tr.train(epochs=1, lr=5e-6, freeze=False)
    assert tr.outputs_test.shape == (8, 5)
    out = tmp_path / "saved"
    tr.save_pretrained(str(out))
    assert json.load(open(out / "config.json"))["image_size"] == 224
    again = T.Encoder.from_pretrained(str(out))
    sd, sd0 = again.state_dict(), tr.model.state_dict()
    assert tuple(sd["vit.embeddings.position_embeddings"].shape) == (1, 197, 64)
    for k in sd0:
        assert torch.equal(sd[k], sd0[k].cpu()), k
    # outputs_test = a plain Encoder forward (flag on) of the preprocessed test frames with the final weights
    again = again.cuda().eval()
    with torch.no_grad():
        logits = again(tr.test_dataloader.x, interpolate_pos_encoding=True).logits
    close(logits, tr.outputs_test, 1e-4, 1e-4, "outputs_test")
    # the position table trained through the adjoint kernel: it differs from the checkpoint's
    assert not np.array_equal(sd["vit.embeddings.position_embeddings"].numpy(), _weights(18)["vit.embeddings.position_embeddings"])
    with pytest.raises(ValueError):
        ImageClassifierTrainer([frames[:8], y[:8], frames[8:], y[8:]], path, batch_size=4, image_size=(112, 8))
