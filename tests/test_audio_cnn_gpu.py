"""AudioModel / train_model (eav_amd/cnn_audio.py) on the MI355X against golden vectors captured from the imported
reference CNN_torch/CNN_audio.py (tests/golden/make_goldens_audio_cnn.py), directly and through a plain-torch CPU
restatement pinned to them.  Logits within 5e-5, gradients and post-step parameters within 1e-3 of each tensor's max."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import synth

pytestmark = pytest.mark.gpu

PN = ["features.0.weight", "features.0.bias", "features.2.weight", "features.2.bias", "features.6.weight",
      "features.6.bias", "features.8.weight", "features.8.bias", "classifier.weight", "classifier.bias"]


def close(got, ref, rtol, atol, what):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = err > atol + rtol * np.abs(ref)
    assert not bad.any(), f"{what}: max err {err.max():.3e} (atol {np.max(atol):.1e}), {int(bad.sum())} of {bad.size} off"


def seeded_model(wseed, dev="cuda"):
    from eav_amd.cnn_audio import AudioModel
    torch.manual_seed(wseed)
    return AudioModel(num_classes=5).to(dev)


def golden_masks(mseed, s, B, T):
    """The keep-masks the golden fed the reference at step s (tests/golden/make_goldens_audio_cnn.py)."""
    return ((synth.uniform(mseed + 2 * s, (B, 128, T)) >= 0.1).astype(np.uint8),
            (synth.uniform(mseed + 2 * s + 1, (B, 128, 22)) >= 0.5).astype(np.uint8))


def cpu_logits(net, x, masks, keep=None, pool_idx=None):
    """Plain-torch CPU restatement of AudioModel.forward (CNN_audio.py:35-38) with explicit dropout keep-masks, applied
    as the golden applied them to the reference (x * keep / (1 - p)).  keep (dict): receives conv1's pre-activation z1
    and its ReLU output a1 (gradient retained), and the MaxPool(8) input h.  pool_idx ([B,128,22] int64, offsets within
    the window): route the pool through these positions instead of the argmax."""
    import torch.nn.functional as F
    f = net.features
    z1 = f[0](x)
    a1 = F.relu(z1)
    if keep is not None:
        a1.retain_grad()
        keep.update(z1=z1.detach(), a1=a1)
    h = F.relu(f[2](a1))
    if masks is not None:
        h = h * torch.from_numpy(masks[0]).float() / (1.0 - 0.1)
    if keep is not None:
        keep["h"] = h.detach()
    if pool_idx is None:
        p = F.max_pool1d(h, 8)
    else:
        p = h[..., :8 * pool_idx.shape[2]].unflatten(2, (pool_idx.shape[2], 8)).gather(3, pool_idx.unsqueeze(3)).squeeze(3)
    h = F.relu(f[8](F.relu(f[6](p))))
    if masks is not None:
        h = h * torch.from_numpy(masks[1]).float() / (1.0 - 0.5)
    return net.classifier(torch.flatten(h, 1))


def pin(t, g, key, rel):
    """A full CPU tensor against the golden's strided sample and whole-tensor (sum |t|, max |t|) of the reference."""
    a = t.detach().numpy().reshape(-1)
    ref = g[key]
    close(a[::-(-a.size // int(g["sample"]))], ref, 0, rel * float(g[key + ".abs"][1]) + 1e-12, key)
    st = np.array([np.abs(a.astype(np.float64)).sum(), np.abs(a).max()])
    close(st, g[key + ".abs"], rel, 1e-12, key + " (sum |t|, max |t|)")


def relu_boundary_slack(x, keep):
    """conv1's ReLU decides at zero: a pre-activation within fp32 rounding of 0 (|z1| <= 3e-7 of max |z1|, a few ulps)
    may be gated either way by two correct fp32 evaluations, and moves conv1's gradients by that position's whole term
    (three Adam steps into the t180_adam golden one such position moves the CPU fp32 gradient 2.6e-3 of its max away from
    float64).  Returns the sum of |those terms| for features.0.weight [256,1,5] and features.0.bias [256]."""
    z1, da1 = keep["z1"], keep["a1"].grad
    amb = (z1.abs() <= 3e-7 * z1.abs().max()).double()
    g = (da1.double() * amb).abs()                                   # [B,256,T]
    xp = torch.nn.functional.pad(x.double(), (2, 2))                  # [B,1,T+4]
    T = z1.shape[2]
    w = torch.stack([(g * xp[:, :, tap:tap + T].abs()).sum((0, 2)) for tap in range(5)], 1).unsqueeze(1)
    return {"features.0.weight": w.numpy(), "features.0.bias": g.sum((0, 2)).numpy()}


def post_close(got, ref, lr, what):
    got = got.detach().cpu().double().numpy()
    ref = ref.detach().cpu().double().numpy()
    err = np.abs(got - ref)
    # within 1e-3 of the tensor's max almost everywhere; an element whose gradient is rounding noise around 0 may take
    # the other sign's Adam step: at most 2 lr away
    assert (err <= 1e-3 * np.abs(ref).max()).mean() > 0.995, f"{what}: tight fraction"
    assert err.max() <= 2 * lr + 1e-3 * np.abs(ref).max(), f"{what}: {err.max():.3e}"


def kernels_match_restatement(model, opt, ref, x, y, masks, keep, ref_logits, ref_loss, rgrads, tag=""):
    """One forward and backward of the kernels from `model`'s parameters against the CPU restatement's (ref_logits,
    ref_loss, rgrads and keep from cpu_logits at the same parameters; ref: a module to copy for the rerouted restatement):
    logits and loss 5e-5, every gradient element 1e-3 of its tensor's max (plus conv1's ReLU boundary slack)."""
    import copy
    from eav_amd.optim import CrossEntropyLoss
    named = dict(model.named_parameters())
    ref_crit = torch.nn.CrossEntropyLoss()
    if masks is not None:
        model.set_dropout_masks(tuple(torch.from_numpy(m).cuda() for m in masks))
    logits = model(torch.from_numpy(x).cuda().permute(0, 2, 1))
    loss = CrossEntropyLoss()(logits, torch.from_numpy(y).cuda())
    opt.zero_grad()
    loss.backward()
    close(logits, ref_logits.detach().numpy(), 0, 5e-5, f"logits{tag}")
    close(loss, ref_loss.detach().numpy(), 0, 5e-5, f"loss{tag}")
    # MaxPool(8) decides by comparison: where the kernels' argmax differs from the restatement's, the two window
    # values must tie to fp32 rounding; the comparison target is then the restatement routed like the kernels
    gidx = model._ws.idx2.long().cpu()
    h = keep["h"][..., :176].unflatten(2, (22, 8))
    cidx = h.argmax(3)
    diff = gidx != cidx
    if diff.any():
        hv = lambda i: h.gather(3, i.unsqueeze(3)).squeeze(3)[diff]  # noqa: E731
        assert ((hv(gidx) - hv(cidx)).abs() <= 1e-5 * h.abs().max()).all(), "pool argmax differs beyond a tie"
        rr = copy.deepcopy(ref)
        with torch.no_grad():
            for k, v in rr.named_parameters():
                v.copy_(named[k].detach().cpu())
        keep = {}
        ref_crit(cpu_logits(rr, torch.from_numpy(x).permute(0, 2, 1), masks, keep, gidx),
                 torch.from_numpy(y)).backward()
        rgrads = {k: v.grad for k, v in rr.named_parameters()}
    slack = relu_boundary_slack(torch.from_numpy(x).permute(0, 2, 1), keep)
    for k in PN:
        r = rgrads[k].numpy()
        close(named[k].grad, r, 0, 1e-3 * np.abs(r).max() + 1e-9 + slack.get(k, 0.0), f"grad{tag}.{k}")


@pytest.mark.parametrize("case", ["t180_adam", "eval", "t176", "t183"])
def test_steps_match_reference_golden(golden_dir, case):
    """The golden holds the imported reference's logits and loss, and strided samples plus |sum| / max of every gradient
    and post-step parameter.  A plain-torch CPU restatement of the same steps is pinned to those; the kernels' full
    tensors are then held to the restatement: logits 5e-5, every gradient element 1e-3 of its tensor's max.
    Every step starts from the restatement's own parameters of that step, so that each step's logits and gradients are
    compared at the same point: Adam turns any rounding difference of a near-zero gradient element into a +-lr move, and
    a free-running trajectory would compare the updates' noise rather than the kernels.  The GPU optimiser's moments are
    its own throughout."""
    import copy
    from eav_amd.cnn_audio import AudioModel
    from eav_amd.optim import FusedAdam
    g = np.load(os.path.join(golden_dir, f"audio_cnn_{case}.npz"))
    B, T, lr, steps = int(g["B"]), int(g["T"]), float(g["lr"]), int(g["steps"])
    training = bool(int(g["train_mode"]))
    torch.manual_seed(int(g["wseed"]))
    model = AudioModel(num_classes=5)
    ref = copy.deepcopy(model).train(training)
    ref_crit, ref_opt = torch.nn.CrossEntropyLoss(), torch.optim.Adam(ref.parameters(), lr=lr)
    model = model.cuda().train(training)
    opt = FusedAdam(model.parameters(), lr=lr)
    named, rnamed = dict(model.named_parameters()), dict(ref.named_parameters())
    for s in range(steps):
        x = synth.normal(int(g["xseed"]) + s, (B, T, 1))
        y = synth.labels(int(g["xseed"]) + 100 + s, B, 5)
        masks = golden_masks(int(g["mseed"]), s, B, T) if training else None
        # the CPU restatement, pinned to the reference
        with torch.no_grad():
            for k in PN:
                named[k].copy_(rnamed[k])
        ref_opt.zero_grad()
        keep = {}
        ref_logits = cpu_logits(ref, torch.from_numpy(x).permute(0, 2, 1), masks, keep)
        ref_loss = ref_crit(ref_logits, torch.from_numpy(y))
        ref_loss.backward()
        ref_opt.step()
        close(ref_logits, g[f"logits{s}"], 0, 1e-5, f"restatement logits{s}")
        close(ref_loss, g[f"loss{s}"], 0, 1e-5, f"restatement loss{s}")
        for k in PN:
            pin(rnamed[k].grad, g, f"grad{s}.{k}", 1e-4)
            if f"post{s}.{k}" in g.files:
                pin(rnamed[k], g, f"post{s}.{k}", 1e-4)
        # the kernels, from the same parameters
        kernels_match_restatement(model, opt, ref, x, y, masks, keep, ref_logits, ref_loss,
                                  {k: rnamed[k].grad for k in PN}, str(s))
        opt.step()
        torch.cuda.synchronize()
        if f"post{s}.{PN[0]}" in g.files:
            for k in PN:
                post_close(named[k], rnamed[k], lr, f"post{s}.{k}")



@pytest.mark.parametrize("B,T", [(1, 181), (130, 177)])
def test_step_matches_restatement_off_golden(B, T):
    """The model's own wiring at two lengths and batch sizes the goldens do not hold, with explicit dropout masks: B = 1
    puts every weight gradient through the clamped nparts path (one 32-position chunk per part), B = 130 through the
    split one; held to the CPU restatement as in test_steps_match_reference_golden."""
    import copy
    from eav_amd.optim import FusedAdam
    ref = seeded_model(31, "cpu").train()
    model = copy.deepcopy(ref).cuda().train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    x = synth.normal(40 + B, (B, T, 1))
    y = synth.labels(41 + B, B, 5)
    masks = golden_masks(42 + B, 0, B, T)
    keep = {}
    ref_logits = cpu_logits(ref, torch.from_numpy(x).permute(0, 2, 1), masks, keep)
    ref_loss = torch.nn.CrossEntropyLoss()(ref_logits, torch.from_numpy(y))
    ref_loss.backward()
    kernels_match_restatement(model, opt, ref, x, y, masks, keep, ref_logits, ref_loss,
                              {k: p.grad for k, p in ref.named_parameters()})

def _one_step(x, y, masks=None, seed=21):
    from eav_amd.optim import CrossEntropyLoss
    model = seeded_model(seed).train()
    if masks is not None:
        model.set_dropout_masks(masks)
    logits = model(x)
    CrossEntropyLoss()(logits, y).backward()
    torch.cuda.synchronize()
    return model, logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def test_step_is_bit_reproducible():
    x = torch.from_numpy(synth.normal(5, (64, 1, 180))).cuda()
    y = torch.from_numpy(synth.labels(6, 64, 5)).cuda()
    _, l0, g0 = _one_step(x, y)
    _, l1, g1 = _one_step(x, y)
    assert torch.equal(l0, l1)
    for k in PN:
        assert torch.equal(g0[k], g1[k]), k


def test_graph_replay_equals_eager_step():
    """One GraphStep replay (gather, forward, loss, backward, FusedAdam) is bit-equal to the same step run eagerly with the
    same dropout masks."""
    from eav_amd.eegnet import GraphStep, gather_batch
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    N, B, T = 96, 32, 180
    xs = torch.from_numpy(synth.normal(8, (N, T, 1))).cuda()
    ys = torch.from_numpy(synth.labels(9, N, 5)).cuda()
    gen = torch.Generator().manual_seed(3)
    masks = ((torch.rand(B, 128, T, generator=gen) >= 0.1).to(torch.uint8).cuda(),
             (torch.rand(B, 128, 22, generator=gen) >= 0.5).to(torch.uint8).cuda())
    orders = [list(range(0, 32)), list(range(32, 64)), list(range(64, 96)), list(range(16, 48))]

    def run(graph):
        model = seeded_model(40).train()
        model.set_dropout_masks(masks)
        crit, opt = CrossEntropyLoss(), FusedAdam(model.parameters(), lr=1e-3, capturable=True)
        step = GraphStep(model, opt, crit, xs, ys, B) if graph else None
        outs = []
        for idx in orders:
            if graph:
                scores, loss = step.run(idx)
            else:
                data, targets = gather_batch(xs, ys, torch.as_tensor(idx, device="cuda"))
                opt.zero_grad()
                scores = model(data)
                loss = crit(scores, targets)
                loss.backward()
                opt.step()
            outs.append((scores.detach().clone(), loss.detach().clone()))
        torch.cuda.synchronize()
        return outs, {k: v.detach().clone() for k, v in model.state_dict().items()}

    eager, pe = run(False)
    replay, pr = run(True)
    for (a, la), (b, lb) in zip(eager, replay):       # steps 3 and 4 are the capture and a replay
        assert torch.equal(a, b) and torch.equal(la, lb)
    for k in PN:
        assert torch.equal(pe[k], pr[k]), k


def test_generated_dropout_rates_and_fresh_masks():
    """Counter-based dropout: the kept fraction of both Dropout layers is within a binomial bound (5 sigma) of 1 - p,
    every training forward draws a fresh mask, eval mode draws none."""
    x = torch.from_numpy(synth.normal(12, (64, 1, 180))).cuda()
    model = seeded_model(22).train()
    model.features[4].p, model.features[10].p = 0.0, 0.0
    model(x)
    ref_p2, ref_a4 = model._ws.p2.clone(), model._ws.a4.clone()
    # Dropout(0.5) after conv4 (nothing pools after it): every live activation is either doubled or zero
    model.features[10].p = 0.5
    model(x)
    live4, a4 = ref_a4 > 0, model._ws.a4
    n4 = int(live4.sum())
    kept4 = int(((a4 > 0) & live4).sum()) / n4
    assert abs(kept4 - 0.5) < 5 * (0.25 / n4) ** 0.5, kept4
    assert torch.equal(a4[(a4 > 0) & live4], ref_a4[(a4 > 0) & live4] * 2.0)
    first = a4.clone()
    model(x)
    assert not torch.equal(first > 0, model._ws.a4 > 0)          # a fresh mask on every training forward
    # Dropout(0.1) before MaxPool(8): a window keeps its scaled maximum exactly when its argmax position was kept
    model.features[4].p, model.features[10].p = 0.1, 0.0
    model(x)
    live2 = ref_p2 > 0
    n2 = int(live2.sum())
    same = (model._ws.p2 - ref_p2 * (1.0 / 0.9)).abs() <= 1e-6 * ref_p2.abs().max()
    kept2 = int((same & live2).sum()) / n2
    assert abs(kept2 - 0.9) < 5 * (0.09 / n2) ** 0.5, kept2
    model.eval()
    model(x)
    assert torch.equal(model._ws.p2, ref_p2) and torch.equal(model._ws.a4, ref_a4)


def test_train_model_matches_reference(golden_dir, tmp_path):
    from eav_amd import cnn_audio as ca
    g = np.load(os.path.join(golden_dir, "audio_cnn_train_model.npz"))
    ntr, nval, T = int(g["ntr"]), int(g["nval"]), int(g["T"])
    x = synth.normal(int(g["xseed"]), (ntr + nval, T, 1))
    y = synth.labels(int(g["yseed"]), ntr + nval, 5)
    torch.manual_seed(int(g["wseed"]))
    model = ca.AudioModel(num_classes=5)
    model.features[4].p = 0.0
    model.features[10].p = 0.0
    train_loader = ca.create_dataloader(x[:ntr], y[:ntr], batch_size=int(g["batch_size"]))
    val_loader = ca.create_dataloader(x[ntr:], y[ntr:], batch_size=int(g["batch_size"]))
    buf = io.StringIO()
    torch.manual_seed(int(g["tseed"]))
    with redirect_stdout(buf):
        ca.train_model(model, train_loader, val_loader, epochs=int(g["epochs"]), lr=float(g["lr"]),
                       save_dir=str(tmp_path))
    assert buf.getvalue() == str(g["stdout"]), (buf.getvalue(), str(g["stdout"]))
    for e in (1, 2):
        got = torch.load(os.path.join(tmp_path, f"activations_epoch_{e}.pth"), weights_only=False)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        # epoch 2 is three more Adam steps down a trajectory whose near-zero gradient elements may take the other sign's
        # +-lr step (see test_steps_match_reference_golden): held to 5e-4 there, as test_cnn_eeg_gpu.py's later steps
        close(got, g[f"act{e}"], 0, 5e-5 if e == 1 else 5e-4, f"activations_epoch_{e}")


def test_nan_in_input_reaches_the_logits():
    x = synth.normal(13, (4, 1, 180))
    x[1, 0, 90] = np.nan
    model = seeded_model(23).eval()
    with torch.no_grad():
        logits = model(torch.from_numpy(x).cuda()).cpu()
    assert torch.isnan(logits[1]).all()
    assert torch.isfinite(logits[[0, 2, 3]]).all()
