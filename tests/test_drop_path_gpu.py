"""Stochastic depth (Encoder.drop_path_rate) of the AST / ViT encoders on the MI355X, in both precisions: Hugging Face goldens
(tests/golden/drop_path_{ast,vit}.npz) under explicit keep tables, head_dim 16 and the geometry combinations against the float64
restatement (tests/drop_path_ref.py), generated tables eagerly and in a captured step, off-means-off by launch lists, the
refusals, the trainer and the command-line option."""
import importlib.util
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import drop_path_ref as R
from tests import patch_keep_ref as PK
from tests.encoder_dropout_ref import summarise
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ["fp32", "split"]
PATH_LAUNCHES = ("eav_drop_path_plan", "eav_drop_path_add")


def close(got, ref, rtol, atol, what):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    print(f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}, bound {atol:.3e} + {rtol:.0e} |ref|")
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}"


def _model(kind, precision, model=None, wseed=None, fused=True, **kw):
    """(Encoder, its config, the oracle's config, the weights) of a reduced model (tests/drop_path_ref.MODEL)."""
    from eav_amd import transformer as T
    from oracle import vit_oracle as vo
    model = model or R.MODEL
    extra = dict(frames=R.AST_FRAMES) if kind == "ast" else {}
    cfg = T.make_config(kind, **model, **extra, **kw)
    ocfg = R.oracle_cfg(kind, model)
    W = tf_weights(R.WSEED[kind] if wseed is None else wseed, vo.param_shapes(ocfg), std=R.STD)
    m = T.Encoder(cfg, W).cuda().train()
    m.precision, m.use_fused_attention = precision, fused
    return m, cfg, ocfg, W


def _batch(kind, ocfg, seed, B):
    x, y = R.batch(kind, ocfg, seed, B)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def _table(keep):
    return torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).cuda()


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


def _check_grads(grads, ref, what):
    """The unfrozen-step gradient bound of test_training_steps_match_hf_under_explicit_masks on full tensors: rtol 1e-3, atol
    1e-3 of the reference tensor's maximum."""
    assert sorted(grads) == sorted(ref)
    for k in sorted(ref):
        r = ref[k].detach().cpu().double().numpy()
        close(grads[k], r, 1e-3, max(1e-3 * np.abs(r).max(), 1e-6), f"{what} grad.{k}")


# ============================================================================================ Hugging Face goldens
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "materialised"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_training_steps_match_hf_under_explicit_tables(golden_dir, kind, precision, fused):
    """tests/golden/drop_path_{kind}.npz: 3 layers, B = 4, r = 0.5 (p = 0, 0.25, 0.5), one unfrozen AdamW step, then one frozen
    step, keep tables through set_drop_path_masks.  Bounds: exactly those of
    test_encoder_dropout_gpu.test_training_steps_match_hf_under_explicit_masks - logits and loss close(1e-4, 1e-4) (logits
    5e-4 on the frozen step), gradients rtol 1e-3 with atol 1e-3 (5e-3) of the tensor's maximum on the stored strided samples,
    max |.| under the same bound and sum |.| under what the element bound implies for a sum, that test's post-step rule.
    Step 0 drops layer 2's MLP branch for the whole batch: fc1 / fc2 / layernorm_after of layer 2 get exactly zero gradients,
    and everything stays finite (the split path measures an all-zero gated gradient: sigma_from_bits gives 1)."""
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    g = np.load(os.path.join(golden_dir, f"drop_path_{kind}.npz"))
    model, cfg, ocfg, _ = _model(kind, precision, fused=fused)
    assert float(g["rate"]) == R.RATE and int(g["B"]) == R.BATCH
    model.drop_path_rate = R.RATE
    assert np.array_equal(model.drop_path_rates(), np.array([0, 0.25, 0.5], np.float32))
    lr = float(g["lr"])
    opt = FusedAdam(model.parameters(), lr=lr, weight_decay=0.01, decoupled=True)
    crit = CrossEntropyLoss()
    for s, freeze in enumerate((False, True)):
        x, y = _batch(kind, ocfg, int(g["xseed"]) + s, R.BATCH)
        keep = R.golden_keep(s)
        assert np.array_equal(keep, g[f"keep{s}"])
        model.set_drop_path_masks(_table(keep))
        for k, p in model.named_parameters():
            p.requires_grad = (not freeze) or k.startswith("classifier.")
        opt.zero_grad()
        out = model(x)
        loss = crit(out.logits, y)
        loss.backward()
        torch.cuda.synchronize()
        if s == 0:
            assert model._ws.fused == fused
        assert np.array_equal(model.last_drop_path().cpu().numpy(), R.plan(3, R.BATCH, R.RATE, 0, keep=keep)[1])
        close(out.logits, g[f"logits{s}"], 1e-4, 1e-4 if s == 0 else 5e-4, f"logits{s}")
        close(loss, g[f"loss{s}"], 1e-4, 1e-4, f"loss{s}")
        named = dict(model.named_parameters())
        pre = f"grad{s}."
        gkeys = sorted(k[len(pre):] for k in g.files if k.startswith(pre) and "#" not in k)
        assert sorted(k for k, p in named.items() if p.grad is not None) == gkeys
        for k in gkeys:
            assert torch.isfinite(named[k].grad).all(), k
            ref, rmax, rsum = g[pre + k], float(g[pre + k + "#maxabs"]), float(g[pre + k + "#sumabs"])
            atol = max((1e-3 if s == 0 else 5e-3) * rmax, 1e-6)
            smp, sa, mx = summarise(named[k].grad)
            err = np.abs(smp.astype(np.float64) - ref)
            assert (err <= atol + 1e-3 * np.abs(ref)).all(), f"grad{s}.{k}: max err {err.max():.3e}, ref max {rmax:.3e}"
            assert abs(mx - rmax) <= atol + 1e-3 * rmax, f"grad{s}.{k}: max {mx:.6e} vs {rmax:.6e}"
            assert abs(sa - rsum) <= atol * named[k].numel() + 1e-3 * rsum, f"grad{s}.{k}: sum {sa:.6e} vs {rsum:.6e}"
        if s == 0:
            dead = [k for k in gkeys if ".layers.2.mlp." in k or ".layers.2.layernorm_after." in k]
            assert len(dead) == 6
            for k in dead:
                assert float(g[pre + k + "#maxabs"]) == 0.0 and not named[k].grad.any(), k
        opt.step()
        torch.cuda.synchronize()
        for k in gkeys:
            assert torch.isfinite(named[k]).all(), k
            err = np.abs(summarise(named[k])[0].astype(np.float64) - g[f"post{s}.{k}"])
            assert err.max() <= 2.1 * lr, f"post{s}.{k}: {err.max():.3e}"
            if not k.endswith("k_proj.bias"):
                assert (err <= 0.05 * lr).mean() >= 0.97, f"post{s}.{k}: tight fraction {(err <= 0.05 * lr).mean():.4f}"


# ============================================================================================ head_dim 16
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_head_dim_16_matches_float64_restatement(kind, precision):
    """hidden 64, 4 heads (materialised scores only), 3 layers, r = 0.5, the golden test's step-0 table, against the float64
    restatement.  Bounds of the golden test's unfrozen step."""
    model, cfg, ocfg, W = _model(kind, precision, model=R.SMALL, wseed=43)
    x, y = _batch(kind, ocfg, 420, R.BATCH)
    keep = R.golden_keep(0)
    model.drop_path_rate = R.RATE
    model.set_drop_path_masks(_table(keep))
    logits, loss, grads = _step(model, x, y)
    assert not model._ws.fused
    rl, rloss, rg = R.float64_step(W, x.cpu().numpy(), y.cpu().numpy(), ocfg, R.scales_of(keep, R.RATE))
    close(logits, rl, 1e-4, 1e-4, "logits")
    close(loss, rloss, 1e-4, 1e-4, "loss")
    _check_grads(grads, rg, f"{kind} {precision}")
    assert not grads[f"{cfg.prefix}.layers.2.mlp.fc2.weight"].any()


# ============================================================================================ generated tables
@pytest.mark.parametrize("precision", PRECISIONS)
def test_generated_tables_are_the_restatements(precision):
    model, cfg, ocfg, _ = _model("vit", precision, model=R.SMALL)
    B = 6
    x, y = _batch("vit", ocfg, 430, B)
    model.drop_path_rate = 0.5
    model.dropout_seed = 987654321
    seen = []
    for step in (1, 2):
        _step(model, x, y)
        assert model.forward_counter() == step
        last = model.last_drop_path().cpu().numpy()
        keep, scale = R.plan(3, B, 0.5, 987654321, step)
        assert np.array_equal(last, scale)
        gen = model.generated_drop_path(B, model.forward_counter())
        assert gen.dtype == torch.uint8 and tuple(gen.shape) == (3, 2, B)
        assert np.array_equal(gen.cpu().numpy(), keep) and np.array_equal(gen.cpu().numpy(), (last != 0).astype(np.uint8))
        seen.append(last)
    assert not np.array_equal(seen[0], seen[1])
    model.mix_dropout_rank(3)                                   # another replica, another table
    other = model.generated_drop_path(B, 1).cpu().numpy()
    assert np.array_equal(other, R.plan(3, B, 0.5, model.dropout_seed, 1)[0]) and not np.array_equal(other, seen[0] != 0)
    assert np.array_equal(model.generated_drop_path(B, 1, seed=987654321).cpu().numpy(), seen[0] != 0)
    model.eval()                                                # evaluation drops nothing and draws nothing
    with torch.no_grad():
        model(x)
    assert model.forward_counter() == 2
    with pytest.raises(_lib.EavError, match="last_drop_path"):
        model.last_drop_path()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_step_draws_a_fresh_table_per_replay(precision):
    """GraphStep over a head_dim-64 AST at 96 frames of a 256-frame checkpoint under drop_path_rate 0.5, built as
    test_patch_dropout_gpu.test_graph_step_draws_a_fresh_subset_per_replay: two eager steps, the capture, three replays.  Every
    step's table is the restatement's at its counter, the replays' differ, and the losses are those of a twin stepped eagerly
    under the same tables, bit for bit."""
    import copy
    from eav_amd import transformer as T
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    from eav_amd.runtime import GraphStep, eager_step, gather_batch
    from tests.ast_length_ref import clips
    torch.manual_seed(11)
    model = T.Encoder(T.make_config("ast", hidden=128, heads=2, ff=256, layers=3, frames=256))
    model.precision, model.overlap_wgrad, model.variable_length = precision, False, True
    with torch.no_grad():
        model.audio_spectrogram_transformer.embeddings.position_embeddings.normal_(0.0, 0.02)
    twin = copy.deepcopy(model)
    model, twin = model.cuda().train(), twin.cuda().train()
    model.drop_path_rate = twin.drop_path_rate = 0.5
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
        tables.append(model.last_drop_path())
        assert np.array_equal(tables[-1].cpu().numpy(), R.plan(3, 2, 0.5, 2468, s)[1]), s
    assert gs.graph is not None
    replays = [t.cpu().numpy() for t in tables[2:]]
    assert len(replays) == 3 and all(not np.array_equal(a, b) for i, a in enumerate(replays) for b in replays[i + 1:])
    for s, idx in enumerate(steps):
        twin.set_drop_path_masks((tables[s] != 0).to(torch.uint8))
        data, targets = gather_batch(xs, ys, torch.as_tensor(idx, dtype=torch.long, device=xs.device))
        want = eager_step(lambda d: twin(d).logits, topt, crit, data, targets)[1]
        torch.cuda.synchronize()
        assert torch.equal(got[s], want), (s, float(got[s]), float(want))
    assert torch.equal(model._flat[0], twin._flat[0])


# ============================================================================================ off means off
@pytest.mark.parametrize("precision", PRECISIONS)
def test_off_means_off(precision, monkeypatch):
    """drop_path_rate = 0 in training mode, 0.5 in eval mode and a model that never set the attribute launch the same list
    and give the same logits, bit for bit; with r > 0 in training mode layer 0 (p_0 = 0) contributes no eav_drop_path_add."""
    x = y = None
    runs = []
    for setup in ("zero", "eval", "untouched"):
        model, cfg, ocfg, _ = _model("vit", precision, model=R.SMALL)
        if x is None:
            x, y = _batch("vit", ocfg, 440, 2)
        if setup == "zero":
            model.drop_path_rate = 0.0
        elif setup == "eval":
            model.drop_path_rate = 0.5
            model.eval()
        names = _log_calls(monkeypatch)
        logits = _step(model, x, y)[0]
        monkeypatch.undo()
        runs.append((list(names), logits))
    assert runs[0][0] and not set(runs[0][0]) & set(PATH_LAUNCHES) and "eav_counter_inc" not in runs[0][0]
    assert runs[0][0] == runs[1][0] == runs[2][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])
    # ... and on: one counter step and one plan per forward, layers 1 and 2 take two adds in the forward and two gates in
    # the backward each, layer 0 none
    model, _, _, _ = _model("vit", precision, model=R.SMALL)
    model.drop_path_rate = 0.5
    names = _log_calls(monkeypatch)
    _step(model, x, y)
    monkeypatch.undo()
    assert names.count("eav_drop_path_plan") == 1 and names.count("eav_counter_inc") == 1
    assert names.count("eav_drop_path_add") == 2 * 2 * 2
    first_add = names.index("eav_drop_path_add")
    ln = "eav_layernorm_fwd_planes" if precision == "split" else "eav_layernorm_fwd"
    assert names[:first_add].count(ln) == 3                     # layer 0's two LayerNorms and layer 1's first: layer 0 is past
    # a one-layer model has p_0 = 0 only: nothing to launch
    one, _, _, _ = _model("vit", precision, model=dict(R.SMALL, layers=1))
    one.drop_path_rate = 0.5
    names = _log_calls(monkeypatch)
    _step(one, x, y)
    monkeypatch.undo()
    assert not set(names) & set(PATH_LAUNCHES) and "eav_counter_inc" not in names


# ============================================================================================ geometry combinations
def _geometry_case(kind, precision, x, y, keep, patch_keep=None, **attrs):
    """One step of a reduced (head_dim 16) model under the explicit table `keep` against the float64 restatement."""
    model, cfg, ocfg, W = _model(kind, precision, model=R.SMALL, wseed=44)
    for k, v in attrs.items():
        setattr(model, k, v)
    model.drop_path_rate = R.RATE
    model.set_drop_path_masks(_table(keep))
    if patch_keep is not None:
        model.set_patch_keep(torch.from_numpy(patch_keep).cuda())
    return model, cfg, ocfg, W, _step(model, x, y)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_with_patch_dropout(precision):
    """patch_dropout 0.5 on the ViT's 196 patches (98 kept) under an explicit keep table and explicit drop-path tables: the
    float64 restatement on the kept tokens; with both generators on, the counter advances by exactly 1 per forward."""
    B = R.BATCH
    x, y = _batch("vit", R.oracle_cfg("vit", R.SMALL), 450, B)
    pk = PK.plan(B, 196, 98, PK.plan_seed(5), 1)[0]
    keep = R.golden_keep(0)
    model, cfg, ocfg, W, (logits, loss, grads) = _geometry_case("vit", precision, x, y, keep, patch_keep=pk, patch_dropout=0.5)
    assert model._active_geo.ntok == 99 and model.forward_counter() == 0
    rows = torch.from_numpy(np.concatenate([np.zeros((B, 1), np.int64), 1 + pk.astype(np.int64)], 1))
    rl, rloss, rg = R.float64_step(W, x.cpu().numpy(), y.cpu().numpy(), ocfg, R.scales_of(keep, R.RATE), rows)
    close(logits, rl, 1e-4, 1e-4, "logits")
    close(loss, rloss, 1e-4, 1e-4, "loss")
    _check_grads(grads, rg, f"patch dropout {precision}")
    model.set_patch_keep(None)
    model.set_drop_path_masks(None)
    model.dropout_seed = 77
    for step in (1, 2):
        _step(model, x, y)
        assert model.forward_counter() == step
        assert np.array_equal(model.last_patch_keep().cpu().numpy(), PK.plan(B, 196, 98, PK.plan_seed(77), step)[0])
        assert np.array_equal(model.last_drop_path().cpu().numpy(), R.plan(3, B, R.RATE, 77, step)[1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_with_variable_length_and_interpolation(precision):
    """An AST clip of 96 frames on the 256-frame checkpoint (variable_length) and a ViT at 112 px (interpolate_pos_encoding):
    config dropout is refused at these geometries, drop path runs.  Logits, loss and gradients against the float64
    restatement at the fitted position table (tests/ast_length_ref.fit / tests/vit_interp_ref.resample; the table's gradient
    through their adjoints), bounds of the golden test's unfrozen step; every sample dropped in a branch keeps its hidden state
    there, checked through output_hidden_states bit for bit, and the gradients of a layer whose MLP branch is dropped for the
    whole batch are exactly zero."""
    from oracle import vit_oracle as vo
    from tests import ast_length_ref as AL, vit_interp_ref as VI
    from tests.ast_length_ref import clips
    fits = {"ast": (vo.cfg_ast(frames=96, **R.SMALL), lambda t: AL.fit(t, 12, 25, 9), lambda d: AL.fit_adjoint(d, 12, 25, 9)),
            "vit": (vo.cfg_vit(image=112, **R.SMALL), lambda t: VI.resample(t, 14, 7, 7), lambda d: VI.resample_adjoint(d, 14, 7, 7))}
    keep = R.golden_keep(0)
    xa, ya = clips(282, R.BATCH, 96)
    cases = [("ast", torch.from_numpy(xa).cuda(), torch.from_numpy(ya).cuda(), dict(variable_length=True), 2 + 12 * 9),
             ("vit", torch.from_numpy(synth.uniform(451, (R.BATCH, 3, 112, 112), -1.0, 1.0)).cuda(),
              torch.from_numpy(synth.labels(452, R.BATCH)).cuda(), dict(interpolate_pos_encoding=True), 1 + 49)]
    for kind, x, y, attrs, ntok in cases:
        model, cfg, ocfg, W, (logits, loss, grads) = _geometry_case(kind, precision, x, y, keep, **attrs)
        assert model._active_geo is not None and model._active_geo.ntok == ntok
        assert torch.isfinite(logits).all() and all(torch.isfinite(v).all() for v in grads.values())
        assert not grads[f"{cfg.prefix}.layers.2.mlp.fc1.weight"].any() and grads[f"{cfg.prefix}.layers.1.mlp.fc1.weight"].any()
        fcfg, fit, adjoint = fits[kind]
        key = f"{cfg.prefix}.embeddings.position_embeddings"
        Wf = dict(W)
        Wf[key] = fit(W[key][0])[None]
        assert Wf[key].shape[1] == ntok
        rl, rloss, rg = R.float64_step(Wf, x.cpu().numpy(), y.cpu().numpy(), fcfg, R.scales_of(keep, R.RATE))
        rg[key] = torch.from_numpy(adjoint(rg[key][0].numpy())[None])
        close(logits, rl, 1e-4, 1e-4, f"{kind} logits")
        close(loss, rloss, 1e-4, 1e-4, f"{kind} loss")
        _check_grads(grads, rg, f"{kind} {precision}")
        out = model(x, output_hidden_states=True)
        torch.cuda.synchronize()
        assert torch.equal(out.logits, logits)
        hs = out.hidden_states
        assert len(hs) == 4 and tuple(hs[0].shape) == (R.BATCH, ntok, 64)
        assert torch.equal(hs[2][1], hs[1][1])                  # sample 1: both branches of layer 1 dropped
        assert not torch.equal(hs[2][0], hs[1][0]) and not torch.equal(hs[1][1], hs[0][1])
        # an undropped twin differs exactly in the samples that dropped something
        plain, _, _, _ = _model(kind, precision, model=R.SMALL, wseed=44)
        for k, v in attrs.items():
            setattr(plain, k, v)
        ph = plain(x, output_hidden_states=True).hidden_states
        assert torch.equal(ph[1], hs[1])                        # layer 0 never drops


@pytest.mark.parametrize("precision", PRECISIONS)
def test_with_output_hidden_states_and_attentions(precision):
    """The extra outputs of a drop-path forward (head_dim 64: csrc/attn_probs.hip): the logits and gradients are those of the
    forward without the flags, and a sample dropped in both branches of layer i has hidden[i + 1][b] bit-equal to
    hidden[i][b]."""
    model, cfg, ocfg, _ = _model("vit", precision)
    x, y = _batch("vit", ocfg, 460, R.BATCH)
    keep = R.golden_keep(0)
    keep[2, 0, 3] = 0                                           # sample 3: both branches of layer 2 (its MLP drops for everybody)
    model.drop_path_rate = R.RATE
    model.set_drop_path_masks(_table(keep))
    plain = _step(model, x, y)
    flagged = _step(model, x, y, output_hidden_states=True, output_attentions=True)
    assert torch.equal(flagged[0], plain[0]) and all(torch.equal(flagged[2][k], plain[2][k]) for k in plain[2])
    out = model(x, output_hidden_states=True, output_attentions=True)
    torch.cuda.synchronize()
    hs = out.hidden_states
    assert len(hs) == 4 and len(out.attentions) == 3
    assert torch.equal(hs[2][1], hs[1][1]) and torch.equal(hs[3][3], hs[2][3])
    assert not torch.equal(hs[2][0], hs[1][0]) and not torch.equal(hs[3][0], hs[2][0])
    for a in out.attentions:
        close(a.sum(-1), np.ones((R.BATCH, 2, cfg.ntok)), 0.0, 1e-5, "attention rows")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_grad_ready_hook_and_head_only_backward(precision):
    """grad_ready_hook sees every layer's slice once, top down, with the gradients of the hook-less step; a head-only
    (frozen) step gates its forward and launches no gate in its backward."""
    model, cfg, ocfg, _ = _model("vit", precision, model=R.SMALL)
    x, y = _batch("vit", ocfg, 470, R.BATCH)
    model.drop_path_rate = R.RATE
    model.set_drop_path_masks(_table(R.golden_keep(0)))
    plain = _step(model, x, y)
    seen = []
    model.grad_ready_hook = lambda lo, hi: seen.append((lo, hi))
    hooked = _step(model, x, y)
    model.grad_ready_hook = None
    assert len(seen) == 3 and seen == sorted(seen, reverse=True)
    assert all(torch.equal(hooked[2][k], plain[2][k]) for k in plain[2])
    for k, p in model.named_parameters():
        p.requires_grad = k.startswith("classifier.")
    names = []
    real = _lib.call
    try:
        _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
        from eav_amd.optim import CrossEntropyLoss
        out = model(x)
        CrossEntropyLoss()(out.logits, y).backward()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    assert names.count("eav_drop_path_plan") == 1 and names.count("eav_drop_path_add") == 4
    close(out.logits, plain[0], 1e-4, 1e-4, "head-only logits")          # (another workspace, the same forward)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for k, p in model.named_parameters() if k.startswith("classifier."))


# ============================================================================================ refusals
def test_refusals_on_the_device():
    model, cfg, ocfg, _ = _model("vit", "split", model=R.SMALL)
    x, y = _batch("vit", ocfg, 480, R.BATCH)
    for bad in (1.0, -0.1, 1.5):
        model.drop_path_rate = bad
        with pytest.raises(ValueError, match="drop_path_rate"):
            model(x)
        model.eval()                                            # the rate is validated whatever the mode
        with pytest.raises(ValueError, match="drop_path_rate"):
            model(x)
        model.train()
    model.drop_path_rate = R.RATE
    good = R.golden_keep(0)
    for bad in (torch.from_numpy(good), _table(good).float(), _table(good[:2]), _table(good[:, :1])):   # device, dtype, L, branches
        with pytest.raises(ValueError, match="set_drop_path_masks"):
            model.set_drop_path_masks(bad)
    model.set_drop_path_masks(_table(good[:, :, :3]))           # another B: the forward that meets it refuses
    with pytest.raises(ValueError, match="set_drop_path_masks"):
        model(x)
    model.set_drop_path_masks(_table(good))
    assert model(x).logits.shape == (R.BATCH, 5)
    model.set_drop_path_masks(None)                             # back to generated tables
    model(x)
    assert model.forward_counter() == 1
    dropping, _, _, _ = _model("vit", "split", model=R.SMALL, hidden_dropout=0.1)
    dropping.drop_path_rate = 0.2
    with pytest.raises(NotImplementedError, match="drop path"):
        dropping(x)
    dropping.eval()                                             # nothing drops in eval mode
    with torch.no_grad():
        assert dropping(x).logits.shape == (R.BATCH, 5)
    dropping.train()
    dropping.drop_path_rate = 0.0                               # config dropout alone is what it was
    assert dropping(x).logits.shape == (R.BATCH, 5) and dropping.forward_counter() == 1


# ============================================================================================ trainer, command line
def test_trainer_drops_paths_in_unfrozen_epochs_only(tmp_path, monkeypatch):
    from eav_amd.audio import AudioModelTrainer
    from tests.test_patch_dropout_gpu import _save_model_dir
    path = _save_model_dir(tmp_path / "model")
    monkeypatch.chdir(tmp_path)
    wav = synth.normal(295, (12, 8000), 0.0, 0.1)
    y = synth.labels(296, 12)
    data = [wav[:8], y[:8], wav[8:], y[8:]]
    frozen = []
    with redirect_stdout(io.StringIO()):
        for r in (0.2, None):
            torch.manual_seed(0)
            tr = AudioModelTrainer(data, path, sub="s", num_classes=5, batch_size=4, max_length="auto")
            if r is not None:
                tr.drop_path = r
            names = _log_calls(monkeypatch)
            tr.train(epochs=1, lr=5e-4, freeze=True)
            monkeypatch.undo()
            monkeypatch.chdir(tmp_path)
            frozen.append(list(names))
            if r is not None:
                kept = tr
    assert frozen[0] and frozen[0] == frozen[1] and not set(frozen[0]) & set(PATH_LAUNCHES)
    tr = kept
    assert tr.model.drop_path_rate == 0.0
    with redirect_stdout(io.StringIO()):
        names = _log_calls(monkeypatch)
        tr.train(epochs=1, lr=5e-6, freeze=False)
        monkeypatch.undo()
        monkeypatch.chdir(tmp_path)
        unfrozen = list(names)
        names = _log_calls(monkeypatch)
        tr._evaluate()
        monkeypatch.undo()
        monkeypatch.chdir(tmp_path)
        evaluate = list(names)
    # two training batches: one plan each, layer 1 of the 2 layers gates twice forward and twice backward
    assert unfrozen.count("eav_drop_path_plan") == 2 and unfrozen.count("eav_drop_path_add") == 2 * 4
    assert tr.model.forward_counter() == 2 and tr.model.drop_path_rate == 0.2
    assert evaluate and not set(evaluate) & set(PATH_LAUNCHES)
    assert tr.outputs_test.shape == (4, 5) and np.isfinite(tr.outputs_test).all()
    tr.drop_path = 1.0
    with pytest.raises(ValueError, match="drop_path"):
        tr.train(epochs=1, lr=5e-6, freeze=False)


def test_drop_path_option_reaches_the_trainer(monkeypatch, capsys):
    """tools/run_finetune_subjects.py --drop-path R sets trainer.drop_path before both phases (a recording trainer stands in
    for the real one: no model runs); a rate outside [0, 1) ends at argparse."""
    import eav_amd.audio as audio
    spec = importlib.util.spec_from_file_location("run_finetune_subjects_dp", os.path.join(ROOT, "tools", "run_finetune_subjects.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    seen = []

    class Recorder:
        drop_path = patch_dropout = None

        def __init__(self, data, **kw):
            self.outputs_test = np.zeros((len(data[3]), 5), np.float32)

        def train(self, epochs, lr, freeze):
            seen.append((freeze, self.drop_path, self.patch_dropout))

    monkeypatch.setattr(audio, "AudioModelTrainer", Recorder)
    monkeypatch.setattr(tool, "synthetic_subject", lambda kind, sub, small: [np.zeros((4, 8), np.float32), np.zeros(4, np.int64)] * 2)
    monkeypatch.setattr(sys, "argv", ["run_finetune_subjects.py", "audio", "--subjects", "1", "--small", "--model-path", "unused",
                                      "--drop-path", "0.2"])
    tool.main()
    assert seen == [(True, 0.2, 0.0), (False, 0.2, 0.0)]
    assert '"subjects": 1' in capsys.readouterr().out
    monkeypatch.setattr(sys, "argv", ["run_finetune_subjects.py", "audio", "--drop-path", "1.0"])
    with pytest.raises(SystemExit):
        tool.main()
