"""Global-norm clipping and gradient accumulation at the optimiser level: FusedAdam(max_grad_norm=...), accumulate(),
clip_grad_norm_, a captured step, the Encoder against the oracle and the vision trainer.

Reference: tests/grad_clip_ref.py in float64 (pinned to torch by tests/test_grad_clip_cpu.py).  The hyper-parameters are
given as fp32-representable values (the kernels take them as C floats), so kernel and reference start from identical
inputs; p, exp_avg and exp_avg_sq are then plain fp32 element-wise chains: rtol 1e-6 + atol 1e-9 (lr 1e-3: the update's own
rounding, ~lr 2^-22, stays under the floor).  The norm bound is the kernel tests' 4 * 2^-23.

exp_avg alone has the floor 1.42e-8 instead of 1e-9.  From the second step on b1 * m and (1 - b1) * g can cancel, and the
rounding of a sum is relative to its terms (~0.03 here: 2^-24 * 0.03 = 1.8e-9 per rounding), not to the result, which
rtol * |result| + 1e-9 does not allow for.  Measured: 3.545e-9 at such an element (1.23 x the 1e-9 form; every p and
exp_avg_sq comparison, and every first step, stays inside rtol 1e-6 + atol 1e-9); the floor is 4 x that measurement
(DESIGN.md section 4.8)."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import grad_clip_ref as R
from tests import problem_type_ref as ptr
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (7,), (3, 5), (129,)]
LR, B1, B2, EPS_ADAM, WD = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8, 0.01))
EPS = 2.0 ** -23
M_ATOL = 4 * 3.545e-9            # exp_avg (module docstring)


class _Loose:
    """Four device tensors (`flat`: as a module put through flatten_parameters, p.grad = the views of its flat gradient
    buffer, the way every KernelModule hands its gradients out)."""

    def __init__(self, flat, seed=1):
        from eav_amd.optim import flatten_parameters
        self.host = [synth.normal(seed + i, s).astype(np.float32) for i, s in enumerate(SHAPES)]
        self.params = [torch.nn.Parameter(torch.from_numpy(h.copy()).cuda()) for h in self.host]
        self.gflat = None
        if flat:
            self.module = torch.nn.Module()
            for i, p in enumerate(self.params):
                self.module.register_parameter(f"w{i}", p)
            _, self.gflat, self.offsets = flatten_parameters(self.module)

    def set_grads(self, grads):
        for i, (p, g) in enumerate(zip(self.params, grads)):
            g = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
            if self.gflat is None:
                p.grad = g
            else:
                off, n = self.offsets[f"w{i}"]
                view = self.gflat[off:off + n].view(p.shape)
                view.copy_(g)
                p.grad = view

    def optimizer(self, **kw):
        from eav_amd.optim import FusedAdam
        kw.setdefault("weight_decay", WD)
        kw.setdefault("decoupled", True)
        return FusedAdam(self.params, lr=LR, betas=(B1, B2), eps=EPS_ADAM, **kw)


def _grads(seed, gain):
    return [synth.normal(seed + i, s).astype(np.float32) * np.float32(gain) for i, s in enumerate(SHAPES)]


def _close(got, ref, what, rtol=1e-6, atol=1e-9):
    got = got.detach().cpu().double().numpy()
    err = np.abs(got - ref)
    lim = atol + rtol * np.abs(ref)
    print(f"{what}: max error {err.max():.3e}, worst error / bound {(err / lim).max():.3f}")
    assert (err <= lim).all(), (what, float(err.max()))


def _state_close(opt, params, ref, what):
    for i, p in enumerate(params):
        _close(p, ref.p[i], f"{what} p{i}")
        _close(opt.state[p]["exp_avg"], ref.m[i], f"{what} exp_avg{i}", atol=M_ATOL)
        _close(opt.state[p]["exp_avg_sq"], ref.v[i], f"{what} exp_avg_sq{i}", atol=1e-12)


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("flat", [False, True])
def test_clipped_steps_match_the_reference(flat, decoupled):
    """Three steps with max_grad_norm = 1: norms ~12, ~3.7 (clipped) and ~0.12 (not clipped)."""
    t = _Loose(flat)
    opt = t.optimizer(max_grad_norm=1.0, decoupled=decoupled)
    ref = R.Stepper(t.host, LR, WD, decoupled, 1.0, (B1, B2), EPS_ADAM)
    for s, gain in enumerate((1.0, 0.3, 0.01)):
        grads = _grads(100 + 10 * s, gain)
        t.set_grads(grads)
        before = [p.grad.clone() for p in t.params]
        opt.step()
        ref.step(grads)
        torch.cuda.synchronize()
        norm = float(opt.last_grad_norm)
        assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda
        assert abs(norm - ref.last_norm) <= R.NORM_RTOL * ref.last_norm, (s, norm, ref.last_norm)
        assert (ref.last_norm > 1.0) == (s < 2)
        for p, b in zip(t.params, before):                         # p.grad is left unscaled
            assert torch.equal(p.grad.view(torch.int32), b.view(torch.int32))
        _state_close(opt, t.params, ref, f"flat={flat} decoupled={decoupled} step {s}")
        assert all(opt.state[p]["step"] == s + 1 for p in t.params)


def test_infinite_bound_measures_and_clips_nothing():
    a, b = _Loose(True), _Loose(True)
    oa, ob = a.optimizer(max_grad_norm=float("inf")), b.optimizer()
    grads = _grads(7, 1.0)
    a.set_grads(grads)
    b.set_grads(grads)
    oa.step()
    ob.step()
    assert abs(float(oa.last_grad_norm) - R.global_norm(grads)) <= R.NORM_RTOL * R.global_norm(grads)
    assert ob.last_grad_norm is None
    for p, q in zip(a.params, b.params):                           # coefficient exactly 1: the same bits
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))


@pytest.mark.parametrize("capturable", [False, True])
def test_off_means_unchanged(capturable, monkeypatch):
    """A default FusedAdam step launches what it launched before the options existed."""
    t = _Loose(True)
    opt = t.optimizer(capturable=capturable)
    t.set_grads(_grads(3, 1.0))
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    opt.step()
    opt.step()
    want = (["eav_counter_inc"] if capturable else []) + ["eav_adam_step"]
    assert names == want * 2, names
    names.clear()
    opt.max_grad_norm = 1.0                                        # and with it on: two more launches, one scaled update
    opt.step()
    assert names == want[:-1] + ["eav_grad_sumsq", "eav_grad_clip_finish", "eav_adam_step_scaled"], names


def test_clip_grad_norm_is_torchs():
    from eav_amd.optim import clip_grad_norm_
    for flat in (False, True):
        for max_norm in (1.0, 1e3):
            t = _Loose(flat)
            grads = _grads(11, 1.0)
            t.set_grads(grads)
            cpu = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in SHAPES]
            for c, g in zip(cpu, grads):
                c.grad = torch.from_numpy(g.astype(np.float64))
            want = float(torch.nn.utils.clip_grad_norm_(cpu, max_norm))
            got = clip_grad_norm_(t.params, max_norm)
            assert got.dim() == 0 and got.is_cuda
            assert abs(float(got) - want) <= R.NORM_RTOL * want
            for p, c in zip(t.params, cpu):
                _close(p.grad, c.grad.numpy(), f"flat={flat} max_norm={max_norm} scaled gradient", atol=0.0)
            if max_norm == 1e3:                                    # not clipped: the gradients keep their bits
                for p, g in zip(t.params, grads):
                    assert np.array_equal(p.grad.cpu().numpy(), g)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(t.params, 1.0, norm_type=1)
    with pytest.raises(_lib.EavError, match="max_norm"):
        clip_grad_norm_(t.params, 0.0)


def test_captured_step_clips_the_replayed_gradients():
    t = _Loose(True)
    opt = t.optimizer(capturable=True, max_grad_norm=0.5)
    ref = R.Stepper(t.host, LR, WD, True, 0.5, (B1, B2), EPS_ADAM)
    g1, g2 = _grads(21, 1.0), _grads(31, 0.2)                      # norms ~12 and ~2.5
    t.set_grads(g1)
    for _ in range(2):                                             # eager warm-up steps, as GraphStep takes them
        opt.step()
        ref.step(g1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    t.set_grads(g2)                                                # the same buffer, other values
    graph.replay()
    ref.step(g2)
    torch.cuda.synchronize()
    assert abs(float(opt.last_grad_norm) - ref.last_norm) <= R.NORM_RTOL * ref.last_norm
    assert abs(ref.last_norm - R.global_norm(g2)) < 1e-12 and abs(R.global_norm(g1) / R.global_norm(g2) - 1) > 0.5
    assert int(opt.device_step_counter()) == 3
    for i, p in enumerate(t.params):
        _close(p, ref.p[i], f"captured p{i}")
        _close(opt.state[p]["exp_avg"], ref.m[i], f"captured exp_avg{i}", atol=M_ATOL)
    with pytest.raises(_lib.EavError, match="capturable"):
        opt.accumulate()


@pytest.mark.parametrize("flat", [False, True])
def test_accumulation(flat):
    """Two groups of three folds (weights 2/8, 2/8, 4/8); optimiser `a` lets the last fold form the norm partials,
    `b` leaves the norm to step()."""
    ta, tb = _Loose(flat), _Loose(flat)
    oa, ob = ta.optimizer(max_grad_norm=1.0), tb.optimizer(max_grad_norm=1.0)
    ref = R.Stepper(ta.host, LR, WD, True, 1.0, (B1, B2), EPS_ADAM)
    weights = (0.25, 0.25, 0.5)
    for group in range(2):
        gs = [_grads(200 + 100 * group + 10 * j, 0.5) for j in range(3)]
        if group == 1:                                             # the first fold of a group does not read the accumulator
            for t, o in ((ta, oa), (tb, ob)):
                for p in t.params:
                    o.accumulated_grad(p).fill_(float("nan"))
        for j, (w, g) in enumerate(zip(weights, gs)):
            ta.set_grads(g)
            tb.set_grads(g)
            oa.accumulate(w, last=j == 2)
            ob.accumulate(w)
        acc = []
        for i, p in enumerate(ta.params):
            got = oa.accumulated_grad(p)
            assert got.shape == p.shape and not torch.isnan(got).any()
            assert torch.equal(got.view(torch.int32), ob.accumulated_grad(tb.params[i]).view(torch.int32))
            terms = [np.abs(np.float64(w) * g[i].astype(np.float64)) for w, g in zip(weights, gs)]
            want = sum(np.float64(w) * g[i].astype(np.float64) for w, g in zip(weights, gs))
            bound = EPS * (terms[0] + (terms[0] + terms[1]) + (terms[0] + terms[1] + terms[2])) * (1 + 1e-6)
            got = got.cpu().double().numpy()
            assert (np.abs(got - want) <= bound).all(), (group, i, float(np.abs(got - want).max()))
            acc.append(got)
        oa.step()
        ob.step()
        ref.step(acc)                      # the update from the accumulated values (just held to the weighted sum)
        torch.cuda.synchronize()
        assert abs(float(oa.last_grad_norm) - ref.last_norm) <= R.NORM_RTOL * ref.last_norm and ref.last_norm > 1.0
        assert torch.equal(oa.last_grad_norm.view(torch.int32), ob.last_grad_norm.view(torch.int32))
        _state_close(oa, ta.params, ref, f"flat={flat} group {group}")
        for p, q in zip(ta.params, tb.params):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32))
        assert all(oa.state[p]["step"] == group + 1 for p in ta.params)
    # a step with nothing accumulated behaves as before: it consumes p.grad
    g = _grads(900, 0.01)
    ta.set_grads(g)
    oa.step()
    ref.step(g)
    _state_close(oa, ta.params, ref, f"flat={flat} plain step after the groups")
    # the parameters with a gradient may not change inside a group
    ta.set_grads(g)
    oa.accumulate(0.5)
    ta.params[1].requires_grad_(False)
    ta.params[1].grad = None
    with pytest.raises(_lib.EavError, match="differ"):
        oa.accumulate(0.5)


# ------------------------------------------------------------------------------------------------------------ Encoder
REDUCED = dict(hidden=64, layers=2, heads=4, ff=128)


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_encoder_accumulates_and_clips_like_the_oracle_on_the_whole_batch(precision):
    """A batch of 4 as two micro-batches of 2 folded with weight 0.5 each, max_grad_norm = half the oracle's norm, AdamW:
    accumulator, norm and first moment against the oracle's gradients of the whole batch (float64 clipping arithmetic).
    Bounds: the gradient bound of tests/test_problem_type_gpu.py (1e-3 of the tensor's maximum), 1e-3 on the norm, and
    moments_close's rule at rel_m = 3e-3 (test_adam_moments_encoder)."""
    from eav_amd import transformer as T
    from eav_amd.optim import FusedAdam
    from oracle import vit_oracle as vo
    NC = 2
    ocfg = vo.cfg_vit(num_labels=NC, **REDUCED)
    W = tf_weights(61, vo.param_shapes(ocfg), std=0.05)
    x = synth.frame_batch(63, 4, 224)[0]
    y = synth.normal(65, (4, NC)).astype(np.float32)
    _, _, gref = ptr.step_reference({k: v.astype(np.float64) for k, v in W.items()}, ocfg, x.astype(np.float64),
                                    y.astype(np.float64), "regression", False)         # the oracle in float64
    gref = {k: g.numpy() for k, g in gref.items()}
    assert all(g.dtype == np.float64 for g in gref.values())
    norm_ref = R.global_norm(gref.values())
    max_norm = 0.5 * norm_ref
    coef_ref = R.clip_coef(norm_ref, max_norm)
    model = T.Encoder(T.make_config("vit", num_labels=NC, problem_type="regression", hidden_dropout=0.0,
                                    attention_dropout=0.0, **REDUCED), W).cuda().train()
    model.precision = precision
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=0.01, decoupled=True, max_grad_norm=max_norm)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for j in range(2):
        opt.zero_grad()
        model(xd[2 * j:2 * j + 2], labels=yd[2 * j:2 * j + 2]).loss.backward()
        opt.accumulate(0.5, last=j == 1)
    named = dict(model.named_parameters())
    assert sorted(named) == sorted(gref)
    for k, g in gref.items():
        if k.endswith("k_proj.bias"):                 # analytically zero gradient: rounding noise only
            continue
        got = opt.accumulated_grad(named[k])
        _close(got, g, f"{precision} accumulated {k}", rtol=1e-3, atol=max(1e-3 * np.abs(g).max(), 1e-6))
    opt.step()
    torch.cuda.synchronize()
    norm = float(opt.last_grad_norm)
    print(f"{precision}: norm {norm:.6e}, oracle {norm_ref:.6e}")
    assert abs(norm - norm_ref) <= 1e-3 * norm_ref
    for k, g in gref.items():
        if k.endswith("k_proj.bias"):
            continue
        rm = 0.1 * coef_ref * g
        m = opt.state[named[k]]["exp_avg"].cpu().double().numpy()
        assert np.abs(m - rm).max() <= 3e-3 * np.abs(rm).max() + 1e-12, (k, float(np.abs(m - rm).max()))
        assert opt.state[named[k]]["step"] == 1


# ------------------------------------------------------------------------------------------------------------ trainer
def _save_model_dir(path, seed):
    """HF-format directory of the reduced ViT (five labels, as the stock fine-tuning checkpoints are laid out)."""
    from safetensors.numpy import save_file
    from oracle import vit_oracle as vo
    path.mkdir()
    ocfg = vo.cfg_vit(**REDUCED)
    W = tf_weights(seed, vo.param_shapes(ocfg), std=0.08)
    save_file({k: np.ascontiguousarray(v) for k, v in W.items()}, str(path / "model.safetensors"))
    cfg = {"hidden_size": 64, "num_hidden_layers": 2, "num_attention_heads": 4, "intermediate_size": 128,
           "patch_size": 16, "layer_norm_eps": 1e-12, "hidden_act": "gelu",
           "id2label": {str(i): f"LABEL_{i}" for i in range(5)}, "model_type": "vit", "image_size": 224, "num_channels": 3}
    json.dump({"do_normalize": True, "do_rescale": True, "do_resize": True, "image_mean": [0.5, 0.5, 0.5],
               "image_std": [0.5, 0.5, 0.5], "image_processor_type": "ViTImageProcessor", "resample": 2,
               "rescale_factor": 1 / 255, "size": {"height": 224, "width": 224}},
              open(path / "preprocessor_config.json", "w"))
    json.dump(cfg, open(path / "config.json", "w"))
    return str(path)


def test_vision_trainer_accumulating_matches_the_large_batch_run(tmp_path, monkeypatch):
    """18 training frames in one unfrozen epoch: batches of 8 (8, 8, 2) against batches of 4 accumulated in pairs
    (4 + 4, 4 + 4, 2) in the same sample order - the same three updates, so outputs_test agrees within the 1e-3 of
    tests/test_transformer_trainers_gpu.py; then the accumulating run with a tight max_grad_norm."""
    from eav_amd.vision import ImageClassifierTrainer
    path = _save_model_dir(tmp_path / "model", 9)
    monkeypatch.chdir(tmp_path)
    x = (synth.uniform(85, (8, 3, 56, 56, 3)) * 255).astype(np.uint8)          # three frames per item: 18 + 6 frames
    y = synth.labels(86, 8)
    head_w, head_b = synth.normal(82, (5, 64), 0.0, 0.05), synth.normal(83, (5,), 0.0, 0.02)
    order = [int(i) for i in np.argsort(synth.uniform(87, (18,)))]

    def run(batch_size, accum, max_grad_norm):
        with redirect_stdout(io.StringIO()):
            tr = ImageClassifierTrainer([x[:6], y[:6], x[6:], y[6:]], path, sub="s", num_labels=5, batch_size=batch_size)
            tr.model.precision = "fp32"
            tr.cache_frozen_features = False
            tr.gradient_accumulation_steps, tr.max_grad_norm = accum, max_grad_norm
            tr.model.reset_head(head_w, head_b)
            tr.optimizer = type(tr.optimizer)(tr.model.parameters(), lr=tr.initial_lr, weight_decay=0.01, decoupled=True)
            assert len(tr.train_dataloader.dataset) == 18 and len(tr.test_dataloader.dataset) == 6
            tr.train_dataloader.order_override = [list(order)]
            tr.train(epochs=1, lr=5e-6, freeze=False)
        steps = {int(tr.optimizer.state[p]["step"]) for p in tr.model.parameters()}
        assert steps == {3}, steps
        assert tr.optimizer.max_grad_norm == max_grad_norm
        return tr.outputs_test

    a = run(8, 1, None)
    b = run(4, 2, None)
    assert a.shape == b.shape == (6, 5)
    err = float(np.abs(a - b).max())
    print(f"max |outputs_test(4 x 2) - outputs_test(8)| = {err:.3e} (max |outputs_test| {np.abs(a).max():.3e})")
    assert err < 1e-3, err
    c = run(4, 2, 1e-3)
    assert np.isfinite(c).all() and not np.array_equal(c, a) and not np.array_equal(c, b)
