"""The learning-rate options of AudioModelTrainer / ImageClassifierTrainer (finetune.FineTuneBase: lr_scheduler_type,
warmup_ratio, layer_decay, decay_bias_and_norm) on the 2-layer, 64-wide AST / ViT directories of
test_transformer_trainers_gpu: 6 training items in batches of 4.

With the options on, every optimiser step is held to torch.optim.AdamW on the CPU in float64 with the same param groups
and a LambdaLR over optim.LRSchedule.factor, fed the gradients the device step consumed (copied back before each step;
the hyper-parameters rounded to fp32 as the kernels receive them), within the compounded bounds of tests/adam_jobs_ref.py."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import _lib
from tests import adam_jobs_ref as A
from tests.test_finetune_regularisers_gpu import _trainer
from tests.test_transformer_trainers_gpu import _save_model_dir

pytestmark = pytest.mark.gpu

KINDS = ["ast", "vit"]
NEW = ("eav_adam_jobs_begin", "eav_adam_step_jobs")
B1, B2, EPS_ADAM, WD = (float(np.float32(v)) for v in (0.9, 0.999, 1e-8, 0.01))


@pytest.fixture
def path(kind, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                     # the trainers append to log files in the cwd
    return _save_model_dir(tmp_path, kind, 5)


def _train(tr, epochs, lr, freeze):
    out = io.StringIO()
    with redirect_stdout(out):
        tr.train(epochs=epochs, lr=lr, freeze=freeze)
    return out.getvalue()


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_launch_what_they_always_did(kind, path, monkeypatch):
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    runs = []
    for explicit in (False, True):
        tr = _trainer(kind, path)
        if explicit:                                # the defaults spelled out: the same thing as leaving them alone
            tr.lr_scheduler_type, tr.warmup_ratio, tr.layer_decay, tr.decay_bias_and_norm = "constant", 0.0, 1.0, True
        names.clear()
        text = _train(tr, 1, 5e-4, True) + _train(tr, 1, 5e-6, False)
        assert not tr.optimizer.multi_tensor and tr.optimizer.schedule is None and len(tr.optimizer.param_groups) == 1
        assert ", lr " not in text
        runs.append(list(names))
    assert runs[0] == runs[1]
    assert not set(NEW) & set(runs[0]) and runs[0].count("eav_adam_step") >= 4         # 2 + 2 steps, one launch per run


def _hook_steps(tr, expected_groups, names):
    """Wrap tr.optimizer.step: before each step copy the gradients it will consume, after it drive the CPU reference."""
    opt = tr.optimizer
    named = dict(tr.model.named_parameters())
    cpu = {k: torch.nn.Parameter(p.detach().cpu().double().clone()) for k, p in named.items()}
    traj = {}
    log = {"lrs": [], "steps": 0, "cpu": cpu, "traj": traj, "new_calls": []}
    real_step = opt.step

    def step():
        if log["steps"] == 0:
            got = [(g["names"], g["lr"], g["weight_decay"]) for g in opt.param_groups]
            assert got == [(g["names"], g["lr"], g["weight_decay"]) for g in expected_groups]
            log["ref_opt"] = torch.optim.AdamW(
                [{"params": [cpu[n] for n in g["names"]], "lr": g["lr"], "weight_decay": WD if g["weight_decay"] else 0.0}
                 for g in expected_groups], betas=(B1, B2), eps=EPS_ADAM, foreach=False)
            log["ref_sched"] = torch.optim.lr_scheduler.LambdaLR(log["ref_opt"], opt.schedule.factor)
            for g in expected_groups:
                for n in g["names"]:
                    traj[n] = (A.Trajectory(cpu[n].detach().numpy().reshape(-1), g["weight_decay"], True, (B1, B2), EPS_ADAM),
                               g["lr"])
        grads = {}
        for n, p in named.items():
            g = opt.accumulated_grad(p) if opt._acc_folds else p.grad
            grads[n] = None if g is None else g.detach().cpu().double().clone()
        before = len(names)
        real_step()
        log["new_calls"].append([x for x in names[before:] if x.startswith("eav_adam")])
        log["lrs"].append(opt.last_lr.cpu().numpy().copy())
        factor = opt.schedule.factor(log["steps"])
        for n, g in grads.items():
            cpu[n].grad = g
            if g is not None:
                traj[n][0].step(g.numpy().reshape(-1), A.lr_f32(traj[n][1], factor))
        log["ref_opt"].step()
        log["ref_sched"].step()
        log["steps"] += 1

    opt.step = step
    return log


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k_acc", [1, 2])
def test_options_on_follow_torch_adamw_with_the_same_groups(kind, k_acc, path, monkeypatch):
    from eav_amd.finetune import encoder_param_groups
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    epochs, lr = 2, 1e-3
    tr = _trainer(kind, path, lr_scheduler_type="linear", warmup_ratio=0.25, layer_decay=0.75, decay_bias_and_norm=False,
                  gradient_accumulation_steps=k_acc)
    expected = encoder_param_groups(tr.model, lr, 0.01, 0.75, False)
    log = _hook_steps(tr, expected, names)
    text = _train(tr, epochs, lr, False)
    torch.cuda.synchronize()
    per_epoch = -(-2 // k_acc)                      # 6 items in batches of 4: two micro-batches
    total = epochs * per_epoch
    assert log["steps"] == total
    sch = tr.optimizer.schedule
    assert (sch.kind, sch.num_training_steps, sch.num_warmup_steps) == ("linear", total, int(np.ceil(0.25 * total)))
    assert all(calls == list(NEW) for calls in log["new_calls"]), log["new_calls"]       # exactly two launches per step
    assert "eav_adam_step" not in names and "eav_adam_step_scaled" not in names
    for t, got in enumerate(log["lrs"]):
        want = A.lr_f32(tr.optimizer.param_groups[0]["lr"], sch.factor(t))
        assert got.view(np.int32) == want.view(np.int32), (t, got, want)
    assert float(log["lrs"][0]) == 0.0 and any(float(x) > 0.0 for x in log["lrs"])
    assert text.count(", lr ") == epochs            # the epoch line carries the last rate
    assert np.isfinite(tr.outputs_test).all() and tr.outputs_test.shape[1] == 5
    moved = 0
    for n, p in tr.model.named_parameters():
        ref, (tj, _) = log["cpu"][n].detach().numpy().reshape(-1), log["traj"][n]
        # the two float64 references differ in the rate alone: torch's is base * factor in double, the trajectory's that
        # product rounded to fp32 as the kernel receives it (2^-24 of each step's change, inside the bound's 16 EPS D)
        np.testing.assert_allclose(tj.p, ref, rtol=1e-6, atol=1e-9)
        st = tr.optimizer.state[p]
        err = np.abs(p.detach().cpu().double().numpy().reshape(-1) - ref)
        assert np.all(err <= tj.tol_p), (n, float(np.max(err / tj.tol_p)))
        tj.check(p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), n)
        moved += int(tj.steps > 0)
    assert moved == len(log["cpu"])
    # the options taken back: one group, no schedule, the default path again
    tr.lr_scheduler_type, tr.layer_decay, tr.decay_bias_and_norm = "constant", 1.0, True
    names.clear()
    del tr.optimizer.step                           # the wrapper of _hook_steps
    _train(tr, 1, 1e-4, False)
    assert len(tr.optimizer.param_groups) == 1 and tr.optimizer.param_groups[0]["weight_decay"] == 0.01
    assert not tr.optimizer.multi_tensor and not set(NEW) & set(names) and "eav_adam_step" in names
