"""The weight-averaging options of AudioModelTrainer / ImageClassifierTrainer (finetune.FineTuneBase: weight_averaging,
ema_decay, ...) on the 2-layer, 64-wide AST / ViT directories of test_transformer_trainers_gpu: 6 training items in
batches of 4, a frozen phase (feature cache) and an unfrozen one, in fp32 precision, where cached and recomputed features
and two models with the same weights agree bit for bit."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import _lib
from tests.test_finetune_regularisers_gpu import _trainer
from tests.test_transformer_trainers_gpu import _save_model_dir

pytestmark = pytest.mark.gpu

KINDS = ["ast", "vit"]
AVG = ("eav_adam_jobs_begin_avg", "eav_adam_step_jobs_avg")


@pytest.fixture
def path(kind, tmp_path, monkeypatch):
    monkeypatch.setenv("EAV_ENCODER_PRECISION", "fp32")
    monkeypatch.chdir(tmp_path)                     # the trainers append to log files in the cwd
    return _save_model_dir(tmp_path, kind, 5)


def _train(tr, epochs, lr, freeze):
    with redirect_stdout(io.StringIO()):
        tr.train(epochs=epochs, lr=lr, freeze=freeze)


def _test_logits(tr, directory):
    """The test split through a fresh Encoder loaded from `directory`, in the trainer's own batches."""
    from eav_amd.transformer import Encoder
    model = Encoder.from_pretrained(directory).to(tr.device).eval()
    dl, out = tr.test_dataloader, []
    with torch.no_grad():
        for idx in dl.index_batches():
            xb, _ = dl.gather(idx)
            out.append(model(xb).logits.cpu().numpy())
    return np.concatenate(out, axis=0), {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("kind", KINDS)
def test_ema_is_evaluated_and_saved_and_does_not_perturb_training(kind, path, tmp_path, monkeypatch):
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    on = _trainer(kind, path, weight_averaging="ema", ema_decay=0.5)
    # the frozen phase: two epochs of two steps on the head, the second epoch on cached features
    _train(on, 2, 5e-3, True)
    opt = on.optimizer
    assert opt.averaging.as_dict() == dict(kind="ema", decay=0.5, warmup=False, start_step=0, every=1)
    assert int(opt.n_averaged) == 4 and on._feat_cache["have_test"]
    assert names.count(AVG[0]) == names.count(AVG[1]) == 4 and names.count("eav_swap_jobs") == 4    # 2 evaluations
    assert "eav_adam_step" not in names and "eav_adam_step_jobs" not in names
    head = {id(p) for p in on.model.classifier.parameters()}
    for p in on.model.parameters():                 # the backbone never trained: its average is the parameter
        assert torch.equal(opt.state[p]["avg"], p) != (id(p) in head)
    rng = torch.get_rng_state()                     # (the shuffles draw from it: the checks must not move it)
    rows = on._evaluate()                           # the head on the cached test features, averaged weights
    got = np.concatenate([r[0] for r in rows], axis=0)
    want, _ = _test_logits(on, _saved(on, tmp_path / "frozen_avg", True))
    last, _ = _test_logits(on, _saved(on, tmp_path / "frozen_last", False))
    assert _same_bits(got, want) and not _same_bits(got, last)
    torch.set_rng_state(rng)
    # the unfrozen phase
    _train(on, 2, 1e-3, False)
    names.clear()
    off = _trainer(kind, path)                      # the same seed, the same shuffles, the option off
    _train(off, 2, 5e-3, True)
    _train(off, 2, 1e-3, False)
    assert not [n for n in names if n.endswith("_avg") or n == "eav_swap_jobs"] and off.optimizer.averaging is None
    assert int(opt.n_averaged) == 8 and on.optimizer.averaging is opt.averaging
    for (k, p), (_, q) in zip(on.model.named_parameters(), off.model.named_parameters()):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), f"{k}: averaging perturbed training"
    want, w_avg = _test_logits(on, _saved(on, tmp_path / "avg", True))
    last, w_last = _test_logits(on, _saved(on, tmp_path / "last", False))
    assert _same_bits(on.outputs_test, want), "outputs_test is not the averaged weights' logits"
    assert not _same_bits(on.outputs_test, last) and _same_bits(off.outputs_test, last)
    moved = 0
    for k, p in on.model.named_parameters():
        assert _same_bits(w_avg[k], opt.state[p]["avg"].cpu().numpy()), k
        assert _same_bits(w_last[k], p.detach().cpu().numpy()), k
        moved += not _same_bits(w_avg[k], w_last[k])
    assert moved == len(w_avg)
    # the option taken back: the averages are dropped, the default step again
    on.weight_averaging = None
    names.clear()
    _train(on, 1, 1e-4, False)
    assert on.optimizer.averaging is None and not on.optimizer.multi_tensor
    assert "eav_adam_step" in names and not [n for n in names if n.endswith("_avg") or n == "eav_swap_jobs"]


def _saved(tr, directory, averaged):
    if averaged:
        tr.save_pretrained(str(directory))          # the default: the averaged weights
    else:
        tr.save_pretrained(str(directory), averaged=False)
    return str(directory)


@pytest.mark.parametrize("kind", KINDS)
def test_option_at_none_launches_what_it_always_did(kind, path, monkeypatch):
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    runs = []
    for explicit in (False, True):
        tr = _trainer(kind, path)
        if explicit:                                # the defaults spelled out: the same thing as leaving them alone
            tr.weight_averaging, tr.ema_decay, tr.ema_warmup, tr.averaging_start_epoch, tr.averaging_every = \
                None, 0.999, False, 0, 1
        names.clear()
        _train(tr, 1, 5e-4, True)
        _train(tr, 1, 5e-6, False)
        assert not tr.optimizer.multi_tensor and tr.optimizer.averaging is None
        assert set(tr.optimizer.state_dict()) == {"state", "param_groups"}
        runs.append(list(names))
    assert runs[0] == runs[1] and runs[0].count("eav_adam_step") >= 4
    assert not [n for n in runs[0] if n.endswith("_avg") or n in ("eav_swap_jobs", "eav_adam_jobs_begin")]


@pytest.mark.parametrize("kind", ["ast"])
def test_start_epoch_counts_optimiser_steps_over_the_phases(kind, path):
    """6 items in batches of 4: two steps per epoch, one with gradient_accumulation_steps = 2."""
    tr = _trainer(kind, path, weight_averaging="swa", averaging_start_epoch=1, averaging_every=2)
    _train(tr, 1, 5e-3, True)
    assert tr.optimizer.averaging.start_step == 3 and int(tr.optimizer.n_averaged) == 0
    _train(tr, 2, 1e-3, False)                      # steps 3 .. 6: averaged at 3 and 5
    assert tr.optimizer._avg_rec.cpu().tolist()[:2] == [6, 2]
    acc = _trainer(kind, path, weight_averaging="swa", averaging_start_epoch=2, gradient_accumulation_steps=2)
    _train(acc, 3, 1e-3, False)
    assert acc.optimizer.averaging.start_step == 3 and acc.optimizer._avg_rec.cpu().tolist()[:2] == [3, 1]
