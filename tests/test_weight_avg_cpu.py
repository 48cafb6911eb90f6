"""Weight averaging without a GPU: tests/weight_avg_ref.py against torch.optim.swa_utils.AveragedModel in float64 (EMA and
SWA, the first-update copy, the start_step / every gating), the float32 restatement of the kernel inside the bound its
docstring derives, the warmup formula, optim.WeightAveraging, the new entry points in header, binding and library, their
bad-argument statuses (nothing is launched) and the host surface of optimiser, trainers and tool."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import weight_avg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("ema", dict(decay=0.9)), ("ema", dict(decay=0.999)), ("swa", {}),
         ("ema", dict(decay=0.9, start_step=4, every=3)), ("swa", dict(start_step=4, every=3)),
         ("swa", dict(start_step=0, every=2))]


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(5, 3).double()
        self.scale = torch.nn.Parameter(torch.ones(7, dtype=torch.float64))


@pytest.mark.parametrize("kind,kw", CASES)
def test_reference_matches_averaged_model_in_float64(kind, kw, request):
    """12 optimiser steps of a small module; AveragedModel.update_parameters is called on the averaging steps only, the
    reference sees every step and gates itself."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn, get_swa_multi_avg_fn
    torch.manual_seed(3)
    model = _Small()
    # get_swa_multi_avg_fn forms 1 / (n_averaged + 1) from an integer tensor, i.e. in torch's DEFAULT dtype
    torch.set_default_dtype(torch.float64)
    request.addfinalizer(lambda: torch.set_default_dtype(torch.float32))
    fn = get_ema_multi_avg_fn(kw["decay"]) if kind == "ema" else get_swa_multi_avg_fn()
    theirs = AveragedModel(model, multi_avg_fn=fn)
    params = list(model.parameters())
    mine = R.Averager([p.detach().numpy() for p in params], kind, **kw)
    modes = []
    for s in range(1, 13):
        with torch.no_grad():
            for i, p in enumerate(params):
                p.add_(torch.from_numpy(0.1 * synth.normal(100 * s + i, tuple(p.shape)).astype(np.float64)))
        mode, c = mine.update([p.detach().numpy() for p in params])
        modes.append(mode)
        if mode != "skip":
            theirs.update_parameters(model)
        assert int(theirs.n_averaged) == mine.n and mine.s == s
        if mine.n:
            for a, b in zip(theirs.module.parameters(), mine.avg):
                np.testing.assert_allclose(b, a.detach().numpy(), rtol=1e-13, atol=1e-15)
        if mode == "copy":              # the first update: the parameters themselves, bit for bit
            for a, p in zip(mine.avg, params):
                assert np.array_equal(a, p.detach().numpy())
    start, every = kw.get("start_step", 0), kw.get("every", 1)
    want = ["skip" if s < start or (s - start) % every else "lerp" for s in range(1, 13)]
    want[want.index("lerp")] = "copy"
    assert modes == want and modes.count("copy") == 1
    assert [(s, n, m) for s, n, m, _ in R.sequence(kind, 12, **kw)] == \
        [(s, sum(x != "skip" for x in modes[:s]), modes[s - 1]) for s in range(1, 13)]


def test_start_step_and_every_gating():
    seq = R.sequence("swa", 14, start_step=7, every=3)
    assert [s for s, _, m, _ in seq if m != "skip"] == [7, 10, 13]
    assert [c for _, _, m, c in seq if m != "skip"] == [1.0, 0.5, 1.0 / 3.0]
    assert [m for _, _, m, _ in R.sequence("ema", 4)] == ["copy", "lerp", "lerp", "lerp"]          # start 0: from step 1
    assert [s for s, _, m, _ in R.sequence("ema", 9, start_step=0, every=3) if m != "skip"] == [3, 6, 9]
    assert [n for _, n, _, _ in R.sequence("ema", 5, start_step=3)] == [0, 0, 1, 2, 3]


def test_warmup_formula_and_host_class():
    from eav_amd.optim import WeightAveraging
    for decay in (0.9, 0.999, 0.9999):
        w = WeightAveraging("ema", decay, warmup=True)
        for n in range(1, 40):
            d = min(decay, (1.0 + n) / (10.0 + n))
            mode, c = R.mode_and_coefficient("ema", n + 1, n, decay=decay, warmup=True)
            assert (mode, c) == ("lerp", 1.0 - d) == w.mode_and_coefficient(n + 1, n)
        # (1 + n) / (10 + n) reaches 0.9 at n = 80, 0.999 at n = 8990: below that the warmup rules
        assert R.mode_and_coefficient("ema", 2, 1, decay=decay, warmup=True)[1] == 1.0 - 2.0 / 11.0
        assert R.mode_and_coefficient("ema", 10 ** 6, 10 ** 6, decay=decay, warmup=True)[1] == 1.0 - decay
        assert R.mode_and_coefficient("ema", 2, 1, decay=decay)[1] == 1.0 - decay
    for kind, kw in CASES:
        w = WeightAveraging(kind, **kw)
        n = 0
        for s, n_after, mode, c in R.sequence(kind, 12, **kw):
            assert w.mode_and_coefficient(s, n) == (mode, c)
            n = n_after
    assert WeightAveraging.KINDS == R.KINDS and [WeightAveraging(k).code for k in R.KINDS] == [0, 1]
    d = WeightAveraging().as_dict()
    assert d == dict(kind="ema", decay=0.999, warmup=False, start_step=0, every=1)
    assert WeightAveraging(**d) == WeightAveraging() and WeightAveraging("swa") != WeightAveraging()
    for bad in (dict(kind="mean"), dict(decay=1.5), dict(decay=-0.1), dict(start_step=-1), dict(start_step=1.5),
                dict(every=0), dict(every=2.5)):
        with pytest.raises(ValueError):
            WeightAveraging(**bad)


@pytest.mark.parametrize("kind,kw", CASES[:3] + [("ema", dict(decay=0.9, warmup=True))])
def test_float32_restatement_stays_inside_the_bound(kind, kw):
    """12 updates of 5000 elements over six orders of magnitude, parameters that move by about a tenth of their size."""
    n = 5000
    p = (synth.normal(7, (n,)) * 10.0 ** (synth.uniform(8, (n,)) * 6 - 4)).astype(np.float32)
    avg32, ref, worst, nn, mxmax = p.copy(), R.Tracked(p), 0.0, 0, np.abs(p).astype(np.float64)
    for s in range(1, 13):
        p = (p * (1.0 + 0.1 * synth.normal(20 + s, (n,)))).astype(np.float32)
        mode, c = R.mode_and_coefficient(kind, s, nn, **kw)
        nn += 1
        c32 = R.coefficient_f32(c)
        avg32 = p.copy() if mode == "copy" else R.lerp_f32(avg32, p, c32)
        ref.update(mode, float(c32), p)
        worst = max(worst, ref.check(avg32, f"{kind} {kw} step {s}")) if ref.updates else worst
        mxmax = np.maximum(mxmax, np.maximum(np.abs(p), np.abs(ref.avg) + ref.tol))
        assert np.all(ref.tol <= 3.0 * ref.updates * R.U * mxmax * (1 + 1e-12))      # never above 3 k 2^-24 Mx
    assert ref.updates == 11 and worst > 0.01              # the bound is not vacuous


def test_new_entry_points_are_declared_bound_and_exported():
    from eav_amd import _lib
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    assert re.search(r"\bEAV_ADAM_AVG_WORDS = (\d+)", header).group(1) == str(_lib.AVG_WORDS)
    for name, code in (("EMA", 0), ("SWA", 1), ("SKIP", _lib.AVG_SKIP), ("COPY", _lib.AVG_COPY), ("LERP", _lib.AVG_LERP)):
        assert re.search(r"#define EAV_AVG_%s %d\b" % (name, code), header), name
    assert _lib.AVG_KINDS == R.KINDS and (_lib.AVG_SKIP, _lib.AVG_COPY, _lib.AVG_LERP) == (0, 1, 2)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("eav_adam_jobs_begin_avg", 19), ("eav_adam_step_jobs_avg", 11), ("eav_swap_jobs", 5)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
    # the begin variant takes eav_adam_jobs_begin's arguments first, the step variant eav_adam_step_jobs' around `avgs`
    assert _lib.SIGNATURES["eav_adam_jobs_begin_avg"][:12] == _lib.SIGNATURES["eav_adam_jobs_begin"][:12]
    src = open(os.path.join(ROOT, "eav_amd", "csrc", "adam_jobs.hip")).read()
    assert "fp contract(off)" in src.split("avg_advance(")[1].split("}")[0]


def test_bad_arguments_return_a_status_without_a_launch():
    from eav_amd import _lib
    buf = np.zeros(64, np.int64)
    a = buf.ctypes.data

    def begin(jobs=a, njobs=1, counts=a, ncounts=1, sched=a, kind=0, warmup=0, total=0, rec=a, avg_kind=0, decay=0.999,
              start=0, every=1):
        _lib.call("eav_adam_jobs_begin_avg", jobs, njobs, counts, ncounts, sched, kind, warmup, total, 0.5, 1e-3, 0.9, 0.999,
                  rec, avg_kind, decay, 0, start, every, None)

    def step(jobs=a, avgs=a, njobs=1, nchunks=1, rec=a):
        _lib.call("eav_adam_step_jobs_avg", jobs, avgs, njobs, nchunks, 0.9, 0.999, 1e-8, 1, None, rec, None)

    def swap(jobs=a, avgs=a, njobs=1, nchunks=1):
        _lib.call("eav_swap_jobs", jobs, avgs, njobs, nchunks, None)

    for kw in (dict(jobs=None), dict(njobs=0), dict(sched=None), dict(counts=None), dict(ncounts=-1), dict(warmup=-1),
               dict(total=-1)):
        with pytest.raises(_lib.EavError, match="eav_adam_jobs_begin_avg"):
            begin(**kw)
    with pytest.raises(_lib.EavError, match="unknown schedule kind"):
        begin(kind=4)
    for kw, word in ((dict(rec=None), "avg_record"), (dict(avg_kind=2), "avg_kind"), (dict(avg_kind=-1), "avg_kind"),
                     (dict(decay=1.5), "decay"), (dict(decay=-0.01), "decay"), (dict(decay=float("nan")), "decay"),
                     (dict(every=0), "every"), (dict(every=-2), "every"), (dict(start=-1), "start_step")):
        with pytest.raises(_lib.EavError, match="eav_adam_jobs_begin_avg: .*" + word):
            begin(**kw)
    for kw in (dict(jobs=None), dict(njobs=0), dict(nchunks=0), dict(nchunks=-1)):
        with pytest.raises(_lib.EavError, match="eav_adam_step_jobs_avg: bad arguments"):
            step(**kw)
    for kw in (dict(avgs=None), dict(rec=None)):
        with pytest.raises(_lib.EavError, match="eav_adam_step_jobs_avg: avgs or avg_record"):
            step(**kw)
    for kw in (dict(jobs=None), dict(avgs=None), dict(njobs=0), dict(nchunks=0)):
        with pytest.raises(_lib.EavError, match="eav_swap_jobs"):
            swap(**kw)


def test_host_surface():
    from eav_amd import _lib, optim
    from eav_amd.finetune import FineTuneBase
    w = torch.nn.Parameter(torch.zeros(3))
    opt = optim.FusedAdam([w])
    assert opt.averaging is None and opt.n_averaged is None and opt.multi_tensor is False
    assert set(opt.state_dict()) == {"state", "param_groups"}
    with pytest.raises(TypeError):
        opt.set_averaging("ema")
    with pytest.raises(_lib.EavError, match="ROCm device"):
        opt.set_averaging(optim.WeightAveraging("ema"))                  # no CPU fallback
    with pytest.raises(_lib.EavError, match="averaging is off"):
        with opt.averaged_parameters():
            pass
    opt.set_averaging(None)
    assert opt.averaging is None and opt.multi_tensor is False and "avg" not in opt.state[w]
    for name in ("set_averaging", "averaged_parameters", "n_averaged"):
        assert "averag" in inspect.getdoc(optim.FusedAdam) and hasattr(optim.FusedAdam, name)
    assert "buffers" in inspect.getdoc(optim.WeightAveraging).lower()
    assert (FineTuneBase.weight_averaging, FineTuneBase.ema_decay, FineTuneBase.ema_warmup,
            FineTuneBase.averaging_start_epoch, FineTuneBase.averaging_every) == (None, 0.999, False, 0, 1)
    sig = inspect.signature(FineTuneBase.save_pretrained).parameters
    assert sig["averaged"].default is True
    tool = open(os.path.join(ROOT, "tools", "run_finetune_subjects.py")).read()
    for flag in ("--weight-averaging", "--ema-decay", "--ema-warmup", "--averaging-start-epoch"):
        assert f'"{flag}"' in tool
