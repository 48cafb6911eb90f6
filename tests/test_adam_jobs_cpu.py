"""Multi-tensor Adam and the learning-rate schedules without a GPU: tests/adam_jobs_ref.py against torch.optim.Adam / AdamW
(two param groups) and transformers.get_scheduler, optim.LRSchedule, finetune.encoder_param_groups on reduced CPU encoders,
the float32 restatement of the kernel inside the bounds the GPU tests use, the new entry points in header, binding and
library, and their bad-argument statuses (nothing is launched)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import adam_jobs_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (7,), (3, 5), (129,)]


@pytest.mark.parametrize("decoupled", [False, True])
def test_reference_matches_torch_with_two_param_groups(decoupled):
    """Three steps, tensors 0 and 2 in a group with lr 1e-2 / wd 0.01, tensors 1 and 3 in one with lr 3e-3 / wd 0."""
    p0 = [synth.normal(20 + i, s).astype(np.float64) for i, s in enumerate(SHAPES)]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": [params[0], params[2]], "lr": 1e-2, "weight_decay": 0.01},
               {"params": [params[1], params[3]], "lr": 3e-3, "weight_decay": 0.0}], foreach=False)
    lrs, wds = [1e-2, 3e-3, 1e-2, 3e-3], [0.01, 0.0, 0.01, 0.0]
    ref = A.Stepper(p0, wds, decoupled)
    for s in range(3):
        grads = [synth.normal(200 + 10 * s + i, sh).astype(np.float64) for i, sh in enumerate(SHAPES)]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        ref.step(grads, lrs)
        for i, p in enumerate(params):
            st = opt.state[p]
            np.testing.assert_allclose(ref.p[i], p.detach().numpy(), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(ref.m[i], st["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
            np.testing.assert_allclose(ref.v[i], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-20)
    assert ref.steps == [3, 3, 3, 3]
    ref.step([None, grads[1], None, None], lrs)             # a tensor without a gradient keeps its count
    assert ref.steps == [3, 4, 3, 3]


@pytest.mark.parametrize("kind", A.KINDS)
def test_factors_match_transformers_get_scheduler(kind):
    transformers = pytest.importorskip("transformers")
    from eav_amd.optim import LRSchedule
    for W, T in ((3, 10), (0, 7), (5, 5)):
        w = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([w], lr=1.0)
        sched = transformers.get_scheduler(kind, opt, num_warmup_steps=W, num_training_steps=T)
        mine = LRSchedule(kind, W, T)
        for t in range(T + 6):
            hf = sched.get_last_lr()[0]                     # base lr 1.0: the lambda's value at step t
            assert A.schedule_factor(kind, t, W, T) == hf, (kind, W, T, t)
            assert mine.factor(t) == hf, (kind, W, T, t)
            opt.step()
            sched.step()
    if kind != "constant":
        assert LRSchedule(kind, 3, 10).factor(0) == 0.0     # LambdaLR's first step of a warmup


def test_lr_schedule_surface():
    from eav_amd.optim import LRSchedule
    assert LRSchedule.KINDS == A.KINDS
    assert [LRSchedule(k, 1, 4).code for k in A.KINDS] == [0, 1, 2, 3]
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    for code, name in enumerate(("CONSTANT", "CONSTANT_WITH_WARMUP", "LINEAR", "COSINE")):
        assert re.search(r"#define EAV_SCHED_%s %d\b" % (name, code), header)
    s = LRSchedule("cosine", 2, 12, num_cycles=1.5)
    assert (s.num_warmup_steps, s.num_training_steps, s.num_cycles) == (2, 12, 1.5)
    assert s.factor(7) == A.schedule_factor("cosine", 7, 2, 12, 1.5)
    assert LRSchedule("constant").factor(10 ** 9) == 1.0 and LRSchedule("constant_with_warmup", 4).factor(2) == 0.5
    assert LRSchedule("linear", 0, 10).factor(15) == 0.0
    for bad in (dict(kind="polynomial"), dict(kind="linear"), dict(kind="cosine", num_training_steps=-1),
                dict(kind="linear", num_warmup_steps=-1, num_training_steps=5),
                dict(kind="linear", num_warmup_steps=1.5, num_training_steps=5)):
        with pytest.raises(ValueError):
            LRSchedule(**bad)


@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_encoder_param_groups(kind):
    from eav_amd import transformer as T
    from eav_amd.finetune import encoder_layer_id, encoder_no_decay, encoder_param_groups
    cfg = T.make_config(kind, hidden=32, layers=2, heads=2, ff=64, image=32)
    model = T.Encoder(cfg)
    named = dict(model.named_parameters())
    groups = encoder_param_groups(model, 1e-3, 0.01, layer_decay=0.75, decay_bias_and_norm=False)
    seen = [n for g in groups for n in g["names"]]
    assert sorted(seen) == sorted(named) and len(seen) == len(set(seen))          # every parameter exactly once
    assert sum(len(g["params"]) for g in groups) == len(named)
    for g in groups:
        assert [id(p) for p in g["params"]] == [id(named[n]) for n in g["names"]]
        assert g["lr_scale"] == 0.75 ** (3 - g["layer_id"]) and g["lr"] == 1e-3 * g["lr_scale"]
        assert g["weight_decay"] in (0.0, 0.01)
        for n in g["names"]:
            assert encoder_layer_id(n, 2) == g["layer_id"], n
            assert encoder_no_decay(n) == (g["weight_decay"] == 0.0), n
    assert sorted({g["layer_id"] for g in groups}) == [0, 1, 2, 3]
    assert sorted({g["lr_scale"] for g in groups}) == [0.75 ** 3, 0.75 ** 2, 0.75, 1.0]
    assert len(groups) == 8             # every id with and without decay (id 0: the patch projection's weight decays)
    p = cfg.prefix
    ids = {n: g["layer_id"] for g in groups for n in g["names"]}
    nodecay = {n for g in groups if g["weight_decay"] == 0.0 for n in g["names"]}
    assert ids[f"{p}.embeddings.cls_token"] == 0 and ids[f"{p}.embeddings.position_embeddings"] == 0
    assert ids[f"{p}.embeddings.patch_embeddings.projection.weight"] == 0
    assert ids[f"{p}.layers.0.attention.q_proj.weight"] == 1 and ids[f"{p}.layers.1.mlp.fc2.bias"] == 2
    assert ids[f"{p}.layernorm.weight"] == 3
    head = "classifier.dense" if kind == "ast" else "classifier"
    assert ids[f"{head}.weight"] == 3 and ids[f"{head}.bias"] == 3
    if kind == "ast":
        assert ids[f"{p}.embeddings.distillation_token"] == 0 and ids["classifier.layernorm.weight"] == 3
        assert {f"{p}.embeddings.distillation_token", "classifier.layernorm.weight", "classifier.layernorm.bias"} <= nodecay
    want_nodecay = {n for n in named if n.endswith(".bias") or "layernorm" in n.split(".")[-2]
                    or n.endswith("_token") or n.endswith("position_embeddings")}
    assert nodecay == want_nodecay
    assert f"{p}.layers.0.layernorm_before.weight" in nodecay and f"{p}.layers.1.mlp.fc1.weight" not in nodecay
    assert f"{head}.weight" not in nodecay and f"{p}.embeddings.patch_embeddings.projection.weight" not in nodecay
    # the defaults: one group that decays everything at the base rate
    (one,) = encoder_param_groups(model, 1e-3, 0.01)
    assert one["lr"] == 1e-3 and one["weight_decay"] == 0.01 and one["layer_id"] is None and one["lr_scale"] == 1.0
    assert one["names"] == list(named)
    two = encoder_param_groups(model, 1e-3, 0.01, decay_bias_and_norm=False)
    assert [g["weight_decay"] for g in two] == [0.01, 0.0] and set(two[1]["names"]) == want_nodecay
    assert len(encoder_param_groups(model, 1e-3, 0.01, layer_decay=0.5)) == 4
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError):
            encoder_param_groups(model, 1e-3, 0.01, layer_decay=bad)
    # torch accepts them as param groups
    torch.optim.AdamW([{k: g[k] for k in ("params", "lr", "weight_decay")} for g in groups])


def _kernel_case(seed, n, step, wd, decoupled, gscale):
    p = synth.normal(seed, (n,)).astype(np.float32)
    g = (synth.normal(seed + 1, (n,)) * 10.0 ** (synth.uniform(seed + 2, (n,)) * 6 - 4)).astype(np.float32)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (0.1 * synth.normal(seed + 3, (n,))).astype(np.float32)
        v = (synth.uniform(seed + 4, (n,)) * 1e-2).astype(np.float32) ** 2
    return p, g, m, v


@pytest.mark.parametrize("step", [1, 11])
@pytest.mark.parametrize("wd,decoupled", [(0.0, True), (0.01, True), (0.01, False)])
@pytest.mark.parametrize("gscale", [None, 0.37])
def test_float32_restatement_stays_inside_the_bounds(step, wd, decoupled, gscale):
    """The bounds the GPU tests assert hold for the kernel's operation order evaluated in numpy float32, on inputs of
    the kind those tests use (gradients over six orders of magnitude, moments that cancel against the gradient)."""
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 3e-3
    p, g, m, v = _kernel_case(40 + step, 5000, step, wd, decoupled, gscale)
    bc1, bc2s = A.bias_corrections_f32(b1, b2, step)
    got = A.adam_step_f32(p, g, m, v, lr, wd, bc1, bc2s, b1, b2, eps, decoupled, gscale)
    pr, mr, vr, tp, tm, tv, _ = A.step_bounds(p, g, m, v, lr, wd, step, b1, b2, eps, decoupled, gscale)
    for name, a, r, tol in (("p", got[0], pr, tp), ("m", got[1], mr, tm), ("v", got[2], vr, tv)):
        err = np.abs(a.astype(np.float64) - r)
        assert np.all(err <= tol), (name, float(np.max(err / np.maximum(tol, 1e-300))))
        assert float(np.max(err / np.maximum(tol, 1e-300))) > 0.01, name       # the bounds are not vacuous


def test_new_entry_points_are_declared_bound_and_exported():
    from eav_amd import _lib
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    words = {k: int(v) for k, v in re.findall(r"#define (EAV_ADAM_\w+_WORDS) (\d+)", header)}
    assert words == {"EAV_ADAM_JOB_WORDS": _lib.JOB_WORDS, "EAV_ADAM_SCHED_WORDS": _lib.SCHED_WORDS}
    assert (_lib.JOB_WORDS * 8) % 16 == 0
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in ("eav_adam_jobs_begin", "eav_adam_step_jobs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"\bint64_t\s+eav_adam_jobs_nchunks\s*\(", header) and "eav_adam_jobs_nchunks" in _lib.PLAIN
    for n in (0, 1, 8191, 8192, 8193, 3 * 8192 + 7, 1 << 40):
        assert _lib.plain("eav_adam_jobs_nchunks", n) == _lib.plain("eav_grad_nchunks", n)
    assert _lib.plain("eav_abi_version") == 3
    src = open(os.path.join(ROOT, "eav_amd", "csrc", "adam_jobs.hip")).read()
    assert "atomic" not in src.replace("No atomics", "") and "job_locate<" in src
    clip = open(os.path.join(ROOT, "eav_amd", "csrc", "grad_clip.hip")).read()
    assert "job_locate<" in clip and "bool locate(" not in clip            # one copy of the chunk walk (job_table.h)


def test_bad_arguments_return_a_status_without_a_launch():
    from eav_amd import _lib
    buf = np.zeros(64, np.int64)
    a = buf.ctypes.data

    def begin(jobs=a, njobs=1, counts=a, ncounts=1, sched=a, kind=0, warmup=0, total=0):
        _lib.call("eav_adam_jobs_begin", jobs, njobs, counts, ncounts, sched, kind, warmup, total, 0.5, 1e-3, 0.9, 0.999, None)

    def step(jobs=a, njobs=1, nchunks=1):
        _lib.call("eav_adam_step_jobs", jobs, njobs, nchunks, 0.9, 0.999, 1e-8, 1, None, None)

    for kw in (dict(jobs=None), dict(njobs=0), dict(njobs=-3), dict(sched=None), dict(counts=None), dict(ncounts=-1),
               dict(warmup=-1), dict(total=-1)):
        with pytest.raises(_lib.EavError, match="eav_adam_jobs_begin"):
            begin(**kw)
    for kind in (-1, 4, 99):
        with pytest.raises(_lib.EavError, match="unknown schedule kind"):
            begin(kind=kind)
    for kw in (dict(jobs=None), dict(njobs=0), dict(nchunks=0), dict(nchunks=-1)):
        with pytest.raises(_lib.EavError, match="eav_adam_step_jobs"):
            step(**kw)


def test_host_surface():
    from eav_amd import _lib, optim
    from eav_amd.finetune import FineTuneBase
    sig = inspect.signature(optim.FusedAdam.__init__).parameters
    assert sig["multi_tensor"].default is False and sig["multi_tensor"].kind is inspect.Parameter.KEYWORD_ONLY
    w = torch.nn.Parameter(torch.zeros(3))
    opt = optim.FusedAdam([w])
    assert opt.multi_tensor is False and opt.schedule is None and opt.last_lr is None
    opt.set_schedule(optim.LRSchedule("linear", 1, 4))
    assert opt.multi_tensor is True and opt.schedule.kind == "linear"
    opt.set_schedule(None)
    assert opt.schedule is None and opt.multi_tensor is True
    with pytest.raises(TypeError):
        opt.set_schedule("linear")
    w.grad = torch.ones(3)
    with pytest.raises(_lib.EavError, match="ROCm device"):
        optim.FusedAdam([w], multi_tensor=True).step()                  # no CPU fallback
    two = optim.FusedAdam([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "eps": 1e-6}], multi_tensor=True)
    with pytest.raises(_lib.EavError, match="equal across the param groups"):
        two.step()
    assert (FineTuneBase.lr_scheduler_type, FineTuneBase.warmup_ratio, FineTuneBase.warmup_steps, FineTuneBase.layer_decay,
            FineTuneBase.decay_bias_and_norm) == ("constant", 0.0, None, 1.0, True)
    tool = open(os.path.join(ROOT, "tools", "run_finetune_subjects.py")).read()
    for flag in ("--lr-scheduler", "--warmup-ratio", "--layer-decay", "--no-decay-bias-norm"):
        assert f'"{flag}"' in tool
