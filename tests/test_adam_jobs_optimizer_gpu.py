"""FusedAdam(multi_tensor=True) and set_schedule at the optimiser level: a module of five tensors (7, 64, 1, 4097 and 300
elements) put through flatten_parameters, synthetic gradients written into the views of its flat gradient buffer, three
or more steps per case.  Bit for bit against the default path with a device step count (FusedAdam(capturable=True): the
same element update, the same bias-correction expressions); within the compounded float64 bounds of
tests/adam_jobs_ref.py where the default path forms its bias corrections on the host."""
import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import adam_jobs_ref as A

pytestmark = pytest.mark.gpu

SIZES = [7, 64, 1, 4097, 300]
LR, LR2, B1, B2, EPS_ADAM, WD = (float(np.float32(v)) for v in (1e-3, 2.5e-4, 0.9, 0.999, 1e-8, 0.01))


class _Net:
    def __init__(self, seed=1, track_dirty=False):
        from eav_amd.optim import flatten_parameters
        self.host = [synth.normal(seed + i, (n,)).astype(np.float32) for i, n in enumerate(SIZES)]
        self.params = [torch.nn.Parameter(torch.from_numpy(h.copy()).cuda()) for h in self.host]
        self.module = torch.nn.Module()
        for i, p in enumerate(self.params):
            self.module.register_parameter(f"w{i}", p)
        self.flat, self.gflat, self.offsets = flatten_parameters(self.module)
        if track_dirty:
            self.flat._eav_track_dirty = True

    def set_grads(self, grads):
        """grads[i] None: the tensor has no gradient in this step."""
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
                continue
            off, n = self.offsets[f"w{i}"]
            view = self.gflat[off:off + n].view(p.shape)
            view.copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)))
            p.grad = view

    def optimizer(self, split=True, **kw):
        """split: tensors 0, 2, 4 in a group (LR, WD), tensors 1, 3 in one (LR2, no decay) - no two neighbours share one."""
        from eav_amd.optim import FusedAdam
        kw.setdefault("decoupled", True)
        groups = ([{"params": self.params[0::2], "lr": LR, "weight_decay": WD},
                   {"params": self.params[1::2], "lr": LR2, "weight_decay": 0.0}] if split
                  else [{"params": self.params, "lr": LR, "weight_decay": WD}])
        return FusedAdam(groups, betas=(B1, B2), eps=EPS_ADAM, **kw)

    def hyper(self, i, split=True):
        return (LR, WD) if not split or i % 2 == 0 else (LR2, 0.0)


def _grads(seed, gain=1.0):
    return [synth.normal(seed + i, (n,)).astype(np.float32) * np.float32(gain) for i, n in enumerate(SIZES)]


def _same_bits(a, oa, b, ob, what):
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (what, "p", i)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[p][k].view(torch.int32), ob.state[q][k].view(torch.int32)), (what, k, i)


def _log_calls(monkeypatch):
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("capturable", [False, True])
def test_two_groups_in_two_launches_give_the_default_paths_bits(decoupled, capturable, monkeypatch):
    a, b = _Net(), _Net()
    oa = a.optimizer(multi_tensor=True, capturable=capturable, decoupled=decoupled)
    ob = b.optimizer(capturable=True, decoupled=decoupled)
    names = _log_calls(monkeypatch)
    for s in range(3):
        g = _grads(50 + 10 * s)
        a.set_grads(g)
        b.set_grads(g)
        names.clear()
        oa.step()
        assert names == (["eav_counter_inc"] if capturable else []) + ["eav_adam_jobs_begin", "eav_adam_step_jobs"], names
        names.clear()
        ob.step()
        assert names == ["eav_counter_inc"] + ["eav_adam_step"] * 5, names        # one launch per run: the groups alternate
        torch.cuda.synchronize()
        _same_bits(a, oa, b, ob, f"step {s}")
        assert all(oa.state[p]["step"] == s + 1 for p in a.params)                 # the host mirror still advances
    assert len(oa._adam_tables) == 1                                               # the steady state found its table
    sd = oa.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == [LR, LR2] and sd["state"][0]["step"] == 3


def test_changed_rates_are_picked_up():
    a, b = _Net(), _Net()
    oa, ob = a.optimizer(multi_tensor=True), b.optimizer(capturable=True)
    for s, (lr, wd) in enumerate(((LR, WD), (LR2, WD), (LR2, 0.0), (LR, WD))):
        for o in (oa, ob):
            o.param_groups[0]["lr"], o.param_groups[0]["weight_decay"] = lr, wd
        g = _grads(70 + s)
        a.set_grads(g)
        b.set_grads(g)
        oa.step()
        ob.step()
        _same_bits(a, oa, b, ob, f"step {s}")
    assert len(oa._adam_tables) == 3                    # part of the cache key; the first table was found again


def test_frozen_then_unfrozen_keeps_per_tensor_step_counts():
    """two steps with a gradient for the last tensor only, then two for all - its count is 4, the others' 2."""
    net = _Net()
    opt = net.optimizer(multi_tensor=True)
    ref = [A.Trajectory(h, net.hyper(i)[1], True, (B1, B2), EPS_ADAM) for i, h in enumerate(net.host)]
    for s in range(4):
        g = _grads(90 + 10 * s)
        if s < 2:
            g = [None] * 4 + g[4:]
        net.set_grads(g)
        opt.step()
        for i, gi in enumerate(g):
            if gi is not None:
                ref[i].step(gi, net.hyper(i)[0])
    torch.cuda.synchronize()
    assert [opt.state[p]["step"] for p in net.params] == [2, 2, 2, 2, 4] and [r.steps for r in ref] == [2, 2, 2, 2, 4]
    for i, p in enumerate(net.params):
        st = opt.state[p]
        ref[i].check(p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), f"tensor {i}")
    # the same history on the default path with host-side counts: the same table shapes, results within the same bounds
    twin = _Net()
    topt = twin.optimizer()
    for s in range(4):
        g = _grads(90 + 10 * s)
        twin.set_grads([None] * 4 + g[4:] if s < 2 else g)
        topt.step()
    for i, p in enumerate(twin.params):
        st = topt.state[p]
        ref[i].check(p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), f"default path {i}")


def test_linear_schedule_trajectory_of_last_lr():
    from eav_amd.optim import LRSchedule
    net = _Net()
    opt = net.optimizer()
    sch = LRSchedule("linear", 2, 6)
    opt.set_schedule(sch)
    assert opt.multi_tensor
    ref = [A.Trajectory(h, net.hyper(i)[1], True, (B1, B2), EPS_ADAM) for i, h in enumerate(net.host)]
    for t in range(7):
        g = _grads(130 + t)
        net.set_grads(g)
        opt.step()
        want = A.lr_f32(LR, A.schedule_factor("linear", t, 2, 6))
        got = opt.last_lr.cpu().numpy()
        assert opt.last_lr.dim() == 0 and opt.last_lr.is_cuda and got.dtype == np.float32
        assert got.view(np.int32) == want.view(np.int32), (t, got, want)
        assert sch.factor(t) == A.schedule_factor("linear", t, 2, 6)
        for i, gi in enumerate(g):
            ref[i].step(gi, A.lr_f32(net.hyper(i)[0], sch.factor(t)))
    assert [float(A.lr_f32(LR, sch.factor(t))) for t in (0, 6)] == [0.0, 0.0]       # LambdaLR: the first step runs at 0
    assert [g["lr"] for g in opt.param_groups] == [LR, LR2]                        # the base rates are not mutated
    for i, p in enumerate(net.params):
        st = opt.state[p]
        ref[i].check(p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), f"scheduled {i}")
    opt.set_schedule(sch)                               # attaching restarts the count
    net.set_grads(_grads(1))
    opt.step()
    assert float(opt.last_lr) == 0.0
    opt.step()
    assert opt.last_lr.cpu().numpy() == A.lr_f32(LR, 0.5)


def test_captured_step_follows_the_schedule_on_every_replay():
    """One eager step (it builds the table and the schedule record), then step() captured once and replayed five times:
    the trajectory of last_lr and the final bits of six eager steps."""
    from eav_amd.optim import LRSchedule
    a, b = _Net(), _Net()
    oa, ob = a.optimizer(capturable=True), b.optimizer(capturable=True)
    for o in (oa, ob):
        o.set_schedule(LRSchedule("cosine", 2, 6))
    g = _grads(170)
    a.set_grads(g)
    b.set_grads(g)
    eager = []
    for _ in range(6):
        ob.step()
        eager.append(ob.last_lr.cpu().numpy().copy())
    oa.step()
    replayed = [oa.last_lr.cpu().numpy().copy()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    for _ in range(5):
        graph.replay()
        replayed.append(oa.last_lr.cpu().numpy().copy())
    torch.cuda.synchronize()
    assert [x.view(np.int32) for x in replayed] == [x.view(np.int32) for x in eager], (replayed, eager)
    assert len({float(x) for x in eager}) >= 5 and eager[0] == 0.0
    assert int(oa.device_step_counter()) == 6 == int(ob.device_step_counter())
    _same_bits(a, oa, b, ob, "captured")


def test_clipping_on_the_jobs_path_gives_the_default_paths_bits(monkeypatch):
    a, b = _Net(), _Net()
    oa, ob = a.optimizer(multi_tensor=True, max_grad_norm=1.0), b.optimizer(capturable=True, max_grad_norm=1.0)
    names = _log_calls(monkeypatch)
    for s, gain in enumerate((1.0, 0.05, 0.001)):                  # norms ~67, ~3.3 (clipped) and ~0.07 (not clipped)
        g = _grads(210 + 10 * s, gain)
        a.set_grads(g)
        b.set_grads(g)
        before = [p.grad.clone() for p in a.params]
        names.clear()
        oa.step()
        assert names == ["eav_grad_sumsq", "eav_grad_clip_finish", "eav_adam_jobs_begin", "eav_adam_step_jobs"], names
        ob.step()
        torch.cuda.synchronize()
        assert float(oa.last_grad_norm) == float(ob.last_grad_norm) and (float(oa.last_grad_norm) > 1.0) == (s < 2)
        for p, q in zip(a.params, before):                         # p.grad is left unscaled
            assert torch.equal(p.grad.view(torch.int32), q.view(torch.int32))
        _same_bits(a, oa, b, ob, f"clipped step {s}")


def test_accumulation_on_the_jobs_path():
    """Two groups of two folds (weights 1/4, 3/4), clipped; the float64 reference steps from the accumulator's own fp32
    contents and the kernel's own coefficient (identical fp32 inputs), compounded bounds."""
    net = _Net()
    opt = net.optimizer(multi_tensor=True, max_grad_norm=1.0)
    ref = [A.Trajectory(h, net.hyper(i)[1], True, (B1, B2), EPS_ADAM) for i, h in enumerate(net.host)]
    for s in range(3):
        for j, w in enumerate((0.25, 0.75)):
            net.set_grads(_grads(300 + 10 * s + j, 0.02))
            opt.accumulate(w, last=j == 1)
        acc = [opt.accumulated_grad(p).cpu().numpy().copy() for p in net.params]
        opt.step()
        torch.cuda.synchronize()
        coef = float(opt._norm_out[1])
        assert 0.0 < coef <= 1.0 and (coef < 1.0) == (float(opt.last_grad_norm) > 1.0)
        for i in range(len(SIZES)):
            ref[i].step(acc[i], net.hyper(i)[0], gscale=coef)
    assert all(opt.state[p]["step"] == 3 for p in net.params)
    for i, p in enumerate(net.params):
        st = opt.state[p]
        ref[i].check(p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), f"accumulated {i}")


def test_dirty_ranges_are_recorded_per_job():
    net = _Net(track_dirty=True)
    opt = net.optimizer(multi_tensor=True)
    net.set_grads(_grads(400))
    opt.step()
    want = [(p.data_ptr(), p.data_ptr() + 4 * p.numel()) for p in net.params]
    assert sorted(net.flat._eav_dirty) == sorted(want)
    net.flat._eav_dirty = []
    one = _Net(track_dirty=True)
    oopt = one.optimizer(split=False, multi_tensor=True)          # one group: the five tensors merge into one job
    one.set_grads(_grads(400))
    oopt.step()
    lo = one.params[0].data_ptr()
    assert one.flat._eav_dirty == [(lo, one.params[-1].data_ptr() + 4 * SIZES[-1])]
    for _ in range(70):                                           # nobody drains the list: it collapses to its hull
        opt.step()
    assert len(net.flat._eav_dirty) <= 64 + 5
    assert min(a for a, _ in net.flat._eav_dirty) == want[0][0] and max(b for _, b in net.flat._eav_dirty) == want[-1][1]
    untracked = _Net()
    uopt = untracked.optimizer(multi_tensor=True)
    untracked.set_grads(_grads(400))
    uopt.step()
    assert not getattr(untracked.flat, "_eav_dirty", [])


def test_default_path_launches_group_by_group_and_records_each_launch(monkeypatch):
    """The default-path twin of test_dirty_ranges_are_recorded_per_job: one eav_adam_step per run, group 0's tensors by
    address and then group 1's, each with its group's lr and weight decay, and one dirty range per launch in that order."""
    net = _Net(track_dirty=True)
    opt = net.optimizer(multi_tensor=False)
    net.set_grads(_grads(400))
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    opt.step()
    monkeypatch.setattr(_lib, "call", real)
    order = [0, 2, 4, 1, 3]
    assert [name for name, _ in calls] == ["eav_adam_step"] * 5
    # (p, g, m, v, n, lr, beta1, beta2, eps, weight decay, step, decoupled, device step count, stream)
    assert [(a[0], a[4], a[5], a[9], a[10]) for _, a in calls] == \
        [(net.params[i].data_ptr(), SIZES[i], *net.hyper(i), 1) for i in order]
    want = [(p.data_ptr(), p.data_ptr() + 4 * p.numel()) for p in net.params]
    assert net.flat._eav_dirty == [want[i] for i in order]
    one = _Net(track_dirty=True)
    oopt = one.optimizer(split=False, multi_tensor=False)         # one group: the five tensors merge into one launch
    one.set_grads(_grads(400))
    oopt.step()
    assert one.flat._eav_dirty == [(one.params[0].data_ptr(), one.params[-1].data_ptr() + 4 * SIZES[-1])]
    for _ in range(70):                                           # nobody drains the list: it collapses to its hull
        opt.step()
    assert len(net.flat._eav_dirty) <= 64
    assert min(a for a, _ in net.flat._eav_dirty) == want[0][0] and max(b for _, b in net.flat._eav_dirty) == want[-1][1]
    untracked = _Net()
    uopt = untracked.optimizer(multi_tensor=False)
    untracked.set_grads(_grads(400))
    uopt.step()
    assert not getattr(untracked.flat, "_eav_dirty", [])
