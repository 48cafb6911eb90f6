"""FusedAdam.set_averaging at the optimiser level: a module of five tensors of odd sizes in two param groups - put through
flatten_parameters, or left as loose tensors - twelve steps with some tensors without a gradient at first; the averages
within the bound of tests/weight_avg_ref.py against float64 driven with the GPU's own parameters; parameters bit-equal to
the same run without averaging under clipping, accumulation and a schedule; a captured step; averaged_parameters() on a
split-precision Encoder; the state_dict round trip."""
import copy

import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import weight_avg_ref as R

pytestmark = pytest.mark.gpu

SIZES = [7, 64, 1, 8197, 300]
LR, LR2, B1, B2, EPS_ADAM, WD = (float(np.float32(v)) for v in (1e-3, 2.5e-4, 0.9, 0.999, 1e-8, 0.01))


class _Net:
    def __init__(self, flat=True, seed=1):
        from eav_amd.optim import flatten_parameters
        self.host = [synth.normal(seed + i, (n,)).astype(np.float32) for i, n in enumerate(SIZES)]
        self.params = [torch.nn.Parameter(torch.from_numpy(h.copy()).cuda()) for h in self.host]
        self.is_flat = flat
        if flat:
            self.module = torch.nn.Module()
            for i, p in enumerate(self.params):
                self.module.register_parameter(f"w{i}", p)
            self.flat, self.gflat, self.offsets = flatten_parameters(self.module)

    def set_grads(self, grads):
        """grads[i] None: the tensor has no gradient in this step."""
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
            elif self.is_flat:
                off, n = self.offsets[f"w{i}"]
                view = self.gflat[off:off + n].view(p.shape)
                view.copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)))
                p.grad = view
            else:
                p.grad = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()

    def optimizer(self, split=True, **kw):
        """split: tensors 0, 2, 4 in a group (LR, WD), tensors 1, 3 in one (LR2, no decay)."""
        from eav_amd.optim import FusedAdam
        kw.setdefault("decoupled", True)
        groups = ([{"params": self.params[0::2], "lr": LR, "weight_decay": WD},
                   {"params": self.params[1::2], "lr": LR2, "weight_decay": 0.0}] if split
                  else [{"params": self.params, "lr": LR, "weight_decay": WD}])
        return FusedAdam(groups, betas=(B1, B2), eps=EPS_ADAM, **kw)


def _grads(seed, gain=1.0):
    return [synth.normal(seed + i, (n,)).astype(np.float32) * np.float32(gain) for i, n in enumerate(SIZES)]


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same_params(a, oa, b, ob, what):
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        assert np.array_equal(_bits(p), _bits(q)), (what, "p", i)
        for k in ("exp_avg", "exp_avg_sq"):
            assert np.array_equal(_bits(oa.state[p][k]), _bits(ob.state[q][k])), (what, k, i)


def _log_calls(monkeypatch):
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("kind,kw", [("ema", dict(decay=0.9)), ("swa", dict(start_step=3, every=2)),
                                     ("ema", dict(decay=0.999, warmup=True))])
def test_twelve_steps_with_late_tensors(flat, kind, kw, monkeypatch):
    """Tensors 1 and 3 have no gradient in the first four steps (the frozen phase): their averages stay the parameters'
    bits, and from step 5 on they are averaged with the coefficient of the global count."""
    from eav_amd.optim import WeightAveraging
    net, twin = _Net(flat), _Net(flat)
    opt, topt = net.optimizer(), twin.optimizer(multi_tensor=True)
    avg = WeightAveraging(kind, **kw)
    opt.set_averaging(avg)
    assert opt.multi_tensor and opt.averaging is avg
    for p, h in zip(net.params, net.host):
        a = opt.state[p]["avg"]
        assert a.shape == p.shape and a.data_ptr() != p.data_ptr() and np.array_equal(_bits(a), h.view(np.int32))
    if flat:                                            # one flat buffer laid out like the parameters
        base = opt.state[net.params[0]]["avg"].data_ptr() - net.params[0].data_ptr()
        assert all(opt.state[p]["avg"].data_ptr() - p.data_ptr() == base for p in net.params)
    assert opt.n_averaged.dim() == 0 and opt.n_averaged.is_cuda and opt.n_averaged.dtype == torch.int64
    refs = [R.Tracked(h) for h in net.host]
    names = _log_calls(monkeypatch)
    n = 0
    for s in range(1, 13):
        g = _grads(50 + 10 * s)
        if s <= 4:
            g[1] = g[3] = None
        net.set_grads(g)
        twin.set_grads(g)
        names.clear()
        opt.step()
        assert names == ["eav_adam_jobs_begin_avg", "eav_adam_step_jobs_avg"], names
        names.clear()
        topt.step()
        assert names == ["eav_adam_jobs_begin", "eav_adam_step_jobs"], names
        torch.cuda.synchronize()
        mode, c = avg.mode_and_coefficient(s, n)
        assert (mode, c) == R.mode_and_coefficient(kind, s, n, **kw)
        n += mode != "skip"
        for i, (p, ref) in enumerate(zip(net.params, refs)):
            if g[i] is not None:
                ref.update(mode, float(R.coefficient_f32(c)), p.detach().cpu().numpy())
            elif s <= 4:
                assert np.array_equal(_bits(opt.state[p]["avg"]), net.host[i].view(np.int32)), (s, i)
                assert np.array_equal(_bits(p), net.host[i].view(np.int32))
    assert int(opt.n_averaged) == n and n == (12 if "start_step" not in kw else 5)
    _same_params(net, opt, twin, topt, "averaging does not perturb the step")
    worst = max(ref.check(opt.state[p]["avg"].cpu().numpy(), f"{kind} flat={flat} tensor {i}")
                for i, (p, ref) in enumerate(zip(net.params, refs)))
    assert worst > 0.01 and all(ref.updates >= 4 for ref in refs)
    assert "avg" not in topt.state[twin.params[0]] and set(topt.state_dict()) == {"state", "param_groups"}
    if flat:
        one = _Net(True)
        oopt = one.optimizer(split=False)
        oopt.set_averaging(WeightAveraging(kind, **kw))
        one.set_grads(_grads(1))
        oopt.step()
        (table,) = oopt._adam_tables.values()
        assert table.njobs == 1 and table.avgs.numel() == 1           # adjacent tensors stay adjacent: one job
    opt.set_averaging(None)
    assert opt.averaging is None and opt.n_averaged is None and all("avg" not in opt.state[p] for p in net.params)
    names.clear()
    opt.step()
    assert names == ["eav_adam_jobs_begin", "eav_adam_step_jobs"], names


@pytest.mark.parametrize("option", ["clip", "accumulate", "cosine"])
def test_parameters_are_bit_equal_to_the_run_without_averaging(option):
    from eav_amd.optim import LRSchedule, WeightAveraging
    a, b = _Net(), _Net()
    kw = dict(max_grad_norm=1.0) if option != "cosine" else {}
    oa, ob = a.optimizer(multi_tensor=True, **kw), b.optimizer(multi_tensor=True, **kw)
    if option == "cosine":
        for o in (oa, ob):
            o.set_schedule(LRSchedule("cosine", 2, 6))
    oa.set_averaging(WeightAveraging("ema", 0.9))
    refs = None
    for s in range(6):
        if option == "accumulate":
            for j, w in enumerate((0.25, 0.75)):
                g = _grads(300 + 10 * s + j, 0.02)
                for net, o in ((a, oa), (b, ob)):
                    net.set_grads(g)
                    o.accumulate(w, last=j == 1)
        else:
            g = _grads(300 + 10 * s, (1.0, 0.05, 0.001)[s % 3])
            a.set_grads(g)
            b.set_grads(g)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        _same_params(a, oa, b, ob, f"{option} step {s}")
        if option != "cosine":
            assert float(oa.last_grad_norm) == float(ob.last_grad_norm)
        else:
            assert _bits(oa.last_lr) == _bits(ob.last_lr)
        ps = [p.detach().cpu().numpy() for p in a.params]
        if refs is None:
            refs = [R.Tracked(p) for p in ps]
        for ref, p in zip(refs, ps):
            ref.update("copy" if s == 0 else "lerp", float(np.float32(1.0 - 0.9)), p)
    assert int(oa.n_averaged) == 6
    for i, (p, ref) in enumerate(zip(a.params, refs)):
        ref.check(oa.state[p]["avg"].cpu().numpy(), f"{option} tensor {i}")


def test_captured_step_averages_on_every_replay():
    """One eager step, then step() captured once and replayed five times: the bits of six eager steps, with a schedule
    and a gating that skips, copies and lerps inside the replays."""
    from eav_amd.optim import LRSchedule, WeightAveraging
    a, b = _Net(), _Net()
    oa, ob = a.optimizer(capturable=True), b.optimizer(capturable=True)
    for o in (oa, ob):
        o.set_schedule(LRSchedule("cosine", 2, 6))
        o.set_averaging(WeightAveraging("ema", 0.9, start_step=2, every=2))
    g = _grads(170)
    a.set_grads(g)
    b.set_grads(g)
    for _ in range(6):
        ob.step()
    oa.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert int(oa.n_averaged) == 3 == int(ob.n_averaged) and oa._avg_rec.cpu().tolist() == ob._avg_rec.cpu().tolist()
    assert oa._avg_rec.cpu().tolist()[0] == 6
    _same_params(a, oa, b, ob, "captured")
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        assert np.array_equal(_bits(oa.state[p]["avg"]), _bits(ob.state[q]["avg"])), i
        assert not np.array_equal(_bits(oa.state[p]["avg"]), _bits(p)) and \
            not np.array_equal(_bits(oa.state[p]["avg"]), a.host[i].view(np.int32))


def test_averaged_parameters_on_a_split_precision_encoder():
    """Inside the block the Encoder computes with the averages - its logits are those of a fresh Encoder built from the
    averaged state_dict, bit for bit as two such models agree (test_transformer_model_gpu.py) - and after it the
    original logits return bit for bit: the swapped ranges reach the operand planes both ways."""
    from eav_amd import transformer as T
    from eav_amd.optim import CrossEntropyLoss, FusedAdam, WeightAveraging
    cfg = T.make_config("vit", hidden=128, layers=2, heads=2, ff=256)
    torch.manual_seed(11)
    x, y = synth.frame_batch(5, 2)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    model = T.Encoder(cfg).cuda().train()
    model.precision = "split"
    opt = FusedAdam(model.parameters(), lr=1e-2, weight_decay=0.01, decoupled=True)
    opt.set_averaging(WeightAveraging("ema", 0.5))
    for _ in range(3):
        opt.zero_grad()
        CrossEntropyLoss()(model(xd).logits, yd).backward()
        opt.step()
    model.eval()

    def logits_of(m):
        with torch.no_grad():
            return m(xd).logits.clone()

    last = logits_of(model)
    last_state = {k: v.clone() for k, v in model.state_dict().items()}
    avgs = {k: opt.state[p]["avg"].clone() for k, p in model.named_parameters()}
    with opt.averaged_parameters():
        inside = logits_of(model)
        state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        for k, p in model.named_parameters():
            assert torch.equal(p.view(torch.int32), avgs[k].view(torch.int32)), k
            assert torch.equal(opt.state[p]["avg"].view(torch.int32), last_state[k].view(torch.int32)), k
        with pytest.raises(_lib.EavError, match="does not nest"):
            with opt.averaged_parameters():
                pass
        with pytest.raises(_lib.EavError, match="inside averaged_parameters"):
            opt.step()
        with pytest.raises(_lib.EavError, match="inside averaged_parameters"):
            opt.set_averaging(None)
    fresh = T.Encoder(cfg, state).cuda().eval()
    fresh.precision = "split"
    assert torch.equal(inside, logits_of(fresh))
    assert not torch.equal(inside, last)
    assert torch.equal(logits_of(model), last), "the last iterate did not return"
    for k, p in model.named_parameters():
        assert torch.equal(p.view(torch.int32), last_state[k].view(torch.int32)), k
        assert torch.equal(opt.state[p]["avg"].view(torch.int32), avgs[k].view(torch.int32)), k
    opt.zero_grad()
    model.train()
    CrossEntropyLoss()(model(xd).logits, yd).backward()
    opt.step()                                              # and training goes on
    assert int(opt.n_averaged) == 4


@pytest.mark.parametrize("flat", [True, False])
def test_state_dict_round_trip(flat):
    from eav_amd.optim import WeightAveraging
    a, b = _Net(flat), _Net(flat, seed=40)
    oa, ob = a.optimizer(), b.optimizer()
    oa.set_averaging(WeightAveraging("swa", start_step=2, every=2))
    for s in range(5):
        a.set_grads(_grads(500 + s))
        oa.step()
    sd = copy.deepcopy(oa.state_dict())                     # (as torch.save / torch.load hand it on: no shared storage)
    assert sd["averaging"] == dict(kind="swa", decay=0.999, warmup=False, start_step=2, every=2, s=5, n=2)
    assert all("avg" in st for st in sd["state"].values())
    with torch.no_grad():
        for p, q in zip(a.params, b.params):
            q.copy_(p)
    ob.load_state_dict(sd)
    assert ob.averaging == oa.averaging and ob.multi_tensor and ob._avg_rec.cpu().tolist()[:2] == [5, 2]
    for p, q in zip(a.params, b.params):
        assert np.array_equal(_bits(oa.state[p]["avg"]), _bits(ob.state[q]["avg"]))
        assert ob.state[q]["avg"].data_ptr() != oa.state[p]["avg"].data_ptr()
    g = _grads(600)
    for net, o in ((a, oa), (b, ob)):
        net.set_grads(g)
        o.step()                                            # step 6: a lerp with c = 1 / 3
    torch.cuda.synchronize()
    assert int(ob.n_averaged) == 3
    for p, q in zip(a.params, b.params):
        assert np.array_equal(_bits(p), _bits(q))
        assert np.array_equal(_bits(oa.state[p]["avg"]), _bits(ob.state[q]["avg"]))
    ob.load_state_dict(b.optimizer().state_dict())          # a state without averaging turns it off
    assert ob.averaging is None and all("avg" not in st for st in ob.state.values())
