"""optim.CrossEntropyLoss(weight=..., label_smoothing=...) and class-probability targets: the default criterion still
launches eav_ce_fwd_bwd / eav_ce_wide_fwd_bwd with the same bits, anything else is eav_ce_general_fwd_bwd's result
handed through autograd unchanged, in accumulate() and inside a captured training step."""
import pytest
import torch

from tests import ce_general_ref as ref
from tests import kernel_check as kc

pytestmark = pytest.mark.gpu


def _direct(name, logits, y, extra=()):
    """loss, din of a direct library call on the device tensors."""
    from eav_amd import _lib
    B, NC = logits.shape
    loss, din = torch.zeros((), device="cuda"), torch.zeros(B, NC, device="cuda")
    flag = torch.zeros((), dtype=torch.int32, device="cuda")
    _lib.call(name, logits.data_ptr(), y.data_ptr(), loss.data_ptr(), din.data_ptr(), None, flag.data_ptr(), *extra, B, NC,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return loss, din


def _general(logits, target, weight, eps):
    from eav_amd import _lib
    B, NC = logits.shape
    soft = target.dtype != torch.int64
    loss, din = torch.zeros((), device="cuda"), torch.zeros(B, NC, device="cuda")
    ws = torch.zeros(_lib.plain("eav_ce_general_ws_floats", B), device="cuda")
    nc = torch.zeros((), dtype=torch.int32, device="cuda")
    _lib.call("eav_ce_general_fwd_bwd", logits.data_ptr(), None if soft else target.data_ptr(),
              target.data_ptr() if soft else None, kc.ptr(weight), float(eps), loss.data_ptr(), din.data_ptr(), nc.data_ptr(),
              None, ws.data_ptr(), B, NC, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return loss, din, nc


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("NC", [5, 527])
def test_defaults_launch_what_they_always_did(NC):
    from eav_amd import _lib
    from eav_amd.optim import CrossEntropyLoss
    logits, y = ref.planted_case(7, NC)
    ld, yd = logits.cuda(), y.cuda()
    if NC <= 16:
        want_loss, want_din = _direct("eav_ce_fwd_bwd", ld, yd)
    else:
        ws = torch.zeros(_lib.plain("eav_ce_wide_ws_floats", 7), device="cuda")
        want_loss, want_din = _direct("eav_ce_wide_fwd_bwd", ld, yd, (ws.data_ptr(),))
    crit = CrossEntropyLoss()
    assert crit.weight is None and crit.label_smoothing == 0.0
    calls = []
    real = _lib.call
    try:
        _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        s = ld.clone().requires_grad_(True)
        loss = crit(s, yd)
        loss.backward()
    finally:
        _lib.call = real
    # (loss.backward() seeds with a torch-made 1.0: the library's scaling launch follows and returns at once)
    assert [c for c in calls if c.startswith("eav_ce")] == ["eav_ce_fwd_bwd" if NC <= 16 else "eav_ce_wide_fwd_bwd"], calls
    assert torch.equal(_bits(loss), _bits(want_loss)) and torch.equal(_bits(s.grad), _bits(want_din))


@pytest.mark.parametrize("NC", [5, 527])
@pytest.mark.parametrize("soft", [False, True])
def test_options_hand_the_kernels_result_through(NC, soft):
    from eav_amd.optim import CrossEntropyLoss
    B = 7
    logits, y = ref.planted_case(B, NC)
    w = ref.class_weights("random", NC, 21)
    ld = logits.cuda()
    target = (ref.probability_targets(B, NC, 22) if soft else y).cuda()
    want_loss, want_din, want_hits = _general(ld, target, w.cuda(), 0.1)
    crit = CrossEntropyLoss(weight=w.tolist(), label_smoothing=0.1)
    assert crit.label_smoothing == 0.1 and torch.equal(crit.weight.cpu(), w)
    with pytest.raises(AttributeError):
        crit.label_smoothing = 0.2
    with pytest.raises(AttributeError):
        crit.weight = None
    crit.head_algo = "narrow"                                           # does not apply to the general kernel
    s = ld.clone().requires_grad_(True)
    loss = crit(s, target)
    loss.backward()
    assert crit.weight.is_cuda                                          # moved with the first scores
    assert torch.equal(_bits(loss), _bits(want_loss)) and torch.equal(_bits(s.grad), _bits(want_din))
    # a non-unit upstream gradient scales a copy: a second backward through the same node is not scaled twice
    s2 = ld.clone().requires_grad_(True)
    loss2 = crit(s2, target)
    (loss2 * 3.0).backward(retain_graph=True)
    assert torch.equal(_bits(s2.grad), _bits(want_din * 3.0))
    s2.grad = None
    loss2.backward()
    assert torch.equal(_bits(s2.grad), _bits(want_din))
    # accumulate(): the evaluation form
    out, hits = torch.zeros((), device="cuda"), torch.full((), 4, dtype=torch.int32, device="cuda")
    crit.accumulate(ld, target, out, hits)
    assert torch.equal(_bits(out), _bits(want_loss)) and int(hits) == 4 + int(want_hits)
    with torch.no_grad():                                               # no gradient buffer under no_grad
        assert torch.equal(_bits(crit(ld, target)), _bits(want_loss))
    crit.check()
    # soft targets alone (no weight, no smoothing) are not the default route either
    if soft:
        plain = CrossEntropyLoss()
        l0, d0, _ = _general(ld, target, None, 0.0)
        s3 = ld.clone().requires_grad_(True)
        plain(s3, target).backward()
        assert torch.equal(_bits(s3.grad), _bits(d0))


def test_wrong_weight_count_and_bad_labels_raise():
    from eav_amd import _lib
    from eav_amd.optim import CrossEntropyLoss
    logits, y = ref.planted_case(7, 5)
    with pytest.raises(ValueError, match="class weights"):
        CrossEntropyLoss(weight=[1.0, 2.0])(logits.cuda(), y.cuda())
    crit = CrossEntropyLoss(label_smoothing=0.1)
    bad = y.clone()
    bad[3] = 9
    crit(logits.cuda(), bad.cuda())
    with pytest.raises(_lib.EavError, match="target 9"):
        crit.check()


def test_graph_replay_equals_eager_with_options():
    """A captured step with a weighted, smoothed criterion at the small generic EEGNet shape: parameters and losses after
    five steps (two eager warm-ups, the capture, two replays) are bit-equal to the eager schedule's."""
    from eav_amd.eegnet import EEGNet_tor
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    from eav_amd.runtime import GraphStep
    from eav_amd import synth
    shape = dict(F1=4, D=2, F2=16, kernLength=32, Chans=5, Samples=128)
    B, n = 4, 12
    torch.manual_seed(7)
    sd = {k: v.clone() for k, v in EEGNet_tor(5, dropoutRate=0.0, **shape).state_dict().items()}
    x, y = synth.eeg_batch(31, n, 5, 128)
    xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    batches = [[(5 * s + 3 * j) % n for j in range(B)] for s in range(5)]
    finals = []
    for use_graph in (False, True):
        m = EEGNet_tor(5, dropoutRate=0.0, **shape)
        m.load_state_dict(sd)
        m = m.cuda().train()
        opt = FusedAdam(m.parameters(), lr=1e-3, capturable=True)
        crit = CrossEntropyLoss(weight=[0.5, 1.0, 2.0, 1.5, 0.75], label_smoothing=0.1)
        losses = []
        if use_graph:
            gs = GraphStep(m, opt, crit, xs, ys, B)
            for idx in batches:
                losses.append(gs.run(idx)[1].clone())
            assert gs.graph is not None
        else:
            for idx in batches:
                it = torch.as_tensor(idx, device="cuda")
                loss = crit(m(xs.index_select(0, it)), ys.index_select(0, it))
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        crit.check()
        finals.append((torch.stack(losses).cpu(), {k: v.clone() for k, v in m.state_dict().items()}))
    assert torch.equal(_bits(finals[0][0]), _bits(finals[1][0])), (finals[0][0], finals[1][0])
    for k in finals[0][1]:
        assert torch.equal(finals[0][1][k], finals[1][1][k]), k
    # the options are in force: the unweighted, unsmoothed loss of the first batch is another number
    m = EEGNet_tor(5, dropoutRate=0.0, **shape)
    m.load_state_dict(sd)
    m = m.cuda().train()
    it = torch.as_tensor(batches[0], device="cuda")
    plain = CrossEntropyLoss()(m(xs.index_select(0, it)), ys.index_select(0, it))
    assert float(plain.detach()) != float(finals[0][0][0])
