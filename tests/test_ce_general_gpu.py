"""eav_ce_general_fwd_bwd (csrc/head_ce_soft.hip): cross-entropy with class weights, label smoothing and class-probability
targets against torch's F.cross_entropy in float64 (tests/ce_general_ref.py).

Parity rule, the one of test_wide_head_gpu._ce_check: the GPU's error against float64 may be at most twice the error of
torch's own fp32 CPU evaluation plus 1e-5 of the largest reference value.  Shapes: the lane stride (63, 64, 65 classes,
one class, 527) and the finish kernel's 64-row trips (1, 7, 64, 65, 300 rows).  Every output sits in a sentinel buffer
with a guard band."""
import pytest
import torch

from tests import ce_general_ref as ref
from tests import kernel_check as kc

pytestmark = pytest.mark.gpu

BS = [1, 7, 64, 65, 300]
NCS = [1, 5, 63, 64, 65, 527]
WEIGHTS = ["none", "random", "zero"]
EPS = [0.0, 0.1, 1.0]


def _run(logits, target, weight, eps, want_din=True, ncorrect=None, flag=None, want_loss=True):
    """One launch on sentinel buffers -> (loss, din) on the host."""
    from eav_amd import _lib
    B, NC = logits.shape
    soft = target.dtype != torch.int64
    ld, td = kc.dev(logits), kc.dev(target)
    wd = None if weight is None else kc.dev(weight)
    loss = kc.sentinel_buf(1) if want_loss else None
    din = kc.sentinel_buf(B * NC) if want_din else None
    nws = _lib.plain("eav_ce_general_ws_floats", B)
    ws = kc.sentinel_buf(nws)
    _lib.call("eav_ce_general_fwd_bwd", ld.data_ptr(), None if soft else td.data_ptr(), td.data_ptr() if soft else None,
              kc.ptr(wd), float(eps), kc.ptr(loss), kc.ptr(din), kc.ptr(ncorrect), kc.ptr(flag), ws.data_ptr(), B, NC,
              torch.cuda.current_stream().cuda_stream)
    kc.take(ws, nws, (nws,), "row terms")
    return (kc.take(loss, 1, (), "loss") if want_loss else None,
            kc.take(din, B * NC, (B, NC), "din") if want_din else None)


def _check(loss, din, logits, target, weight, eps, what):
    l64, g64 = ref.cross_entropy(logits, target, weight, eps, torch.float64)
    l32, g32 = ref.cross_entropy(logits, target, weight, eps, torch.float32)
    for name, g, r, c in (("loss", loss, l64, l32), ("din", din, g64, g32)):
        assert torch.isfinite(g).all(), (what, name)
        e_gpu, e_cpu = float((g.double() - r).abs().max()), float((c.double() - r).abs().max())
        lim = 2 * e_cpu + 1e-5 * float(r.abs().max())
        print(f"{what} {name}: GPU error {e_gpu:.3e}, CPU fp32 error {e_cpu:.3e}, limit {lim:.3e}")
        assert e_gpu <= lim, (what, name, e_gpu, lim)


@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("B", BS)
def test_index_targets(B, NC):
    logits, y = ref.planted_case(B, NC)
    hits = int(((logits.argmax(1) == y) & (y >= 0)).sum())                # torch's argmax: the first maximum
    if NC >= 3:
        assert int((logits[0] == logits[0].max()).sum()) == 2 and hits >= 1 and (B < 3 or int(logits[2].argmax()) == 1)
    for wk in WEIGHTS:
        w = ref.class_weights(wk, NC, kc.seed_of("w", B, NC))
        for eps in EPS:
            what = f"index B={B} NC={NC} weight={wk} eps={eps}"
            ncorrect = kc.dev(torch.full((1,), 5, dtype=torch.int32))
            flag = kc.dev(torch.zeros(1, dtype=torch.int32))
            loss, din = _run(logits, y, w, eps, ncorrect=ncorrect, flag=flag)
            assert int(ncorrect.cpu()) == 5 + hits and int(flag.cpu()) == 0, what
            if B > 1:
                assert not din[1].any(), what                             # the ignored row
            if ref.divisor(y, w, NC) == 0.0:                              # every valid label carries weight 0
                assert torch.isnan(loss) and not din.any(), what
                continue
            _check(loss, din, logits, y, w, eps, what)


@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("B", BS)
def test_probability_targets(B, NC):
    logits, _ = ref.planted_case(B, NC)
    t = ref.probability_targets(B, NC, kc.seed_of("t", B, NC))
    hits = int((logits.argmax(1) == t.argmax(1)).sum())
    for wk in WEIGHTS:
        w = ref.class_weights(wk, NC, kc.seed_of("w", B, NC))
        for eps in EPS:
            what = f"probabilities B={B} NC={NC} weight={wk} eps={eps}"
            ncorrect = kc.dev(torch.full((1,), 3, dtype=torch.int32))
            loss, din = _run(logits, t, w, eps, ncorrect=ncorrect)
            assert int(ncorrect.cpu()) == 3 + hits, what
            _check(loss, din, logits, t, w, eps, what)


@pytest.mark.parametrize("B,NC", [(7, 5), (65, 64), (300, 527)])
@pytest.mark.parametrize("eps", EPS)
def test_one_hot_probabilities_agree_with_the_index_path(B, NC, eps):
    """The two forms of the same targets: both inside the parity bound of the index reference (unweighted: with weights
    torch itself divides by the batch for probabilities and by the weights of the labels for indices)."""
    logits, y = ref.planted_case(B, NC)
    y = torch.where(y < 0, torch.zeros_like(y), y)                        # probabilities cannot say "ignored"
    onehot = torch.nn.functional.one_hot(y, NC).float()
    li, di = _run(logits, y, None, eps)
    lp, dp = _run(logits, onehot, None, eps)
    _check(li, di, logits, y, None, eps, f"index form B={B} NC={NC} eps={eps}")
    _check(lp, dp, logits, y, None, eps, f"one-hot form B={B} NC={NC} eps={eps}")


@pytest.mark.parametrize("B,NC", [(7, 5), (300, 527)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_zero_divisor_gives_nan_loss_and_zero_gradient(B, NC, eps):
    logits, y = ref.planted_case(B, NC)
    ncorrect, flag = kc.dev(torch.zeros(1, dtype=torch.int32)), kc.dev(torch.zeros(1, dtype=torch.int32))
    # every row ignored
    loss, din = _run(logits, torch.full((B,), -100, dtype=torch.int64), None, eps, ncorrect=ncorrect, flag=flag)
    assert torch.isnan(loss) and not din.any() and int(ncorrect.cpu()) == 0 and int(flag.cpu()) == 0
    # valid labels, all on classes of weight 0
    w = ref.class_weights("random", NC, 11)
    y2 = torch.where(torch.arange(B) % 2 == 0, torch.full((B,), 1, dtype=torch.int64), torch.full((B,), NC - 1, dtype=torch.int64))
    w[1], w[NC - 1] = 0.0, 0.0
    loss, din = _run(logits, y2, w, eps)
    assert torch.isnan(loss) and not din.any()


@pytest.mark.parametrize("B,NC", [(7, 5), (300, 527)])
def test_bad_label_is_reported_like_the_narrow_kernel(B, NC):
    from eav_amd import _lib
    logits, y = ref.planted_case(B, NC)
    w = ref.class_weights("random", NC, 12)
    bad = y.clone()
    bad[B - 1] = NC
    flag, old_flag = kc.dev(torch.zeros(1, dtype=torch.int32)), kc.dev(torch.zeros(1, dtype=torch.int32))
    loss, din = _run(logits, bad, w, 0.1, flag=flag)
    ld, yd = kc.dev(logits), kc.dev(bad)
    _lib.call("eav_ce_fwd_bwd", ld.data_ptr(), yd.data_ptr(), None, None, None, old_flag.data_ptr(), B, NC,
              torch.cuda.current_stream().cuda_stream)
    assert int(flag.cpu()) == int(old_flag.cpu()) == NC + 1
    assert not din[B - 1].any()
    as_ignored = y.clone()
    as_ignored[B - 1] = -100
    _check(loss, din, logits, as_ignored, w, 0.1, f"bad label as ignored B={B} NC={NC}")
    bad[B - 1] = -7
    flag.zero_()
    _run(logits, bad, w, 0.1, flag=flag)
    assert int(flag.cpu()) == -7


@pytest.mark.parametrize("soft", [False, True])
def test_hits_accumulate_and_runs_are_bit_equal(soft):
    B, NC = 300, 527
    logits, y = ref.planted_case(B, NC)
    target = ref.probability_targets(B, NC, 13) if soft else y
    w = ref.class_weights("random", NC, 14)
    hits = int((logits.argmax(1) == (target.argmax(1) if soft else y)).sum())
    ncorrect = kc.dev(torch.full((1,), 5, dtype=torch.int32))
    l1, d1 = _run(logits, target, w, 0.1, ncorrect=ncorrect)
    l2, d2 = _run(logits, target, w, 0.1, ncorrect=ncorrect)
    assert int(ncorrect.cpu()) == 5 + 2 * hits
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    l3, _ = _run(logits, target, w, 0.1, want_din=False, ncorrect=ncorrect)           # no gradient asked
    assert int(ncorrect.cpu()) == 5 + 3 * hits and torch.equal(l3.view(torch.int32), l1.view(torch.int32))
    _, d4 = _run(logits, target, w, 0.1, want_loss=False)                              # the gradient alone: no finish launch
    assert torch.equal(d4.view(torch.int32), d1.view(torch.int32))


def test_arguments_are_refused_on_the_host():
    from eav_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    a = kc.dev(torch.zeros(64))
    yl = kc.dev(torch.zeros(4, dtype=torch.int64))
    P = a.data_ptr()
    for args in ((P, yl.data_ptr(), P, None, 0.0, P, None, None, None, P, 4, 5),      # both kinds of target
                 (P, None, None, None, 0.0, P, None, None, None, P, 4, 5),            # neither
                 (P, yl.data_ptr(), None, None, 1.5, P, None, None, None, P, 4, 5),   # smoothing outside [0, 1]
                 (P, yl.data_ptr(), None, None, 0.0, P, None, None, None, P, 4, 32769),
                 (P, yl.data_ptr(), None, None, 0.0, P, None, None, None, None, 4, 5)):
        with pytest.raises(_lib.EavError, match="eav_ce_general_fwd_bwd"):
            _lib.call("eav_ce_general_fwd_bwd", *args, st)
    assert _lib.plain("eav_ce_general_ws_floats", 0) == 0 and _lib.plain("eav_ce_general_ws_floats", 7) == 14
