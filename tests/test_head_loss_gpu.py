"""csrc/head_loss.hip (eav_bce_logits_fwd_bwd, eav_mse_fwd_bwd) against torch on the CPU in float64, and the two criteria
of criteria.py on top of them.

Kernel rule, as tests/test_wide_head_gpu.py::_ce_check: GPU error <= 2 x (torch CPU fp32 error against float64) + 1e-5 x
max|reference|, for the loss and for every element of the gradient.  The reference loss is tests/problem_type_ref.loss,
which tests/test_problem_type_cpu.py pins to the Hugging Face classes.  Shapes: B around the four rows of a block and the
64 rows of a trip of the finish kernel, NC around the 64 lanes that stride a row."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import kernel_check as kc
from tests import problem_type_ref as ptr

pytestmark = pytest.mark.gpu

BS = [1, 4, 5, 65, 130]
NCS = [1, 2, 63, 64, 65, 527, 4097]
KINDS = {"bce": "multi_label_classification", "mse": "regression"}


def _case(kind, B, NC):
    """Logits N(0, 3^2) with one row linspace(-1e4, 1e4) and the elements x = 0, x = -0.0 with t = 0.5 planted (as many of
    the three as the shape has room for); BCE targets in {0, 1} with every seventh in (0, 1), MSE targets N(0, 1)."""
    s = kc.seed_of("head_loss", kind, B, NC)
    x = kc.normal(s, (B, NC), 3.0)
    if kind == "bce":
        t = torch.from_numpy((synth.uniform(s + 1, (B, NC)) < 0.3).astype(np.float32))
        frac = torch.from_numpy(synth.uniform(s + 2, (B, NC)).astype(np.float32))
        soft = (torch.arange(B * NC).view(B, NC) % 7) == 3
        t[soft] = frac[soft]
    else:
        t = kc.normal(s + 1, (B, NC))
    x[B - 1] = torch.linspace(-1e4, 1e4, NC)
    first = NC // 2 if B == 1 and NC >= 3 else 0      # one row only: plant in the middle of the ramp, keep its two ends
    for k, v in enumerate((0.0, -0.0)):
        if first + k < B * NC:
            x.view(-1)[first + k], t.view(-1)[first + k] = v, 0.5
    if B * NC > 1:
        assert (x == 0).sum() >= 2 and bool(torch.signbit(x.view(-1)[first + 1]))
    return x, t


def _run(kind, x, t, want_din=True, nhits=None):
    from eav_amd import _lib
    B, NC = x.shape
    xd, td = kc.dev(x), kc.dev(t)
    nws = _lib.plain("eav_head_loss_ws_floats", B)
    assert nws == 2 * B
    loss, din, ws = kc.sentinel_buf(1), kc.sentinel_buf(B * NC) if want_din else None, kc.sentinel_buf(nws)
    st = torch.cuda.current_stream().cuda_stream
    if kind == "bce":
        _lib.call("eav_bce_logits_fwd_bwd", xd.data_ptr(), td.data_ptr(), loss.data_ptr(), kc.ptr(din), kc.ptr(nhits),
                  ws.data_ptr(), B, NC, st)
        kc.take(ws, 2 * B, (2 * B,), "row terms and row hits")
    else:
        _lib.call("eav_mse_fwd_bwd", xd.data_ptr(), td.data_ptr(), loss.data_ptr(), kc.ptr(din), ws.data_ptr(), B, NC, st)
        kc.take(ws, B, (B,), "row terms")                     # the hit half of the scratch is not MSE's to write
    return kc.take(loss, 1, (), "loss"), (kc.take(din, B * NC, (B, NC), "dlogits") if want_din else None)


def _check(kind, loss, din, x, t):
    r64 = x.double().requires_grad_(True)
    l64 = ptr.loss(r64, t, KINDS[kind])
    l64.backward()
    r32 = x.clone().requires_grad_(True)
    l32 = ptr.loss(r32, t, KINDS[kind])
    l32.backward()
    for name, g, ref, c in (("loss", loss, l64.detach(), l32.detach()), ("dlogits", din, r64.grad, r32.grad)):
        assert torch.isfinite(g).all(), name
        e_gpu, e_cpu = float((g.double() - ref).abs().max()), float((c.double() - ref).abs().max())
        lim = 2 * e_cpu + 1e-5 * float(ref.abs().max())
        print(f"{kind} {name} {tuple(x.shape)}: GPU error {e_gpu:.3e}, CPU fp32 error {e_cpu:.3e}, limit {lim:.3e}")
        assert e_gpu <= lim, (name, e_gpu, lim)


@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("B", BS)
def test_bce_logits_kernel(B, NC):
    x, t = _case("bce", B, NC)
    nhits = kc.dev(torch.full((1,), 5, dtype=torch.int32))
    loss, din = _run("bce", x, t, nhits=nhits)
    _check("bce", loss, din, x, t)
    hits = int(((x > 0) == (t > 0.5)).sum())
    assert int(nhits.cpu()) == 5 + hits                                   # exact, onto the start value
    loss2, _ = _run("bce", x, t, want_din=False, nhits=nhits)             # no gradient asked: the same loss bits
    assert int(nhits.cpu()) == 5 + 2 * hits
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    loss3, din3 = _run("bce", x, t)                                       # no hit count asked; two runs, the same bits
    assert torch.equal(loss3.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(din3.view(torch.int32), din.view(torch.int32))
    assert int(nhits.cpu()) == 5 + 2 * hits


@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("B", BS)
def test_mse_kernel(B, NC):
    x, t = _case("mse", B, NC)
    loss, din = _run("mse", x, t)
    _check("mse", loss, din, x, t)
    loss2, _ = _run("mse", x, t, want_din=False)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    loss3, din3 = _run("mse", x, t)
    assert torch.equal(loss3.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(din3.view(torch.int32), din.view(torch.int32))


def test_head_loss_kernels_refuse_shapes_outside_their_range():
    """Refused on the host, before anything is launched: classes beyond EAV_HEAD_MAX_CLASSES, B x NC = 2^31, no scratch."""
    from eav_amd import _lib
    buf = kc.dev(torch.zeros(64))
    st = torch.cuda.current_stream().cuda_stream
    p = buf.data_ptr()
    for B, NC, ws in ((1, 32769, p), (65536, 32768, p), (4, 0, p), (0, 4, p), (4, 4, None)):
        with pytest.raises(_lib.EavError, match="bad arguments"):
            _lib.call("eav_bce_logits_fwd_bwd", p, p, p, None, None, ws, B, NC, st)
        with pytest.raises(_lib.EavError, match="bad arguments"):
            _lib.call("eav_mse_fwd_bwd", p, p, p, None, ws, B, NC, st)
    assert _lib.plain("eav_head_loss_ws_floats", 0) == 0


# ------------------------------------------------------------------------------------------------------------ criteria
@pytest.mark.parametrize("kind", ["bce", "mse"])
def test_criteria(kind):
    from eav_amd.optim import BCEWithLogitsLoss, MSELoss, unit_gradient
    B, NC = 5, 65
    x, t = _case(kind, B, NC)
    _, kernel_grad = _run(kind, x, t)
    crit = (BCEWithLogitsLoss if kind == "bce" else MSELoss)()
    td = t.cuda()
    s = x.cuda().requires_grad_(True)
    loss = crit(s, td)
    loss.backward(retain_graph=True)
    assert torch.equal(s.grad.cpu(), kernel_grad)                          # the forward launch's gradient, untouched
    s.grad = None
    loss.backward(gradient=unit_gradient(loss.device), retain_graph=True)  # the recognised seed: nothing scaled
    assert torch.equal(s.grad.cpu(), kernel_grad)
    s.grad = None
    (3 * loss).backward(retain_graph=True)
    assert torch.equal(s.grad.cpu(), 3 * kernel_grad)
    s.grad = None
    (3 * loss).backward()                                                  # a second backward is not scaled twice
    assert torch.equal(s.grad.cpu(), 3 * kernel_grad)
    crit.check()
    assert len(crit._scratch) == 1                                         # one cached buffer, none per call

    # evaluation form: the same loss bits, hits added on the device
    lo = torch.zeros((), device="cuda")
    if kind == "bce":
        nh = torch.full((), 7, dtype=torch.int32, device="cuda")
        crit.accumulate(s.detach(), td, lo, nh)
        assert int(nh) == 7 + int(((x > 0) == (t > 0.5)).sum())
    else:
        crit.accumulate(s.detach(), td, lo)
    assert torch.equal(lo.view(torch.int32), loss.detach().view(torch.int32))
    assert len(crit._scratch) == 1

    # no gradient buffer under no_grad: the loss scalar is all that is allocated
    big = torch.zeros(130, 4097, device="cuda")
    bt = torch.zeros(130, 4097, device="cuda")
    crit(big, bt)                                                          # the scratch of this batch size exists now
    torch.cuda.synchronize()
    # (device tensors that earlier tests left in reference cycles go now, not at a collection between the two readings:
    # with more tests in front of this one such a collection fell here and freed 160 MB in the middle)
    import gc
    gc.collect()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        l0 = crit(big.requires_grad_(True), bt)
    assert l0.grad_fn is None and torch.cuda.memory_allocated() - before < big.numel() * 4
    l1 = crit(big, bt)
    assert l1.grad_fn is not None and torch.cuda.memory_allocated() - before >= big.numel() * 4
    assert torch.equal(l0, l1)


def test_criteria_targets():
    """[B] targets for one class, integer targets converted to fp32, shapes and devices checked."""
    from eav_amd import _lib
    from eav_amd.optim import BCEWithLogitsLoss, MSELoss
    x = kc.normal(3, (6, 1)).cuda()
    t = kc.normal(4, (6,)).cuda()
    mse = MSELoss()
    assert torch.equal(mse(x, t), mse(x, t.view(6, 1)))
    ti = torch.tensor([0, 1, 1, 0, 1, 0], device="cuda")
    bce = BCEWithLogitsLoss()
    assert torch.equal(bce(x, ti), bce(x, ti.float().view(6, 1)))
    x3 = kc.normal(5, (6, 3)).cuda()
    for crit in (mse, bce):
        with pytest.raises(_lib.EavError, match="targets"):
            crit(x3, t)                                                    # [B] only for one class
        with pytest.raises(_lib.EavError, match="targets"):
            crit(x3, torch.zeros(5, 3, device="cuda"))
        with pytest.raises(_lib.EavError, match="device"):
            crit(x3, torch.zeros(6, 3))
        with pytest.raises(_lib.EavError, match="contiguous"):
            crit(x3.t(), torch.zeros(3, 6, device="cuda"))
