"""The video CNN (eav_amd.cnn_vision.VideoModel, csrc/video_cnn.hip) against the plain-torch restatement of
tests/video_cnn_ref.py.

Parity rule, per tensor (logits, loss, every gradient, every running statistic): the GPU's max |error| against the
float64 restatement must be at most RATIO = 2 times CPU torch fp32's own max |error| against it, plus a floor of
FLOOR x max|reference| (for the loss, x max|logits|, whose error it inherits).  CPU torch fp32's error is the larger of
its NCHW and its channels-last run (two summation orders).

Both references take the GPU's routing (gpu_routes): the argmax of both max pools and the gate of every ReLU.  A tie,
or a pre-activation within rounding of zero, may be decided differently by two implementations, and the decision moves
a whole gradient element; with a random 50-layer trunk such flips otherwise dominate the comparison.  The AdamW step is
checked from the GPU's own gradients."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import video_cnn_ref as ref

pytestmark = pytest.mark.gpu

FLOOR = 1e-5
RATIO = 2


def make_model(seed=0, num_labels=5):
    from eav_amd.cnn_vision import VideoModel
    torch.manual_seed(seed)
    m = VideoModel(num_labels)
    # BatchNorm affine and running statistics away from their 1 / 0 init, so that every term of the step is exercised
    with torch.no_grad():
        for i, (k, v) in enumerate(m.state_dict().items()):
            if k.endswith("bn3.weight") or k.endswith("downsample.1.weight"):
                # residual branches scaled down (the role of torchvision's zero_init_residual): the random 50-layer
                # trunk stays well conditioned, so that fp32 rounding is not amplified beyond what it measures
                v.copy_(torch.from_numpy(synth.uniform(100 + i, tuple(v.shape), 0.1, 0.3)))
            elif k.endswith("bn1.weight") or k.endswith("bn2.weight") or k == "feature_extractor.1.weight":
                v.copy_(torch.from_numpy(synth.uniform(100 + i, tuple(v.shape), 0.7, 1.3)))
            elif k.startswith("attn_fc") and k.endswith(".weight"):
                v.mul_(0.1)
            elif k.endswith(".bias") and not k.startswith(("attn", "classifier")):
                v.copy_(torch.from_numpy(synth.uniform(100 + i, tuple(v.shape), -0.2, 0.2)))
            elif k.endswith("running_mean"):
                v.copy_(torch.from_numpy(synth.uniform(100 + i, tuple(v.shape), -0.1, 0.1)))
            elif k.endswith("running_var"):
                v.copy_(torch.from_numpy(synth.uniform(100 + i, tuple(v.shape), 0.5, 1.5)))
    return m


def batch(seed, B, H, W, nc=5):
    x = torch.from_numpy(synth.normal(seed, (B, 3, H, W), 0.0, 1.0))
    y = torch.from_numpy((synth.splitmix64(seed + 1, B) % np.uint64(nc)).astype(np.int64))
    return x, y


def check(name, gpu, r64, c32, scale=None):
    """c32: one CPU fp32 result or a tuple of them (the worst counts); scale: the magnitude the floor is relative to
    (default max |reference|; the loss uses its logits')."""
    gpu, r64 = gpu.double().cpu(), r64.double()
    c32 = c32 if isinstance(c32, tuple) else (c32,)
    eg = float((gpu - r64).abs().max())
    ec = max(float((c.double() - r64).abs().max()) for c in c32)
    tol = RATIO * ec + FLOOR * (float(r64.abs().max()) if scale is None else scale) + 1e-30
    assert eg <= tol, f"{name}: GPU error {eg:.3e} > {RATIO} x CPU fp32 error {ec:.3e} + floor ({tol:.3e})"
    return eg, ec


def run_gpu_step(m, x, y, lr=None):
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    m = m.cuda().train()
    opt = FusedAdam(m.parameters(), lr=lr or 1e-3, weight_decay=0.01, decoupled=True) if lr else None
    out = m(x.cuda())
    loss = CrossEntropyLoss()(out, y.cuda())
    loss.backward()
    grads = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    if opt is not None:
        opt.step()
    torch.cuda.synchronize()
    return out.detach().cpu(), loss.detach().cpu(), grads, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def gpu_routes(m):
    """The routing of the model's last forward: the stem MaxPool's window argmax [B,64,PH,PW] as torch's flat indices into
    the stem map, the head's max-pool argmax [B,2048] as positions in the final map, and every ReLU's gate (stored
    output > 0) in NCHW."""
    ws = m._ws
    B, PH, PW = ws.B, ws.PH, ws.PW
    SW = ws.stem.OW
    w = ws.pidx.view(B, PH, PW, 64).permute(0, 3, 1, 2).long().cpu()
    oh = torch.arange(PH).view(1, 1, PH, 1)
    ow = torch.arange(PW).view(1, 1, 1, PW)
    ih, iw = 2 * oh - 1 + w // 3, 2 * ow - 1 + w % 3

    def gate(u):
        return (ws.a[id(u)][:u.M * u.Co].view(B, u.OH, u.OW, u.Co) > 0).permute(0, 3, 1, 2).cpu()

    gates = {"stem": gate(ws.stem), "h": (ws.h[:B * 1024].view(B, 1024) > 0).cpu()}
    for i, (u1, u2, u3, _) in enumerate(ws.blocks):
        gates[(i, 1)], gates[(i, 2)], gates[(i, 3)] = gate(u1), gate(u2), gate(u3)
    return ih * SW + iw, ws.hidx.view(B, 2048).long().cpu(), gates


ROUTE_TOL = 1e-4      # a routing decision may differ from float64's only between values this close (x max |map|)


def check_routes_agree(routes, rec):
    """Every GPU routing decision is float64's, except between values within rounding of each other: a ReLU gate may
    differ only where |float64 pre-activation| <= ROUTE_TOL x max |pre-activation| of that map, a max-pool argmax only
    where its float64 value is within ROUTE_TOL x max |map| of the window's float64 maximum."""
    import torch.nn.functional as F
    pool_idx, head_idx, gates = routes
    for key, gate in gates.items():
        pre = rec[key]
        flip = gate != (pre > 0)
        lim = ROUTE_TOL * float(pre.abs().max())
        assert bool((pre[flip].abs() <= lim).all()), \
            f"ReLU {key}: {int(flip.sum())} gates differ from float64, up to |pre| {float(pre[flip].abs().max()):.3e}"
    a = F.relu(rec["stem"])
    gap = F.max_pool2d(a, 3, 2, 1) - ref._routed_pool(a, pool_idx)
    assert float(gap.max()) <= ROUTE_TOL * float(a.max()), f"stem MaxPool argmax off by {float(gap.max()):.3e}"
    y = F.relu(rec[(len(ref.block_names()) - 1, 3)])
    gap = y.flatten(2).max(2).values - ref._routed_pool(y, head_idx)
    assert float(gap.max()) <= ROUTE_TOL * float(y.max()), f"head max-pool argmax off by {float(gap.max()):.3e}"


def compare_step(B, H, W, seed, lr=1e-3):
    m = make_model(seed)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    x, y = batch(seed + 7, B, H, W)
    logits, loss, grads, sd1 = run_gpu_step(m, x, y, lr=lr)
    # both references pool with the GPU's argmax and gate with its ReLU decisions: a tie, or a near-tie within rounding,
    # decided differently would move a whole gradient element (the conditions of the comparison, not an error of either)
    routes = gpu_routes(m)
    rec = {}
    l64, s64, g64, o64 = ref.step(sd0, x, y, dtype=torch.float64, routes=routes, record=rec)
    check_routes_agree(routes, rec)
    l32, s32, g32, o32 = ref.step(sd0, x, y, dtype=torch.float32, routes=routes)
    l3c, s3c, g3c, o3c = ref.step(sd0, x, y, dtype=torch.float32, routes=routes, channels_last=True)
    check("logits", logits, l64, (l32, l3c))
    check("loss", loss.reshape(()), s64, (s32, s3c), scale=float(l64.abs().max()))
    for k in g64:
        check(f"grad {k}", grads[k], g64[k], (g32[k], g3c[k]))
    for k in o64:
        if k.endswith(("running_mean", "running_var")):
            check(k, sd1[k], o64[k], (o32[k], o3c[k]))
        elif k.endswith("num_batches_tracked"):
            assert int(sd1[k]) == int(o64[k]) == 1, k
    # AdamW (weight decay 0.01, decoupled) from the GPU's own gradients: torch.optim.AdamW in float64
    for k, g in grads.items():
        p64 = sd0[k].double().clone().requires_grad_(True)
        p64.grad = g.double()
        torch.optim.AdamW([p64], lr=lr).step()
        err = float((sd1[k].double() - p64.detach()).abs().max())
        assert err <= 1e-6 * float(p64.detach().abs().max()) + 1e-9, f"param {k} after AdamW: {err:.3e}"


def test_train_step_parity_b4():
    compare_step(4, 112, 112, 11)


def test_train_step_parity_b32_224():
    compare_step(32, 224, 224, 12)


def test_odd_image_size_and_b1():
    compare_step(1, 93, 125, 13)


def test_frozen_step_leaves_backbone_and_advances_bn():
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    m = make_model(3).cuda()
    for p in m.feature_extractor.parameters():
        p.requires_grad = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=0.01, decoupled=True)
    x, y = batch(5, 4, 64, 64)
    m.train()
    opt.zero_grad()
    loss = CrossEntropyLoss()(m(x.cuda()), y.cuda())
    loss.backward()
    head_grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
    opt.step()
    torch.cuda.synchronize()
    sd1 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    named = dict(m.named_parameters())
    for k, v in sd0.items():
        if k.startswith("feature_extractor.") and k in named:
            assert torch.equal(v, sd1[k]), f"{k} changed in a frozen step"
            assert not opt.state.get(named[k]), f"{k} has AdamW state"
        elif k.endswith("num_batches_tracked"):
            assert int(sd1[k]) == int(v) + 1, k
        elif k.endswith("running_mean"):
            assert not torch.equal(v, sd1[k]), f"{k} did not advance"
    l64, s64, g64, o64 = ref.step(sd0, x, y, freeze=True, dtype=torch.float64)
    l32, s32, g32, o32 = ref.step(sd0, x, y, freeze=True, dtype=torch.float32)
    assert set(head_grads) == {k for k, g in g64.items() if g is not None}
    for k, g in head_grads.items():
        check(f"grad {k}", g, g64[k], g32[k])
    for k in o64:
        if k.endswith(("running_mean", "running_var")):
            check(k, sd1[k], o64[k], o32[k])


def test_eval_uses_running_stats():
    m = make_model(4).cuda().eval()
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, _ = batch(6, 3, 64, 64)
    with torch.no_grad():
        out = m(x.cuda()).cpu()
    s64 = {k: v.clone() for k, v in sd0.items()}
    s32 = {k: v.clone() for k, v in sd0.items()}
    with torch.no_grad():
        r64 = ref.head(ref.trunk(x.double(), {k: (v.double() if v.is_floating_point() else v) for k, v in s64.items()},
                                 False), {k: v.double() if v.is_floating_point() else v for k, v in s64.items()})
        r32 = ref.head(ref.trunk(x, s32, False), s32)
    check("eval logits", out, r64, r32)
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), sd0[k]), f"{k} changed in eval mode"


def test_two_runs_bit_identical():
    outs = []
    for _ in range(2):
        m = make_model(8)
        x, y = batch(9, 4, 64, 64)
        outs.append(run_gpu_step(m, x, y, lr=1e-3))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_host_tensor_raises():
    from eav_amd._lib import EavError
    m = make_model(0)
    with pytest.raises(EavError):
        m(torch.zeros(1, 3, 64, 64))


def test_sliced_batch_with_unaligned_start():
    """x[1:] of a contiguous [B,3,93,125] batch starts 3*93*125 floats in (not a multiple of 4): the stem reads it
    with scalar loads, so it runs and equals the same images copied to an aligned buffer."""
    m = make_model(14).cuda().eval()
    x, _ = batch(15, 3, 93, 125)
    xd = x.cuda()
    assert xd[1:].data_ptr() % 16 != 0
    with torch.no_grad():
        a = m(xd[1:]).cpu()
        b = m(xd[1:].clone()).cpu()
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- golden fixtures
def golden_step_on_gpu(name, golden_dir):
    """The fixture's step on the GPU from `torch.manual_seed(wseed); VideoModel()`, with the golden's inputs."""
    import os
    from eav_amd.cnn_vision import VideoModel
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    g, pins = ref.load_golden(os.path.join(golden_dir, f"video_cnn_{name}.npz"))
    torch.manual_seed(int(g["wseed"]))
    m = VideoModel().cuda()
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    train, freeze, steps, lr = bool(g["train"]), bool(g["freeze"]), int(g["steps"]), float(g["lr"])
    for p in m.feature_extractor.parameters():
        p.requires_grad = not freeze
    opt, crit = FusedAdam(m.parameters(), lr=lr, weight_decay=0.01, decoupled=True), CrossEntropyLoss()
    outs = []
    for s in range(steps):
        x, y = ref.golden_inputs(g, s)
        m.train(train)
        if not train:
            with torch.no_grad():
                outs.append((m(x.cuda()).cpu(), None, None))
            continue
        opt.zero_grad()
        logits = m(x.cuda())
        loss = crit(logits, y.cuda())
        loss.backward()
        outs.append((logits.detach().cpu(), loss.detach().cpu(),
                     {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}))
        opt.step()
    torch.cuda.synchronize()
    return g, pins, m, sd0, outs


def ref_pair(g, sd0):
    """The fp32 and float64 restatements of the fixture's steps (fp32 reproduces the golden bit for bit, the CPU tests
    pin that): their differences are the yardstick of fp32 rounding in this network."""
    res = {}
    for dt in (torch.float32, torch.float64):
        sd, r = {k: v.clone() for k, v in sd0.items()}, []
        leaves = {}
        for s in range(int(g["steps"])):
            x, y = ref.golden_inputs(g, s)
            if not bool(g["train"]):
                with torch.no_grad():
                    sdd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
                    r.append((ref.head(ref.trunk(x.to(dt), sdd, False), sdd), None, None))
                continue
            logits, loss, grads, sd = ref.step(sd, x, y, freeze=bool(g["freeze"]), dtype=dt)
            r.append((logits, loss, grads))
            for k, gr in grads.items():
                if gr is None:
                    continue
                if k not in leaves:
                    leaf = sd[k].clone().requires_grad_(True)
                    leaves[k] = (leaf, torch.optim.AdamW([leaf], lr=float(g["lr"])))
                leaf, opt = leaves[k]
                leaf.grad = gr.clone()
                opt.step()
                sd[k] = leaf.detach().clone()
        res[dt] = (r, sd)
    return res[torch.float32], res[torch.float64]


@pytest.mark.parametrize("name", ["unfrozen_b4", "frozen_b4", "eval_b3", "adamw2_b4"])
def test_gpu_step_pinned_to_golden(name, golden_dir):
    """The GPU step against the imported reference's fixture: logits and loss of every step, and of every gradient and
    BatchNorm running statistic its whole-tensor sum |.| (a strided sample would compare single elements that a ReLU
    decision within rounding of zero may route differently).  Tolerance: twice the fp32 restatement's distance from the
    float64 one (max for the logits, L1 over the tensor for the sums) plus 1e-5 of the value; the loss is held to the
    logits it is computed from (first order: |d loss| <= 2 max |d logit|)."""
    g, pins, m, sd0, outs = golden_step_on_gpu(name, golden_dir)
    (r32, sd32), (r64, sd64) = ref_pair(g, sd0)
    for s, (logits, loss, grads) in enumerate(outs):
        gl = torch.from_numpy(g[f"logits{s}"]).double()
        tol = 2 * float((r32[s][0].double() - r64[s][0]).abs().max()) + 1e-5 * float(gl.abs().max())
        assert float((logits.double() - gl).abs().max()) <= tol, f"logits of step {s}"
        if loss is None:
            continue
        # the mean cross-entropy moves by at most 2 max |d logit| (each row's gradient p - onehot has L1 norm <= 2),
        # plus the loss's own rounding
        tol = 2 * float((logits.double() - gl).abs().max()) + 1e-6 * abs(float(g[f"loss{s}"]))
        assert abs(float(loss) - float(g[f"loss{s}"])) <= tol, f"loss of step {s}"
        assert set(grads) == {k[len(f"grad{s}."):] for k in pins if k.startswith(f"grad{s}.")}
        for k, gr in grads.items():
            gold = pins[f"grad{s}." + k][1][0]
            l1 = float((r32[s][2][k].double() - r64[s][2][k]).abs().sum())
            assert abs(float(gr.double().abs().sum()) - gold) <= 2 * l1 + 1e-5 * gold, f"grad {k} of step {s}"
    sd1 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    nbt = [int(v) for k, v in sd1.items() if k.endswith("num_batches_tracked")]
    assert nbt == list(g["post.num_batches_tracked"])
    for k, v in sd1.items():
        if k.endswith(("running_mean", "running_var")):
            gold = pins["post." + k][1][0]
            l1 = float((sd32[k].double() - sd64[k]).abs().sum())
            assert abs(float(v.double().abs().sum()) - gold) <= 2 * l1 + 1e-5 * gold, k
        elif bool(g["freeze"]) and k.startswith("feature_extractor.") and not k.endswith("num_batches_tracked"):
            assert torch.equal(v, sd0[k]), f"{k} changed in a frozen step"


def test_trainer_lines_equal_golden(capsys, golden_dir):
    """ImageClassifierTrainer on the fixture's frames and seed prints the imported reference's lines.  Every logit row
    behind a printed accuracy (recorded from the model's forward, in call order) is within a tenth of the reference
    row's top-1 / top-2 margin of it, and that margin is asserted, so no printed accuracy can flip on rounding."""
    import os
    from eav_amd import synth
    from eav_amd.cnn_vision import ImageClassifierTrainer
    g = np.load(os.path.join(golden_dir, "video_cnn_trainer.npz"))
    F_, ntr, nte, Hf = (int(v) for v in g["frames"])
    tr_x = synth.uniform(501, (ntr, F_, Hf, Hf, 3), 0.0, 256.0).astype(np.uint8)
    te_x = synth.uniform(502, (nte, F_, Hf, Hf, 3), 0.0, 256.0).astype(np.uint8)
    torch.manual_seed(int(g["tseed"]))
    capsys.readouterr()
    t = ImageClassifierTrainer([tr_x, g["tr_y"], te_x, g["te_y"]], num_labels=5, lr=5e-5, batch_size=4)
    rec = []
    fwd = t.model.forward

    def recording(x):
        o = fwd(x)
        rec.append(o.detach().cpu().clone())
        return o
    t.model.forward = recording
    t.train(epochs=1, lr=5e-4, freeze=True)
    assert not hasattr(t, "outputs_test")
    t.train(epochs=2, lr=5e-6, freeze=False)
    lines = capsys.readouterr().out.splitlines()
    pre = [ln for ln in lines if ln.startswith("VideoModel: backbone is not pretrained")]
    assert len(pre) == 1
    assert [ln for ln in lines if ln not in pre] == [str(v) for v in g["lines"]]
    assert [r.shape[0] for r in rec] == list(g["row_counts"])
    rows, gold = torch.cat(rec).double().numpy(), g["rows"].astype(np.float64)
    srt = np.sort(gold, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    dev = np.abs(rows - gold).max(axis=1)
    assert float(margin.min()) >= float(g["margin"])
    assert bool((dev <= margin / 10).all()), f"logit rows off by {dev.max():.3e}, margins down to {margin.min():.3e}"
    assert t.outputs_test.shape == g["outputs_test"].shape
    d = np.abs(t.outputs_test.astype(np.float64) - g["outputs_test"]).max(axis=1)
    so = np.sort(g["outputs_test"].astype(np.float64), axis=1)
    assert bool((d <= (so[:, -1] - so[:, -2]) / 10).all())
    t.clear_loaders()
