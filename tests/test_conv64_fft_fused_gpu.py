"""The fused launches of the frequency-domain separableConv (csrc/eegnet_conv64_fft.hip) against the composition of the entry
points they replace, bit for bit (torch.equal) - the existing kernels are the reference; they are pinned to float64 by
test_eegnet_kernels_gpu.py::test_conv64_fft and ::test_pool_fwd_bwd.

  eav_conv64_fft_bwd      one pack launch that writes the du spectra of the data gradient AND of the weight gradient,
                          (a) from du, (b) from (dp3, u3, bn3, m12) = eav_bn_elu_pool_bwd_apply(P = 8) formed while loading
                          == [eav_bn_elu_pool_bwd_apply] -> eav_conv64_fft_fwd(bwd = 2) -> eav_conv64_fft_wgrad
  filter spectra          formed by the leading workgroups of the forward's pack launch: bwd = 2 on the forward's workspace
                          == bwd = 1 on a fresh one
  EEGNet_tor.conv_fuse    one step with it on == one step with it off, train and eval mode

Shapes (B, T): T = 98 one full column per sample, 49 one block (empty imaginary half), 50 one block + 1, 147 an odd block
count; T = 98 and 50 are no multiples of the pooling window 8 (a dropped tail, where g = 0 but du = -scale (m1 + uhat m2)
is not); B = 130 gives more than 128 columns (a second GEMM tile row, zero padding columns); B = 2100 more than 2048, so
that a wave of the pack grid takes a second column."""
import pytest
import torch

from eav_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(3, 98), (1, 49), (2, 50), (2, 147), (130, 98)]
DROPS = ["none", "seed", "mask", "row"]
P = lambda t: None if t is None else t.data_ptr()  # noqa: E731


@pytest.fixture(scope="module")
def L():
    from eav_amd import _lib
    _lib.load()
    return _lib


_cache = {}


def prepared(L, B, T):
    """Inputs of one step at (B, T) on the device and a workspace the forward call has been made on (shared, read-only:
    the tests below only call entry points that leave the forward's filter and input spectra alone)."""
    if (B, T) not in _cache:
        d = {}
        d["x"] = torch.from_numpy(synth.normal(51, (B, 64, T))).cuda()
        d["w"] = torch.from_numpy(synth.uniform(52, (64, 64, 16), -0.05, 0.05)).cuda()
        d["du"] = torch.from_numpy(synth.normal(53, (B, 64, T))).cuda()
        d["u"] = torch.from_numpy(synth.normal(54, (B, 64, T))).cuda()
        d["dp"] = torch.from_numpy(synth.normal(55, (B, 64, T // 8))).cuda()
        bn = torch.empty(4, 64)
        bn[0] = torch.from_numpy(synth.uniform(56, (64,), -0.3, 0.3))       # mean
        bn[1] = torch.from_numpy(synth.uniform(57, (64,), 0.5, 2.0))        # invstd
        bn[2] = torch.from_numpy(synth.uniform(58, (64,), -1.5, 1.5))       # scale (weight x invstd, either sign)
        bn[3] = torch.from_numpy(synth.uniform(59, (64,), -0.5, 0.5))       # shift
        d["bn"] = bn.cuda()
        d["m12"] = torch.from_numpy(synth.uniform(60, (2, 64), -0.2, 0.2)).cuda()      # non-zero m1, m2
        d["mask"] = (torch.from_numpy(synth.uniform(61, (B, 64, T // 8), 0.0, 1.0)) >= 0.5).to(torch.uint8).cuda()
        d["cnt"] = torch.full((), 3, dtype=torch.int64, device="cuda")      # a non-zero device step counter
        d["ws"] = torch.zeros(L.plain("eav_conv64_fft_ws_floats", B, T), device="cuda")
        out = torch.empty(B, 64, T, device="cuda")
        L.call("eav_conv64_fft_fwd", P(d["x"]), P(d["w"]), P(out), None, P(d["ws"]), B, T, 0, None)
        torch.cuda.synchronize()
        _cache[(B, T)] = d
    return _cache[(B, T)]


def drop_args(d, mode):
    """(drop_p, seed, mask, seed_dev) of eav_bn_elu_pool_bwd_apply / eav_conv64_fft_bwd"""
    if mode == "none":
        return 0.0, 0, None, None
    if mode == "seed":
        return 0.5, 0x5EED, None, P(d["cnt"])
    if mode == "mask":
        return 0.5, 0, P(d["mask"]), None
    return -0.5, 0x5EED, None, P(d["cnt"])      # one draw per (sample, channel) row


def separate(L, d, du, B, T):
    dx = torch.full((B, 64, T), float("nan"), device="cuda")
    dw = torch.full((64, 64, 16), float("nan"), device="cuda")
    L.call("eav_conv64_fft_fwd", P(du), P(d["w"]), P(dx), None, P(d["ws"]), B, T, 2, None)
    L.call("eav_conv64_fft_wgrad", P(du), P(dw), P(d["ws"]), B, T, None)
    return dx, dw


def fused(L, d, du, drop, B, T):
    dx = torch.full((B, 64, T), float("nan"), device="cuda")
    dw = torch.full((64, 64, 16), float("nan"), device="cuda")
    L.call("eav_conv64_fft_bwd", P(du), P(d["dp"]), P(d["u"]), P(d["bn"]), P(d["m12"]), *drop, P(dx), P(dw), P(d["ws"]),
           B, T, None)
    return dx, dw


@pytest.mark.parametrize("B,T", SHAPES)
def test_bwd_from_du_matches_dgrad_then_wgrad(L, B, T):
    d = prepared(L, B, T)
    dx0, dw0 = separate(L, d, d["du"], B, T)
    dx1, dw1 = fused(L, d, d["du"], (0.0, 0, None, None), B, T)
    dx2, dw2 = fused(L, d, d["du"], (0.0, 0, None, None), B, T)
    # the forward's input spectra survive it and a data-gradient-only call of the old entry point in between
    dx3 = torch.empty_like(dx0)
    L.call("eav_conv64_fft_fwd", P(d["du"]), P(d["w"]), P(dx3), None, P(d["ws"]), B, T, 2, None)
    dx4, dw4 = fused(L, d, d["du"], (0.0, 0, None, None), B, T)
    torch.cuda.synchronize()
    assert torch.isfinite(dx0).all() and torch.isfinite(dw0).all()
    assert torch.equal(dx1, dx0), "data gradient"
    assert torch.equal(dw1, dw0), "weight gradient"
    assert torch.equal(dx2, dx0) and torch.equal(dw2, dw0), "second call"
    assert torch.equal(dx4, dx0) and torch.equal(dw4, dw0), "call after a data-gradient-only call"


@pytest.mark.parametrize("drop", DROPS)
@pytest.mark.parametrize("B,T", SHAPES)
def test_bwd_from_dp_matches_apply_then_dgrad_then_wgrad(L, B, T, drop):
    d = prepared(L, B, T)
    da = drop_args(d, drop)
    du = torch.full((B, 64, T), float("nan"), device="cuda")
    L.call("eav_bn_elu_pool_bwd_apply", P(d["dp"]), P(d["u"]), P(d["bn"]), P(d["m12"]), P(du), B, 64, T, 8, *da, None)
    dx0, dw0 = separate(L, d, du, B, T)
    dx1, dw1 = fused(L, d, None, da, B, T)
    dx2, dw2 = fused(L, d, None, da, B, T)
    torch.cuda.synchronize()
    assert torch.isfinite(dx0).all() and torch.isfinite(dw0).all()
    if T % 8:
        assert (du[:, :, T - T % 8:] != 0).all(), "the dropped tail carries a gradient"
    assert torch.equal(dx1, dx0), "data gradient"
    assert torch.equal(dw1, dw0), "weight gradient"
    assert torch.equal(dw2, dw0) and torch.equal(dx2, dx0), "second call"


def test_bwd_second_column_per_wave(L):
    """More than 2048 columns: the pack grid is 512 workgroups of 4 waves, so a wave takes a second column and re-uses its
    tile (the pooled-gradient table, the transpose, the parked weight-gradient block) - GPU comparison only."""
    B, T = 2100, 98
    gen = torch.Generator("cuda").manual_seed(9)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)  # noqa: E731
    small = prepared(L, 3, 98)
    d = dict(small, x=rnd(B, 64, T), u=rnd(B, 64, T), dp=rnd(B, 64, T // 8))
    d["ws"] = torch.zeros(L.plain("eav_conv64_fft_ws_floats", B, T), device="cuda")
    out = torch.empty(B, 64, T, device="cuda")
    L.call("eav_conv64_fft_fwd", P(d["x"]), P(d["w"]), P(out), None, P(d["ws"]), B, T, 0, None)
    da = drop_args(d, "seed")
    du = torch.full((B, 64, T), float("nan"), device="cuda")
    L.call("eav_bn_elu_pool_bwd_apply", P(d["dp"]), P(d["u"]), P(d["bn"]), P(d["m12"]), P(du), B, 64, T, 8, *da, None)
    dx0, dw0 = separate(L, d, du, B, T)
    dx1, dw1 = fused(L, d, None, da, B, T)
    dx2, dw2 = fused(L, d, du, (0.0, 0, None, None), B, T)
    torch.cuda.synchronize()
    assert torch.isfinite(dx0).all() and torch.isfinite(dw0).all()
    assert torch.equal(dx1, dx0) and torch.equal(dw1, dw0), "du formed while loading"
    assert torch.equal(dx2, dx0) and torch.equal(dw2, dw0), "du read"


def test_bwd_refuses_missing_source(L):
    d = prepared(L, 1, 49)
    dx = torch.zeros(1, 64, 49, device="cuda")
    dw = torch.zeros(64, 64, 16, device="cuda")
    with pytest.raises(L.EavError, match="neither du nor"):
        L.call("eav_conv64_fft_bwd", None, P(d["dp"]), None, P(d["bn"]), P(d["m12"]), 0.0, 0, None, None, P(dx), P(dw),
               P(d["ws"]), 1, 49, None)


def test_filter_spectra_in_pack_launch(L):
    B, T = 3, 49
    d = prepared(L, B, T)
    dx2 = torch.full((B, 64, T), float("nan"), device="cuda")
    L.call("eav_conv64_fft_fwd", P(d["du"]), P(d["w"]), P(dx2), None, P(d["ws"]), B, T, 2, None)
    dx1 = torch.full((B, 64, T), float("nan"), device="cuda")
    ws1 = torch.zeros_like(d["ws"])
    L.call("eav_conv64_fft_fwd", P(d["du"]), P(d["w"]), P(dx1), None, P(ws1), B, T, 1, None)
    torch.cuda.synchronize()
    assert torch.isfinite(dx1).all() and float(dx1.abs().max()) > 0
    assert torch.equal(dx2, dx1), "bwd = 2 (the forward's filter spectra) and bwd = 1 (its own) differ"
    tables = 2 * 64 * 128 * 128
    assert torch.equal(d["ws"][tables // 2:tables], ws1[tables // 2:tables]), "data-gradient table"
    assert float(d["ws"][:tables // 2].abs().max()) > 0, "forward table"


@pytest.mark.parametrize("train", [True, False])
def test_model_conv_fuse_on_matches_off(train):
    from eav_amd.eegnet import EEGNet_tor
    from eav_amd.optim import CrossEntropyLoss
    B, S = 4, 392
    x, y = synth.eeg_batch(7, B, 30, S)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    torch.manual_seed(0)
    sd = None
    res = []
    for fuse in (True, False):
        model = EEGNet_tor(nb_classes=5, Chans=30, Samples=S, dropoutRate=0.5)
        if sd is None:
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model.load_state_dict(sd)
        model = model.cuda()
        model.train(train)
        model.conv_algo, model.conv_fuse = "fft", fuse
        scores = model(xd)
        CrossEntropyLoss()(scores, yd).backward()
        torch.cuda.synchronize()
        res.append((scores.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0]), "scores"
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    assert float(res[0][1]["separableConv.weight"].abs().max()) > 0
