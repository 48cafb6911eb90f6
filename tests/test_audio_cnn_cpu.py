"""CPU-side checks of the audio CNN (eav_amd/cnn_audio.py, csrc/audio_cnn.hip): the reference's signatures and defaults,
state_dict keys and seeded default initialisation (against the golden's fresh weights), the input-length range, the
C ABI's argument validation without a device, and a scratch-free gfx950 compile of every kernel."""
import hashlib
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["features.0.weight", "features.0.bias", "features.2.weight", "features.2.bias", "features.6.weight",
        "features.6.bias", "features.8.weight", "features.8.bias", "classifier.weight", "classifier.bias"]


def test_signatures_and_defaults_match_reference():
    from eav_amd import cnn_audio as ca
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]  # noqa: E731
    assert sig(ca.AudioModel.__init__) == [("self", inspect.Parameter.empty), ("num_classes", 5)]
    assert sig(ca.create_dataloader) == [("x", inspect.Parameter.empty), ("y", inspect.Parameter.empty),
                                         ("batch_size", 64), ("shuffle", True)]
    assert [p for p, _ in sig(ca.ActivationSaver.__init__)] == ["self", "model", "val_loader", "save_dir"]
    assert sig(ca.train_model) == [("model", inspect.Parameter.empty), ("train_loader", inspect.Parameter.empty),
                                   ("val_loader", inspect.Parameter.empty), ("epochs", 100), ("lr", 1e-3),
                                   ("save_dir", "activations"), ("subject_id", None), ("device", None)]
    assert ca.MODEL_DIR == r"D:\.spyder-py3\finetuned_cnn_7030"


def test_modules_state_dict_and_seeded_init(golden_dir):
    from eav_amd.cnn_audio import AudioModel
    g = np.load(os.path.join(golden_dir, "audio_cnn_train_model.npz"))
    torch.manual_seed(int(g["wseed"]))
    m = AudioModel(num_classes=5)
    sd = m.state_dict()
    assert list(sd) == KEYS == list(g["fresh_keys"])
    assert [type(m.features[i]).__name__ for i in range(11)] == [
        "Conv1d", "ReLU", "Conv1d", "ReLU", "Dropout", "MaxPool1d", "Conv1d", "ReLU", "Conv1d", "ReLU", "Dropout"]
    assert (m.features[4].p, m.features[10].p, m.features[5].kernel_size) == (0.1, 0.5, 8)
    assert tuple(m.classifier.weight.shape) == (5, 128 * 22)
    for k, h in zip(KEYS, g["fresh_sha256"]):
        assert hashlib.sha256(np.ascontiguousarray(sd[k].numpy()).tobytes()).hexdigest() == str(h), k
    for k in ("features.0.weight", "features.0.bias", "classifier.bias"):
        assert np.array_equal(sd[k].numpy(), g[f"fresh.{k}"])


@pytest.mark.parametrize("T", [175, 184, 100])
def test_input_length_outside_the_classifier_range_raises(T):
    from eav_amd.cnn_audio import AudioModel
    with pytest.raises(NotImplementedError, match="176 <= T <= 183"):
        AudioModel()(torch.zeros(2, 1, T))
    with pytest.raises(NotImplementedError, match="176 <= T <= 183"):
        AudioModel()(torch.zeros(2, T, 1))


def test_no_cpu_fallback():
    from eav_amd import _lib
    from eav_amd.cnn_audio import AudioModel
    with pytest.raises(_lib.EavError, match="no CPU fallback"):
        AudioModel()(torch.zeros(2, 1, 180))


def test_abi_argument_validation_without_gpu():
    """Bad sizes, lengths and pointers return an error string and launch nothing."""
    from eav_amd import _lib
    call = _lib.call
    with pytest.raises(_lib.EavError, match=r"T = 184 gives 23 pooled positions.*176\.\.\.183"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, 8, 4, 256, 128, 184, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="T = 175"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, 8, 4, 256, 128, 175, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="null tensor"):
        call("eav_audio_conv5_fwd", None, 8, 8, 8, 8, 4, 256, 128, 180, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="argmax"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, None, 4, 256, 128, 180, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="dropout probability"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, None, 4, 128, 128, 22, 22, 0, 1.0, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="input channels"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, None, 4, 24, 128, 22, 22, 0, 0.0, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="pool scatter"):
        call("eav_audio_conv5_dgrad", 8, None, 1.0, 8, 8, None, None, 1.0, 4, 128, 128, 22, 22, 1, None)
    with pytest.raises(_lib.EavError, match="null tensor"):
        call("eav_audio_conv5_dgrad", None, None, 1.0, 8, 8, None, None, 1.0, 4, 128, 128, 22, 22, 0, None)
    n = _lib.plain("eav_audio_wgrad_nparts", 64, 256, 128, 176)
    assert 1 <= n <= 64 * 6
    with pytest.raises(_lib.EavError, match="nparts"):
        call("eav_audio_conv5_wgrad", 8, None, 1.0, 8, 8, 64, 256, 128, 180, 176, n + 1, None)
    with pytest.raises(_lib.EavError, match="null tensor"):
        call("eav_audio_conv5_wgrad", 8, None, 1.0, None, 8, 64, 256, 128, 180, 176, n, None)
    assert _lib.plain("eav_audio_wgrad_nparts", 0, 256, 128, 176) == 0
    with pytest.raises(_lib.EavError, match=r"pool form needs a multiple of 16 input channels"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, 8, 4, 1, 128, 176, 176, 1, 0.0, 0, None, None, None)
    with pytest.raises(_lib.EavError, match=r"dgrad: bad sizes \(B 4, C 24,"):
        call("eav_audio_conv5_dgrad", 8, None, 1.0, 8, 8, None, None, 1.0, 4, 24, 128, 22, 22, 0, None)
    with pytest.raises(_lib.EavError, match="dgrad: mode 2"):
        call("eav_audio_conv5_dgrad", 8, None, 1.0, 8, 8, 8, 8, 1.0, 4, 128, 128, 22, 22, 2, None)
    with pytest.raises(_lib.EavError, match=r"wgrad: bad sizes \(B 0,"):
        call("eav_audio_conv5_wgrad", 8, None, 1.0, 8, 8, 0, 256, 128, 180, 176, 1, None)


def test_kernels_compile_for_gfx950_without_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.resources(os.path.join(ROOT, "eav_amd", "csrc", "audio_cnn.hip"))
    names = [r["demangled"] for r in rows]
    assert len(rows) == 6 and sum("conv5_kernel" in n for n in names) == 5 and any("wgrad" in n for n in names), names
    for r in rows:
        assert int(r["ScratchSize"]) == 0, (r["demangled"], r["ScratchSize"])
        assert int(r["LDS Size"]) <= 64 * 1024 and int(r["Occupancy"]) >= 3, r


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


@pytest.mark.parametrize("B,C,N,Lin,Lout", [(2, 3, 4, 11, 11), (1, 2, 3, 9, 14), (3, 4, 2, 17, 12), (1, 1, 1, 1, 1)])
def test_conv_references_equal_autograd(B, C, N, Lin, Lout):
    """The float64 references of tests/audio_conv_ref.py, which the kernel tests hold the kernels to, against torch
    autograd of F.conv1d on integer data (every sum exact): the data gradient at Lout >= Lin and Lout < Lin, with and
    without the ReLU' gate and the dropout gate scale, and the weight and bias gradients with the activation zero past
    Lact and the output gradient zero past Lout."""
    from tests.audio_conv_ref import dgrad_ref, wgrad_ref
    gen = torch.Generator().manual_seed(B * 1000 + C * 100 + N * 10 + Lin + Lout)
    # data gradient: the layer y = conv1d(z, w) with z [B][N][L], w [C][N][5]; its output gradient is zero past Lin
    L = max(Lin, Lout)
    z = _ints(gen, (B, N, L), -3, 3).requires_grad_()
    w = (_ints(gen, (C, N, 5), -3, 3) / 4).requires_grad_()
    g = _ints(gen, (B, C, Lin), -3, 3)
    gate = _ints(gen, (B, C, Lin), -1, 1)
    gate[0, 0, 0] = float("nan")
    aux = _ints(gen, (B, N, Lout), -1, 2)
    aux.view(-1)[::3] = float("nan")
    aux.view(-1)[1::5] = -0.0
    y = F.conv1d(z, w, padding=2)
    dz = torch.autograd.grad(y, z, F.pad(g * torch.where(gate > 0, 2.0, 0.0).double(), (0, L - Lin)),
                             retain_graph=True)[0][..., :Lout]
    assert torch.equal(dgrad_ref(g, w.detach(), Lout, gate, 2.0), dz)
    assert torch.equal(dgrad_ref(g, w.detach(), Lout), torch.autograd.grad(y, z, F.pad(g, (0, L - Lin)))[0][..., :Lout])
    ref = dgrad_ref(g, w.detach(), Lout, gate, 2.0, 0, aux)
    assert torch.equal(ref, torch.where(torch.isnan(aux) | (aux > 0), dz, 0.0))
    # weight gradient: act [B][C][Lact] with Lact = Lin (zero beyond), output gradient [B][N][Lout] (zero beyond)
    act = _ints(gen, (B, C, Lin), 0, 3)
    wt = (_ints(gen, (N, C, 5), -3, 3) / 4).requires_grad_()
    bt = (_ints(gen, (N,), -8, 8) / 4).requires_grad_()
    dout = _ints(gen, (B, N, Lout), -3, 3)
    gate = _ints(gen, (B, N, Lout), -1, 1)
    gate.view(-1)[::7] = float("nan")
    yt = F.conv1d(F.pad(act, (0, L - Lin)), wt, bt, padding=2)
    yt.backward(F.pad(dout * torch.where(gate > 0, 2.0, 0.0).double(), (0, L - Lout)))
    dw, db = wgrad_ref(dout, act, gate, 2.0)
    assert torch.equal(dw, wt.grad) and torch.equal(db, bt.grad)


@pytest.mark.parametrize("p", [0.5, 0.75])
def test_pool_references_equal_autograd(p):
    """fwd_ref's ReLU -> dropout -> MaxPool1d(8) and dgrad_ref's mode-1 scatter (gated by the pooled value, scaled by the
    dropout scale) against autograd of the same torch ops, on integer data with many tied and all-zero windows: the
    scatter routes each window's gradient where autograd does."""
    from tests.audio_conv_ref import dgrad_ref, f32_scale, fwd_ref
    gen = torch.Generator().manual_seed(int(p * 100))
    B, C, N, Lin, Lout = 3, 2, 4, 45, 40
    x = _ints(gen, (B, C, Lin), -3, 3)
    w = _ints(gen, (N, C, 5), -3, 3) / 4
    b = _ints(gen, (N,), -8, 8) / 4
    mask = (torch.rand(B, N, Lin, generator=gen) >= p).to(torch.uint8)
    pooled, idx = fwd_ref(x, w, b, Lout, 1, mask, p)
    z = F.conv1d(x, w, b, padding=2).requires_grad_()
    a = F.relu(z) * mask.double() * f32_scale(p)
    v, i = F.max_pool1d(a[..., :Lout], 8, return_indices=True)
    assert torch.equal(v, pooled) and torch.equal(i, idx.long() + 8 * torch.arange(Lout // 8))
    windows = a.detach()[..., :Lout].unflatten(2, (Lout // 8, 8))
    assert ((windows == windows[..., :1]).all(3) & (idx == 0)).any(), "no all-tied window"
    assert ((windows.amax(3, keepdim=True) == windows).sum(3) > 1).any(), "no tie on the maximum"
    gp = _ints(gen, v.shape, -3, 3)
    v.backward(gp)
    # dgrad_ref's mode 1 with an identity conv: the scatter alone (its conv_transpose1d with a centred unit tap)
    eye = torch.zeros(N, N, 5, dtype=torch.float64)
    eye[range(N), range(N), 2] = 1.0
    got = dgrad_ref(gp, eye, Lout // 8, mode=1, aux=pooled, idx=idx, gscale_out=f32_scale(p))
    assert torch.equal(got, z.grad[..., :Lout])
    assert not z.grad[..., Lout:].any()


def test_relu_and_pool_propagate_nan_like_the_header():
    """The references keep a NaN through ReLU and dropout, and MaxPool1d(8) records the last NaN of a window (what the
    header's 'NaN propagates' means with torch's CPU scan), the first index on ties."""
    from tests.audio_conv_ref import fwd_ref
    x = torch.ones(1, 1, 16, dtype=torch.float64)
    x[0, 0, 6] = float("nan")                       # conv outputs 4..8: window 0 positions 4-7, window 1 position 0
    w = torch.zeros(1, 1, 5, dtype=torch.float64)   # 0 * NaN is NaN
    v, idx = fwd_ref(x, w, torch.zeros(1), 16, 1, torch.zeros(1, 1, 16, dtype=torch.uint8), 0.5)
    assert torch.isnan(v).all() and idx.tolist() == [[[7, 0]]]
