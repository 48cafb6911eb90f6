"""The per-bin GEMMs of the frequency-domain separableConv (csrc/eegnet_conv64_fft.hip) at the smallest shapes that reach
their loops: every shape of test_eegnet_kernels_gpu.py::test_conv64_fft has at most 128 columns, i.e. one 32-column tile
per workgroup of c64_bin_gemm_kernel and one K-block per chunk of c64_bin_wgemm_kernel.

Columns = B x ceil(ceil(T / 49) / 2), padded to a multiple of 128.  With T = 98 (two blocks = one column per sample):

  B = 129 -> 256 columns    8 tiles on 8 workgroups per bin; 127 zero padding columns in the weight gradient's contraction;
                           2 K-blocks per chunk
  B = 300 -> 384 columns   12 tiles on 8 workgroups per bin: the tile walk (its start rotates with the bin) wraps with an
                           uneven tail; chunks of 96 columns = 3 K-blocks: the whole LDS ring is primed, nothing refilled
  B = 520 -> 640 columns   20 tiles: every workgroup loops at least twice, four of them three times (both LDS tile buffers
                           re-used); 5 K-blocks per chunk: the ring of 4 stages wraps and a stage is refilled
  B = 33, T = 147 -> 66 -> 128 columns   an odd block count (half-empty last pair) together with more than one tile

Reference: F.conv1d in float64 on the CPU and its autograd; the tolerances are test_conv64_fft's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eav_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from eav_amd import _lib
    _lib.load()
    return _lib


def close(got, ref, rtol, atol, what=""):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    tol = atol + rtol * np.abs(ref)
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}"


@pytest.mark.parametrize("B,T", [(129, 98), (300, 98), (520, 98), (33, 147)])
def test_conv64_fft_gemm_loops(L, B, T):
    x = synth.normal(41, (B, 64, T))
    w = synth.uniform(42, (64, 64, 16), -0.05, 0.05)
    du = synth.normal(43, (B, 64, T))
    xd, wd, dud = (torch.from_numpy(a).cuda() for a in (x, w, du))
    P = lambda t: t.data_ptr()  # noqa: E731
    ws = torch.zeros(L.plain("eav_conv64_fft_ws_floats", B, T), device="cuda")
    part = torch.zeros(L.plain("eav_conv64_fft_nparts", B, T), 128, device="cuda")
    out = torch.full((B, 64, T), float("nan"), device="cuda")
    L.call("eav_conv64_fft_fwd", P(xd), P(wd), P(out), P(part), P(ws), B, T, 0, None)
    # bwd = 2: on the filter spectra the forward call left in ws (the model's sequence); bwd = 1: its own, in a fresh ws
    dx = torch.full((B, 64, T), float("nan"), device="cuda")
    L.call("eav_conv64_fft_fwd", P(dud), P(wd), P(dx), None, P(ws), B, T, 2, None)
    dx1 = torch.full((B, 64, T), float("nan"), device="cuda")
    ws1 = torch.zeros_like(ws)
    L.call("eav_conv64_fft_fwd", P(dud), P(wd), P(dx1), None, P(ws1), B, T, 1, None)
    dw = torch.full((64, 64, 16), float("nan"), device="cuda")
    L.call("eav_conv64_fft_wgrad", P(dud), P(dw), P(ws), B, T, None)
    dw2 = torch.full((64, 64, 16), float("nan"), device="cuda")
    L.call("eav_conv64_fft_wgrad", P(dud), P(dw2), P(ws), B, T, None)
    torch.cuda.synchronize()

    xt = torch.from_numpy(x).double().requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    ref = F.conv1d(F.pad(xt, (7, 8)), wt)
    ref.backward(torch.from_numpy(du).double())
    ref = ref.detach()
    e_dw = float((dw.double().cpu() - wt.grad).abs().max() / wt.grad.abs().max())
    print(f"conv64_fft gemm loops B={B} T={T}: max |out - ref| {float((out.double().cpu() - ref).abs().max()):.2e}, "
          f"max |dx - ref| {float((dx.double().cpu() - xt.grad).abs().max()):.2e}, max |dW - ref| / max |dW| {e_dw:.2e}")
    close(out, ref, 1e-4, 1e-5, "conv out")
    st = part.sum(0).cpu().double().numpy()
    close(st[:64], ref.sum((0, 2)), 1e-4, 1e-3, "sum")
    close(st[64:], (ref ** 2).sum((0, 2)), 1e-4, 1e-3, "sumsq")
    close(dx, xt.grad, 1e-4, 1e-5, "dgrad")
    assert torch.equal(dx, dx1), "bwd = 1 (own filter spectra) and bwd = 2 (the forward's) differ"
    close(dw, wt.grad, 1e-4, 1e-4 * float(wt.grad.abs().max()), "wgrad")
    assert torch.equal(dw, dw2), "the frequency-domain weight gradient is not bit-reproducible"
