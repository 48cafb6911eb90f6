"""Packed row tails of the FFT FIR kernels (csrc/eegnet_fir_fft.hip): where the last block of a row needs at most 512 input
samples, two tails share one 1024-point transform.  Same references and tolerances as test_eegnet_kernels_gpu.py
(test_fir_fwd_fft / test_fir_wgrad_fft): torch conv on the CPU, a float64 einsum for the weight gradient.  Every output
lies inside a larger NaN-filled buffer, so a packed unit that writes to the wrong row or past S is caught.

Shapes, the smallest at which each piece can go wrong:
  (1, 2, 705, 300)    one tail of one sample, alone in its packed unit: empty upper half
  (2, 3, 705, 300)    odd electrode count: the second pair has one electrode
  (3, 1, 1409, 321)   321 taps; three tails = one packed unit + one alone, tail pairs cross the sample boundary
  (2, 4, 917 | 918, 300)   last S that packs (Lt = 213) and first that does not
  (2, 4, 896 | 897, 321)   the same pair at 321 taps
  (1, 3, 1100, 64)    short filter: Lt = 396 packs only because the condition uses the actual klen (7 rows per half)
  (4, 30, 1500, 300)  120 main + 30 packed units: weight-gradient groups of both kinds on several workgroups, forward
                      waves with and without an extra unit"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eav_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 705, 300), (2, 3, 705, 300), (3, 1, 1409, 321), (2, 4, 917, 300), (2, 4, 918, 300), (2, 4, 896, 321),
          (2, 4, 897, 321), (1, 3, 1100, 64), (4, 30, 1500, 300)]
GUARD = 4096


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


class Guarded:
    """n floats between two guards, everything NaN until a kernel writes it"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def check(self, what, filled=True):
        assert bool(torch.isnan(self.buf[:GUARD]).all()), f"{what}: written in front of the buffer"
        assert bool(torch.isnan(self.buf[GUARD + self.n:]).all()), f"{what}: written behind the buffer"
        if filled:
            assert not bool(torch.isnan(self.t).any()), f"{what}: elements left unwritten"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def fwd_case(B, C, S, K, indexed):
    N = B + 3 if indexed else B
    xs = synth.normal(1, (N, C, S))
    idx = np.array([(3 * i + 1) % N for i in range(B)], np.int64)
    x = xs[idx] if indexed else xs
    w = synth.uniform(2, (8, K), -0.1, 0.1)
    xt = torch.from_numpy(x).unsqueeze(1)
    left = (K - 1) // 2
    ref = F.conv2d(F.pad(xt, (left, K - 1 - left)), torch.from_numpy(w).view(8, 1, 1, K))
    ref64 = F.conv2d(F.pad(xt.double(), (left, K - 1 - left)), torch.from_numpy(w).double().view(8, 1, 1, K))
    return xs, idx, x, w, ref, ref64


@pytest.mark.parametrize("B,C,S,K", SHAPES)
@pytest.mark.parametrize("indexed", [False, True])
def test_fir_fwd_fft_packed_tails(L, B, C, S, K, indexed):
    xs, idx, x, w, ref, ref64 = fwd_case(B, C, S, K, indexed)
    xd, wd, idxd = dev(xs), dev(w), dev(idx)
    y = Guarded(B, 8, C, S)
    part = Guarded(L.plain("eav_eegnet_fir_fwd_fft_nparts", B, C, S), 16)
    L.call("eav_eegnet_fir_fwd_fft", xd.data_ptr(), idxd.data_ptr() if indexed else None, wd.data_ptr(), y.t.data_ptr(),
           part.t.data_ptr(), B, C, S, K, None)
    torch.cuda.synchronize()
    y.check("y1")
    part.check("stat_part")          # every row the sizing export counts is written: the consumers sum all of them
    close(y.t, ref, 1e-4, 2e-5, "y1")
    st = part.t.sum(0).cpu().double().numpy()
    close(st[:8], ref.double().sum((0, 2, 3)), 1e-5, 1e-3, "sum")
    close(st[8:], (ref.double() ** 2).sum((0, 2, 3)), 1e-5, 1e-3, "sumsq")
    # a second call gives the same bits
    y2 = Guarded(B, 8, C, S)
    part2 = Guarded(part.t.shape[0], 16)
    L.call("eav_eegnet_fir_fwd_fft", xd.data_ptr(), idxd.data_ptr() if indexed else None, wd.data_ptr(), y2.t.data_ptr(),
           part2.t.data_ptr(), B, C, S, K, None)
    torch.cuda.synchronize()
    assert torch.equal(y.t, y2.t) and torch.equal(part.t, part2.t), "the FFT forward is not bit-reproducible"
    # against float64 the FFT form must not be worse than the direct fp32 MFMA kernel
    if K <= 300:
        yd = torch.empty(B, 8, C, S, device="cuda")
        partd = torch.zeros(L.plain("eav_eegnet_fir_fwd_nparts", B, C, S), 16, device="cuda")
        xc = dev(x)
        L.call("eav_eegnet_fir_fwd", xc.data_ptr(), wd.data_ptr(), yd.data_ptr(), partd.data_ptr(), B, C, S, K, None)
        torch.cuda.synchronize()
        e_fft = float((y.t.double().cpu() - ref64).abs().max())
        e_dir = float((yd.double().cpu() - ref64).abs().max())
        print(f"fir_fwd_fft B={B} C={C} S={S} K={K}: max error vs float64 {e_fft:.2e} (direct fp32 MFMA kernel {e_dir:.2e})")
        assert e_fft <= 4.0 * e_dir + 1e-6


@pytest.mark.parametrize("B,C,S,K", SHAPES)
def test_fir_fwd_fft_packed_tails_without_statistics(L, B, C, S, K):
    xs, _, _, w, ref, _ = fwd_case(B, C, S, K, False)
    xd, wd = dev(xs), dev(w)
    y = Guarded(B, 8, C, S)
    L.call("eav_eegnet_fir_fwd_fft", xd.data_ptr(), None, wd.data_ptr(), y.t.data_ptr(), None, B, C, S, K, None)
    torch.cuda.synchronize()
    y.check("y1")
    close(y.t, ref, 1e-4, 2e-5, "y1")


@functools.lru_cache(maxsize=None)
def wgrad_case(B, C, S, K):
    x = synth.normal(3, (B, C, S))
    y1 = synth.normal(4, (B, 8, C, S))
    g1 = synth.normal(5, (B, 8, C, S))
    mean, invstd = synth.uniform(6, (8,), -0.2, 0.2), synth.uniform(7, (8,), 0.5, 2.0)
    scale = synth.uniform(8, (8,), 0.5, 1.5)
    m1, m2 = synth.uniform(9, (8,), -0.1, 0.1), synth.uniform(10, (8,), -0.1, 0.1)
    bc = lambda v: torch.from_numpy(v).double()[None, :, None, None]  # noqa: E731
    left = (K - 1) // 2
    win = F.pad(torch.from_numpy(x).double(), (left, K - 1 - left)).unfold(2, S, 1)
    g64, y64 = torch.from_numpy(g1).double(), torch.from_numpy(y1).double()
    refs = {}
    for eval_mode in (False, True):
        a1, a2 = (np.zeros(8, np.float32),) * 2 if eval_mode else (m1, m2)
        dy = bc(scale) * (g64 - bc(a1) - (y64 - bc(mean)) * bc(invstd) * bc(a2))
        refs[eval_mode] = torch.einsum("bfcs,bcks->fk", dy, win)
    return x, y1, g1, (mean, invstd, scale, m1, m2), refs


@pytest.mark.parametrize("B,C,S,K", SHAPES)
@pytest.mark.parametrize("eval_mode", [False, True])
def test_fir_wgrad_fft_packed_tails(L, B, C, S, K, eval_mode):
    x, y1, g1, (mean, invstd, scale, m1, m2), refs = wgrad_case(B, C, S, K)
    ref = refs[eval_mode]
    z = np.zeros(8, np.float32)
    bn = dev(np.concatenate([mean, invstd, scale, z, z if eval_mode else m1, z if eval_mode else m2]).astype(np.float32))
    xd, yd, gd = dev(x), dev(y1), dev(g1)
    ws = Guarded(L.plain("eav_eegnet_fir_wgrad_fft_ws_floats", B, C, S))
    outs = []
    for _ in range(2):
        out = Guarded(8, K)
        L.call("eav_eegnet_fir_wgrad_fft", xd.data_ptr(), None, None if eval_mode else yd.data_ptr(), gd.data_ptr(),
               bn.data_ptr(), ws.t.data_ptr(), out.t.data_ptr(), B, C, S, K, None)
        torch.cuda.synchronize()
        out.check("dW1")
        outs.append(out)
    ws.check("workspace", filled=False)
    assert torch.equal(outs[0].t, outs[1].t), "the FFT weight gradient is not bit-reproducible"
    close(outs[0].t, ref, 2e-4, 2e-4 * float(ref.abs().max()), "dW1")
    err = float((outs[0].t.double().cpu() - ref).abs().max()) / float(ref.abs().max())
    print(f"fir_wgrad_fft B={B} C={C} S={S} K={K} eval={eval_mode}: max error / max |dW| = {err:.2e}")
