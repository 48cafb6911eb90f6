"""The kernels of csrc/grad_clip.hip and eav_adam_step_scaled through _lib.call, against tests/grad_clip_ref.py (numpy
float64, pinned to torch by tests/test_grad_clip_cpu.py).

Bounds.  Norm: |norm - ref| <= 4 * 2^-23 * ref - the kernel adds squares in fp64 (exact to ~n 2^-53), what remains is the
square root and one cast to fp32.  Coefficient: float32(max_norm) / (float32(norm) + float32(1e-6)) clamped to 1, formed in
numpy float32 from the kernel's OWN norm, bit for bit (an IEEE fp32 division).  Fold: first = 1 gives float32(w * g) bit
for bit; first = 0 stays within 2^-23 * (|acc_old| + |w g|) of the float64 value per element, which a fused and an
unfused multiply-add both meet.  Scaled Adam and eav_scale_ranges: bit for bit against eav_adam_step / torch on a
gradient scaled beforehand."""
import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import grad_clip_ref as R

pytestmark = pytest.mark.gpu

C = _lib.plain("eav_grad_chunk_elems")
EPS = 2.0 ** -23


def _table(ranges):
    """Device job table of (tensor view) ranges; returns (table, njobs, nchunks)."""
    nchunks = sum(_lib.plain("eav_grad_nchunks", r.numel()) for r in ranges)
    t = torch.tensor([[r.data_ptr(), r.numel()] for r in ranges], dtype=torch.int64).cuda()
    return t, len(ranges), nchunks


def _finish(partials, nchunks, max_norm):
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    _lib.call("eav_grad_clip_finish", partials.data_ptr(), nchunks, float(max_norm), out.data_ptr(), _lib.stream_ptr())
    return out


def _norm(ranges, max_norm=1.0):
    """(out2 as numpy float32 [norm, coefficient], partials as numpy) of eav_grad_sumsq + eav_grad_clip_finish."""
    t, nj, nc = _table(ranges)
    partials = torch.full((nc,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("eav_grad_sumsq", t.data_ptr(), nj, nc, partials.data_ptr(), _lib.stream_ptr())
    out = _finish(partials, nc, max_norm)
    torch.cuda.synchronize()
    return out.cpu().numpy(), partials.cpu().numpy()


def _aligned(n, offset=0):
    """n device floats that begin `offset` floats after a 16-byte boundary (+ the buffer they live in)."""
    buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + n], buf


def _check_norm(host_ranges, dev_ranges, max_norm, what):
    ref = R.global_norm(host_ranges)
    out, _ = _norm(dev_ranges, max_norm)
    again, _ = _norm(dev_ranges, max_norm)
    print(f"{what}: norm {out[0]!r} reference {ref!r} relative error {abs(float(out[0]) - ref) / ref:.3e}; "
          f"coefficient {out[1]!r}")
    assert abs(float(out[0]) - ref) <= R.NORM_RTOL * ref, (what, out[0], ref)
    want = R.coef_f32(out[0], max_norm)
    assert out[1].view(np.int32) == np.float32(want).view(np.int32), (what, out[1], want)
    assert np.array_equal(out.view(np.int32), again.view(np.int32)), what          # two runs, the same bits
    return out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, C - 1, C, C + 1, 3 * C + 7])
def test_norm_of_one_job(n):
    x = synth.normal(n, (n,)).astype(np.float32)
    d, _ = _aligned(n)
    d.copy_(torch.from_numpy(x))
    big = _check_norm([x], [d], 1.0, f"n={n}")
    small = _check_norm([x], [d], 1e6, f"n={n} max_norm=1e6")            # the clamp: exactly 1
    assert big[0] == small[0] and small[1] == np.float32(1.0)


def test_norm_of_a_misaligned_job_and_of_a_table():
    n = 2 * C + 9
    x = synth.normal(5, (n,)).astype(np.float32)
    d, _ = _aligned(n, 1)                                                 # one float past a 16-byte boundary
    assert d.data_ptr() % 16 == 4
    d.copy_(torch.from_numpy(x))
    _check_norm([x], [d], 2.0, "misaligned")
    # 37 jobs of mixed sizes in one buffer, gaps of 0 .. 3 floats (every alignment; adjacent ranges where the gap is 0)
    sizes = [1, 2, 3, 5, 17, 64, 255, 256, 257, 1000, 1023, C - 1, C, C + 3, 4097, 1, 7, 33, 2 * C + 1, 129, 511, 6, 1,
             8, 9, 10, 11, 12, 13, 14, 15, 16, 100, 300, 700, 1025, 2049]
    assert len(sizes) == 37 and 1 in sizes
    gaps = [(3 * i) % 4 for i in range(37)]
    assert gaps[0] == 0 and gaps[4] == 0                                  # jobs 3 | 4 and the first job are adjacent
    total = sum(sizes) + sum(gaps)
    host = synth.normal(6, (total,)).astype(np.float32)
    buf = torch.from_numpy(host).cuda()
    hr, dr, pos = [], [], 0
    for s, g in zip(sizes, gaps):
        pos += g
        hr.append(host[pos:pos + s])
        dr.append(buf[pos:pos + s])
        pos += s
    assert any(dr[i].data_ptr() + 4 * sizes[i] == dr[i + 1].data_ptr() for i in range(36))
    _check_norm(hr, dr, 3.0, "37 jobs")


def test_norm_over_24_orders_of_magnitude():
    n = C + 77
    mag = 10.0 ** (synth.uniform(7, (n,)) * 24 - 12)                      # 1e-12 .. 1e12
    x = (synth.normal(8, (n,)) * mag).astype(np.float32)
    d, _ = _aligned(n)
    d.copy_(torch.from_numpy(x))
    _check_norm([x], [d], 1.0, "wide range")


def test_one_job_or_five_jobs_cut_at_chunk_boundaries_give_the_same_bits():
    n = 4 * C + 100
    x = synth.normal(9, (n,)).astype(np.float32)
    for offset in (0, 3):
        d, _ = _aligned(n, offset)
        d.copy_(torch.from_numpy(x))
        one, p1 = _norm([d], 1.0)
        five, p5 = _norm([d[i * C:min((i + 1) * C, n)] for i in range(5)], 1.0)
        assert p1.shape == p5.shape == (5,)
        assert np.array_equal(p1.view(np.int64), p5.view(np.int64))
        assert np.array_equal(one.view(np.int32), five.view(np.int32))


def test_non_finite_gradients():
    n = C + 5
    x = synth.normal(10, (n,)).astype(np.float32)
    d, _ = _aligned(n)
    for bad, at in ((np.nan, 3), (np.inf, C + 2), (-np.inf, 0)):
        y = x.copy()
        y[at] = bad
        d.copy_(torch.from_numpy(y))
        out, _ = _norm([d], 1.0)
        if np.isnan(bad):
            assert np.isnan(out[0]) and np.isnan(out[1])
        else:
            assert np.isposinf(out[0]) and out[1] == 0.0


@pytest.mark.parametrize("weight", [1.0, 0.5, 3.0 / 7.0])
def test_fold(weight):
    """Two jobs (one over a chunk long, one tiny); the gradient ranges sit at another alignment than the accumulator's."""
    sizes = [C + 5, 7]
    w32 = np.float32(weight)
    wdev = torch.tensor(float(weight), dtype=torch.float32).cuda()
    g_host = [synth.normal(20 + i, (s,)).astype(np.float32) for i, s in enumerate(sizes)]
    g2_host = [synth.normal(30 + i, (s,)).astype(np.float32) for i, s in enumerate(sizes)]
    for acc_off, g_off in ((0, 0), (0, 1), (2, 3)):
        gd = [_aligned(s, g_off)[0] for s in sizes]
        ad = [_aligned(s, acc_off)[0] for s in sizes]
        for a in ad:
            a.fill_(float("nan"))                                         # first = 1 must not read it
        for t, h in zip(gd, g_host):
            t.copy_(torch.from_numpy(h))
        tg, nj, nc = _table(gd)
        ta, _, _ = _table(ad)
        _lib.call("eav_grad_fold", tg.data_ptr(), ta.data_ptr(), nj, nc, wdev.data_ptr(), 1, None, _lib.stream_ptr())
        first = [a.cpu().numpy() for a in ad]
        for f, h in zip(first, g_host):
            assert not np.isnan(f).any()
            assert np.array_equal(f.view(np.int32), (w32 * h).view(np.int32))
        for t, h in zip(gd, g2_host):
            t.copy_(torch.from_numpy(h))
        partials = torch.full((nc,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.call("eav_grad_fold", tg.data_ptr(), ta.data_ptr(), nj, nc, wdev.data_ptr(), 0, partials.data_ptr(),
                  _lib.stream_ptr())
        folded = _finish(partials, nc, 1.0).cpu().numpy()
        worst = 0.0
        for a, old, h in zip(ad, first, g2_host):
            got = a.cpu().numpy().astype(np.float64)
            ref = R.fold(old, h, w32, False)
            bound = EPS * (np.abs(old.astype(np.float64)) + np.abs(np.float64(w32) * h))
            worst = max(worst, float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
            assert (np.abs(got - ref) <= bound).all()
        print(f"weight {weight!r} offsets {(acc_off, g_off)}: worst |acc - ref| / bound = {worst:.3f}")
        # the partials of the fold are those of eav_grad_sumsq over the accumulator afterwards
        after, pa = _norm(ad, 1.0)
        assert np.array_equal(partials.cpu().numpy().view(np.int64), pa.view(np.int64))
        assert np.array_equal(folded.view(np.int32), after.view(np.int32))
        assert abs(float(after[0]) - R.global_norm([a.cpu().numpy() for a in ad])) <= R.NORM_RTOL * float(after[0])


def _adam(name, p, g, m, v, n, wd, decoupled, step, step_dev, gscale=None):
    args = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-2, 0.9, 0.999, 1e-8, wd, step, int(decoupled),
            _lib.ptr(step_dev)]
    if gscale is not None:
        args.append(gscale.data_ptr())
    _lib.call(name, *args, _lib.stream_ptr())


@pytest.mark.parametrize("n", [1, 5, 1027])
@pytest.mark.parametrize("mode", ["adam", "adam-wd", "adamw"])
def test_scaled_adam_is_adam_on_a_gradient_scaled_beforehand(mode, n):
    wd, decoupled = {"adam": (0.0, False), "adam-wd": (0.01, False), "adamw": (0.01, True)}[mode]
    p0 = torch.from_numpy(synth.normal(40, (n,)).astype(np.float32)).cuda()
    g0 = torch.from_numpy(synth.normal(41, (n,)).astype(np.float32)).cuda()
    m0 = torch.from_numpy((0.1 * synth.normal(42, (n,))).astype(np.float32)).cuda()
    v0 = torch.from_numpy((0.01 * synth.normal(43, (n,)) ** 2).astype(np.float32)).cuda()
    dev3 = torch.tensor(3, dtype=torch.int64).cuda()
    for step, step_dev in ((3, None), (0, dev3)):                         # the host's count / the device's
        for scale in (1.0, 0.25, 0.3):
            sc = torch.tensor(scale, dtype=torch.float32).cuda()
            fed = g0 if scale == 1.0 else g0 * sc                         # torch's fp32 product, rounded on the device
            if scale == 0.25:
                assert torch.equal(fed, g0 * 0.25)
            ref = [t.clone() for t in (p0, m0, v0)]
            _adam("eav_adam_step", ref[0], fed, ref[1], ref[2], n, wd, decoupled, step, step_dev)
            got = [t.clone() for t in (p0, m0, v0)]
            g = g0.clone()
            _adam("eav_adam_step_scaled", got[0], g, got[1], got[2], n, wd, decoupled, step, step_dev, sc)
            torch.cuda.synchronize()
            assert torch.equal(g.view(torch.int32), g0.view(torch.int32))                 # the gradient is not written
            for a, b, what in zip(got, ref, "pmv"):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (mode, n, step, scale, what)
            assert not torch.equal(got[0], p0)


def test_scale_ranges():
    sizes, gaps = [1, C + 6, 5, 300], [1, 2, 0, 3]
    total = sum(sizes) + sum(gaps) + 4
    host = synth.normal(50, (total,)).astype(np.float32)
    for scalar in (0.37, 1.0, 0.0):
        buf = torch.from_numpy(host).cuda()
        want = torch.from_numpy(host).cuda()
        sc = torch.tensor(scalar, dtype=torch.float32).cuda()
        ranges, pos = [], 0
        for s, g in zip(sizes, gaps):
            pos += g
            ranges.append(buf[pos:pos + s])
            want[pos:pos + s] *= sc
            pos += s
        t, nj, nc = _table(ranges)
        _lib.call("eav_scale_ranges", t.data_ptr(), nj, nc, sc.data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), want.view(torch.int32)), scalar      # the gaps included: untouched
        if scalar == 1.0:
            assert torch.equal(buf.view(torch.int32), torch.from_numpy(host).cuda().view(torch.int32))
