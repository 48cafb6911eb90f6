"""The kernels of csrc/adam_jobs.hip through _lib.call: eav_adam_jobs_begin + eav_adam_step_jobs against eav_adam_step /
eav_adam_step_scaled with a device step count (bit for bit: one launch of the existing kernel per job, on copies of the
same buffers), against themselves (a range as one job or cut into several; two runs) and against the float64 reference of
tests/adam_jobs_ref.py within the bounds its docstring derives (tests/test_adam_jobs_cpu.py confirms them for the float32
restatement of the kernel).  eav_adam_jobs_begin's own outputs - counts, schedule factor, rates - are compared with numpy
float64 arithmetic rounded once to fp32."""
import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import adam_jobs_ref as A

pytestmark = pytest.mark.gpu

C = _lib.plain("eav_grad_chunk_elems")
W = _lib.JOB_WORDS
B1, B2, EPS_ADAM = 0.9, 0.999, 1e-8


def _at(host, offset):
    """A device copy of `host` (1-D float32) that begins `offset` floats after a 16-byte boundary."""
    buf = torch.zeros(host.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + host.size]
    view.copy_(torch.from_numpy(host))
    return view


class Job:
    """One job: host inputs, two device copies (new kernel / existing kernel), hyper-parameters."""

    def __init__(self, seed, n, step, lr, wd, offsets=(0, 0, 0, 0)):
        self.n, self.step, self.lr, self.wd = n, step, lr, wd
        self.p0 = synth.normal(seed, (n,)).astype(np.float32)
        self.g = (synth.normal(seed + 1, (n,)) * 10.0 ** (synth.uniform(seed + 2, (n,)) * 6 - 4)).astype(np.float32)
        if step == 1:
            self.m0, self.v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            self.m0 = (0.1 * synth.normal(seed + 3, (n,))).astype(np.float32)
            self.v0 = (synth.uniform(seed + 4, (n,)) * 1e-2).astype(np.float32) ** 2
        self.new = [_at(a, o) for a, o in zip((self.p0, self.g, self.m0, self.v0), offsets)]
        self.old = [_at(a, o) for a, o in zip((self.p0, self.g, self.m0, self.v0), offsets)]


def _table(ranges, lrs, wds, step_ptrs):
    """Device rows (include/eav_hip.h) for ranges = [(p, g, m, v) tensor views]; returns (rows, njobs, nchunks)."""
    n = len(ranges)
    rows = torch.zeros(n, W, dtype=torch.int64)
    for j, r in enumerate(ranges):
        rows[j, :4] = torch.tensor([t.data_ptr() for t in r], dtype=torch.int64)
        rows[j, 4] = r[0].numel()
        rows[j, 6] = step_ptrs[j]
    rows[:, 5] = torch.tensor(lrs, dtype=torch.float64).view(torch.int64)
    rows[:, 7] = torch.tensor(wds, dtype=torch.float32).view(torch.int32).to(torch.int64) & 0xffffffff
    nchunks = sum(_lib.plain("eav_adam_jobs_nchunks", r[0].numel()) for r in ranges)
    return rows.cuda(), n, nchunks


def _sched(t=0):
    return torch.tensor([t, 0, 0, 0], dtype=torch.int64).cuda()


def _begin(rows, njobs, counts, sched, kind=0, warmup=0, total=0, cycles=0.5, report_lr=1.0):
    _lib.call("eav_adam_jobs_begin", rows.data_ptr(), njobs, _lib.ptr(counts), 0 if counts is None else counts.numel(),
              sched.data_ptr(), kind, warmup, total, cycles, report_lr, B1, B2, _lib.stream_ptr())


def _step(rows, njobs, nchunks, decoupled, gscale=None):
    _lib.call("eav_adam_step_jobs", rows.data_ptr(), njobs, nchunks, B1, B2, EPS_ADAM, int(decoupled), _lib.ptr(gscale),
              _lib.stream_ptr())


def _run_new(jobs, decoupled, gscale=None):
    """begin + step over the jobs' `new` buffers with per-job counts; returns the rows read back (int64 [n, W])."""
    counts = torch.tensor([j.step - 1 for j in jobs], dtype=torch.int64).cuda()
    rows, nj, nc = _table([j.new for j in jobs], [j.lr for j in jobs], [j.wd for j in jobs],
                          [counts.data_ptr() + 8 * i for i in range(len(jobs))])
    sched = _sched()
    _begin(rows, nj, counts, sched)
    _step(rows, nj, nc, decoupled, gscale)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [j.step for j in jobs]            # advanced by exactly 1
    assert sched.cpu().tolist()[0] == 1
    return rows.cpu()


def _run_old(jobs, decoupled, gscale=None):
    """The existing kernel, one launch per job, bias corrections from a device step count (its step_dev branch)."""
    for j in jobs:
        cnt = torch.tensor(j.step, dtype=torch.int64).cuda()
        p, g, m, v = j.old
        args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), j.n, float(np.float32(j.lr)), B1, B2, EPS_ADAM,
                j.wd, 0, int(decoupled), cnt.data_ptr())
        if gscale is None:
            _lib.call("eav_adam_step", *args, _lib.stream_ptr())
        else:
            _lib.call("eav_adam_step_scaled", *args, gscale.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _check(jobs, decoupled, gscale, what):
    """Bit for bit against the existing kernel; within the float64 bounds; g untouched."""
    gs = None if gscale is None else float(gscale.cpu())
    worst = 0.0
    for i, j in enumerate(jobs):
        for name, a, b in zip("pgmv", j.new, j.old):
            assert np.array_equal(_bits(a), _bits(b)), (what, i, name, j.n, j.step)
        assert np.array_equal(_bits(j.new[1]), j.g.view(np.int32)), (what, i, "g was written")
        pr, mr, vr, tp, tm, tv, _ = A.step_bounds(j.p0, j.g, j.m0, j.v0, np.float32(j.lr), j.wd, j.step, B1, B2, EPS_ADAM,
                                                  decoupled, gs)
        for name, got, ref, tol in (("p", j.new[0], pr, tp), ("m", j.new[2], mr, tm), ("v", j.new[3], vr, tv)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            ratio = float(np.max(err / np.maximum(tol, 1e-300)))
            worst = max(worst, ratio)
            assert np.all(err <= tol), (what, i, name, ratio)
    print(f"{what}: worst error / float64 bound {worst:.3f}")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, C - 1, C, C + 1, 3 * C + 7])
def test_one_job_at_every_alignment(n):
    """p beginning 0 .. 3 floats past a 16-byte boundary, g / m / v each at a different offset from p."""
    for o in range(4):
        offsets = (o, (o + 1) % 4, (o + 2) % 4, (o + 3) % 4)
        step, decoupled, wd = (1, 11, 1, 11)[o], o < 2, (0.01, 0.0, 0.01, 0.01)[o]
        job = Job(100 * n + 10 * o, n, step, 3e-3, wd, offsets)
        assert [t.data_ptr() % 16 for t in job.new] == [4 * x for x in offsets]
        rows = _run_new([job], decoupled)
        _run_old([job], decoupled)
        _check([job], decoupled, None, f"n={n} offsets={offsets}")
        lr, bc1, bc2s = rows.view(torch.float32)[0, 16:19].numpy()
        want = A.bias_corrections_f32(B1, B2, step)
        assert lr == np.float32(3e-3) and (bc1, bc2s) == want, (lr, bc1, bc2s, want)


SIZES = [1, 2, 3, 5, 17, 64, 255, 256, 257, 1000, 1023, C - 1, C, C + 3, 4097, 1, 7, 33, 2 * C + 1, 129, 511, 6, 1,
         8, 9, 10, 11, 12, 13, 14, 15, 16, 100, 300, 700, 1025, 2049]


@pytest.mark.parametrize("decoupled", [0, 1])
@pytest.mark.parametrize("scaled", [False, True])
def test_table_of_37_jobs(decoupled, scaled):
    """Mixed sizes (several of one element), step counts 1 and 11, three rates, weight decay 0 and 0.01, every alignment."""
    assert len(SIZES) == 37 and SIZES.count(1) == 3
    jobs = [Job(1000 + 7 * i, n, (1, 11)[i % 2], (1e-3, 3e-3, 2.5e-4)[i % 3], (0.0, 0.01)[(i // 2) % 2],
                (i % 4, (i // 4) % 4, (i // 2) % 4, (3 * i) % 4)) for i, n in enumerate(SIZES)]
    gscale = torch.tensor(0.37, dtype=torch.float32).cuda() if scaled else None
    rows = _run_new(jobs, decoupled, gscale)
    _run_old(jobs, decoupled, gscale)
    _check(jobs, decoupled, gscale, f"37 jobs decoupled={decoupled} scaled={scaled}")
    derived = rows.view(torch.float32)[:, 16:19].numpy()
    for i, j in enumerate(jobs):
        assert derived[i, 0] == np.float32(j.lr) and tuple(derived[i, 1:]) == A.bias_corrections_f32(B1, B2, j.step), i
    # a second run from the same inputs gives the same bits
    again = [Job(1000 + 7 * i, j.n, j.step, j.lr, j.wd, tuple(t.data_ptr() % 16 // 4 for t in j.new)) for i, j in enumerate(jobs)]
    _run_new(again, decoupled, gscale)
    for a, b in zip(jobs, again):
        for x, y in zip(a.new, b.new):
            assert np.array_equal(_bits(x), _bits(y))


def test_one_job_or_several_cut_anywhere_give_the_same_bits():
    n = 3 * C + 100
    cuts = [0, 5, 6, C + 3, 2 * C + 2, 2 * C + 1025, n]                   # arbitrary element boundaries: every alignment
    for o in (0, 3):
        one = Job(77, n, 11, 2e-3, 0.01, (o, (o + 1) % 4, (o + 2) % 4, o))
        cut = Job(77, n, 11, 2e-3, 0.01, (o, (o + 1) % 4, (o + 2) % 4, o))
        _run_new([one], 1)
        counts = torch.full((len(cuts) - 1,), 10, dtype=torch.int64).cuda()
        ranges = [tuple(t[a:b] for t in cut.new) for a, b in zip(cuts[:-1], cuts[1:])]
        k = len(ranges)
        rows, nj, nc = _table(ranges, [2e-3] * k, [0.01] * k, [counts.data_ptr() + 8 * i for i in range(k)])
        assert nc == 6 and _lib.plain("eav_adam_jobs_nchunks", n) == 4
        _begin(rows, nj, counts, _sched())
        _step(rows, nj, nc, 1)
        torch.cuda.synchronize()
        for name, a, b in zip("pgmv", one.new, cut.new):
            assert np.array_equal(_bits(a), _bits(b)), (o, name)
        assert not np.array_equal(_bits(one.new[0]), one.p0.view(np.int32))


def test_more_chunks_than_the_grid():
    """One job of 2049 chunks + 5 elements: the grid stride wraps.  Checked against the existing kernel only."""
    n = 2049 * C + 5
    gen = torch.Generator(device="cuda").manual_seed(5)
    p = torch.randn(n, device="cuda", generator=gen)
    g = torch.randn(n, device="cuda", generator=gen) * 0.1
    m = torch.randn(n, device="cuda", generator=gen) * 0.05
    v = torch.rand(n, device="cuda", generator=gen) * 1e-3
    new, old = [t.clone() for t in (p, g, m, v)], [t.clone() for t in (p, g, m, v)]
    counts = torch.tensor([4], dtype=torch.int64).cuda()
    rows, nj, nc = _table([tuple(new)], [1e-3], [0.01], [counts.data_ptr()])
    assert nc == 2050 > 2048
    _begin(rows, nj, counts, _sched())
    _step(rows, nj, nc, 1)
    cnt = torch.tensor(5, dtype=torch.int64).cuda()
    _lib.call("eav_adam_step", old[0].data_ptr(), old[1].data_ptr(), old[2].data_ptr(), old[3].data_ptr(), n,
              float(np.float32(1e-3)), B1, B2, EPS_ADAM, 0.01, 0, 1, cnt.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    for name, a, b in zip("pgmv", new, old):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert not torch.equal(new[0], p) and torch.equal(new[1], g)
    # nchunks smaller than the table holds: the jobs beyond are not touched; larger: nothing out of range is touched
    q = [t.clone() for t in (p, g, m, v)]
    rows2, _, _ = _table([tuple(t[:C + 1] for t in q)], [1e-3], [0.0], [counts.data_ptr()])
    _begin(rows2, 1, None, _sched())
    _step(rows2, 1, 1, 1)
    torch.cuda.synchronize()
    assert not torch.equal(q[0][:C], p[:C]) and torch.equal(q[0][C:], p[C:])
    _step(rows2, 1, 7, 1)
    torch.cuda.synchronize()
    assert torch.equal(q[0][C + 1:], p[C + 1:]) and not torch.equal(q[0][C:C + 1], p[C:C + 1])


TS = [0, 1, 2, 3, 4, 9, 10, 15]           # {0, 1, W - 1, W, W + 1, T - 1, T, T + 5} for W = 3, T = 10


@pytest.mark.parametrize("kind", A.KINDS)
def test_begin_evaluates_the_schedule_on_the_device(kind):
    Wm, T = 3, 10
    bases = [5e-6, 1e-3, 0.75 ** 3 * 5e-6, 3.3e-4]
    steps = [1, 11, 2, 7]
    dummy = torch.zeros(16, dtype=torch.float32, device="cuda")
    for t in TS:
        counts = torch.tensor([s - 1 for s in steps], dtype=torch.int64).cuda()
        rows, nj, _ = _table([(dummy, dummy, dummy, dummy)] * 4, bases, [0.0] * 4,
                             [counts.data_ptr() + 8 * i for i in range(4)])
        sched = _sched(t)
        _begin(rows, nj, counts, sched, A.KINDS.index(kind), Wm, T, 0.5, report_lr=bases[1])
        torch.cuda.synchronize()
        assert counts.cpu().tolist() == steps
        rec = sched.cpu()
        f64 = A.schedule_factor(kind, t, Wm, T)
        got_f = float(rec.view(torch.float64)[1])
        got = rows.cpu().view(torch.float32)[:, 16:19].numpy()
        assert int(rec[0]) == t + 1
        for i, base in enumerate(bases):
            want = A.lr_f32(base, f64)
            if kind == "cosine":
                # the device's cos may differ from the host's in the last double bits: one fp32 ulp of the value, plus
                # the factor's own absolute error (a few ulps of 1.0 in double) times the base rate - what is left
                # where the value itself is 0 (t = T)
                assert abs(float(got[i, 0]) - float(want)) <= float(np.spacing(want)) + base * 2.0 ** -50, (t, i, got[i, 0], want)
            else:                                      # an exact IEEE division
                assert got[i, 0].view(np.int32) == want.view(np.int32), (kind, t, i, got[i, 0], want)
            assert tuple(got[i, 1:]) == A.bias_corrections_f32(B1, B2, steps[i])
        if kind == "cosine":
            assert abs(got_f - f64) <= 2.0 ** -51, (t, got_f, f64)           # 0.5 (1 + cos): a few ulps of 1.0
        else:
            assert got_f == f64, (kind, t, got_f, f64)
        assert rec.view(torch.float32)[4].numpy() == np.float32(np.float64(bases[1]) * got_f)
    # ncounts = 0: a count the caller advances itself (a capturable optimiser's) is read, not written
    shared = torch.tensor([6], dtype=torch.int64).cuda()
    rows, nj, _ = _table([(dummy, dummy, dummy, dummy)] * 2, bases[:2], [0.0] * 2, [shared.data_ptr()] * 2)
    _begin(rows, nj, None, _sched())
    torch.cuda.synchronize()
    assert shared.item() == 6
    got = rows.cpu().view(torch.float32)[:, 17:19].numpy()
    assert tuple(got[0]) == tuple(got[1]) == A.bias_corrections_f32(B1, B2, 6)
