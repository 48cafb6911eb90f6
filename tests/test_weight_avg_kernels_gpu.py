"""The averaging kernels of csrc/adam_jobs.hip through _lib.call: eav_adam_jobs_begin_avg + eav_adam_step_jobs_avg against
eav_adam_jobs_begin + eav_adam_step_jobs on copies of the same buffers (p, m, v, rates, counts and schedule record bit for
bit), the average in its three modes - copy: the new p's bits; skip: a sentinel pattern untouched; lerp: within the bound
tests/weight_avg_ref.py derives, against float64 fed with the kernel's own p - against themselves (one job or several,
two runs), eav_swap_jobs, and the record's s, n, mode and c over 25 steps against numpy float64 rounded once."""
import numpy as np
import pytest
import torch

from eav_amd import _lib, synth
from tests import weight_avg_ref as R

pytestmark = pytest.mark.gpu

C = _lib.plain("eav_grad_chunk_elems")
W = _lib.JOB_WORDS
B1, B2, EPS_ADAM = 0.9, 0.999, 1e-8
SIZES = [1, 3, 8191, 8192, 8193, 3 * 8192 + 5]
SENTINEL = np.array([0x7fc12345, -1, 0x7f800001, 0x00000001, 0x7fffffff, -0x7fffffff], dtype=np.int64).astype(np.int32)


def _at(host, offset):
    """A device copy of `host` (1-D float32) that begins `offset` floats after a 16-byte boundary."""
    buf = torch.zeros(host.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + host.size]
    view.copy_(torch.from_numpy(host))
    return view


def _bits(t):
    return t.cpu().numpy().view(np.int32)


class Job:
    """One job: host inputs; device copies for the averaging kernels (p, g, m, v, avg) and for the plain ones (p, g, m, v)."""

    def __init__(self, seed, n, step, lr, wd, offsets=(0, 0, 0, 0), avg_offset=0, avg=None):
        self.n, self.step, self.lr, self.wd = n, step, lr, wd
        self.p0 = synth.normal(seed, (n,)).astype(np.float32)
        self.g = (synth.normal(seed + 1, (n,)) * 10.0 ** (synth.uniform(seed + 2, (n,)) * 6 - 4)).astype(np.float32)
        self.m0 = (0.1 * synth.normal(seed + 3, (n,))).astype(np.float32)
        self.v0 = (synth.uniform(seed + 4, (n,)) * 1e-2).astype(np.float32) ** 2
        self.a0 = (self.p0 + 0.05 * synth.normal(seed + 5, (n,))).astype(np.float32) if avg is None else avg
        self.new = [_at(a, o) for a, o in zip((self.p0, self.g, self.m0, self.v0), offsets)]
        self.old = [_at(a, o) for a, o in zip((self.p0, self.g, self.m0, self.v0), offsets)]
        self.avg = _at(self.a0, avg_offset)


class Tables:
    """The averaging table over the jobs' `new` buffers and the plain one over `old`, with their counts, schedule records
    and the averaging record; step() runs one optimiser step on both."""

    def __init__(self, ranges_new, ranges_old, avgs, steps, lrs, wds, kind="ema", decay=0.9, warmup=False, start=0, every=1,
                 s=0, n=0):
        k = len(ranges_new)
        self.k = k
        self.counts = [torch.tensor([st - 1 for st in steps], dtype=torch.int64).cuda() for _ in range(2)]
        self.sched = [torch.zeros(_lib.SCHED_WORDS, dtype=torch.int64).cuda() for _ in range(2)]
        self.rows = []
        for ranges, counts in zip((ranges_new, ranges_old), self.counts):
            rows = torch.zeros(k, W, dtype=torch.int64)
            for j, r in enumerate(ranges):
                rows[j, :4] = torch.tensor([t.data_ptr() for t in r], dtype=torch.int64)
                rows[j, 4] = r[0].numel()
                rows[j, 6] = counts.data_ptr() + 8 * j
            rows[:, 5] = torch.tensor(lrs, dtype=torch.float64).view(torch.int64)
            rows[:, 7] = torch.tensor(wds, dtype=torch.float32).view(torch.int32).to(torch.int64) & 0xffffffff
            self.rows.append(rows.cuda())
        self.avgs = torch.tensor([a.data_ptr() for a in avgs], dtype=torch.int64).cuda()
        self.nchunks = sum(_lib.plain("eav_adam_jobs_nchunks", r[0].numel()) for r in ranges_new)
        self.rec = torch.tensor([s, n, 0, 0], dtype=torch.int64).cuda()
        assert self.rec.numel() == _lib.AVG_WORDS
        self.avg_args = (R.KINDS.index(kind), decay, int(warmup), start, every)
        self.sched_args = (0, 0, 0, 0.5, 1.0)

    @classmethod
    def of(cls, jobs, **kw):
        return cls([j.new for j in jobs], [j.old for j in jobs], [j.avg for j in jobs], [j.step for j in jobs],
                   [j.lr for j in jobs], [j.wd for j in jobs], **kw)

    def begin(self, plain=True):
        st = _lib.stream_ptr()
        _lib.call("eav_adam_jobs_begin_avg", self.rows[0].data_ptr(), self.k, self.counts[0].data_ptr(), self.k,
                  self.sched[0].data_ptr(), *self.sched_args, B1, B2, self.rec.data_ptr(), *self.avg_args, st)
        if plain:
            _lib.call("eav_adam_jobs_begin", self.rows[1].data_ptr(), self.k, self.counts[1].data_ptr(), self.k,
                      self.sched[1].data_ptr(), *self.sched_args, B1, B2, st)

    def step(self, decoupled, gscale=None, plain=True):
        """Returns (mode, c as an fp32 numpy scalar) of the step, read from the record."""
        self.begin(plain)
        st = _lib.stream_ptr()
        _lib.call("eav_adam_step_jobs_avg", self.rows[0].data_ptr(), self.avgs.data_ptr(), self.k, self.nchunks, B1, B2,
                  EPS_ADAM, int(decoupled), _lib.ptr(gscale), self.rec.data_ptr(), st)
        if plain:
            _lib.call("eav_adam_step_jobs", self.rows[1].data_ptr(), self.k, self.nchunks, B1, B2, EPS_ADAM, int(decoupled),
                      _lib.ptr(gscale), st)
        torch.cuda.synchronize()
        return self.record()[2:]

    def record(self):
        """(s, n, mode, c)."""
        rec = self.rec.cpu().numpy()
        return int(rec[0]), int(rec[1]), R.MODES[int(rec[2]) >> 32], rec[2:3].view(np.float32)[0]


def _same_as_plain(jobs, what):
    for i, j in enumerate(jobs):
        for name, a, b in zip("pgmv", j.new, j.old):
            assert np.array_equal(_bits(a), _bits(b)), (what, i, name, j.n)
        assert np.array_equal(_bits(j.new[1]), j.g.view(np.int32)), (what, i, "g was written")


@pytest.mark.parametrize("n", SIZES)
def test_every_offset_of_p_and_avg(n):
    """p and avg each 0 .. 3 floats past a 16-byte boundary, independently: the average is accessed as vectors where the
    offsets agree and element-wise otherwise, with head and tail elements.  Adam and AdamW, with and without gscale.
    Step 1 copies, step 2 lerps."""
    gscale = torch.tensor(0.37, dtype=torch.float32).cuda()
    worst = 0.0
    for po in range(4):
        for ao in range(4):
            for decoupled, scaled in ((0, False), (1, True), (1, False), (0, True)):
                job = Job(10 * n + 4 * po + ao, n, 11, 3e-3, 0.01, (po, (po + 1) % 4, (po + 2) % 4, (po + 3) % 4), ao)
                assert job.new[0].data_ptr() % 16 == 4 * po and job.avg.data_ptr() % 16 == 4 * ao
                t = Tables.of([job], kind="ema", decay=0.9)
                what = f"n={n} p+{po} avg+{ao} decoupled={decoupled} scaled={scaled}"
                mode, c = t.step(decoupled, gscale if scaled else None)
                assert (mode, c) == ("copy", np.float32(1.0)), what
                _same_as_plain([job], what)
                assert np.array_equal(_bits(job.avg), _bits(job.new[0])), (what, "copy")
                assert not np.array_equal(_bits(job.new[0]), job.p0.view(np.int32))
                ref = R.Tracked(job.new[0].cpu().numpy())
                mode, c = t.step(decoupled, gscale if scaled else None)
                assert (mode, c) == ("lerp", np.float32(1.0 - 0.9)), what
                _same_as_plain([job], what)
                ref.update("lerp", float(c), job.new[0].cpu().numpy())
                worst = max(worst, ref.check(job.avg.cpu().numpy(), what))
                assert not np.array_equal(_bits(job.avg), _bits(job.new[0]))
                assert np.array_equal(t.rows[0].cpu()[:, 8:], t.rows[1].cpu()[:, 8:])          # lr, bc1, bc2s
    assert n < 8 or worst > 0.01                       # the bound is not vacuous


TABLE_SIZES = [1, 3, 5, 17, 255, 257, 1000, C - 1, C, C + 3, 4097, 1, 7, 2 * C + 1, 129, 6, 8, 9, 10, 11, 300, 1025]


@pytest.mark.parametrize("kind,decoupled,scaled", [("ema", 1, False), ("swa", 0, True)])
def test_table_of_22_jobs_five_steps_and_a_second_run(kind, decoupled, scaled):
    """Mixed sizes, step counts, rates and weight decays, every alignment of p and avg; one copy and four lerps against
    float64 fed with the kernel's own p; a second run from the same inputs gives the same bits."""
    def make():
        return [Job(2000 + 7 * i, n, (1, 11)[i % 2], (1e-3, 3e-3, 2.5e-4)[i % 3], (0.0, 0.01)[(i // 2) % 2],
                    (i % 4, (i // 4) % 4, (i // 2) % 4, (3 * i) % 4), (i // 3) % 4) for i, n in enumerate(TABLE_SIZES)]
    gscale = torch.tensor(0.37, dtype=torch.float32).cuda() if scaled else None
    runs = []
    for run in range(2):
        jobs = make()
        t = Tables.of(jobs, kind=kind, decay=0.999, warmup=True)
        refs = [R.Tracked(j.p0) for j in jobs]
        n = 0
        for s in range(1, 6):
            mode, c = t.step(decoupled, gscale, plain=run == 0)
            want_mode, want_c = R.mode_and_coefficient(kind, s, n, decay=0.999, warmup=True)
            n += 1
            assert mode == want_mode and c.view(np.int32) == R.coefficient_f32(want_c).view(np.int32), (s, mode, c, want_c)
            if run == 0:
                _same_as_plain(jobs, f"{kind} step {s}")
                for j, ref in zip(jobs, refs):
                    ref.update(mode, float(c), j.new[0].cpu().numpy())
        if run == 0:
            worst = max(ref.check(j.avg.cpu().numpy(), f"{kind} job {i} ({j.n})")
                        for i, (j, ref) in enumerate(zip(jobs, refs)))
            assert worst > 0.05 and all(ref.updates == 4 for ref in refs)
        runs.append([[_bits(x) for x in j.new + [j.avg]] for j in jobs])
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_skip_leaves_a_sentinel_average_untouched():
    """Not an averaging step: the averages - NaN payloads, infinities' neighbours, denormals - are neither read nor
    written, p, m and v are stepped all the same; n stays 0 and the next averaging step copies."""
    jobs = []
    for i, n in enumerate(SIZES):
        sentinel = np.resize(SENTINEL, n).view(np.float32)
        jobs.append(Job(3000 + 7 * i, n, 11, 1e-3, 0.01, (i % 4, 0, 1, 2), (i + 1) % 4, avg=sentinel))
    t = Tables.of(jobs, kind="ema", decay=0.9, start=3, every=2)
    for s in (1, 2):
        assert t.step(1) == ("skip", np.float32(0.0))
        assert t.record()[:2] == (s, 0)
        _same_as_plain(jobs, f"skip {s}")
        for j in jobs:
            assert np.array_equal(_bits(j.avg), np.resize(SENTINEL, j.n)), j.n
            assert not np.array_equal(_bits(j.new[0]), j.p0.view(np.int32))
    assert t.step(1)[0] == "copy" and t.record()[:2] == (3, 1)
    for j in jobs:
        assert np.array_equal(_bits(j.avg), _bits(j.new[0]))
    assert t.step(1)[0] == "skip" and t.record()[:2] == (4, 1)
    for j in jobs:
        assert not np.array_equal(_bits(j.avg), _bits(j.new[0]))
    assert t.step(1)[0] == "lerp" and t.record()[:2] == (5, 2)


def test_one_job_or_several_cut_anywhere_give_the_same_bits():
    n = 3 * C + 100
    cuts = [0, 5, 6, C + 3, 2 * C + 2, 2 * C + 1025, n]                   # arbitrary element boundaries: every alignment
    for o, ao in ((0, 0), (3, 1)):
        offs = (o, (o + 1) % 4, (o + 2) % 4, o)
        one, cut = Job(77, n, 11, 2e-3, 0.01, offs, ao), Job(77, n, 11, 2e-3, 0.01, offs, ao)
        t1 = Tables.of([one], s=4, n=4)
        assert t1.step(1, plain=False)[0] == "lerp"
        k = len(cuts) - 1
        rn = [tuple(x[a:b] for x in cut.new) for a, b in zip(cuts[:-1], cuts[1:])]
        t2 = Tables(rn, rn, [cut.avg[a:b] for a, b in zip(cuts[:-1], cuts[1:])], [11] * k, [2e-3] * k, [0.01] * k, s=4, n=4)
        assert t2.nchunks == 6 and t1.nchunks == 4
        assert t2.step(1, plain=False)[0] == "lerp"
        for name, a, b in zip("pgmva", one.new + [one.avg], cut.new + [cut.avg]):
            assert np.array_equal(_bits(a), _bits(b)), (o, name)
        assert not np.array_equal(_bits(one.avg), one.a0.view(np.int32))


def test_swap_twice_restores_both_buffers():
    jobs = [Job(4000 + 7 * i, n, 1, 1e-3, 0.0, (i % 4, 0, 0, 0), (2 * i + 1) % 4) for i, n in enumerate(SIZES + [2 * C + 2])]
    for i, j in enumerate(jobs):                                    # any bit pattern is data to a swap
        j.avg[:min(j.n, SENTINEL.size)] = torch.from_numpy(np.resize(SENTINEL, min(j.n, SENTINEL.size)).view(np.float32))
    t = Tables.of(jobs)
    p0, a0 = [_bits(j.new[0]).copy() for j in jobs], [_bits(j.avg).copy() for j in jobs]
    for flip in (1, 2):
        _lib.call("eav_swap_jobs", t.rows[0].data_ptr(), t.avgs.data_ptr(), t.k, t.nchunks, _lib.stream_ptr())
        torch.cuda.synchronize()
        for j, p, a in zip(jobs, p0, a0):
            assert np.array_equal(_bits(j.new[0]), a if flip == 1 else p), (flip, j.n)
            assert np.array_equal(_bits(j.avg), p if flip == 1 else a), (flip, j.n)
            for x, h in zip(j.new[1:], (j.g, j.m0, j.v0)):
                assert np.array_equal(_bits(x), h.view(np.int32))


CONFIGS = [("ema", d, w) for d in (0.9, 0.999, 0.9999) for w in (False, True)] + [("swa", 0.999, False)]


@pytest.mark.parametrize("kind,decay,warmup", CONFIGS)
def test_begin_variant_over_25_steps(kind, decay, warmup):
    """s, n, mode and c of 25 consecutive steps equal numpy float64 rounded once, for start_step 0 / 7 and every 1 / 3;
    schedule record, counts and the rows' rates and bias corrections are eav_adam_jobs_begin's, bit for bit (cosine
    schedule with warmup, four jobs with their own base rates and counts)."""
    dummy = torch.zeros(16, dtype=torch.float32, device="cuda")
    for start in (0, 7):
        for every in (1, 3):
            t = Tables([(dummy,) * 4] * 4, [(dummy,) * 4] * 4, [dummy] * 4, [1, 11, 2, 7], [5e-6, 1e-3, 2.1e-6, 3.3e-4],
                       [0.0] * 4, kind=kind, decay=decay, warmup=warmup, start=start, every=every)
            t.sched_args = (3, 3, 20, 0.5, 1e-3)
            want = R.sequence(kind, 25, decay=decay, warmup=warmup, start_step=start, every=every)
            seen = set()
            for s, n, mode, c in want:
                t.begin()
                torch.cuda.synchronize()
                got = t.record()
                assert got[:3] == (s, n, mode), (start, every, got, (s, n, mode))
                assert got[3].view(np.int32) == R.coefficient_f32(c).view(np.int32), (start, every, s, got[3], c)
                seen.add(mode)
                assert torch.equal(t.sched[0], t.sched[1]) and torch.equal(t.counts[0], t.counts[1])
                assert torch.equal(t.rows[0][:, 8:], t.rows[1][:, 8:])
            assert seen == {"copy", "lerp"} | ({"skip"} if start or every > 1 else set())
            assert int(t.sched[0][0]) == 25 and t.counts[0].cpu().tolist() == [25, 35, 26, 31]
            assert [s for s, _, m, _ in want if m != "skip"][0] == (max(start, 1) if every == 1 else (start or every))
