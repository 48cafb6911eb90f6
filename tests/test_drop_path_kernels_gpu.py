"""The two kernels of csrc/drop_path.hip through the C ABI against the numpy restatement of tests/drop_path_ref.py: the plan's
keep table by integer equality and its scales within 1 ulp of float32 1 / (1 - p_i) (exact under an explicit keep table), the
add / gate bit for bit - signed zeros included, and NaN exactly where numpy has NaN (the Inf of a dropped sample: IEEE 754
leaves a NaN's sign and payload open, x86 and gfx950 choose differently) - in place and out of place, twice.  Every output
sits between sentinel bands that are compared after the launch."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import drop_path_ref as R

pytestmark = pytest.mark.gpu

BAND = 256
SEED = 20240607


@pytest.fixture(scope="module")
def L():
    import gc
    from eav_amd import _lib
    _lib.load()
    yield _lib
    gc.collect()


class Banded:
    """A contiguous float32 device tensor of `shape` between two NaN sentinel bands."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * BAND,), float("nan"), dtype=torch.float32, device="cuda")
        self.t = self.whole[BAND:BAND + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def host(self, what):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert np.isnan(np.concatenate([w[:BAND], w[-BAND:]])).all(), what + ": wrote outside its output"
        return self.t.cpu().numpy()


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """Bit equality; where `want` is NaN, `got` must be NaN (of any sign and payload)."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def plan_seed(seed):
    return R.site_seed(seed, R.site_ids(0)[0])


def run_plan(L, layers, B, r, seed, cnt=None, keep=None):
    scale = Banded((layers, 2, B))
    c = None if cnt is None else torch.tensor(int(cnt), dtype=torch.int64, device="cuda")
    k = None if keep is None else dev(keep, np.uint8)
    L.call("eav_drop_path_plan", scale.ptr(), layers, B, float(r), plan_seed(seed), None if c is None else c.data_ptr(),
           None if k is None else k.data_ptr(), None)
    return scale.host(f"plan L={layers} B={B} r={r}")


# ============================================================================================ plan
@pytest.mark.parametrize("cnt", R.PLAN_COUNTERS)
@pytest.mark.parametrize("r", R.PLAN_RATES)
@pytest.mark.parametrize("layers,B", R.PLAN_CASES)
def test_plan_is_the_restatement(L, layers, B, r, cnt):
    keep, scale = R.plan(layers, B, r, SEED, cnt)
    got = run_plan(L, layers, B, r, SEED, cnt)
    assert np.array_equal((got != 0).astype(np.uint8), keep)
    p = R.rates(r, layers)
    for i in range(layers):
        row = got[i]
        if p[i] == 0:
            assert (bits(row) == bits(np.float32(1.0))).all(), i
            continue
        want = R.scale32(p[i])
        kept = row[row != 0]
        assert (bits(row[row == 0]) == 0).all()                      # +0.0, not -0.0
        assert (np.abs(kept.astype(np.float64) - np.float64(want)) <= np.spacing(want)).all(), (i, kept[:1], want)
    assert np.array_equal(bits(got), bits(scale))                    # (the division is the restatement's: the same bits)
    # without a counter the seed itself draws; another counter, another table (where there is anything to draw)
    assert np.array_equal((run_plan(L, layers, B, r, SEED) != 0).astype(np.uint8), R.plan(layers, B, r, SEED)[0])
    if layers > 1 and layers * B >= 24:
        assert not np.array_equal(R.plan(layers, B, r, SEED, cnt + 1)[0], keep)


@pytest.mark.parametrize("r", R.PLAN_RATES)
@pytest.mark.parametrize("layers,B", R.PLAN_CASES)
def test_plan_from_an_explicit_table_is_exact(L, layers, B, r):
    keep = (synth.uniform(700 + layers + B, (layers, 2, B)) >= 0.4).astype(np.uint8)
    keep[-1, 1] = 0                                                  # a branch dropped for the whole batch
    keep[-1, 0, 0] = 1
    want_keep, want = R.plan(layers, B, r, SEED, 3, keep=keep)
    got = run_plan(L, layers, B, r, SEED, 3, keep=keep)
    assert np.array_equal(bits(got), bits(want))
    if layers > 1:
        assert np.array_equal(want_keep[1:], keep[1:]) and not got[-1, 1].any() and got[-1, 0, 0] == R.scale32(R.rates(r, layers)[-1])
    assert (got[0] == 1).all()                                       # p_0 = 0: the table's row is not read


# ============================================================================================ add / gate
def _inputs(B, per):
    y = synth.normal(800 + B, (B, per), 0.0, 1.0)
    resid = synth.normal(801 + B, (B, per), 0.0, 1.0)
    y[0, 0], y[-1, -1], y[0, per // 2] = -0.0, -0.0, 0.0
    resid[0, 0], resid[-1, -2] = -0.0, -0.0
    return y, resid


def _rows(B):
    """name -> (scale row, the sample that holds the Inf or None)."""
    s = R.scale32(np.float32(0.25))
    mixed = np.where(np.arange(B) % 2 == 0, s, np.float32(0)).astype(np.float32)
    if B > 1:
        mixed[-1] = 0
    return {"kept": (np.full(B, s, np.float32), None), "dropped": (np.zeros(B, np.float32), B - 1),
            "mixed": (mixed, B - 1 if B > 1 else None)}


@pytest.mark.parametrize("B,per", R.ADD_CASES)
def test_add_and_gate_match_numpy_bit_for_bit(L, B, per):
    y0, resid = _inputs(B, per)
    for name, (row, inf_at) in _rows(B).items():
        y = y0.copy()
        if inf_at is not None:
            y[inf_at, per // 3] = np.inf                             # Inf x 0 = NaN, as x * 0 gives in torch
        srow = dev(row)
        for with_resid in (True, False):
            want = R.add(y, resid if with_resid else None, row)
            if inf_at is not None:
                assert np.isnan(want[inf_at, per // 3])
            rt = dev(resid) if with_resid else None                  # (kept alive across the launches)
            rp = None if rt is None else rt.data_ptr()
            for in_place in (False, True):
                runs = []
                for _ in range(2):
                    out = Banded((B, per))
                    if in_place:
                        out.t.copy_(dev(y))
                        src = out.ptr()
                    else:
                        yt = dev(y)
                        src = yt.data_ptr()
                    L.call("eav_drop_path_add", src, rp, out.ptr(), srow.data_ptr(), B, per, None)
                    runs.append(out.host(f"add B={B} per={per} {name} resid={with_resid} in_place={in_place}"))
                what = (name, with_resid, in_place)
                assert same(runs[0], want), what
                assert np.array_equal(bits(runs[0]), bits(runs[1])), what


def test_add_beyond_one_pass_of_the_grid(L):
    """More float4 than the 8192 x 256 threads of the largest grid: the grid-stride loop comes round, a workgroup's second
    pass lies in another sample."""
    B, per = R.ADD_LOOP_CASE
    assert B * per // 4 > 8192 * 256
    y, resid = _inputs(B, per)
    row = _rows(B)["mixed"][0]
    out, rt, srow = Banded((B, per)), dev(resid), dev(row)
    out.t.copy_(dev(y))
    L.call("eav_drop_path_add", out.ptr(), rt.data_ptr(), out.ptr(), srow.data_ptr(), B, per, None)
    assert same(out.host("add beyond one pass"), R.add(y, resid, row))
