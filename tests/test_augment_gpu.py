"""eav_augment_gather (csrc/augment.hip) against the NumPy restatement of tests/augment_ref.py, and BatchAugment.apply on
a planned epoch.

Bounds: a masked cell equals `fill` exactly; a record with lambda = 1 hands the source's bits through (and is bit-equal
to gather_batch where it neither flips nor masks), whatever its partner holds - a NaN is planted there; a mixed cell lies
within 2^-22 (lambda |a| + (1 - lambda) |b|) of float64: four fp32 roundings of at most 2^-24 each - the two products,
1 - lambda and the sum; the soft targets are exact.  Shapes: C % 4 != 0 (scalar path), C = 4 k (16-byte path, flips
reversing inside and across the vectors), the one-element sample, several rows of a short vector row."""
import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests import kernel_check as kc

pytestmark = pytest.mark.gpu

SHAPES = [(9, 4, 3, 5), (5, 3, 7, 128), (3, 2, 1, 1), (6, 5, 9, 12)]
NC = 5
FILL = -1.5


def _pool(N, R, C):
    """Records over the samples 0 .. N - 2; sample N - 1 holds a NaN and is the partner of lambda = 1 records only."""
    M, nan = N - 1, N - 1
    s = lambda k: k % M                                                   # noqa: E731
    half_r, half_c = (R + 1) // 2, C // 2 + 1
    return [
        ar.record(s(0), nan, 1.0),                                                          # the plain gather
        ar.record(s(1), nan, 1.0, flip=True),
        ar.record(s(0), s(1), 0.7),
        ar.record(s(1), s(0), 0.5, flip=True),
        ar.record(s(2), s(2), 0.8),                                                         # i == j
        ar.record(s(0), s(1), 0.9, rows=((0, R), (0, 0))),                                  # full row band
        ar.record(s(1), s(2), 0.6, flip=True, cols=((0, 0), (0, C))),                       # full column band
        ar.record(s(2), s(0), 0.75, rows=((0, half_r), (R // 3, R)),                        # overlapping bands
                  cols=((0, min(half_c, C)), (C // 4, min(half_c + 1, C)))),
        ar.record(s(0), s(2), 0.65, rows=((2, 1), (R, R)), cols=((C, 0), (3, 3))),          # empty bands of every spelling
        ar.record(s(1), s(0), 0.55, flip=True, rows=((R // 2, R // 2 + 1), (0, 0)),
                  cols=((1, min(3, C)), (C - 1, C))),
        ar.record(s(2), nan, 1.0, flip=True, rows=((0, 0), (R - 1, R)), cols=((0, 1), (0, 0))),
        ar.record(s(0), s(1), 0.51, cols=((C // 2, C // 2 + 1), (0, 0))),                   # one column, no flip
    ]


def _launch(xd, yd, table, fill, shape, want_targets):
    from eav_amd import _lib
    N, B, R, C = shape
    td = kc.dev(torch.from_numpy(table))
    out = kc.sentinel_buf(B * R * C)
    tout = kc.sentinel_buf(B * NC) if want_targets else None
    _lib.call("eav_augment_gather", xd.data_ptr(), yd.data_ptr() if want_targets else None, td.data_ptr(), float(fill),
              out.data_ptr(), kc.ptr(tout), B, R, C, NC if want_targets else 0, torch.cuda.current_stream().cuda_stream)
    return (kc.take(out, B * R * C, (B, R, C), "out"),
            kc.take(tout, B * NC, (B, NC), "tout") if want_targets else None)


def _check(got, tout, x, y, table, fill, what):
    ref, masked, mag = ar.gather(x, table, fill)
    got64 = got.double().numpy()
    assert not np.isnan(got64).any(), f"{what}: a NaN came through"
    assert (got64[masked] == fill).all(), f"{what}: masked cells differ from fill"
    lam = ar.lam_of(table)
    for b in range(table.shape[0]):
        live = ~masked[b]
        if lam[b] == 1.0:
            assert (got64[b][live] == ref[b][live]).all(), f"{what}: record {b} (lambda 1) is not the source's bits"
        else:
            err = np.abs(got64[b] - ref[b])[live]
            tol = 2.0 ** -22 * mag[b][live]
            assert (err <= tol).all(), f"{what}: record {b} off by {float((err - tol).max()):.3e} beyond the bound"
    if tout is not None:
        assert np.array_equal(tout.double().numpy(), ar.soft_targets(y, table, NC)), f"{what}: soft targets"


@pytest.mark.parametrize("shape", SHAPES)
def test_augment_gather(shape):
    from eav_amd.runtime import gather_batch
    N, B, R, C = shape
    x = kc.normal(kc.seed_of("aug", shape), (N, R, C)).numpy()
    x[N - 1, R // 2, C // 2] = np.nan
    y = (np.arange(N) * 2 % NC).astype(np.int64)
    y[1] = y[0]                                                           # a pair of equal labels: target exactly 1
    xd, yd = kc.dev(torch.from_numpy(x)), kc.dev(torch.from_numpy(y))
    pool = _pool(N, R, C)
    pool += pool[:(-len(pool)) % B]                                       # whole launches of B records
    for k in range(0, len(pool), B):
        table = np.asarray(pool[k:k + B], dtype=np.int32)
        got, tout = _launch(xd, yd, table, FILL, shape, True)
        _check(got, tout, x, y, table, FILL, f"shape {shape} records {k}..{k + B - 1}")
        got2, _ = _launch(xd, yd, table, FILL, shape, False)              # no soft targets asked, no labels given
        assert torch.equal(got2.view(torch.int32), got.view(torch.int32))
    # plain records reproduce gather_batch bit for bit
    idx = [(3 * b + 1) % (N - 1) for b in range(B)]
    table = np.asarray([ar.record(i, N - 1, 1.0) for i in idx], dtype=np.int32)
    got, _ = _launch(xd, yd, table, 0.0, shape, False)
    want, _ = gather_batch(xd, yd, torch.as_tensor(idx, device="cuda"))
    assert torch.equal(got.view(torch.int32), want.cpu().view(torch.int32))


def test_arguments_are_refused_on_the_host():
    from eav_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    a = kc.dev(torch.zeros(64))
    t = kc.dev(torch.zeros(ar.RECORD_INTS, dtype=torch.int32))
    for args in ((None, None, t.data_ptr(), 0.0, a.data_ptr(), None, 1, 2, 2, 0),
                 (a.data_ptr(), None, t.data_ptr(), 0.0, a.data_ptr(), None, 0, 2, 2, 0),
                 (a.data_ptr(), None, t.data_ptr(), 0.0, a.data_ptr(), a.data_ptr(), 1, 2, 2, 5)):     # targets without labels
        with pytest.raises(_lib.EavError, match="eav_augment_gather"):
            _lib.call("eav_augment_gather", *args, st)


@pytest.mark.parametrize("view", [(6, 16), (2, 3, 8)])
def test_batch_augment_apply_replays_its_plan(view):
    """plan_epoch -> one device copy -> apply per micro-batch, on a DeviceLoader whose samples are [T, mel] or [3, H, W]."""
    from eav_amd.augment import RECORD_INTS, BatchAugment, EpochPlan, sample_matrix_shape
    from eav_amd.runtime import DeviceLoader
    assert RECORD_INTS == ar.RECORD_INTS
    N = 7
    x = kc.normal(kc.seed_of("apply", view), (N,) + view).numpy()
    y = (np.arange(N) % NC).astype(np.int64)
    dl = DeviceLoader(x, y, 3, False, "cuda")
    R, C = sample_matrix_shape(dl.x)
    assert (R, C) == (int(np.prod(view[:-1])), view[-1])
    aug = BatchAugment(mixup_alpha=0.4, time_mask=3, freq_mask=4, hflip=True, seed=5)
    batches = [[4, 0, 6], [2, 5, 1], [3]]
    for soft in (True, False):
        plan = EpochPlan(aug, dl, batches, 2, soft, NC)
        assert np.array_equal(plan.host_table, aug.plan_epoch(batches, 2, (R, C)))
        pos = 0
        for idx in batches:
            xb, tb = plan.next(len(idx))
            part = plan.host_table[pos:pos + len(idx)]
            pos += len(idx)
            assert tuple(xb.shape) == (len(idx),) + view
            _check(xb.cpu().reshape(len(idx), R, C), tb.cpu() if soft else None, x.reshape(N, R, C), y, part, 0.0,
                   f"apply {view} {idx}")
            if not soft:
                assert tb.dtype == torch.int64 and tb.cpu().tolist() == [int(y[i]) for i in idx]
