"""The glue kernels every trainer's step goes through, at their edges: eav_gather_rows / eav_gather_i64 (batch
assembly), eav_scale_by_scalar (the upstream gradient of a criterion), eav_norm_max_multi (the one-launch table of row /
column norms behind the a-priori operand scales, and WeightPlanes' use of it) and eav_video_counters_inc.

Copies and products are bit-compared in NaN-sentinel buffers with a guard band (tests/kernel_check.py).  A norm is held
to the float64 norm within

    (n / 2 + 2) * 2^-24 * ref,        n = elements summed

- a float32 sum of n squares in any order carries a relative error of at most n 2^-24 (to first order), the square root
halves it and adds its own rounding, one more to spare - and is bit-equal to the single-matrix entry point on the same
matrix.  The scales that consume these norms overshoot the true maxima by about sqrt(D) / 4, so an under-estimate - a
dropped row, column or block - is invisible to the model tests; here the largest row / column sits last.
Measured on the MI355X: worst error / bound 0.161 over the 55 jobs of the table."""
import numpy as np
import pytest
import torch

from tests import kernel_check as kc
from eav_amd import _lib, synth

pytestmark = pytest.mark.gpu
P = kc.ptr


def bits32(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("row_elems", [1, 3, 4, 1023, 1024, 65540])
def test_gather_rows_is_a_copy_on_both_paths(row_elems):
    """65 540 floats are more than 64 blocks x 256 float4: the grid-stride loop takes a second trip.  Views offset by one
    float are not 16-byte aligned and take the scalar path."""
    nsrc = 7
    flat = kc.normal(kc.seed_of("gather", row_elems), (nsrc * row_elems + 1,))
    flat[5] = float("nan")
    flat_dev = kc.dev(flat)
    for nrows, idx in ((1, [nsrc - 1]), (1, [0]), (5, [3, 0, nsrc - 1, 3, 3])):
        idx_dev = kc.dev(torch.tensor(idx, dtype=torch.int64))
        for src_off, dst_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
            src = flat[src_off:src_off + nsrc * row_elems].view(nsrc, row_elems)
            buf = kc.sentinel_buf(nrows * row_elems + dst_off, guard=kc.GUARD - dst_off)
            assert flat_dev.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
            _lib.call("eav_gather_rows", flat_dev.data_ptr() + 4 * src_off, P(idx_dev), buf.data_ptr() + 4 * dst_off, nrows,
                      row_elems, _lib.stream_ptr())
            torch.cuda.synchronize()
            got = buf.cpu()
            assert (bits32(got[:dst_off]) == kc.SENT).all() and (bits32(got[dst_off + nrows * row_elems:]) == kc.SENT).all(), \
                "written outside the output"
            assert torch.equal(bits32(got[dst_off:dst_off + nrows * row_elems]), bits32(src[idx]).view(-1)), \
                (row_elems, idx, src_off, dst_off)


@pytest.mark.parametrize("n", [1, 256, 257])
def test_gather_i64(n):
    src = torch.from_numpy(synth.splitmix64(kc.seed_of("labels", n), 300).astype(np.int64))
    idx = torch.from_numpy((synth.splitmix64(kc.seed_of("idx", n), n) % np.uint64(300)).astype(np.int64))
    idx[0], idx[-1] = 299, 0
    guard = -0x0123456789ABCDEF
    out = kc.dev(torch.full((n + 64,), guard, dtype=torch.int64))
    _lib.call("eav_gather_i64", P(kc.dev(src)), P(kc.dev(idx)), P(out), n, _lib.stream_ptr())
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:n], src[idx]) and (got[n:] == guard).all()


# ------------------------------------------------------------------------------------------------ scale by a device scalar
SPECIAL = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFC00001, 0x7F800000, 0x00800000], np.uint32)  # -0.0,
# subnormals, NaN payloads, inf, the smallest normal


@pytest.mark.parametrize("n", [1, 255, 1024 * 256 + 3])
def test_scale_by_scalar(n):
    """1024 x 256 + 3 elements: the grid is capped at 1024 blocks, the loop takes a second trip.  With the scalar 1.0 the
    buffer keeps its bits (-0.0, subnormals, NaN payloads); otherwise every element is the float32 product."""
    data = synth.normal(kc.seed_of("scale", n), (n,)).astype(np.float32)
    k = min(n, len(SPECIAL))
    data[n - k:] = SPECIAL[:k].view(np.float32)
    for scalar in (1.0, 0.0, -2.5, 3e-41):
        sc = np.float32(scalar)
        assert float(sc) == scalar or (scalar == 3e-41 and 0 < sc < np.finfo(np.float32).tiny)
        buf = kc.sentinel_buf(n)
        buf[:n] = torch.from_numpy(data)
        _lib.call("eav_scale_by_scalar", buf.data_ptr(), P(kc.dev(np.array([sc]))), n, _lib.stream_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[n:].view(np.uint32) == kc.SENT).all(), f"scalar {scalar}: guard band written"
        if scalar == 1.0:
            assert np.array_equal(got[:n].view(np.uint32), data.view(np.uint32))
            continue
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            want = data * sc
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[:n]), nan), f"scalar {scalar}: NaN elsewhere"
        assert np.array_equal(got[:n].view(np.uint32)[~nan], want.view(np.uint32)[~nan]), f"scalar {scalar}"


# ------------------------------------------------------------------------------------------------ norm tables
ROW_JOBS = [(R, C, ld) for R in (1, 3, 5, 513, 3072) for C, ld in ((40, 40), (1027, 1031), (1300, 1300))]
COL_JOBS = [(R, C, C + 4) for R in (1, 15, 16, 17, 63, 64, 65, 113) for C in (4, 60, 64, 68, 200)]


def norm_bound(n, ref):
    return (n / 2 + 2) * 2.0 ** -24 * ref


def build_table():
    """One flat buffer holding every matrix at a 16-byte aligned offset: the last row carries 9 x the norm of the others
    (row jobs: it is the maximum; column jobs: the tail loop's row weighs most), in a column job every entry of the last
    column is 3 x the largest of its row (it is the maximum, in the last block).  -> (flat, [(offset, R, C, ld, cols, float64 norm, n)])"""
    jobs, chunks, off = [], [], 0
    for cols, (R, C, ld) in [(0, j) for j in ROW_JOBS] + [(1, j) for j in COL_JOBS]:
        w = synth.normal(kc.seed_of("norm", cols, R, C), (R, ld)).astype(np.float32)
        if cols:
            w[:, C - 1] = 3 * np.abs(w[:, :C]).max(1)
        w[R - 1] *= 9
        live = w[:, :C].astype(np.float64)
        norms = np.sqrt((live * live).sum(0 if cols else 1))
        assert norms.argmax() == (C - 1 if cols else R - 1)
        jobs.append((off, R, C, ld, cols, float(norms.max()), R if cols else C))
        chunks.append(w.reshape(-1))
        off += (R * ld + 3) // 4 * 4
        chunks.append(np.zeros(off - sum(len(c) for c in chunks), np.float32))
    return np.concatenate(chunks), jobs


@pytest.mark.parametrize("twice", [1, 2])
def test_norm_max_multi_against_float64_and_the_single_matrix_kernels(twice):
    flat, jobs = build_table()
    flat_dev = kc.dev(flat)
    base = flat_dev.data_ptr()
    assert base % 16 == 0
    out = kc.sentinel_buf(len(jobs))
    out[:len(jobs)] = 0
    table = torch.tensor([[base + 4 * off, ld, out.data_ptr() + 4 * k, R | (C << 32), cols]
                          for k, (off, R, C, ld, cols, _, _) in enumerate(jobs)], dtype=torch.int64)
    largest = max((C + 63) // 64 if cols else min((R + 3) // 4, 128) for _, R, C, _, cols, _, _ in jobs)
    assert largest == 128
    _lib.call("eav_norm_max_multi", P(kc.dev(table)), len(jobs), largest * twice, _lib.stream_ptr())
    got = kc.take(out, len(jobs), (len(jobs),), "norm table")
    single = torch.zeros(len(jobs), device="cuda")
    for k, (off, R, C, ld, cols, _, _) in enumerate(jobs):
        _lib.call("eav_colnorm_max" if cols else "eav_rownorm_max", base + 4 * off, R, C, ld, single.data_ptr() + 4 * k,
                  _lib.stream_ptr())
    single = single.cpu()
    worst = 0.0
    for k, (off, R, C, ld, cols, ref, n) in enumerate(jobs):
        what = f"{'column' if cols else 'row'} job R {R}, C {C}, ld {ld}"
        assert bits32(got[k:k + 1]).item() == bits32(single[k:k + 1]).item(), f"{what}: table {float(got[k])} != single {float(single[k])}"
        ratio = abs(float(got[k]) - ref) / norm_bound(n, ref)
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what}: {float(got[k])} against {ref}, error / bound {ratio:.3f}"
    print(f"norm table x{twice}: worst error / bound {worst:.3f}")


def test_weight_planes_refresh_launches_enough_blocks_for_a_wide_fc2():
    """fc2 [D, FF] with FF / 64 = 131 column blocks, more than the 128 a row job is capped at: max_blocks must come from
    the column job, or the last columns - where the largest one sits - are never read."""
    from eav_amd.weight_planes import WeightPlanes
    D, FF = 32, 8384
    shapes = [("qkv0", 3 * D, D), ("fc10", FF, D), ("fc20", D, FF)]
    ws = {}
    for k, out, inn in shapes:
        w = synth.normal(kc.seed_of("planes", k), (out, inn)).astype(np.float32) * 0.05
        if k == "fc20":
            w[:, inn - 1] = 3 * np.abs(w).max(1)
        w[out - 1] *= 9
        ws[k] = w
    flat = kc.dev(np.concatenate([ws[k].reshape(-1) for k, _, _ in shapes]))
    mats, off = [], 0
    for k, out, inn in shapes:
        mats.append((k, 4 * off, out, inn))
        off += out * inn
    wp = WeightPlanes(mats, 1, flat.device, True)
    wp.main = torch.cuda.current_stream()
    wp.refresh([k for k, _, _ in shapes], flat.data_ptr(), (0,), None)
    torch.cuda.synchronize()
    assert wp._tables[4] == (FF + 63) // 64 == 131
    for k, arr, axis in (("fc10", wp.wnorm_fc1, 1), ("qkv0", wp.wnorm_qkv, 1), ("fc20", wp.wcolnorm_fc2, 0)):
        w = ws[k].astype(np.float64)
        norms = np.sqrt((w * w).sum(axis))
        assert norms.argmax() == len(norms) - 1
        ref, got = float(norms.max()), float(arr[0])
        assert abs(got - ref) <= norm_bound(w.shape[axis], ref), (k, got, ref)


# ------------------------------------------------------------------------------------------------ counters
@pytest.mark.parametrize("n", [1, 256, 257, 4096])
def test_video_counters_inc(n):
    guard = -0x0123456789ABCDEF
    start = torch.from_numpy(synth.splitmix64(kc.seed_of("counters", n), n).astype(np.int64) >> 8)
    buf = kc.dev(torch.cat([start, torch.full((64,), guard, dtype=torch.int64)]))
    _lib.call("eav_video_counters_inc", P(buf), n, _lib.stream_ptr())
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got[:n], start + 1) and (got[n:] == guard).all()


def test_video_counters_inc_refuses_more_than_4096():
    buf = kc.dev(torch.zeros(4097 + 64, dtype=torch.int64))
    with pytest.raises(_lib.EavError, match="eav_video_counters_inc"):
        _lib.call("eav_video_counters_inc", P(buf), 4097, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (buf.cpu() == 0).all()
