"""Checking helpers shared by the kernel-level GPU tests (test_audio_cnn_kernels_gpu.py, test_eegnet_canon_kernels_gpu.py,
test_shallow_tf_kernels_gpu.py, test_encoder_dropout_kernels_gpu.py, test_eegnet_direct_kernels_gpu.py, test_fir_fft_kernels_gpu.py,
test_preprocess_kernels_gpu.py, test_preprocess_ref_cpu.py, test_batch_glue_kernels_gpu.py, test_conv64_fft_kernels_gpu.py): sentinel-filled output buffers with a guard band,
deterministic data, and the two comparisons - bit equality and an element-wise bound; and the operand preparation of the
split attention kernels (attn_prep, decode_planes: shared with test_split_kernels_gpu.py).

Every output is filled with a NaN sentinel (payload 0x7fc0dead; 0xFF for uint8) and carries a guard band past its end:
everything the contract says is written must be overwritten, the guard band must be untouched."""
import zlib

import numpy as np
import torch

from eav_amd import synth

SENT = 0x7FC0DEAD           # fp32 sentinel: a NaN no arithmetic on the data produces
GUARD = 4096                # default guard band (elements) past every output

_KEEP = []


def dev(a):
    """Host array -> device tensor that stays alive until the test module is torn down
    (a temporary's memory would be recycled by the caching allocator before the kernel ran)."""
    t = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).contiguous().cuda()
    _KEEP.append(t)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return t


def ptr(t):
    return None if t is None else t.data_ptr()


def sentinel_buf(n, dtype=torch.float32, guard=GUARD):
    """n elements plus the guard band, all sentinel."""
    if dtype == torch.uint8:
        return dev(torch.full((n + guard,), 0xFF, dtype=torch.uint8))
    return dev(torch.full((n + guard,), SENT, dtype=torch.int32)).view(torch.float32)


def take(buf, n, shape, what):
    """The first n elements of a sentinel buffer after the launch: all written, guard band intact."""
    torch.cuda.synchronize()
    h = buf.cpu()
    bits = h if h.dtype == torch.uint8 else h.view(torch.int32)
    s = 0xFF if h.dtype == torch.uint8 else SENT
    unwritten = int((bits[:n] == s).sum())
    assert unwritten == 0, f"{what}: {unwritten} of {n} elements never written"
    assert (bits[n:] == s).all(), f"{what}: guard band written at {int((bits[n:] != s).nonzero()[0])} past the end"
    return h[:n].view(shape)


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def ints(seed, shape, lo, hi):
    """float32 integers uniform in [lo, hi]."""
    n = int(np.prod(shape))
    return torch.from_numpy((lo + (synth.splitmix64(seed, n) % np.uint64(hi - lo + 1)).astype(np.int64))
                            .astype(np.float32).reshape(shape))


def normal(seed, shape, std=1.0):
    return torch.from_numpy(synth.normal(seed, shape, 0.0, std))


def keep_mask(seed, shape, p):
    return torch.from_numpy((synth.uniform(seed, shape) >= p).astype(np.uint8))


SLOT = 4128                 # floats of one scale slot of the split-operand kernels


def attn_prep(x, B, N, ncols, secw, tmask):
    """fp32 [B*N, ncols] on the device -> (scale slot, row planes, T planes) of the split attention kernels (eav_attn_sp_prep)."""
    from eav_amd import _lib
    Npad = _lib.plain("eav_attn_sp_npad", N)
    slot = torch.zeros(SLOT, device="cuda")
    _lib.call("eav_sp_absmax", ptr(x), B * N, ncols, ncols, ptr(slot), None)
    rowp = torch.empty(B * N, 2 * ncols, dtype=torch.float16, device="cuda")
    tp = torch.empty(B, ncols // 64, 64, 2 * Npad, dtype=torch.float16, device="cuda")
    _lib.call("eav_attn_sp_prep", ptr(x), ptr(slot), ptr(rowp), ptr(tp), B, N, ncols, secw, tmask, None)
    return slot, rowp, tp


def decode_planes(pl, R, C, sigma):
    """planes [Rp, 2*Cp] f16 ([R][Cp/8][2][8]) -> fp64 [R, C]: (hi + lo 2^-11) / sigma"""
    v = pl[:R].view(R, -1, 2, 8).double()
    return ((v[:, :, 0, :] + v[:, :, 1, :] / 2048.0).reshape(R, -1)[:, :C]) / sigma


def slot_max(slot):
    """The maximum a kernel published in a scale slot's shard words (non-negative floats: compared as integers)."""
    return float(slot[:2048:32].view(torch.int32).max().view(torch.float32))


def assert_exact(bound, quantum, what):
    """Every partial sum is a multiple of quantum of magnitude <= bound: exact in fp32 if bound / quantum < 2^24."""
    assert bound / quantum < 2.0 ** 24, f"{what}: partial sums up to {bound} in steps of {quantum} are not exact in fp32"


def same(got, ref, what):
    """Bit-for-bit as values (NaN equal to NaN)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN at {int((gn != rn).sum())} other places"
    bad = (got != ref) & ~gn
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} differ, max "
                           f"{(got - ref)[bad].abs().max():.3e}, first at {tuple(bad.nonzero()[0].tolist())}")


def within(got, ref, tol, what):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not torch.isnan(got).any(), f"{what}: NaN"
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} beyond the bound, worst {(err - tol).max():.3e}, "
                           f"first at {tuple(bad.nonzero()[0].tolist())}")
