"""csrc/attn_probs.hip through the C ABI against the float64 restatement (tests/attn_probs_ref.py): eav_attn_probs on the
fp32 qkv and eav_attn_probs_sp on the row planes, each with the lse of the project's own forward kernel on the same operands,
at one token, either side of the 32- and 128-row tiles, ViT's 197 tokens (rows not 16-byte aligned) and AST's 1214; and
eav_rollout_step."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_probs_ref as R

pytestmark = pytest.mark.gpu

B, H, HD = R.B, R.H, R.HD
SCALE = HD ** -0.5
SENTINEL, GUARD = 12345.0, 1024


def _guarded(n):
    """A NaN-filled output of n floats followed by GUARD sentinel floats, in one allocation."""
    buf = torch.full((n + GUARD,), SENTINEL, device="cuda")
    buf[:n] = float("nan")
    return buf


def launch(precision, qkv_d, N, want_probs=True, want_mean=True):
    """(probs [B, H, N, N] | None, mean [B, N, N] | None, their guard regions): one launch of the entry point of `precision`
    on qkv (device, [B*N, 3 H 64]); lse from eav_attn_fwd / eav_attn_sp_prep + eav_attn_fwd_sp on the same operands."""
    from eav_amd import _lib
    from tests.kernel_check import SLOT
    P = _lib.ptr
    D = H * HD
    ao = torch.empty(B * N, D, device="cuda")
    lse = torch.empty(B * H, N, device="cuda")
    pb = _guarded(B * H * N * N) if want_probs else None
    mb = _guarded(B * N * N) if want_mean else None
    if precision == "fp32":
        _lib.call("eav_attn_fwd", P(qkv_d), P(ao), P(lse), B, H, N, HD, SCALE, None)
        _lib.call("eav_attn_probs", P(qkv_d), P(lse), P(pb), P(mb), B, H, N, HD, SCALE, None)
    else:
        slot = torch.zeros(SLOT, device="cuda")
        _lib.call("eav_sp_absmax", P(qkv_d), B * N, 3 * D, 3 * D, P(slot), None)
        rowp = torch.empty(B * N, 6 * D, dtype=torch.float16, device="cuda")
        _lib.call("eav_attn_sp_prep", P(qkv_d), P(slot), P(rowp), None, B, N, 3 * D, D, 0, None)
        _lib.call("eav_attn_fwd_sp", P(rowp), None, P(slot), P(ao), P(lse), None, B, H, N, HD, SCALE, None)
        _lib.call("eav_attn_probs_sp", P(rowp), P(slot), P(lse), P(pb), P(mb), B, H, N, HD, SCALE, None)
    torch.cuda.synchronize()
    return pb, mb


@functools.lru_cache(maxsize=2)
def reference(seed, N):
    """(qkv fp32, float64 probabilities, their head mean) - computed once per (seed, N), shared, never written."""
    qkv = R.inputs(seed, N)
    Pref = R.probs(qkv, B, H, N, SCALE)
    for a in (qkv, Pref):
        a.setflags(write=False)
    return qkv, Pref, R.head_mean(Pref)


def figures(precision, N, seed):
    """The measured errors of one case: what the constants of attn_probs_ref.BOUNDS are taken from."""
    qkv, Pref, Mref = reference(seed, N)
    pb, mb = launch(precision, torch.from_numpy(qkv.copy()).cuda(), N)
    got = pb[:B * H * N * N].cpu().double().numpy().reshape(B, H, N, N)
    gm = mb[:B * N * N].cpu().double().numpy().reshape(B, N, N)
    pa, pr = R.split_errors(got, Pref)
    ma, mr = R.split_errors(gm, Mref)
    return dict(precision=precision, N=N, seed=seed, probs_abs=pa, probs_rel=pr, mean_abs=ma, mean_rel=mr,
                rowsum=float(np.abs(got.sum(-1) - 1.0).max()), mean_rowsum=float(np.abs(gm.sum(-1) - 1.0).max()))


@pytest.mark.parametrize("N", R.SHAPES)
@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_probabilities_against_float64(precision, N):
    seed = R.SEEDS[0]
    qkv, Pref, Mref = reference(seed, N)
    qkv_d = torch.from_numpy(qkv.copy()).cuda()
    n, nm = B * H * N * N, B * N * N
    pb, mb = launch(precision, qkv_d, N)
    got = pb[:n].cpu().double().numpy().reshape(B, H, N, N)
    gm = mb[:nm].cpu().double().numpy().reshape(B, N, N)
    what = f"{precision} N={N}"
    print(what, "probs (abs, rel)", R.split_errors(got, Pref), "mean (abs, rel)", R.split_errors(gm, Mref),
          "rowsum", np.abs(got.sum(-1) - 1.0).max(), np.abs(gm.sum(-1) - 1.0).max())
    # every element written, finite, non-negative; nothing beyond the outputs touched
    assert np.isfinite(got).all() and (got >= 0).all(), what
    assert np.isfinite(gm).all() and (gm >= 0).all(), what
    assert bool((pb[n:] == SENTINEL).all()) and bool((mb[nm:] == SENTINEL).all()), what + ": sentinel overwritten"
    # the hostile rows are what they were built to be: a near one-hot row, and a row whose other probabilities underflow
    if N > 1:
        assert Pref[:, :, 0, N - 1].min() > 0.5 and Pref[:, :, N // 2].min() < 1e-40
    err, errm = np.abs(got - Pref), np.abs(gm - Mref)
    assert (err <= R.error_bounds(Pref, precision)).all(), (what, err.max())
    assert (errm <= R.error_bounds(Mref, precision)).all(), (what, errm.max())
    tol = R.BOUNDS[precision][2]
    assert np.abs(got.sum(-1) - 1.0).max() <= tol and np.abs(gm.sum(-1) - 1.0).max() <= tol, what
    # the same bits on every run; the mean alone equals the mean beside the probabilities
    pb2, mb2 = launch(precision, qkv_d, N)
    assert torch.equal(pb2[:n], pb[:n]) and torch.equal(mb2[:nm], mb[:nm]), what + ": not deterministic"
    _, mb3 = launch(precision, qkv_d, N, want_probs=False)
    assert torch.equal(mb3[:nm], mb[:nm]) and bool((mb3[nm:] == SENTINEL).all()), what + ": mean alone differs"
    pb4, _ = launch(precision, qkv_d, N, want_mean=False)
    assert torch.equal(pb4[:n], pb[:n]), what + ": probs alone differ"


def test_arguments_are_checked():
    from eav_amd import _lib
    t = torch.zeros(4096, device="cuda")
    p = t.data_ptr()
    with pytest.raises(_lib.EavError, match="head_dim 16 unsupported"):
        _lib.call("eav_attn_probs", p, p, p, p, 1, 1, 4, 16, 0.25, None)
    with pytest.raises(_lib.EavError, match="neither probs nor probs_mean"):
        _lib.call("eav_attn_probs", p, p, None, None, 1, 1, 4, 64, 0.125, None)
    with pytest.raises(_lib.EavError, match="head_dim 32 unsupported"):
        _lib.call("eav_attn_probs_sp", p, p, p, p, p, 1, 1, 4, 32, 0.125, None)
    with pytest.raises(_lib.EavError, match="neither probs nor probs_mean"):
        _lib.call("eav_attn_probs_sp", p, p, p, None, None, 1, 1, 4, 64, 0.125, None)
    with pytest.raises(_lib.EavError, match="bad arguments"):
        _lib.call("eav_rollout_step", p, p, p, 1, 1, 4, None)          # r_out aliases r_in


@pytest.mark.parametrize("N", R.SHAPES)
@pytest.mark.parametrize("Rr", [1, 2])
def test_rollout_step_against_float64(Rr, N):
    from eav_amd import _lib, synth
    r = np.abs(synth.normal(700 + N + Rr, (B, Rr, N)))
    a = R.softmax(synth.normal(800 + N, (B, N, N)).astype(np.float64) * 3.0).astype(np.float32)
    r_d, a_d = torch.from_numpy(r).cuda(), torch.from_numpy(a).cuda()
    outs = [_guarded(B * Rr * N) for _ in range(2)]
    for o in outs:
        _lib.call("eav_rollout_step", r_d.data_ptr(), a_d.data_ptr(), o.data_ptr(), B, Rr, N, None)
    torch.cuda.synchronize()
    n = B * Rr * N
    got = outs[0][:n].cpu().double().numpy().reshape(B, Rr, N)
    err = np.abs(got - R.rollout_step(r, a))
    assert np.isfinite(got).all() and (err <= R.rollout_step_bound(r, a)).all(), (Rr, N, err.max())
    assert bool((outs[0][n:] == SENTINEL).all()) and torch.equal(outs[0], outs[1])
