"""Per-kernel parity of the AST / ViT encoder's dropout kernels through the C ABI against the float64 references of
tests/encoder_dropout_kernel_ref.py: the generator (eav_tf_dropout_mask against the numpy restatement of eav_hash32),
eav_tf_dropout_add, eav_softmax_dropout_fwd / _bwd, and the DROP instantiations of the fused attention kernels in both
precisions (eav_attn_fwd_dropout / eav_attn_bwd_dropout, eav_attn_fwd_sp_dropout / eav_attn_bwd_sp_dropout).

Every output goes into a NaN-sentinel buffer with a guard band (tests/kernel_check.py): all the contract says is written
must be written, pad columns and the band must be untouched.  Explicit masks come from hash_keep with planted rows and
columns; generator-mode runs (site-style seed, device counter) must equal, bit for bit, the explicit-mask run on the mask
eav_tf_dropout_mask dumps for that seed and counter - which pins the element index every kernel hashes.

Each group notes its worst error / bound ratio and the module prints them at teardown (pytest -s)."""
import numpy as np
import pytest
import torch

from eav_amd import _lib
from tests import encoder_dropout_kernel_ref as R
from tests.kernel_check import GUARD, SENT, SLOT, attn_prep, dev, normal, ptr, same, seed_of, sentinel_buf, slot_max, take, within
from tests.test_transformer_kernels_gpu import close
from tests.test_video_cnn_kernels_gpu import gamma

pytestmark = pytest.mark.gpu
call = _lib.call
SCALE = 0.125               # head_dim^-0.5
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def L():
    _lib.load()
    yield _lib
    for group, r in sorted(WORST.items()):
        print(f"\n[{group}] worst error / bound: {r:.3f}")


def note(group, got, ref, tol, what):
    """Record and print max error / bound of one comparison (the assertion itself is the caller's)."""
    err = (got.double() - ref.double()).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    r = float(torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0
    WORST[group] = max(WORST.get(group, 0.0), r)
    print(f"{what}: max err {float(err.max()):.3e}, error / bound {r:.3f}")
    return r


def closer(group, got, ref, rtol, atol, what):
    note(group, got, ref, atol + rtol * ref.double().abs(), what)
    close(got, ref, rtol, atol, what)


def counter(c):
    return dev(torch.tensor([c], dtype=torch.int64))


def site_seed(k):
    return (k + 1) << 40    # encoder_dropout.site_seed with dropout_seed 0


def dump_mask(n, p, seed, cnt, what="dumped mask"):
    """eav_tf_dropout_mask into a sentinel buffer: (device buffer, host uint8 [n])."""
    buf = sentinel_buf(n, torch.uint8)
    call("eav_tf_dropout_mask", ptr(buf), n, p, seed, ptr(cnt), None)
    return buf, take(buf, n, (n,), what)


def zeros_like_exact(x, what):
    same(x, torch.zeros_like(x), what)


# ============================================================================================ a. the generator
@pytest.mark.parametrize("p", R.GEN_P)
@pytest.mark.parametrize("n", R.MASK_N)
def test_generator_equals_hash_keep(n, p):
    """eav_tf_dropout_mask == hash_keep bit for bit, without and with a device counter (5); the largest n enters the
    grid-stride loop of dropout_mask_kernel."""
    seed = site_seed(seed_of("gen", n) % 13) + seed_of("gen", n, p)
    _, got = dump_mask(n, p, seed, None)
    assert np.array_equal(got.numpy(), R.hash_keep(seed, n, p)), "seed_dev NULL"
    _, got = dump_mask(n, p, seed, counter(5))
    assert np.array_equal(got.numpy(), R.hash_keep(seed, n, p, counter=5)), "counter 5"


@pytest.mark.parametrize("n", R.MASK_N)
def test_generator_p0_keeps_everything(n):
    _, got = dump_mask(n, 0.0, 77, counter(5))
    assert bool((got == 1).all())


# ============================================================================================ b. eav_tf_dropout_add
def _drop_add(y, resid, n, p, seed, mask, cnt, inplace):
    if inplace:
        out = sentinel_buf(n)
        out[:n].copy_(y)
        src = out
    else:
        out, src = sentinel_buf(n), y
    call("eav_tf_dropout_add", ptr(src), ptr(resid), ptr(out), n, p, seed, ptr(mask), ptr(cnt), None)
    return take(out, n, (n,), "dropout_add out")


@pytest.mark.parametrize("p", [0.1, 0.9])
@pytest.mark.parametrize("n", R.ADD_N)
def test_dropout_add(n, p):
    """out = resid + Dropout(y) with resid, with resid NULL (the backward's gate) and in place, under an explicit mask and in
    generator mode.  Dropped: out is resid (or 0) bit for bit.  Kept: |out - (y s + resid)| <= 2^-23 (|y| s + |resid|) against
    float64 with s = scale32(p) - two fp32 roundings, or one where the compiler contracts to an fma; resid NULL: exactly
    fp32(y s).  Generator mode equals the explicit-mask run on the dumped mask bit for bit."""
    seed = seed_of("add", n, p)
    yh, rh = normal(seed, (n,)), normal(seed + 1, (n,), 2.0)
    mh = torch.from_numpy(R.hash_keep(seed, n, p))
    y, r, m = dev(yh), dev(rh), dev(mh)
    s = R.scale32(p)
    kept = mh.bool()
    gseed, cnt = site_seed(2) + 11, counter(4)
    gm_dev, gm = dump_mask(n, p, gseed, cnt)
    assert np.array_equal(gm.numpy(), R.hash_keep(gseed, n, p, counter=4))
    for variant, resid, rhost, inplace in (("resid", r, rh, False), ("gate", None, None, False), ("in place", r, rh, True)):
        out = _drop_add(y, resid, n, p, 0, m, None, inplace)
        base = rhost if rhost is not None else torch.zeros(n)
        same(out[~kept], base[~kept], f"{variant}: dropped elements")
        if rhost is None:
            same(out[kept], (yh * torch.tensor(s, dtype=torch.float32))[kept], f"{variant}: kept elements")
        else:
            ref = yh.double() * s + rhost.double()
            tol = 2.0 ** -23 * (yh.double().abs() * s + rhost.double().abs())
            note("b dropout_add", out[kept], ref[kept], tol[kept], f"dropout_add n={n} p={p} {variant}")
            within(out[kept], ref[kept], tol[kept], f"{variant}: kept elements")
        got_g = _drop_add(y, resid, n, p, gseed, None, cnt, inplace)
        got_e = _drop_add(y, resid, n, p, 0, gm_dev, None, inplace)
        same(got_g, got_e, f"{variant}: generator mode vs its dumped mask")


# ============================================================================================ c. softmax + dropout
def padded_buf(rows, N, ld, data=None):
    """[rows, ld] + guard band, all sentinel, with data [rows, N] in the columns [0, N)."""
    h = torch.full((rows * ld + GUARD,), SENT, dtype=torch.int32)
    if data is not None:
        h[:rows * ld].view(rows, ld)[:, :N] = data.contiguous().view(torch.int32)
    return dev(h).view(torch.float32)


def take_padded(buf, rows, N, ld, what):
    """Columns [0, N) all written; columns [N, ld) and the guard band keep the sentinel."""
    if ld == N:
        return take(buf, rows * N, (rows, N), what)
    torch.cuda.synchronize()
    h = buf.cpu()
    bits = h.view(torch.int32)
    body = bits[:rows * ld].view(rows, ld)
    unwritten = int((body[:, :N] == SENT).sum())
    assert unwritten == 0, f"{what}: {unwritten} of {rows * N} elements never written"
    assert bool((body[:, N:] == SENT).all()), f"{what}: pad columns written"
    assert bool((bits[rows * ld:] == SENT).all()), f"{what}: guard band written"
    return h[:rows * ld].view(rows, ld)[:, :N].clone()


def _softmax_pair(sh, dph, rows, N, ld, p, seed, mask, cnt, with_pd=True):
    """Forward then backward on fresh sentinel buffers: host (P, Pd, dS, pd regenerated by the backward or None)."""
    s, pd = padded_buf(rows, N, ld, sh), padded_buf(rows, N, ld)
    call("eav_softmax_dropout_fwd", ptr(s), ptr(pd), rows, N, ld, p, seed, ptr(mask), ptr(cnt), None)
    P, Pd = take_padded(s, rows, N, ld, "P"), take_padded(pd, rows, N, ld, "Pd")
    dP, pd2 = padded_buf(rows, N, ld, dph), (padded_buf(rows, N, ld) if with_pd else None)
    call("eav_softmax_dropout_bwd", ptr(s), ptr(dP), ptr(pd2), rows, N, ld, p, seed, ptr(mask), ptr(cnt), None)
    dS = take_padded(dP, rows, N, ld, "dS")
    same(take_padded(s, rows, N, ld, "P after the backward"), P, "the backward's P is read-only")
    return P, Pd, dS, (take_padded(pd2, rows, N, ld, "pd") if with_pd else None)


@pytest.mark.parametrize("p", R.SOFTMAX_P)
@pytest.mark.parametrize("N", R.SOFTMAX_N)
@pytest.mark.parametrize("rows", R.SOFTMAX_ROWS)
def test_softmax_dropout(rows, N, p):
    """eav_softmax_dropout_fwd / _bwd on [rows, N] with row pitch ld = N + 5 (ld = N at (8, 257)): an index formed with ld
    instead of N reads another mask element.  P to eav_softmax_fwd's bound close(1e-5, 1e-7); Pd exactly fp32(P s) / 0; the
    backward regenerates Pd bit for bit (pd NULL accepted), dS within gamma(N + 3) |P| (|M o dP s| + sum |P o M o dP s|) of
    float64 on the kernel's own P; pad columns of every buffer keep the sentinel.  Generator mode (device counter) equals
    the explicit-mask run on the dumped mask, both kernels."""
    ld = N if (rows, N) == (8, 257) else N + 5
    seed = seed_of("softmax", rows, N, p)
    sh, dph = normal(seed, (rows, N), 2.0), normal(seed + 1, (rows, N))
    mh = torch.from_numpy(R.hash_keep(seed, rows * N, p).reshape(rows, N))
    m = dev(mh)
    s32 = torch.tensor(R.scale32(p), dtype=torch.float32)
    P, Pd, dS, pdb = _softmax_pair(sh, dph, rows, N, ld, p, 0, m, None)
    Pref, _, dSref, mag = R.softmax_dropout_ref(sh, dph, mh, p, P=P)
    closer("c softmax_dropout", P, Pref, 1e-5, 1e-7, f"P rows={rows} N={N} p={p}")
    same(Pd, torch.where(mh.bool(), P * s32, torch.zeros_like(P)), "Pd")
    same(pdb, Pd, "pd regenerated by the backward")
    tol = gamma(N + 3) * mag
    note("c softmax_dropout", dS, dSref, tol, f"dS rows={rows} N={N} p={p}")
    within(dS, dSref, tol, "dS")
    _, _, dS2, _ = _softmax_pair(sh, dph, rows, N, ld, p, 0, m, None, with_pd=False)
    same(dS2, dS, "dS with pd NULL")
    gseed, cnt = site_seed(4) + 3, counter(6)
    gm_dev, gm = dump_mask(rows * N, p, gseed, cnt)
    assert np.array_equal(gm.numpy(), R.hash_keep(gseed, rows * N, p, counter=6))
    gen = _softmax_pair(sh, dph, rows, N, ld, p, gseed, None, cnt)
    exp = _softmax_pair(sh, dph, rows, N, ld, p, 0, gm_dev, None)
    for a, b, what in zip(gen, exp, ("P", "Pd", "dS", "pd")):
        same(a, b, f"generator mode vs its dumped mask: {what}")


# ============================================================================================ d. fused fp32 attention
def fused_fwd(Q, B, H, N, p, seed, mask, cnt):
    D = H * 64
    ao, lse = sentinel_buf(B * N * D), sentinel_buf(B * H * N)
    call("eav_attn_fwd_dropout", ptr(Q), ptr(ao), ptr(lse), B, H, N, 64, SCALE, p, seed, ptr(mask), ptr(cnt), None)
    return ao, lse, take(ao, B * N * D, (B * N, D), "ao"), take(lse, B * H * N, (B * H, N), "lse")


def fused_bwd(Q, ao, dO, lse, B, H, N, p, seed, mask, cnt):
    D = H * 64
    delta, dqkv = sentinel_buf(B * H * N), sentinel_buf(B * N * 3 * D)
    call("eav_attn_bwd_dropout", ptr(Q), ptr(ao), ptr(dO), ptr(lse), ptr(delta), ptr(dqkv), B, H, N, 64, SCALE, p, seed,
         ptr(mask), ptr(cnt), None)
    return take(dqkv, B * N * 3 * D, (B * N, 3 * D), "dqkv"), take(delta, B * H * N, (B * H, N), "delta")


def planted_zeros(ao, dqkv, B, H, N, what):
    """The fully dropped query rows (image-head 0 row 0, last image-head last row) and the fully dropped key column 2 of
    image-head 0 (tests/encoder_dropout_kernel_ref.planted_mask): O, dQ and dV there are exact zeros."""
    if N == 1:
        return
    D, last = H * 64, B * N - 1
    if ao is not None:
        zeros_like_exact(ao[0, :64], f"{what}: O of the dropped row")
        zeros_like_exact(ao[last, D - 64:], f"{what}: O of the dropped last row")
    if dqkv is not None:
        zeros_like_exact(dqkv[0, :64], f"{what}: dQ of the dropped row")
        zeros_like_exact(dqkv[last, D - 64:D], f"{what}: dQ of the dropped last row")
        zeros_like_exact(dqkv[2, 2 * D:2 * D + 64], f"{what}: dV of the dropped key column")


def delta_check(group, delta, ao, doh, B, H, N, what):
    """delta [B*H, N] = rowsum(dO o O) per head with the kernel's own dropped O, to 2^-22 sum |dO O|."""
    prod = (doh.double() * ao.double()).view(B, N, H, 64)
    ref, mag = prod.sum(-1).permute(0, 2, 1).reshape(B * H, N), prod.abs().sum(-1).permute(0, 2, 1).reshape(B * H, N)
    note(group, delta, ref, 2.0 ** -22 * mag, what)
    within(delta, ref, 2.0 ** -22 * mag, what)


@pytest.mark.parametrize("p", R.ATTN_P)
@pytest.mark.parametrize("B,H,N", R.ATTN_CASES)
def test_fused_attention_dropout_forward(B, H, N, p):
    """eav_attn_fwd_dropout on the data of test_fused_attention_forward under a planted hash_keep mask: ao to
    close(1e-4, 2e-6 s) (that test's bound with the absolute term carried through s = 1 / (1 - p)), lse - the undropped
    statistics - to close(1e-5, 1e-5), fully dropped rows exactly 0; generator mode (site seed, device counter 3) bit-equal to
    the explicit run on the dumped mask."""
    D = H * 64
    qh = normal(101, (B * N, 3 * D), 1.5)
    mh = R.planted_mask(seed_of("fused", B, H, N, p), B, H, N, p)
    ro, _, rl = R.attention_ref(qh, torch.zeros(B * N, D), mh, B, H, N, p)
    Q = dev(qh)
    _, _, ao, lse = fused_fwd(Q, B, H, N, p, 0, dev(mh), None)
    closer("d fused fp32", ao, ro, 1e-4, 2e-6 * R.scale32(p), f"ao {B, H, N} p={p}")
    closer("d fused fp32", lse, rl, 1e-5, 1e-5, f"lse {B, H, N} p={p}")
    planted_zeros(ao, None, B, H, N, "explicit")
    gseed, cnt = site_seed(4), counter(3)
    gm_dev, gm = dump_mask(B * H * N * N, p, gseed, cnt)
    assert np.array_equal(gm.numpy(), R.hash_keep(gseed, B * H * N * N, p, counter=3))
    _, _, ao_g, lse_g = fused_fwd(Q, B, H, N, p, gseed, None, cnt)
    _, _, ao_e, lse_e = fused_fwd(Q, B, H, N, p, 0, gm_dev, None)
    same(ao_g, ao_e, "generator mode vs its dumped mask: ao")
    same(lse_g, lse_e, "generator mode vs its dumped mask: lse")
    same(lse_g, lse, "lse does not depend on the mask")


@pytest.mark.parametrize("p", R.ATTN_P)
@pytest.mark.parametrize("B,H,N", R.ATTN_CASES)
def test_fused_attention_dropout_backward(B, H, N, p):
    """eav_attn_bwd_dropout on the data of test_fused_attention_backward: dqkv to close(2e-4, 2e-5 max|ref|) (an all-zero
    reference - N = 1 with its one element dropped - leaves no tolerance: compared absolutely), delta = rowsum(dO o O) with the
    dropped O to 2^-22 sum |dO O|, dQ of fully dropped rows and dV of the fully dropped key exactly 0; generator mode
    bit-equal to the explicit run on the dumped mask, both fed the same ao and lse."""
    D = H * 64
    qh, doh = normal(111, (B * N, 3 * D), 1.2), normal(112, (B * N, D))
    mh = R.planted_mask(seed_of("fused", B, H, N, p), B, H, N, p)
    ro, rg, rl = R.attention_ref(qh, doh, mh, B, H, N, p)
    Q, dO, m = dev(qh), dev(doh), dev(mh)
    ao_b, lse_b, ao, lse = fused_fwd(Q, B, H, N, p, 0, m, None)
    closer("d fused fp32", ao, ro, 1e-4, 2e-6 * R.scale32(p), f"ao {B, H, N} p={p}")
    closer("d fused fp32", lse, rl, 1e-5, 1e-5, f"lse {B, H, N} p={p}")
    dqkv, delta = fused_bwd(Q, ao_b, dO, lse_b, B, H, N, p, 0, m, None)
    closer("d fused fp32", dqkv, rg, 2e-4, 2e-5 * float(rg.abs().max()), f"dqkv {B, H, N} p={p}")
    delta_check("d fused fp32", delta, ao, doh, B, H, N, f"delta {B, H, N} p={p}")
    planted_zeros(ao, dqkv, B, H, N, "explicit")
    gseed, cnt = site_seed(7), counter(3)
    gm_dev, _ = dump_mask(B * H * N * N, p, gseed, cnt)
    ao_e, lse_e, _, _ = fused_fwd(Q, B, H, N, p, 0, gm_dev, None)
    dq_g, de_g = fused_bwd(Q, ao_e, dO, lse_e, B, H, N, p, gseed, None, cnt)
    dq_e, de_e = fused_bwd(Q, ao_e, dO, lse_e, B, H, N, p, 0, gm_dev, None)
    same(dq_g, dq_e, "generator mode vs its dumped mask: dqkv")
    same(de_g, de_e, "generator mode vs its dumped mask: delta")


# ============================================================================================ e. split-precision attention
def sp_fwd(rowp, s_qkv, B, H, N, p, seed, mask, cnt):
    D = H * 64
    ao, lse, amax = sentinel_buf(B * N * D), sentinel_buf(B * H * N), torch.zeros(SLOT, device="cuda")
    call("eav_attn_fwd_sp_dropout", ptr(rowp), ptr(s_qkv), ptr(ao), ptr(lse), ptr(amax), B, H, N, 64, SCALE, p, seed,
         ptr(mask), ptr(cnt), None)
    aoh, lseh = take(ao, B * N * D, (B * N, D), "sp ao"), take(lse, B * H * N, (B * H, N), "sp lse")
    assert slot_max(amax) == float(aoh.abs().max()), "forward amax_slot"
    return ao, lse, aoh, lseh


def sp_bwd(rowp, dorow, s_qkv, s_do, ao, dO, lse, B, H, N, p, seed, mask, cnt):
    """attn_bwd_q_sp_kernel and attn_bwd_kv_sp_kernel both publish the maximum of what they store (dQ; dK and dV) in
    amax_slot under DROP: the slot decodes to exactly max|dqkv|."""
    D = H * 64
    s_ds, amax = torch.zeros(SLOT, device="cuda"), torch.zeros(SLOT, device="cuda")
    delta, dqkv = sentinel_buf(B * H * N), sentinel_buf(B * N * 3 * D)
    call("eav_attn_bwd_sp_dropout", ptr(rowp), ptr(dorow), ptr(s_qkv), ptr(s_do), ptr(s_ds), ptr(ao), ptr(dO), ptr(lse),
         ptr(delta), ptr(dqkv), ptr(amax), B, H, N, 64, SCALE, p, seed, ptr(mask), ptr(cnt), None)
    dqh, deh = take(dqkv, B * N * 3 * D, (B * N, 3 * D), "sp dqkv"), take(delta, B * H * N, (B * H, N), "sp delta")
    assert slot_max(amax) == float(dqh.abs().max()), "backward amax_slot"
    return dqh, deh


def rel(a, r, mag=None):
    """Largest error as a fraction of the reference's maximum (or of the magnitude given)."""
    return (a.double() - r).abs().max().item() / (r.abs().max().item() if mag is None else mag)


# Cases where the correct split kernel misses the 1.5 rel(fp32 kernel) rule: the bound is 4 x the error of the float32 CPU
# form of attention_ref against float64 at that case (the factor for the different summation order) - see
# test_split_attention_dropout_is_fp32_grade
FP32_REF_BOUND = {(4, 4, 70, 0.9): ("ao",)}


def _sp_case(B, H, N, p, dos, qs=1.0, spike=False, data=None, scale_of=None):
    """scale_of (optional): {section: magnitude} - errors of that section are measured against the magnitude given instead
    of the section's own maximum."""
    D = H * 64
    if data is None:
        qh, doh = normal(seed_of("sp", B, N), (B * N, 3 * D), qs), normal(seed_of("sp dO", B, N), (B * N, D)) * dos
        if spike:      # one key aligned with one query: the running maximum jumps inside a key tile (rescale branch)
            qh[5, D:D + 64] = qh[3, :64] * 6.0
        mh = R.planted_mask(seed_of("sp", B, H, N, p), B, H, N, p)
    else:
        qh, doh, mh = data
    ro, rg, rl = R.attention_ref(qh, doh, mh, B, H, N, p)
    Q, dO, m = dev(qh), dev(doh), dev(mh)
    # exact-fp32 dropout kernels: the anchor
    ao32_b, lse32_b, ao32, lse32 = fused_fwd(Q, B, H, N, p, 0, m, None)
    dq32, _ = fused_bwd(Q, ao32_b, dO, lse32_b, B, H, N, p, 0, m, None)
    # split
    s_qkv, rowp, _ = attn_prep(Q, B, N, 3 * D, D, 7)
    s_do, dorow, _ = attn_prep(dO, B, N, D, D, 1)
    ao_b, lse_b, ao, lse = sp_fwd(rowp, s_qkv, B, H, N, p, 0, m, None)
    dqkv, delta = sp_bwd(rowp, dorow, s_qkv, s_do, ao_b, dO, lse_b, B, H, N, p, 0, m, None)
    tag = f"{B, H, N} p={p} dO={dos}"
    grp = "e fused split"

    def rule(got, got32, ref, slack, what):
        mag = (scale_of or {}).get(what)
        a, b = rel(got, ref, mag), 1.5 * rel(got32, ref, mag) + slack
        if what in FP32_REF_BOUND.get((B, H, N, p), ()):
            ref32 = R.attention_ref(qh, doh, mh, B, H, N, p, dtype=torch.float32)[0 if what == "ao" else 1]
            b = max(b, 4.0 * rel(ref32, ref))
        WORST[grp] = max(WORST.get(grp, 0.0), a / b)
        print(f"{what} {tag}: rel {a:.3e} (fp32 kernel {rel(got32, ref, mag):.3e}), error / bound {a / b:.3f}")
        assert a <= b, (what, a, b)
    rule(ao, ao32, ro, 2e-7, "ao")
    # (+ 3 ulp of the largest lse: with a spike it reaches 64, one fp32 ulp there is 7.6e-6)
    a = (lse.double() - rl).abs().max().item()
    b = 1.5 * (lse32.double() - rl).abs().max().item() + 1e-6 + 3 * 2.0 ** -24 * rl.abs().max().item()
    WORST[grp] = max(WORST.get(grp, 0.0), a / b)
    assert a <= b, ("lse", a, b)
    for i, sec in enumerate("QKV"):
        sl = slice(i * D, (i + 1) * D)
        rule(dqkv[:, sl], dq32[:, sl], rg[:, sl], 3e-7, f"d{sec}")
    delta_check(grp, delta, ao, doh, B, H, N, f"delta {tag}")
    planted_zeros(ao, dqkv, B, H, N, "split, explicit")
    # generator mode against its dumped mask: the forward, then the backward on one (ao, lse)
    gseed, cnt = site_seed(10), counter(3)
    gm_dev, _ = dump_mask(B * H * N * N, p, gseed, cnt)
    _, _, ao_g, lse_g = sp_fwd(rowp, s_qkv, B, H, N, p, gseed, None, cnt)
    ao_eb, lse_eb, ao_e, lse_e = sp_fwd(rowp, s_qkv, B, H, N, p, 0, gm_dev, None)
    same(ao_g, ao_e, "generator mode vs its dumped mask: ao")
    same(lse_g, lse_e, "generator mode vs its dumped mask: lse")
    dq_g, de_g = sp_bwd(rowp, dorow, s_qkv, s_do, ao_eb, dO, lse_eb, B, H, N, p, gseed, None, cnt)
    dq_e, de_e = sp_bwd(rowp, dorow, s_qkv, s_do, ao_eb, dO, lse_eb, B, H, N, p, 0, gm_dev, None)
    same(dq_g, dq_e, "generator mode vs its dumped mask: dqkv")
    same(de_g, de_e, "generator mode vs its dumped mask: delta")


@pytest.mark.parametrize("dos", R.SP_DO)
@pytest.mark.parametrize("p", R.SP_P)
@pytest.mark.parametrize("B,H,N", R.SP_CASES)
def test_split_attention_dropout_is_fp32_grade(B, H, N, p, dos):
    """eav_attn_fwd_sp_dropout / eav_attn_bwd_sp_dropout beside the exact-fp32 dropout kernels of the same mask (held to
    float64 by the tests above), by the rule of test_attention_sp_is_fp32_grade: rel(split) <= 1.5 rel(fp32 kernel) + 2e-7
    for ao, + 3e-7 per section of dqkv, lse by that test's lse line.  p = 0.1 / 0.5 / 0.51 / 0.75 / 0.9 give the dS down-scale
    exponents e = 1, 1, 2, 2, 4 of make_sp_drop; dO at 1e-3 and at 1.  Both amax slots decode to the exact maxima, planted
    rows give exact zeros, generator mode equals the explicit run on the dumped mask.

    One case is held to 4 x the float32 CPU reference's own error instead (FP32_REF_BOUND): ao at (4, 4, 70), p = 0.9.  There
    the split kernel's rel is 8.665e-7 against 1.5 * 4.298e-7 + 2e-7 = 8.447e-7, on ONE element (the next ones: 6.7e-7,
    5.9e-7; query 45 of image 1, head 3: five kept keys, one of which carries 0.97 of sum |Pd| |V|).  The kernel is correct
    there: its rms error over the tensor is 2.51e-8 of the maximum against 2.54e-8 of the exact-fp32 kernel and 2.85e-8 of
    attention_ref evaluated in float32 on the CPU; the operand format alone (hi + lo pieces and the missing lo.lo term in
    float64 arithmetic) accounts for 5.7e-8 of the element's error, the rest is fp32 rounding of the score, the exponential and
    the row sum that every fp32 evaluation has - the float32 CPU reference's own maximum at this case is 7.70e-7, so the bound
    is 3.08e-6."""
    _sp_case(B, H, N, p, dos)


def test_split_attention_dropout_spike():
    B, H, N, qs = R.SP_SPIKE
    _sp_case(B, H, N, 0.1, 1e-3, qs=qs, spike=True)


def test_split_attention_dropout_at_the_top_of_the_operand_range():
    """The backward's dS at the top of the range make_sp_drop's down-scale 2^-22 2^-e is sized for.  p = 0.9 (1 / (1 - p) = 10,
    e = 4); query 7 sees keys 20 and 41 with probability 1/2 each (equal K rows, far above every other score), both kept,
    their V rows are +1.99 and -1.99 in every dimension and the query's dO row is 1.99 - the maxima of their tensors, so in
    operand units (sigma = 2^14 for both) |dP| = 64 (1.99 2^14)^2 = 2^35.99 and |dS| = P |10 dP - 0| = 5 |dP| = 2^38.3.  With
    the down-scale t = dS 2^-26 = 5069; with the 2^-22 of the kernel without dropout t = 81 100 is beyond fp16.  Same rule as
    test_split_attention_dropout_is_fp32_grade, except that errors of dQ are measured against max_q,d scale sum_k |dS| |K|
    (about 600) instead of max|dQ| (0.27): the two keys share one K row and dS_a = -dS_b, so the query's dQ row is the
    cancelled difference of two terms of that size in any arithmetic, the exact-fp32 kernel's included."""
    B, H, N, p = 1, 1, 64, 0.9
    seed = seed_of("sp top", N)
    qh, doh = normal(seed, (N, 192), 0.4).clamp(-1.9, 1.9), normal(seed + 1, (N, 64), 0.4).clamp(-1.9, 1.9)
    u = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    q0, ka, kb = 7, 20, 41
    qh[q0, :64] = 1.9 * u
    qh[ka, 64:128] = qh[kb, 64:128] = 1.9 * u
    qh[ka, 128:], qh[kb, 128:], doh[q0] = 1.99, -1.99, 1.99
    mh = R.planted_mask(seed, B, H, N, p)
    mh[0, 0, q0, ka] = mh[0, 0, q0, kb] = 1
    sigma = 2.0 ** 14
    assert float(qh.abs().max()) == float(doh.abs().max()) == float(np.float32(1.99))
    t = 0.5 * R.scale32(p) * 64 * (1.99 * sigma) ** 2 * 2.0 ** -22
    assert t > 65520 and t / 2 ** R.sp_exponent(p) < 2.0 ** 15
    x = qh.double()
    P = torch.softmax(x[:, :64] @ x[:, 64:128].t() * SCALE, -1)
    g = torch.from_numpy(mh[0, 0]).double() * (doh.double() @ x[:, 128:].t()) * R.scale32(p)
    dS = P * (g - (P * g).sum(-1, keepdim=True))
    assert abs(float(dS[q0, ka]) * sigma * sigma * 2.0 ** -22 / t - 1.0) < 1e-6          # the element the case is built for
    _sp_case(B, H, N, p, 1.0, data=(qh, doh, mh), scale_of={"dQ": float((dS.abs() @ x[:, 64:128].abs()).max()) * SCALE})


# ============================================================================================ f. argument rejections
def test_argument_rejections():
    """Host-side EAV_REQUIRE checks: they return before any launch."""
    B, H, N, D = 1, 1, 4, 64
    f = torch.zeros(B * N * 3 * D, device="cuda")
    h = torch.zeros(B * N * 6 * D, dtype=torch.float16, device="cuda")
    slot = torch.zeros(SLOT, device="cuda")
    for p in (0.0, 1.0):
        with pytest.raises(_lib.EavError, match="drop_p"):
            call("eav_attn_fwd_dropout", ptr(f), ptr(f), ptr(f), B, H, N, 64, SCALE, p, 0, None, None, None)
        with pytest.raises(_lib.EavError, match="drop_p"):
            call("eav_attn_bwd_dropout", ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), B, H, N, 64, SCALE, p, 0, None, None,
                 None)
        with pytest.raises(_lib.EavError, match="drop_p"):
            call("eav_attn_fwd_sp_dropout", ptr(h), ptr(slot), ptr(f), ptr(f), ptr(slot), B, H, N, 64, SCALE, p, 0, None, None,
                 None)
        with pytest.raises(_lib.EavError, match="drop_p"):
            call("eav_attn_bwd_sp_dropout", ptr(h), ptr(h), ptr(slot), ptr(slot), ptr(slot), ptr(f), ptr(f), ptr(f), ptr(f),
                 ptr(f), ptr(slot), B, H, N, 64, SCALE, p, 0, None, None, None)
    a, b, c = (torch.zeros(8 * 2049, device="cuda") for _ in range(3))
    for rows, n, ld, s, pd in ((2, 2049, 2049, a, b), (2, 16, 16, a, a), (2, 16, 15, a, b)):
        with pytest.raises(_lib.EavError, match="eav_softmax_dropout_fwd"):
            call("eav_softmax_dropout_fwd", ptr(s), ptr(pd), rows, n, ld, 0.1, 0, None, None, None)
    for rows, n, ld, P, dP, pd in ((2, 2049, 2049, a, b, c), (2, 16, 16, a, a, c), (2, 16, 16, a, b, b), (2, 16, 16, a, b, a),
                                   (2, 16, 15, a, b, c)):
        with pytest.raises(_lib.EavError, match="eav_softmax_dropout_bwd"):
            call("eav_softmax_dropout_bwd", ptr(P), ptr(dP), ptr(pd), rows, n, ld, 0.1, 0, None, None, None)
    for n in (1, 6, 1027):
        with pytest.raises(_lib.EavError, match="eav_tf_dropout_add"):
            call("eav_tf_dropout_add", ptr(a), None, ptr(b), n, 0.1, 0, None, None, None)
    torch.cuda.synchronize()
    assert not f.any() and not a.any() and not b.any() and not c.any() and not slot.any()
