"""Float64 restatement of what output_attentions / attention_rollout return, written independently of csrc/attn_probs.hip:
softmax(scale Q K^T) per (image, head) from the fp32 qkv [B*N, 3 H hd] (Q | K | V, head h at columns h hd), the head mean,
the rollout recursion r <- r (0.5 A + 0.5 I) from the top layer down (Abnar & Zuidema 2020), and a float64 restatement of
the encoder's per-layer hidden states (HF's hidden_states), following oracle/vit_oracle.py op by op.

The element-wise bound of the GPU tests has the form atol + rtol P.  Its constants cannot be derived from outside the kernels
(they depend on the accumulation order of the score MFMAs and on v_exp_f32), so they are MEASURED: the largest error against
this restatement over N in SHAPES, seeds SEEDS, B = 2, H = 3 (inputs(): synth.normal plus the two hostile rows), per
precision - the absolute error where the reference is below ATOL_BELOW, the relative error elsewhere - and set at 4 x that
maximum (the margin covers seeds and shapes not sampled).  The row-sum deviation from 1 the same way.

    measured on the MI355X (probabilities and head mean together)
                                        max |err|, P < 1e-6    max |err| / P, P >= 1e-6    max |rowsum - 1|
    eav_attn_probs    ("fp32")          1.02e-12 (N = 128)     3.31e-6 (N = 129)           2.69e-6 (N = 31)
    eav_attn_probs_sp ("split")         5.98e-12 (N = 128)     7.96e-6 (N = 128)           4.53e-6 (N = 197)
The relative figure is that of the hostile rows: a score of 120 is 173 in the kernels' base-2 units, where one fp32 ulp is
1.5e-5 - the forward's lse carries the same rounding.  Rows of ordinary scores are within 1e-6.
"""
import numpy as np

SHAPES = [1, 31, 32, 33, 127, 128, 129, 197, 1214]      # one token, either side of the 32- and 128-row tiles, ViT's, AST's
SEEDS = [11, 12, 13]
B, H, HD = 2, 3, 64
ATOL_BELOW = 1e-6

# precision -> (atol, rtol, row-sum tolerance): 4 x the measured maxima of the table above
MEASURED = {"fp32": (1.02e-12, 3.31e-6, 2.69e-6), "split": (5.98e-12, 7.96e-6, 4.53e-6)}
BOUNDS = {k: tuple(4.0 * v for v in m) for k, m in MEASURED.items()}
# model(x, output_hidden_states=True) against hidden_states() below, relative to max|ref| of each tensor (measured over
# the configurations of tests/test_encoder_outputs_gpu.py, 4 x): precision -> bound
HIDDEN_MEASURED = {"fp32": 8.27e-7, "split": 3.34e-7}
HIDDEN_BOUND = {k: 4.0 * v for k, v in HIDDEN_MEASURED.items()}
# model(x, output_attentions=True) against layer_probs() of the model's own hidden state: (atol, rtol) of the same
# form; beside the kernels' error it holds that of the model's LayerNorm and q/k projection.  rtol: measured, 4 x.  No
# reference probability of those small encoders lies below ATOL_BELOW, so nothing was measured for atol: it is the kernels' own
# (how a probability far below the row's largest is rounded is a property of the kernels, not of the projection)
ENCODER_MEASURED = {"fp32": (0.0, 2.08e-6), "split": (0.0, 1.77e-6)}
ENCODER_BOUNDS = {k: (BOUNDS[k][0], 4.0 * m[1]) for k, m in ENCODER_MEASURED.items()}


def inputs(seed, N, B=B, H=H):
    """qkv [B*N, 3 H 64] fp32 from synth.normal with two hostile query rows per (image, head): query 0 aligned with key
    N - 1 so that its score is 40 (scaled, natural-log units) and the others about 40 lower - a near one-hot row - and query
    N // 2 aligned with key 0 at a score of 120: the other probabilities (centred 120 lower, spread about 15) underflow in
    fp32 but for a few.  (N = 1: the two coincide.)"""
    from eav_amd import synth
    D = H * HD
    qkv = synth.normal(seed * 1000 + N, (B * N, 3 * D)).reshape(B, N, 3, H, HD)
    scale = HD ** -0.5
    for qa, ka, top in ((0, N - 1, 40.0), (N // 2, 0, 120.0)):
        k = qkv[:, ka, 1].astype(np.float64)                                # [B, H, hd]
        qkv[:, qa, 0] = (k * (top / (scale * (k * k).sum(-1, keepdims=True)))).astype(np.float32)
    return np.ascontiguousarray(qkv.reshape(B * N, 3 * D))


def scores(qkv, B, H, N, scale, hd=HD):
    """float64 [B, H, N, N]: scale Q K^T."""
    x = np.asarray(qkv, np.float64).reshape(B, N, 3, H, hd)
    return scale * np.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1])


def softmax(s):
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def probs(qkv, B, H, N, scale, hd=HD):
    """float64 [B, H, N, N]: softmax(scale Q K^T) per (image, head)."""
    return softmax(scores(qkv, B, H, N, scale, hd))


def head_mean(P):
    """[B, H, N, N] -> [B, N, N]."""
    return np.asarray(P, np.float64).mean(1)


def rollout_step(r, abar):
    """r [B, R, N], abar [B, N, N] -> 0.5 r abar + 0.5 r (float64)."""
    r, abar = np.asarray(r, np.float64), np.asarray(abar, np.float64)
    return 0.5 * np.einsum("brq,bqk->brk", r, abar) + 0.5 * r


def rollout_step_bound(r, abar):
    """Element-wise fp32 bound of one step: N fused multiply-adds into one accumulator, the two halvings (exact) and the
    final addition - (N + 2) 2^-24 of the sum of magnitudes (every operation rounds once, relative 2^-24; first order, the
    constant 2 covers the last addition and the second-order terms)."""
    r, abar = np.abs(np.asarray(r, np.float64)), np.abs(np.asarray(abar, np.float64))
    return (r.shape[-1] + 2) * 2.0 ** -24 * (0.5 * np.einsum("brq,bqk->brk", r, abar) + 0.5 * r)


def rollout(attentions, nextra):
    """attentions: per layer [B, H, N, N] (bottom layer first) -> float64 [B, N]: the readout rows e_0 .. e_{nextra-1}
    propagated from the top layer down, r <- r (0.5 mean_h A_l + 0.5 I), averaged over the readout rows at the end."""
    A = [head_mean(a) for a in attentions]
    Bn, N = A[0].shape[0], A[0].shape[-1]
    r = np.zeros((Bn, nextra, N))
    for k in range(nextra):
        r[:, k, k] = 1.0
    for a in reversed(A):
        r = rollout_step(r, a)
    return r.mean(1)


def error_bounds(P, precision, table=None):
    """Element-wise bound atol + rtol P of an fp32 result against the float64 P (probabilities or their head mean)."""
    atol, rtol = (table or BOUNDS)[precision][:2]
    return atol + rtol * np.abs(np.asarray(P, np.float64))


def split_errors(got, ref):
    """(max |err| where ref < ATOL_BELOW, max |err| / ref elsewhere): the two figures the constants are measured from."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    small = ref < ATOL_BELOW
    return (float(err[small].max()) if small.any() else 0.0,
            float((err[~small] / ref[~small]).max()) if (~small).any() else 0.0)


# ----------------------------------------------------------------------------- the encoder's hidden states, float64
def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def _erf(x):
    import math
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def layer_probs(W, cfg, i, h):
    """The attention probabilities of layer i given its input h [B, N, D]: LayerNorm, q / k projection with bias, softmax."""
    W = {k: np.asarray(v, np.float64) for k, v in W.items() if f".layers.{i}." in k}
    L = f"{cfg['prefix']}.layers.{i}"
    d, Hn = cfg["hidden"], cfg["heads"]
    Bn, N = h.shape[0], h.shape[1]
    y = _ln(np.asarray(h, np.float64), W[f"{L}.layernorm_before.weight"], W[f"{L}.layernorm_before.bias"], cfg["eps"])
    q = (y @ W[f"{L}.attention.q_proj.weight"].T + W[f"{L}.attention.q_proj.bias"]).reshape(Bn, N, Hn, d // Hn)
    k = (y @ W[f"{L}.attention.k_proj.weight"].T + W[f"{L}.attention.k_proj.bias"]).reshape(Bn, N, Hn, d // Hn)
    return softmax((d // Hn) ** -0.5 * np.einsum("bqhd,bkhd->bhqk", q, k))


def hidden_states(W, x, cfg):
    """(hidden states, final sequence): layers + 1 float64 arrays [B, N, D] - the embedding output, then every layer's
    output, the last one before the final LayerNorm - and that LayerNorm's output, which is what
    oracle.vit_oracle.forward(..., return_hidden=True) returns beside the logits (tests/test_attn_probs_cpu.py pins the two)."""
    W = {k: np.asarray(v, np.float64) for k, v in W.items()}
    x = np.asarray(x, np.float64)
    p, d, Hn, eps = cfg["prefix"], cfg["hidden"], cfg["heads"], cfg["eps"]
    w, b = W[f"{p}.embeddings.patch_embeddings.projection.weight"], W[f"{p}.embeddings.patch_embeddings.projection.bias"]
    ps = cfg["patch"]
    if cfg["kind"] == "ast":
        img, sy, sx = x.transpose(0, 2, 1)[:, None], cfg["fstride"], cfg["tstride"]
    else:
        img, sy, sx = x, ps, ps
    Bn, _, Hi, Wi = img.shape
    ny, nx = (Hi - ps) // sy + 1, (Wi - ps) // sx + 1
    emb = np.empty((Bn, ny * nx, d))
    for iy in range(ny):
        for ix in range(nx):
            patch = img[:, :, iy * sy:iy * sy + ps, ix * sx:ix * sx + ps].reshape(Bn, -1)
            emb[:, iy * nx + ix] = patch @ w.reshape(d, -1).T + b
    toks = [np.broadcast_to(W[f"{p}.embeddings.cls_token"], (Bn, 1, d))]
    if cfg["kind"] == "ast":
        toks.append(np.broadcast_to(W[f"{p}.embeddings.distillation_token"], (Bn, 1, d)))
    h = np.concatenate(toks + [emb], 1) + W[f"{p}.embeddings.position_embeddings"]
    N = h.shape[1]
    out = [h]
    for i in range(cfg["layers"]):
        L = f"{p}.layers.{i}"
        y = _ln(h, W[f"{L}.layernorm_before.weight"], W[f"{L}.layernorm_before.bias"], eps)
        v = (y @ W[f"{L}.attention.v_proj.weight"].T + W[f"{L}.attention.v_proj.bias"]).reshape(Bn, N, Hn, d // Hn)
        a = layer_probs(W, cfg, i, h)
        o = np.einsum("bhqk,bkhd->bqhd", a, v).reshape(Bn, N, d)
        h = h + o @ W[f"{L}.attention.o_proj.weight"].T + W[f"{L}.attention.o_proj.bias"]
        y = _ln(h, W[f"{L}.layernorm_after.weight"], W[f"{L}.layernorm_after.bias"], eps)
        y = y @ W[f"{L}.mlp.fc1.weight"].T + W[f"{L}.mlp.fc1.bias"]
        y = y * 0.5 * (1.0 + _erf(y / np.sqrt(2.0)))
        h = h + y @ W[f"{L}.mlp.fc2.weight"].T + W[f"{L}.mlp.fc2.bias"]
        out.append(h)
    return out, _ln(h, W[f"{p}.layernorm.weight"], W[f"{p}.layernorm.bias"], eps)
