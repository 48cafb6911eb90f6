"""Host-only restatement of stochastic depth (timm.layers.DropPath, scale_by_keep) as the AST / ViT encoders run it
(eav_amd/encoder_drop_path.py, csrc/drop_path.hip), written independently of the package: the rates, the site ids, the hash,
the plan of a forward's scale table, the add / gate in numpy float32, and a float64 torch forward with per-sample scales that
extends tests/encoder_dropout_ref.forward.  Also what the goldens tests/golden/drop_path_{ast,vit}.npz and their tests share.

Layer i of L drops with p_i = r i / (L - 1) (torch.linspace(0, r, L); 0 for L = 1), formed in float64 and rounded once to
float32.  Sample b of branch (i, k) - k = 0 the attention branch, 1 the MLP branch - is kept when
hash32(site seed + 2 counter, b) 2^-24 >= p_i, site id (1 << 23) + 1 + 2 i + k; its scale is float32 1 / (1 - p_i), 0 when
dropped, 1 in the rows of layers with p_i = 0."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.encoder_dropout_kernel_ref import M64
from tests.patch_keep_ref import hash32

PATCH_KEEP_SITE = 1 << 23                          # encoder_dropout.SITES["patch_keep"]: the ids below sit above it

# (L, B) / rates / counters of the plan cases: one layer (nothing drops), the smallest that drops, odd sizes, the workload's
# 12 layers at AST's and ViT's batch, and more than one 256-thread block per row
PLAN_CASES = [(1, 1), (2, 2), (3, 4), (12, 8), (12, 128), (3, 1000)]
PLAN_RATES = [0.1, 0.5]
PLAN_COUNTERS = [1, 77]
# (B, per_sample) of the add cases: one float4; a sample that is no multiple of the 256-thread block; 302 x 128 and 197 x 64
# (the reduced models: workgroups straddle samples); AST's 1214 x 768.  ADD_LOOP_CASE: more float4 than the 8192 x 256 threads
# of the largest grid, split over three samples so that no pass of the grid-stride loop ends on a sample's edge
ADD_CASES = [(1, 4), (2, 4 * 257), (3, 302 * 128), (5, 197 * 64), (2, 1214 * 768)]
ADD_LOOP_CASE = (3, 4 * 700001)

# the model of the Hugging Face goldens: encoder_dropout_ref.MODEL widened to 3 layers (head_dim 64), AST at 256 frames
MODEL = dict(hidden=128, layers=3, heads=2, ff=256)
SMALL = dict(hidden=64, layers=3, heads=4, ff=128)            # head_dim 16: the materialised scores
AST_FRAMES = 256
RATE, BATCH = 0.5, 4                                          # p = 0, 0.25, 0.5
WSEED = {"ast": 41, "vit": 42}
XSEED, STD, LR = 410, 0.08, 1e-3


def rates(r, L):
    """float32 [L]: torch.linspace(0, r, L) in float64, rounded once."""
    return np.array([float(r) * i / (L - 1) if L > 1 else 0.0 for i in range(L)], np.float64).astype(np.float32)


def site_ids(i):
    return PATCH_KEEP_SITE + 1 + 2 * i, PATCH_KEEP_SITE + 2 + 2 * i


def site_seed(seed, sid):
    """encoder_dropout.site_seed."""
    return (int(seed) + ((sid + 1) << 40)) & M64


def scale32(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def draws(seed, sid, B, counter=None):
    """The uniform draws of a site's B samples: hash32 2^-24 as float32 (exact)."""
    return hash32(site_seed(seed, sid), B, counter).astype(np.float32) * np.float32(2.0 ** -24)


def plan(L, B, r, seed, counter=None, keep=None):
    """(keep uint8 [L, 2, B], scale float32 [L, 2, B]) of a forward under the MODEL seed `seed`; keep: an explicit table
    instead of the hash (rows of layers with p_i = 0 are not read: they come back as ones)."""
    p = rates(r, L)
    k = np.ones((L, 2, B), np.uint8)
    s = np.ones((L, 2, B), np.float32)
    for i in range(L):
        if p[i] > 0:
            for br in range(2):
                k[i, br] = (draws(seed, site_ids(i)[br], B, counter) >= p[i]) if keep is None else (np.asarray(keep)[i, br] != 0)
                s[i, br] = np.where(k[i, br] != 0, scale32(p[i]), np.float32(0.0))
    return k, s


def add(y, resid, scale_row):
    """float32 resid + y * s per sample (the product rounded, then the sum); resid None: the gate y * s.  y [B, n]."""
    with np.errstate(invalid="ignore"):
        prod = np.asarray(y, np.float32) * np.asarray(scale_row, np.float32)[:, None]
        return prod if resid is None else np.asarray(resid, np.float32) + prod


def scales_of(keep, r):
    """float64 scale table of an explicit keep table [L, 2, B] (the scale is float32 1 / (1 - p_i), as the kernels form it)."""
    keep = np.asarray(keep)
    p = rates(r, keep.shape[0])
    s = np.ones(keep.shape, np.float64)
    for i in range(keep.shape[0]):
        if p[i] > 0:
            s[i] = np.where(keep[i] != 0, np.float64(scale32(p[i])), 0.0)
    return s


def golden_keep(step):
    """The explicit keep tables [3, 2, 4] of the two golden steps.  Step 0: sample 0 is kept wherever anybody is, sample 1 is
    dropped in both branches of layer 1, layer 2's MLP branch is dropped for the whole batch (fc1 / fc2 of layer 2 get exactly
    zero gradients).  Step 1 (frozen): other drops.  Layer 0 (p = 0) is not read."""
    k = np.ones((3, 2, 4), np.uint8)
    if step == 0:
        k[1, 0], k[1, 1] = [1, 0, 1, 1], [1, 0, 1, 0]
        k[2, 0], k[2, 1] = [1, 1, 0, 1], [0, 0, 0, 0]
    else:
        k[1, 0], k[1, 1] = [1, 1, 0, 1], [0, 1, 1, 1]
        k[2, 0], k[2, 1] = [1, 0, 1, 1], [1, 1, 0, 1]
    return k


def oracle_cfg(kind, model=None):
    from oracle import vit_oracle as vo
    model = model or MODEL
    return vo.cfg_ast(frames=AST_FRAMES, **model) if kind == "ast" else vo.cfg_vit(**model)


def batch(kind, cfg, seed, B):
    from eav_amd import synth
    return synth.mel_batch(seed, B, cfg["frames"], cfg["mel"]) if kind == "ast" else synth.frame_batch(seed, B, cfg["image"])


def forward(P, x, cfg, scales=None, rows=None, hidden=None):
    """tests/encoder_dropout_ref.forward with per-sample branch scales instead of element masks.  scales: None or
    [L, 2, B] (anything torch.as_tensor takes); rows: None or an int64 [B, n] tensor - the token rows every sample keeps after the
    embeddings (patch dropout: the readout tokens, then nextra + the kept patches); hidden: a list that receives the embedding
    output and every layer's output."""
    p, d, H = cfg["prefix"], cfg["hidden"], cfg["heads"]
    hd, eps = d // H, cfg["eps"]
    w, b = P[f"{p}.embeddings.patch_embeddings.projection.weight"], P[f"{p}.embeddings.patch_embeddings.projection.bias"]
    if cfg["kind"] == "ast":
        emb = F.conv2d(x.unsqueeze(1).transpose(2, 3), w, b, stride=(cfg["fstride"], cfg["tstride"]))
    else:
        emb = F.conv2d(x, w, b, stride=cfg["patch"])
    emb = emb.flatten(2).transpose(1, 2)
    B = emb.shape[0]
    toks = [P[f"{p}.embeddings.cls_token"].expand(B, -1, -1)]
    if cfg["kind"] == "ast":
        toks.append(P[f"{p}.embeddings.distillation_token"].expand(B, -1, -1))
    h = torch.cat(toks + [emb], dim=1) + P[f"{p}.embeddings.position_embeddings"]
    if rows is not None:
        h = torch.gather(h, 1, rows[:, :, None].expand(-1, -1, d))
    N = h.shape[1]
    S = None if scales is None else torch.as_tensor(np.asarray(scales, np.float64)).to(h.dtype)
    gate = lambda t, i, br: t if S is None else t * S[i, br][:, None, None]  # noqa: E731
    if hidden is not None:
        hidden.append(h.detach().clone())
    for i in range(cfg["layers"]):
        L = f"{p}.layers.{i}"
        y = F.layer_norm(h, (d,), P[f"{L}.layernorm_before.weight"], P[f"{L}.layernorm_before.bias"], eps)
        q, k, v = (F.linear(y, P[f"{L}.attention.{n}_proj.weight"], P[f"{L}.attention.{n}_proj.bias"])
                   .view(B, N, H, hd).transpose(1, 2) for n in "qkv")
        a = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * (hd ** -0.5), dim=-1)
        o = torch.matmul(a, v).transpose(1, 2).reshape(B, N, d)
        o = F.linear(o, P[f"{L}.attention.o_proj.weight"], P[f"{L}.attention.o_proj.bias"])
        h = h + gate(o, i, 0)
        y = F.layer_norm(h, (d,), P[f"{L}.layernorm_after.weight"], P[f"{L}.layernorm_after.bias"], eps)
        y = F.linear(y, P[f"{L}.mlp.fc1.weight"], P[f"{L}.mlp.fc1.bias"])
        y = y * 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0)))
        y = F.linear(y, P[f"{L}.mlp.fc2.weight"], P[f"{L}.mlp.fc2.bias"])
        h = h + gate(y, i, 1)
        if hidden is not None:
            hidden.append(h.detach().clone())
    seq = F.layer_norm(h, (d,), P[f"{p}.layernorm.weight"], P[f"{p}.layernorm.bias"], eps)
    if cfg["kind"] == "ast":
        pooled = (seq[:, 0] + seq[:, 1]) / 2
        pooled = F.layer_norm(pooled, (d,), P["classifier.layernorm.weight"], P["classifier.layernorm.bias"], eps)
        return F.linear(pooled, P["classifier.dense.weight"], P["classifier.dense.bias"])
    return F.linear(seq[:, 0], P["classifier.weight"], P["classifier.bias"])


def float64_step(W, x, y, cfg, scales=None, rows=None):
    """(logits, loss, {name: gradient}) of one cross-entropy step of `forward` in float64."""
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in W.items()}
    logits = forward(P, torch.as_tensor(x).double(), cfg, scales, rows)
    loss = F.cross_entropy(logits, torch.as_tensor(y))
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in P.items()}
