"""Pure-torch restatement of the AST / ViT classification forward WITH the four dropout sites of the Hugging Face classes
(models/vit/modeling_vit.py, models/audio_spectrogram_transformer/modeling_audio_spectrogram_transformer.py), driven by
explicit keep-masks, plus what the encoder-dropout goldens and their tests share: the cases, the mask generator (a pure
function of a recorded seed, eav_amd.synth) and the per-tensor summaries the fixtures store.

Sites, in HF's call order (the order the golden generator's patched F.dropout consumed the masks in):
    emb          [B, ntok, D]   after cls/[dist]/patch tokens + position embeddings       hidden_dropout
    attn.{i}     [B, H, N, N]   softmax probabilities, before P.V                          attention_dropout
    attn_out.{i} [B, N, D]      o_proj output (after bias), before the residual add        hidden_dropout
    mlp_out.{i}  [B, N, D]      fc2 output (after bias), before the residual add           hidden_dropout
Inverted dropout: kept values are scaled by 1 / (1 - p); p = 0 means the site does not exist.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from eav_amd import synth

# golden cases: (hidden_dropout, attention_dropout); "d" is the p = 0 control on the same configuration
CASES = {"a": (0.1, 0.1), "b": (0.0, 0.3), "c": (0.25, 0.0), "d": (0.0, 0.0)}
MODEL = dict(hidden=128, layers=2, heads=2, ff=256)          # head_dim 64: the fused attention kernels are under test
AST_FRAMES = 256                                              # 12 x 25 + 2 = 302 tokens = 4*64 + 46: a ragged key tail
WSEED = {"ast": 21, "vit": 22}
XSEED, MSEED, STD, LR, BATCH = 150, 7100, 0.08, 1e-3, 2
SAMPLE = 257                                                  # elements of a tensor's strided sample (all of a smaller one)


def site_names(layers, ph, pa):
    names = ["emb"] if ph > 0 else []
    for i in range(layers):
        if pa > 0:
            names.append(f"attn.{i}")
        if ph > 0:
            names += [f"attn_out.{i}", f"mlp_out.{i}"]
    return names


def site_shape(name, B, ntok, hidden, heads):
    return (B, heads, ntok, ntok) if name.startswith("attn.") else (B, ntok, hidden)


def site_masks(mseed, step, B, ntok, hidden, heads, layers, ph, pa):
    """{site: uint8 keep-mask}: keep = uniform(seed of (mseed, step, site)) >= p, the repo's own generator."""
    out = {}
    for n, name in enumerate(site_names(layers, 1.0, 1.0)):          # (site numbering independent of which sites exist)
        p = pa if name.startswith("attn.") else ph
        if p > 0:
            u = synth.uniform(mseed * 100003 + step * 1009 + n, site_shape(name, B, ntok, hidden, heads))
            out[name] = (u >= np.float32(p)).astype(np.uint8)
    return out


def _drop(t, masks, name, p):
    if p <= 0.0:
        return t
    m = masks[name]
    m = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m))
    return t * m.to(t.dtype) * (1.0 / (1.0 - p))


def forward(P, x, cfg, masks, ph, pa):
    """cfg: a dict of oracle.vit_oracle.cfg_ast / cfg_vit.  P: {HF key: tensor} (any floating dtype; x follows it).
    masks None or p = 0 everywhere: the plain forward."""
    p, d, H = cfg["prefix"], cfg["hidden"], cfg["heads"]
    hd, eps = d // H, cfg["eps"]
    masks = masks or {}
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
    h = _drop(torch.cat(toks + [emb], dim=1) + P[f"{p}.embeddings.position_embeddings"], masks, "emb", ph)
    N = h.shape[1]
    for i in range(cfg["layers"]):
        L = f"{p}.layers.{i}"
        y = F.layer_norm(h, (d,), P[f"{L}.layernorm_before.weight"], P[f"{L}.layernorm_before.bias"], eps)
        q, k, v = (F.linear(y, P[f"{L}.attention.{n}_proj.weight"], P[f"{L}.attention.{n}_proj.bias"])
                   .view(B, N, H, hd).transpose(1, 2) for n in "qkv")
        a = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * (hd ** -0.5), dim=-1)
        a = _drop(a, masks, f"attn.{i}", pa)
        o = torch.matmul(a, v).transpose(1, 2).reshape(B, N, d)
        o = F.linear(o, P[f"{L}.attention.o_proj.weight"], P[f"{L}.attention.o_proj.bias"])
        h = h + _drop(o, masks, f"attn_out.{i}", ph)
        y = F.layer_norm(h, (d,), P[f"{L}.layernorm_after.weight"], P[f"{L}.layernorm_after.bias"], eps)
        y = F.linear(y, P[f"{L}.mlp.fc1.weight"], P[f"{L}.mlp.fc1.bias"])
        y = y * 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0)))
        y = F.linear(y, P[f"{L}.mlp.fc2.weight"], P[f"{L}.mlp.fc2.bias"])
        h = h + _drop(y, masks, f"mlp_out.{i}", ph)
    seq = F.layer_norm(h, (d,), P[f"{p}.layernorm.weight"], P[f"{p}.layernorm.bias"], eps)
    if cfg["kind"] == "ast":
        pooled = (seq[:, 0] + seq[:, 1]) / 2
        pooled = F.layer_norm(pooled, (d,), P["classifier.layernorm.weight"], P["classifier.layernorm.bias"], eps)
        return F.linear(pooled, P["classifier.dense.weight"], P["classifier.dense.bias"])
    return F.linear(seq[:, 0], P["classifier.weight"], P["classifier.bias"])


def sample_index(numel):
    """Flat indices of a tensor's stored sample: every element of a small tensor, else SAMPLE evenly strided ones."""
    if numel <= SAMPLE:
        return np.arange(numel)
    return (np.arange(SAMPLE, dtype=np.int64) * (numel - 1)) // (SAMPLE - 1)


def summarise(t):
    """(strided sample, sum |.|, max |.|) of a tensor, as float32 / float64 / float64."""
    a = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).reshape(-1)
    return a[sample_index(a.size)].astype(np.float32), np.float64(np.abs(a.astype(np.float64)).sum()), \
        np.float64(np.abs(a).max())


def oracle_cfg(kind):
    from oracle import vit_oracle as vo
    return vo.cfg_ast(frames=AST_FRAMES, **MODEL) if kind == "ast" else vo.cfg_vit(**MODEL)


def batch(kind, cfg, seed, B):
    return synth.mel_batch(seed, B, cfg["frames"], cfg["mel"]) if kind == "ast" else synth.frame_batch(seed, B, cfg["image"])


def adamw_step_(p, g, m, v, t, lr, wd=0.01, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.AdamW (decoupled weight decay), restated."""
    p.mul_(1.0 - lr * wd)
    m.mul_(b1).add_(g, alpha=1.0 - b1)
    v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
    denom = (v.sqrt() / math.sqrt(1.0 - b2 ** t)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / (1.0 - b1 ** t))


def run_case(kind, case, dtype=torch.float32):
    """The two training steps of a golden case (unfrozen, then frozen: classifier only) with this module's forward and
    AdamW: {"logits{s}", "loss{s}", "grad{s}.{k}", "post{s}.{k}"} as tensors."""
    from oracle import vit_oracle as vo
    from tests.golden_util import tf_weights
    ph, pa = CASES[case]
    cfg = oracle_cfg(kind)
    W = tf_weights(WSEED[kind], vo.param_shapes(cfg), std=STD)
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in W.items()}
    m = {k: torch.zeros_like(v) for k, v in P.items()}
    v2 = {k: torch.zeros_like(v) for k, v in P.items()}
    t = {k: 0 for k in P}
    hk = set(vo.head_keys(cfg))
    out = {}
    for s, freeze in enumerate((False, True)):
        x, y = batch(kind, cfg, XSEED + s, BATCH)
        masks = site_masks(MSEED, s, BATCH, cfg["ntok"], cfg["hidden"], cfg["heads"], cfg["layers"], ph, pa)
        for k, p in P.items():
            p.grad = None
            p.requires_grad_((not freeze) or (k in hk))
        logits = forward(P, torch.from_numpy(x).to(dtype), cfg, masks, ph, pa)
        loss = F.cross_entropy(logits, torch.from_numpy(y))
        loss.backward()
        out[f"logits{s}"], out[f"loss{s}"] = logits.detach().clone(), loss.detach().clone()
        with torch.no_grad():
            for k, p in P.items():
                if p.grad is None:
                    continue
                out[f"grad{s}.{k}"] = p.grad.clone()
                t[k] += 1
                adamw_step_(p, p.grad, m[k], v2[k], t[k], LR)
                out[f"post{s}.{k}"] = p.detach().clone()
    return out
