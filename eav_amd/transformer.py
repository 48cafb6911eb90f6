"""AST / ViT classification encoders on MI355X: forward, backward and weight hand-off.

The reference never defines these models - it instantiates Hugging Face classes
(`AutoModelForAudioClassification.from_pretrained`, Transformer_Audio.py:22;
`AutoModelForImageClassification.from_pretrained`, Transformer_Vision.py:29) and trains them
with `loss.backward()`.  This module restates that arithmetic as an explicit schedule of
libeav_hip.so kernels, keeps the HF 5.x parameter names so `state_dict()` / safetensors
checkpoints interchange (HF 4.x names are accepted on load), and exposes the pieces the
reference trainers touch: `model(x).logits`, `model.classifier`, `model.parameters()`,
`train()/eval()`, `.to(device)`.

Two arithmetic paths behind `Encoder.precision` (env EAV_ENCODER_PRECISION), same parity bounds:
  "split" (default)  every dense projection and the fused attention on the fp16 matrix cores with
                     fp16 hi + lo operand planes, three MFMAs per product, fp32 accumulation -
                     fp32-grade (gemm_sp.hip, attention_sp.hip).  Weight-gradient
                     GEMMs, the final bias / LayerNorm gradient reductions and the refresh of the
                     weight planes run on a side HIP stream.
  "fp32"             the same schedule on the exact-fp32 MFMA (gemm_f32.hip, attention.hip).

Everything is kept resident (288 GB HBM): what a backward needs is saved, nothing is recomputed
(split: the fp16 planes of the layer inputs of every GEMM and of q | k | v, the pre-activations of
the MLP and the attention outputs / log-sum-exps; the fused attention never materialises the
[B*H, N, N] probabilities - only the reduced test configurations with head_dim != 64 do).
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import _lib, pos_interp, pos_time
from .optim import HEAD_NARROW_CLASSES, BCEWithLogitsLoss, CrossEntropyLoss, MSELoss, flatten_parameters
from .runtime import KernelFn, KernelModule, gather_batch
from .weight_planes import SLOT, WeightPlanes


DEFAULT_PRECISION = "split"
# Classes the classification head takes: up to HEAD_NARROW_CLASSES (16, optim.py) on eav_dense_softmax_* (the classes in
# registers), beyond that on eav_dense_wide_* (csrc/head_wide.hip; EAV_HEAD_MAX_CLASSES of include/eav_hip.h) - AudioSet's
# 527, ImageNet's 1000, ImageNet-21k's 21 843.
HEAD_MAX_CLASSES = 32768
# Tokens per sequence the attention / softmax kernels take
MAX_TOKENS = 2048
# HF config.problem_type: which loss a labelled forward takes (transformers/loss/loss_utils.py, ForSequenceClassificationLoss)
PROBLEM_TYPES = ("regression", "single_label_classification", "multi_label_classification")

# ----------------------------------------------------------------------------- configuration
def make_config(kind, hidden=768, layers=12, heads=12, ff=3072, eps=1e-12, num_labels=5, patch=16, mel=128,
                frames=1024, fstride=10, tstride=10, image=224, channels=3, hidden_dropout=0.0, attention_dropout=0.0,
                id2label=None, problem_type=None):
    """hidden_dropout / attention_dropout: HF hidden_dropout_prob / attention_probs_dropout_prob, applied in training mode
    at the four sites of Encoder.dropout_sites; 0 <= p < 1 (0: the site does not exist).  problem_type: HF's
    config.problem_type, one of PROBLEM_TYPES or None (resolved by the first labelled forward, resolve_problem_type)."""
    if problem_type is not None and problem_type not in PROBLEM_TYPES:
        raise ValueError(f"problem_type {problem_type!r}: expected None or one of {PROBLEM_TYPES}")
    _check_single_label(problem_type, num_labels)
    for name, p in (("hidden_dropout", hidden_dropout), ("attention_dropout", attention_dropout)):
        if not (isinstance(p, (int, float)) and 0.0 <= float(p) < 1.0):
            raise ValueError(f"make_config: {name} must satisfy 0 <= p < 1, got {p!r}")
    if kind == "ast":
        ny, nx = (mel - patch) // fstride + 1, (frames - patch) // tstride + 1
        geo = dict(C=1, H=mel, W=frames, sy=fstride, sx=tstride, transposed=1)
        nextra, prefix = 2, "audio_spectrogram_transformer"
    elif kind == "vit":
        ny = nx = image // patch
        geo = dict(C=channels, H=image, W=image, sy=patch, sx=patch, transposed=0)
        nextra, prefix = 1, "vit"
    else:
        raise ValueError(kind)
    return SimpleNamespace(kind=kind, hidden=hidden, layers=layers, heads=heads, ff=ff, eps=eps,
                           num_labels=num_labels, patch=patch, ny=ny, nx=nx, npatch=ny * nx, nextra=nextra,
                           ntok=ny * nx + nextra, prefix=prefix, kp=geo["C"] * patch * patch,
                           hidden_dropout=float(hidden_dropout), attention_dropout=float(attention_dropout),
                           id2label=id2label, problem_type=problem_type, **geo)


def config_from_hf(cfg_json: dict):
    """cfg.id2label: the label names of the checkpoint's config.json as a list ordered by class index (None without them)."""
    mt = cfg_json.get("model_type", "")
    names = cfg_json.get("id2label")
    common = dict(hidden=cfg_json.get("hidden_size", 768), layers=cfg_json.get("num_hidden_layers", 12),
                  heads=cfg_json.get("num_attention_heads", 12), ff=cfg_json.get("intermediate_size", 3072),
                  eps=cfg_json.get("layer_norm_eps", 1e-12), patch=cfg_json.get("patch_size", 16),
                  num_labels=len(cfg_json["id2label"]) if "id2label" in cfg_json else cfg_json.get("num_labels", 2),
                  hidden_dropout=cfg_json.get("hidden_dropout_prob", 0.0),
                  attention_dropout=cfg_json.get("attention_probs_dropout_prob", 0.0),
                  id2label=[names[k] for k in sorted(names, key=int)] if names else None,
                  problem_type=cfg_json.get("problem_type"))
    if cfg_json.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError("only the exact erf GELU is implemented")
    if mt == "audio-spectrogram-transformer":
        return make_config("ast", mel=cfg_json.get("num_mel_bins", 128), frames=cfg_json.get("max_length", 1024),
                           fstride=cfg_json.get("frequency_stride", 10), tstride=cfg_json.get("time_stride", 10),
                           **common)
    if mt == "vit":
        return make_config("vit", image=cfg_json.get("image_size", 224), channels=cfg_json.get("num_channels", 3),
                           **common)
    raise NotImplementedError(f"model_type {mt!r}")


def _check_single_label(problem_type, num_labels):
    """HF's configuration refuses this pair too: a cross-entropy over one class is identically 0."""
    if problem_type == "single_label_classification" and num_labels == 1:
        raise ValueError('problem_type "single_label_classification" requires num_labels > 1: use num_labels = 2 for a '
                         'binary classification, or problem_type "regression" for a single-output head')


def interpolated_geometry(cfg, H, W):
    """The geometry of a forward of a ViT `cfg` on H x W images with interpolate_pos_encoding on: a copy of cfg whose H, W,
    ny, nx, npatch and ntok are those of the input (ny = H // patch, nx = W // patch: the remainder pixels are dropped, as the
    strided patch convolution drops them), everything else unchanged, plus pos_grid - the side g of the stored g x g position
    grid when the table has to be resampled to ny x nx, None when HF uses the stored table as it is (ny nx == g g and
    H == W: HF's own shortcut, kept literally).  Pure: needs no device.  ValueError for an image smaller than a patch,
    NotImplementedError beyond MAX_TOKENS tokens and for AST (HF's AST has no such argument)."""
    if cfg.kind != "vit":
        raise NotImplementedError("interpolate_pos_encoding exists for ViT only (HF's AST takes no such argument)")
    H, W = int(H), int(W)
    if H < cfg.patch or W < cfg.patch:
        raise ValueError(f"interpolate_pos_encoding: a {H} x {W} image holds no {cfg.patch} x {cfg.patch} patch")
    ny, nx = H // cfg.patch, W // cfg.patch
    if ny * nx + cfg.nextra > MAX_TOKENS:
        raise NotImplementedError(f"at most {MAX_TOKENS} tokens: a {H} x {W} image gives {ny * nx + cfg.nextra}")
    g = int(cfg.npatch ** 0.5)
    if g * g != cfg.npatch:
        raise NotImplementedError(f"interpolate_pos_encoding needs a square stored position grid, not {cfg.ny} x {cfg.nx}")
    geo = SimpleNamespace(**vars(cfg))
    geo.H, geo.W, geo.ny, geo.nx, geo.npatch, geo.ntok = H, W, ny, nx, ny * nx, ny * nx + cfg.nextra
    geo.pos_grid = None if (ny * nx == g * g and H == W) else g
    return geo


def ast_length_geometry(cfg, T):
    """The geometry of a forward of an AST `cfg` on clips of T frames with variable_length on (the AST twin of
    interpolated_geometry): a copy of cfg whose W, nx, npatch and ntok are those of the input
    (nx = (T - patch) // tstride + 1; ny, the mel side, is the checkpoint's), everything else unchanged, plus time_grid - the
    number nx0 of time patches of the stored position table when that table has to be fitted to nx (pos_time: a centre cut for
    nx < nx0, linear interpolation for nx > nx0), None when nx == nx0 and the stored table serves as it is.  Pure: needs no
    device.  ValueError for a clip shorter than a patch, NotImplementedError beyond MAX_TOKENS tokens and for ViT (which has
    interpolate_pos_encoding)."""
    if cfg.kind != "ast":
        raise NotImplementedError("variable_length exists for AST only (a ViT takes interpolate_pos_encoding)")
    T = int(T)
    if T < cfg.patch:
        raise ValueError(f"variable_length: a clip of {T} frames holds no {cfg.patch}-frame patch")
    nx = (T - cfg.patch) // cfg.sx + 1
    if cfg.ny * nx + cfg.nextra > MAX_TOKENS:
        raise NotImplementedError(f"at most {MAX_TOKENS} tokens: a clip of {T} frames gives {cfg.ny * nx + cfg.nextra}")
    geo = SimpleNamespace(**vars(cfg))
    geo.W, geo.nx, geo.npatch, geo.ntok = T, nx, cfg.ny * nx, cfg.ny * nx + cfg.nextra
    geo.time_grid = None if nx == cfg.nx else cfg.nx
    return geo


def resolve_problem_type(num_labels, labels):
    """The problem_type HF's ForSequenceClassificationLoss settles on when the config leaves it unset: one label is a
    regression, several labels with integer targets (torch.long / torch.int) a single-label classification, anything
    else - float targets - a multi-label one."""
    if num_labels == 1:
        return "regression"
    if num_labels > 1 and labels.dtype in (torch.long, torch.int):
        return "single_label_classification"
    return "multi_label_classification"


def config_to_hf(cfg):
    """config.json of `cfg` (the inverse of config_from_hf): what HF needs to rebuild the model, and everything
    config_from_hf reads.  problem_type is left out while it is unset; labels without names are LABEL_i, HF's default."""
    names = list(cfg.id2label) if cfg.id2label is not None else [f"LABEL_{i}" for i in range(cfg.num_labels)]
    if len(names) != cfg.num_labels:
        raise ValueError(f"{len(names)} label names for {cfg.num_labels} labels")
    out = dict(hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
               intermediate_size=cfg.ff, hidden_act="gelu", layer_norm_eps=cfg.eps, patch_size=cfg.patch, qkv_bias=True,
               hidden_dropout_prob=cfg.hidden_dropout, attention_probs_dropout_prob=cfg.attention_dropout)
    if cfg.kind == "ast":
        out.update(model_type="audio-spectrogram-transformer", architectures=["ASTForAudioClassification"],
                   num_mel_bins=cfg.H, max_length=cfg.W, frequency_stride=cfg.sy, time_stride=cfg.sx)
    else:
        out.update(model_type="vit", architectures=["ViTForImageClassification"], image_size=cfg.H, num_channels=cfg.C)
    if cfg.problem_type is not None:
        out["problem_type"] = cfg.problem_type
    out["id2label"] = {str(i): n for i, n in enumerate(names)}
    out["label2id"] = {n: i for i, n in enumerate(names)}
    return out


def param_shapes(cfg):
    """Ordered {HF 5.x key: shape}.  Order = flat-buffer order: q,k,v weights (and biases) adjacent so the
    three projections run as one [3D, D] GEMM."""
    d, ff, p = cfg.hidden, cfg.ff, cfg.prefix
    s = {f"{p}.embeddings.cls_token": (1, 1, d)}
    if cfg.kind == "ast":
        s[f"{p}.embeddings.distillation_token"] = (1, 1, d)
    s[f"{p}.embeddings.position_embeddings"] = (1, cfg.ntok, d)
    s[f"{p}.embeddings.patch_embeddings.projection.weight"] = (d, cfg.C, cfg.patch, cfg.patch)
    s[f"{p}.embeddings.patch_embeddings.projection.bias"] = (d,)
    for i in range(cfg.layers):
        L = f"{p}.layers.{i}"
        for n in ("q", "k", "v"):
            s[f"{L}.attention.{n}_proj.weight"] = (d, d)
        for n in ("q", "k", "v"):
            s[f"{L}.attention.{n}_proj.bias"] = (d,)
        s[f"{L}.attention.o_proj.weight"] = (d, d)
        s[f"{L}.attention.o_proj.bias"] = (d,)
        for n in ("layernorm_before", "layernorm_after"):
            s[f"{L}.{n}.weight"] = (d,)
            s[f"{L}.{n}.bias"] = (d,)
        s[f"{L}.mlp.fc1.weight"] = (ff, d)
        s[f"{L}.mlp.fc1.bias"] = (ff,)
        s[f"{L}.mlp.fc2.weight"] = (d, ff)
        s[f"{L}.mlp.fc2.bias"] = (d,)
    s[f"{p}.layernorm.weight"] = (d,)
    s[f"{p}.layernorm.bias"] = (d,)
    if cfg.kind == "ast":
        s["classifier.layernorm.weight"] = (d,)
        s["classifier.layernorm.bias"] = (d,)
        s["classifier.dense.weight"] = (cfg.num_labels, d)
        s["classifier.dense.bias"] = (cfg.num_labels,)
    else:
        s["classifier.weight"] = (cfg.num_labels, d)
        s["classifier.bias"] = (cfg.num_labels,)
    return s


_HF4 = [  # (HF 4.x fragment, HF 5.x fragment)
    (".encoder.layer.", ".layers."), (".attention.attention.query.", ".attention.q_proj."),
    (".attention.attention.key.", ".attention.k_proj."), (".attention.attention.value.", ".attention.v_proj."),
    (".attention.output.dense.", ".attention.o_proj."), (".intermediate.dense.", ".mlp.fc1."),
    (".output.dense.", ".mlp.fc2."),
]


def normalise_key(k):
    for a, b in _HF4:
        k = k.replace(a, b)
    return k


def rank_dropout_seed(seed, rank):
    """The dropout seed of replica `rank` of a data-parallel group: replicas of one model see different shards of the batch
    and must draw different masks (rank 0 keeps the seed).  The rank goes through a splitmix64 finaliser of its own before it
    is added: eav_hash32 forms seed + (index + 1) * 0x9E3779B97F4A7C15, so an offset that is a small multiple of that
    constant (or of anything the index stride reaches within a tensor) would hand rank r the mask of rank 0 shifted by r
    elements; the finalised value is a multiple of the stride only for a shift of ~2^63 elements."""
    if int(rank) == 0:
        return int(seed) & 0xFFFFFFFFFFFFFFFF
    m = 0xFFFFFFFFFFFFFFFF
    z = (int(rank) * 0xD6E8FEB86659FD93) & m
    z = ((z ^ (z >> 32)) * 0xD6E8FEB86659FD93) & m
    z = ((z ^ (z >> 32)) * 0xD6E8FEB86659FD93) & m
    z ^= z >> 32
    return (int(seed) + z) & m


class _Node(nn.Module):
    """Anonymous container so that dotted HF names become real sub-modules (model.classifier.dense ...)."""


def _set_param(root, dotted, value):
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if not hasattr(m, p):
            m.add_module(p, _Node())
        m = getattr(m, p)
    m.register_parameter(parts[-1], nn.Parameter(value))


class _Out:
    def __init__(self, logits, loss=None):
        self.logits, self.loss = logits, loss


class _HeadFn(torch.autograd.Function):
    """The classification head alone on cached backbone features (Encoder.head): the same kernels, in the same order and
    with the same arguments, as the tail of _launch_forward / the start of _launch_backward."""

    @staticmethod
    def forward(ctx, feat, model, *params):
        ctx.model, ctx.B = model, feat.shape[0]
        hw = model._head_ws(feat.shape[0], feat.device)
        hw.feat.copy_(feat)
        model._begin()
        model._head_forward(hw.feat, hw, feat.shape[0])
        hw.token = model._token = model._token + 1
        ctx.token = hw.token
        return hw.logits.clone()

    @staticmethod
    def backward(ctx, dlogits):
        model = ctx.model
        hw = model._head_ws(ctx.B, dlogits.device)
        if hw.token != ctx.token:
            raise _lib.EavError("Encoder.head backward: activations were overwritten by a later head forward")
        model._begin()
        model._head_backward(dlogits.contiguous(), hw.feat, hw, ctx.B, False)
        return (None, None, *model._trained_grads(False))


class Encoder(KernelModule):
    """ASTForAudioClassification / ViTForImageClassification on the HIP kernels, with a head of 1 .. HEAD_MAX_CLASSES
    classes (the reference's 5, or the 527 / 1000 of the stock checkpoints it starts from).  The flat parameter
    layout is the param_shapes order (q, k, v weights adjacent), not the named_parameters() order."""

    def __init__(self, cfg, weights=None):
        super().__init__()
        self.cfg = cfg
        shapes = param_shapes(cfg)
        for k, shp in shapes.items():
            if weights is not None and k in weights:
                v = torch.as_tensor(np.asarray(weights[k]), dtype=torch.float32).reshape(shp).clone()
            elif k.endswith("layernorm.weight") or k.endswith("layernorm_before.weight") or k.endswith("layernorm_after.weight"):
                v = torch.ones(shp)
            elif k.endswith(".bias") or "token" in k or "position_embeddings" in k:
                v = torch.zeros(shp)
            else:
                v = torch.randn(shp) * 0.02          # HF initializer_range
            _set_param(self, k, v)
        self._names = list(shapes)
        self._hws = {}                # batch size -> head-only workspace (Encoder.head)
        self._criteria = {}           # problem type -> the criterion of forward(labels=...), built on first use
        self._inferred_problem_type = None      # what a labelled forward resolved cfg.problem_type to (reset_head)
        self.source_dir = None        # the directory from_pretrained read
        self.kernel_events = None
        # Dropout (cfg.hidden_dropout / cfg.attention_dropout, training mode only): every keep decision is a hash of
        # (dropout_seed, site, device-resident forward counter, element index) - no mask is stored, the backward
        # regenerates it, and a captured step draws fresh masks on every replay.  The default seed follows
        # torch.manual_seed; set_dropout_masks (tests) replaces the generator by explicit masks, keyed and shaped as in
        # dropout_sites(B).
        self.dropout_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        # GEMM / attention operand precision: "split" (default: fp32-grade on the fp16 matrix cores - every operand as
        # fp16 hi + lo planes, three MFMAs per product, csrc/gemm_sp.hip + attention_sp.hip; measured against float64
        # it is not worse than the exact-fp32 kernels and it passes the same parity bounds), "fp32" (exact-fp32 MFMA),
        # "bf16" (bf16 MFMA operands everywhere, fp32 accumulate: ~5e-3 logit drift) or "bf16_bwd" (fp32 forward -
        # logits unchanged - and bf16 operands for the backward products only).  EAV_ENCODER_PRECISION overrides.
        self.precision = os.environ.get("EAV_ENCODER_PRECISION", DEFAULT_PRECISION)
        # classification Linear: "auto" (default) takes eav_dense_wide_* above HEAD_NARROW_CLASSES classes and
        # eav_dense_softmax_* up to there, "wide" forces the former at any width (tests), "narrow" the latter - it raises
        # above HEAD_NARROW_CLASSES.  EAV_HEAD_ALGO overrides.
        self.head_algo = os.environ.get("EAV_HEAD_ALGO", "auto")
        # split mode: weight-gradient GEMMs on a side stream (see _wgrad_sp).  "auto" (default): two streams from 8192 token
        # rows per step on, one stream below - at the per-rank batches of a data-parallel group (ViT B = 16: 3152 rows) the
        # ~100 events / waits of the two-stream schedule cost more host time than the overlap returns (20.1 -> 13.1 ms;
        # AST B = 4 21.1 -> 16.8 ms; ViT B = 128 49.2 two streams / 51.3 one: tools/encoder_graph_step.py).  True / False pin it.
        self.overlap_wgrad = "auto"
        # split mode, backward GEMMs only (data and weight gradients): 3 = the fp32-grade three-term product (default),
        # 1 = the hi.hi term alone - operands rounded to fp16 under the planes' scales (11-bit mantissas; fp32
        # accumulation), i.e. classic fp16 mixed-precision gradients: 3e-4 relative gradient error instead of 3e-7, a
        # third of the backward's matrix work.  The forward - the logits - always runs on three terms.
        self.grad_terms = int(os.environ.get("EAV_GRAD_TERMS", "3"))
        # per-kind overrides of grad_terms (None: follow it): the weight-gradient products (their rounding stays in that
        # tensor's update) and the data-gradient products (their rounding travels down the layers) priced separately -
        # tools/encoder_trajectory.py, profiles/r05_term_budget.txt, r06_term_budget.txt.  wgrad_terms = 2 (round 6, opt-in):
        # hi_grad.hi_act + lo_grad.hi_act - the ACTIVATION operand rounded to fp16 (11-bit mantissa, random signs over >= 1576
        # tokens), the gradient operand and the accumulation at full split precision, the producers' a-priori gradient planes
        # still in use.  Weight-gradient error 2-4e-4 of the tensor's maximum (three terms: 1e-7); -20 % on the fc1 / fc2
        # weight gradients, -3.2 % (ViT B = 128) / -2.6 % (AST B = 8) on the step.  40 AdamW steps move the held-out logits by
        # 3.9e-5 (ViT) / 2.3e-5 (AST) at the reference's learning rate 5e-6, but by 5.8e-4 / 1.5e-4 at 5e-5 (three terms:
        # 3.6e-5 / 4.3e-5) - AdamW's early updates are ~lr x sign(g), so gradient rounding that flips near-zero elements is
        # amplified; outside the 3e-4 this repository holds trajectories to, hence not the default.
        self.wgrad_terms = int(os.environ["EAV_WGRAD_TERMS"]) if os.environ.get("EAV_WGRAD_TERMS") else None
        self.dgrad_terms = int(os.environ["EAV_DGRAD_TERMS"]) if os.environ.get("EAV_DGRAD_TERMS") else None
        # the same switch for the forward products (comparison only: 16-bit matrix operands everywhere - the logits then
        # move by a few 1e-3, outside north_star's bound; bench.py reports the leg beside the literal bf16 one)
        self.fwd_terms = int(os.environ.get("EAV_FWD_TERMS", "3"))
        # split mode: LayerNorm / fc1 write their consumers' operand planes (a-priori scales); EAV_FUSED_PLANES=0 for A/B runs
        self.fused_planes = os.environ.get("EAV_FUSED_PLANES", "1") != "0"
        # split mode, backward: fc2's data-gradient GEMM writes the planes of dact (and the partials of fc1's bias gradient)
        # itself, scaled by a bound of |dact| known before the launch - no fp32 dact, no conversion pass; EAV_FUSED_DACT=0
        self.fused_dact = os.environ.get("EAV_FUSED_DACT", "1") != "0"
        # split mode, forward: the fused attention writes its output as the o-proj planes itself (EAV_FUSED_AO=0 for A/B runs)
        self.fused_ao = os.environ.get("EAV_FUSED_AO", "1") != "0"
        # split mode, forward: the fused q/k/v projection writes the attention kernels' row planes itself (scale from a bound of
        # |qkv|), the per-head transposes are made from those planes - no fp32 qkv tensor (EAV_FUSED_QKV=0 for A/B runs)
        self.fused_qkv = os.environ.get("EAV_FUSED_QKV", "1") != "0"
        # split mode, backward: the attention backward writes dqkv as the planes of the q/k/v projection's gradient products
        # itself (scale from a rigorous bound of |dqkv|, eav_attn_dqkv_bound) and leaves the bias-gradient partials - no fp32
        # dqkv, no conversion pass (EAV_FUSED_DQKV=0 for A/B runs)
        self.fused_dqkv = os.environ.get("EAV_FUSED_DQKV", "1") != "0"
        # split mode, backward: the LayerNorm backward kernels write the residual-stream gradient they produce as operand
        # planes as well (scale from a rigorous bound, eav_layernorm_bwd_bound) and leave the bias-gradient partials of the
        # linear layer that consumes it - two conversion passes per layer disappear (EAV_FUSED_DH=0 for A/B runs)
        self.fused_dh = os.environ.get("EAV_FUSED_DH", "1") != "0"
        self._main = self._st = None  # the stream of the current launch sequence and its handle (_begin)
        self._side, self._aux, self._wgrad_done = None, None, {}
        self._part_busy, self._ring_pos = {}, {}
        self._wplanes = None          # split mode: the WeightPlanes of the GEMM weights
        self._phase = "fwd"
        self._scales_all = False
        # multi-GPU: called as hook(lo, hi) from inside the backward whenever flat_grad[lo:hi] is final
        self.grad_ready_hook = None
        # ViT, HF's forward(..., interpolate_pos_encoding=True): images of any size >= one patch, the position table resampled
        # to their patch grid (csrc/pos_interp.hip).  This attribute is the default of forward()'s argument - what
        # forward_batch, a captured step and the trainers run with.  The geometry (H, W, ny, nx, npatch, ntok) then belongs to
        # the forward, not to the model: _geo is that of the forward in flight (or of the one whose backward runs), cfg itself
        # - param_shapes, state_dict, save_pretrained - never changes.
        self.interpolate_pos_encoding = False
        # AST: clips of any length from one patch up to MAX_TOKENS tokens, input_values [B, T', mel], the position table
        # fitted along time (csrc/pos_time.hip; ast_length_geometry).  An attribute only: HF's AST forward has no such
        # argument, and forward()'s parameter list is HF's.
        self.variable_length = False
        self._active_geo = None       # None: the geometry of cfg
        if cfg.hidden % cfg.heads or (cfg.hidden // cfg.heads) % 4 or cfg.hidden % 4 or cfg.hidden > 1024:
            raise NotImplementedError("hidden size must be <= 1024, a multiple of 4, head_dim a multiple of 4")
        if cfg.ntok > MAX_TOKENS:
            raise NotImplementedError(f"at most {MAX_TOKENS} tokens")
        if not 1 <= cfg.num_labels <= HEAD_MAX_CLASSES:
            raise NotImplementedError(f"the classification head takes 1 .. HEAD_MAX_CLASSES = {HEAD_MAX_CLASSES} classes, "
                                      f"not {cfg.num_labels}")

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_pretrained(cls, model_path):
        """HF directory: config.json + model.safetensors (pytorch_model.bin accepted)."""
        cfg = config_from_hf(json.load(open(os.path.join(model_path, "config.json"))))
        st = os.path.join(model_path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.numpy import load_file
            raw = load_file(st)
        elif os.path.exists(os.path.join(model_path, "pytorch_model.bin")):
            raw = {k: v.numpy() for k, v in torch.load(os.path.join(model_path, "pytorch_model.bin"), map_location="cpu").items()}
        else:
            raise OSError(f"no model.safetensors / pytorch_model.bin under {model_path}")
        w = {normalise_key(k): v for k, v in raw.items()}
        shapes = param_shapes(cfg)
        missing = [k for k in shapes if k not in w]
        if missing:
            raise KeyError(f"checkpoint lacks {missing[:4]} ...")
        model = cls(cfg, w)
        model.source_dir = str(model_path)
        return model

    def save_pretrained(self, save_directory, max_length=None):
        """The inverse of from_pretrained: config.json (config_to_hf) and model.safetensors - state_dict() as it stands,
        HF 5.x key names, fp32, read from the parameters (views of the flat buffer: current after any number of optimiser
        steps; the fp16 operand planes are never read).  Works for a CPU- or device-resident model; the Hugging Face
        classes load the directory.  max_length (AST, an int): config.json gets that max_length and the position table is
        written fitted to it (pos_time.fit_time, on the host) - a stock HF AST of that length; None keeps the checkpoint's."""
        from safetensors.numpy import save_file
        shapes = param_shapes(self.cfg)
        hf = config_to_hf(self.cfg)
        geo = None
        if max_length is not None:
            geo = ast_length_geometry(self.cfg, max_length)          # (refuses a ViT and an inadmissible length)
            hf["max_length"] = geo.W
        os.makedirs(save_directory, exist_ok=True)
        sd = self.state_dict()
        assert sorted(sd) == sorted(shapes), set(sd) ^ set(shapes)
        tensors = {k: np.ascontiguousarray(sd[k].detach().cpu().numpy().reshape(shapes[k])) for k in shapes}
        if geo is not None and geo.time_grid is not None:
            key = f"{self.cfg.prefix}.embeddings.position_embeddings"
            fitted = pos_time.fit_time(tensors[key][0], geo.ny, geo.time_grid, geo.nx, geo.nextra)
            tensors[key] = np.ascontiguousarray(fitted.astype(np.float32)[None])
        save_file(tensors, os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(hf, f, indent=2)
            f.write("\n")

    def reset_head(self, weight, bias):
        """Replace the classification Linear (the reference does `classifier.dense = nn.Linear(768, n)`,
        Transformer_Audio.py:24 / `classifier = nn.Linear(...)`, Transformer_Vision.py:30)."""
        head = self.classifier.dense if self.cfg.kind == "ast" else self.classifier
        dev = head.weight.device
        weight = torch.as_tensor(weight, dtype=torch.float32)
        if not 1 <= weight.shape[0] <= HEAD_MAX_CLASSES:      # refused before anything is replaced
            raise NotImplementedError(f"the classification head takes 1 .. HEAD_MAX_CLASSES = {HEAD_MAX_CLASSES} classes, "
                                      f"not {weight.shape[0]}")
        head.weight = nn.Parameter(weight.clone().to(dev))
        head.bias = nn.Parameter(torch.as_tensor(bias, dtype=torch.float32).clone().to(dev))
        self.cfg.num_labels = head.weight.shape[0]
        self.cfg.id2label = None            # the checkpoint's names belonged to the head that just left
        # so did a problem type that a labelled forward inferred from that head's width; one set in the config or by the
        # caller stays
        if self._inferred_problem_type is not None and self.cfg.problem_type == self._inferred_problem_type:
            self.cfg.problem_type = None
        self._inferred_problem_type = None
        self._flat = None
        self._ws = None
        self._wss, self._hws = {}, {}

    def head_parameters(self):
        return list(self.classifier.parameters())

    # Anything that rewrites parameters wholesale drops the cached fp16 weight planes of the split path (the version key
    # in _refresh_weight_planes would catch these too; this makes it independent of how torch implements them).
    def invalidate_weight_planes(self):
        """Call after writing parameters in a way torch cannot see (`p.data.mul_(...)`, raw-pointer kernels): `.data`
        writes move neither the parameter's nor the flat buffer's version counter."""
        if self._wplanes is not None:
            self._wplanes.invalidate()

    def load_state_dict(self, *args, **kwargs):
        self.invalidate_weight_planes()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._wplanes = None
        self._ws = None
        self._wss, self._hws = {}, {}
        return super()._apply(fn, *args, **kwargs)

    def head_grad_ranges(self):
        """[(lo, hi)] element ranges of the classifier's gradients in the flat gradient buffer."""
        self._ensure_flat()
        offs = self._flat[2]
        return [(offs[k][0], offs[k][0] + offs[k][1]) for k in self._names if k.startswith("classifier.")]

    # ------------------------------------------------------------------ plumbing
    def _ensure_flat(self):
        p0 = next(self.parameters())
        ok = (self._flat is not None and getattr(p0, "_eav_flat", None) is not None
              and p0._eav_flat[0] is self._flat[0] and p0.data_ptr() == self._flat[0].data_ptr()
              and all(getattr(p, "_eav_flat", (None,))[0] is self._flat[0] for p in self.parameters()))
        if not ok:
            self._flat = flatten_parameters(self, order=self._names)
            self._pmap = dict(self.named_parameters())

    @property
    def _geo(self):
        """The geometry the launch functions read: cfg, or what interpolated_geometry / ast_length_geometry derived for the
        forward in flight."""
        return self._active_geo if self._active_geo is not None else self.cfg

    def forward(self, x=None, labels=None, pixel_values=None, input_values=None, interpolate_pos_encoding=None):
        x = x if x is not None else (pixel_values if pixel_values is not None else input_values)
        self._require_gpu(x)
        c = self.cfg
        interp = self.interpolate_pos_encoding if interpolate_pos_encoding is None else bool(interpolate_pos_encoding)
        varlen = bool(self.variable_length)
        geo = None
        if varlen and c.kind != "ast":
            raise NotImplementedError("variable_length exists for AST only (a ViT takes interpolate_pos_encoding)")
        if interp:
            if c.kind != "vit":
                raise NotImplementedError("interpolate_pos_encoding exists for ViT only (HF's AST takes no such argument)")
            if x.dim() != 4 or x.shape[1] != c.C:
                raise ValueError(f"expected input [B,{c.C},H,W], got {tuple(x.shape)}")
            if (x.shape[2], x.shape[3]) != (c.H, c.W):          # (the native size keeps cfg: today's launches, bit for bit)
                geo = interpolated_geometry(c, x.shape[2], x.shape[3])
                if self.training and self.dropout_active():
                    raise NotImplementedError("dropout at a non-native image size is not implemented (DESIGN.md section 11): "
                                              "the dropout sites are laid out for cfg.ntok tokens")
        elif varlen:
            if x.dim() != 3 or x.shape[2] != c.H:
                raise ValueError(f"expected input [B,T,{c.H}], got {tuple(x.shape)}")
            if x.shape[1] != c.W:                               # (the native length keeps cfg: today's launches, bit for bit)
                geo = ast_length_geometry(c, x.shape[1])
                if self.training and self.dropout_active():
                    raise NotImplementedError("dropout at a non-native clip length is not implemented (DESIGN.md section "
                                              "11): the dropout sites are laid out for cfg.ntok tokens")
        else:
            want = (c.W, c.H) if c.kind == "ast" else (c.C, c.H, c.W)
            if tuple(x.shape[1:]) != want:
                raise ValueError(f"expected input [B,{','.join(map(str, want))}], got {tuple(x.shape)}")
        self._active_geo = geo
        x = x.contiguous().float()
        self._ensure_flat()
        self._want_full = torch.is_grad_enabled() and any(
            p.requires_grad for k, p in self._pmap.items() if not k.startswith("classifier."))
        logits = KernelFn.apply(x, self, *[self._pmap[k] for k in self._names])
        loss = None
        if labels is not None:
            loss = self.criterion(labels)(logits, labels)
        return _Out(logits, loss)

    def criterion(self, labels=None):
        """The criterion of cfg.problem_type, held on the encoder: CrossEntropyLoss, BCEWithLogitsLoss or MSELoss
        (optim.py).  While the type is unset, `labels` resolve it as HF does (resolve_problem_type) and it is written into
        cfg.problem_type, where it stays - HF mutates its config in the same way."""
        c = self.cfg
        if c.problem_type is None:
            if labels is None:
                raise ValueError("Encoder.criterion: cfg.problem_type is unset and there are no labels to resolve it from")
            c.problem_type = self._inferred_problem_type = resolve_problem_type(c.num_labels, labels)
        if c.problem_type not in PROBLEM_TYPES:
            raise ValueError(f"problem_type {c.problem_type!r}: expected one of {PROBLEM_TYPES}")
        _check_single_label(c.problem_type, c.num_labels)
        if c.problem_type not in self._criteria:
            self._criteria[c.problem_type] = {"regression": MSELoss, "single_label_classification": CrossEntropyLoss,
                                              "multi_label_classification": BCEWithLogitsLoss}[c.problem_type]()
        return self._criteria[c.problem_type]

    def forward_batch(self, xs, ys, idx, optimizer):
        data, targets = gather_batch(xs, ys, idx)
        return self(data).logits, targets

    # ------------------------------------------------------------------ kernel schedule
    def _call(self, name, *args):
        ev = self.kernel_events
        if ev is not None and name in ev:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.call(name, *args)
            b.record()
            ev[name].append((a, b))
        else:
            _lib.call(name, *args)

    def _gemm(self, A, B, C, M, N, K, lda, ldb, ldc, tA=0, tB=0, batch=1, heads=1, sA=(0, 0), sB=(0, 0), sC=(0, 0),
              alpha=1.0, bias=None, gelu=0, pre=None, resid=None, ldr=0, acc=0):
        self._call(self._gemm_name(), A, B, C, M, N, K, lda, ldb, ldc, tA, tB, batch, heads, sA[0], sA[1], sB[0],
                   sB[1], sC[0], sC[1], float(alpha), bias, gelu, pre, resid, ldr, acc, self._st)

    def _fused_attention(self):
        """Flash-style fused attention kernels exist for head_dim 64 (AST, ViT-B); other head sizes take the
        materialised-score path (GEMM + softmax kernels).  `use_fused_attention = False` forces the latter."""
        return getattr(self, "use_fused_attention", True) and self.cfg.hidden // self.cfg.heads == 64

    # ------------------------------------------------------------------ dropout
    def dropout_active(self):
        """Whether a training-mode forward of this model drops anything."""
        return self.cfg.hidden_dropout > 0.0 or self.cfg.attention_dropout > 0.0

    def dropout_sites(self, B):
        """{site name: (site id, shape, probability)} of the dropout sites that exist for a batch of B, in HF's call order:
        "emb" [B, ntok, D] after tokens + position embeddings; per layer i "attn.i" [B, H, N, N] on the softmax
        probabilities, "attn_out.i" and "mlp_out.i" [B, N, D] on the o_proj / fc2 outputs before their residual adds."""
        c = self.cfg
        ph, pa = c.hidden_dropout, c.attention_dropout
        sites = {}
        if ph > 0.0:
            sites["emb"] = (0, (B, c.ntok, c.hidden), ph)
        for i in range(c.layers):
            if pa > 0.0:
                sites[f"attn.{i}"] = (1 + 3 * i, (B, c.heads, c.ntok, c.ntok), pa)
            if ph > 0.0:
                sites[f"attn_out.{i}"] = (2 + 3 * i, (B, c.ntok, c.hidden), ph)
                sites[f"mlp_out.{i}"] = (3 + 3 * i, (B, c.ntok, c.hidden), ph)
        return sites

    def _site_seed(self, site_id):
        return (int(self.dropout_seed) + ((site_id + 1) << 40)) & 0xFFFFFFFFFFFFFFFF

    def mix_dropout_rank(self, rank):
        """Data parallelism: give replica `rank` its own dropout stream (rank_dropout_seed)."""
        self.dropout_seed = rank_dropout_seed(self.dropout_seed, rank)

    def forward_counter(self):
        """Number of generator-mode dropout forwards so far (reads the device counter back)."""
        return 0 if self._fwd_counter is None else int(self._fwd_counter.item())

    def generated_dropout_masks(self, B, counter, seed=None):
        """The keep-masks the generator draws in the forward whose counter value is `counter` (the value
        forward_counter() returns after that forward), as set_dropout_masks takes them."""
        dev = next(self.parameters()).device
        cnt = torch.tensor(int(counter), dtype=torch.int64, device=dev)
        old = self.dropout_seed
        if seed is not None:
            self.dropout_seed = seed
        out = {}
        try:
            for name, (sid, shape, p) in self.dropout_sites(B).items():
                m = torch.empty(shape, dtype=torch.uint8, device=dev)
                _lib.call("eav_tf_dropout_mask", m.data_ptr(), m.numel(), float(p), self._site_seed(sid), cnt.data_ptr(),
                          _lib.stream_ptr())
                out[name] = m
        finally:
            self.dropout_seed = old
        return out

    def _begin_dropout(self, ws, B, dev):
        """Dropout state of this forward, kept on the workspace for its backward: probabilities (0 in eval mode), the
        explicit masks or the device counter (advanced here, by a launch)."""
        c = self.cfg
        ph, pa = (c.hidden_dropout, c.attention_dropout) if self.training else (0.0, 0.0)
        d = SimpleNamespace(ph=ph, pa=pa, masks=None, cnt=None)
        if ph > 0.0 or pa > 0.0:
            if self._dropout_masks is not None:
                d.masks = dict(self._dropout_masks)
                for name, (_, shape, _) in self.dropout_sites(B).items():
                    m = d.masks.get(name)
                    if not (isinstance(m, torch.Tensor) and m.dtype == torch.uint8 and m.device == dev
                            and tuple(m.shape) == shape and m.is_contiguous()):
                        raise _lib.EavError(f"set_dropout_masks: site {name!r} needs a contiguous uint8 mask {shape} on {dev}")
            else:
                d.cnt = self._counter(dev).data_ptr()
                self._call("eav_counter_inc", d.cnt, self._st)
        d.mk = (lambda name: d.masks[name].data_ptr()) if d.masks is not None else (lambda name: None)
        ws.drop = d
        return d

    def _drop_add(self, y, resid, out, n, p, site_id, name):
        """out = resid + Dropout(y) at a hidden-dropout site (resid None: the gate alone - the site's backward)."""
        d = self._ws.drop
        self._call("eav_tf_dropout_add", y, resid, out, n, float(p), self._site_seed(site_id), d.mk(name), d.cnt, self._st)

    def _gemm_name(self):
        p = self.precision
        if p not in ("fp32", "split", "bf16", "bf16_bwd"):
            raise ValueError(f"unknown precision {p!r}")
        low = p == "bf16" or (p == "bf16_bwd" and self._phase == "bwd")
        return "eav_gemm_bf16" if low else "eav_gemm_f32"

    def _alloc(self, B, dev, full_backward):
        c = self._geo
        D, FF, N, H, Lr = c.hidden, c.ff, c.ntok, c.heads, c.layers
        M = B * N
        ldn = (N + 3) // 4 * 4
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        sp = self.precision == "split"
        ws = SimpleNamespace(B=B, M=M, ldn=ldn, full=full_backward, sp=sp)
        nsave = Lr if full_backward else 1
        ws.col = f(B * c.npatch, c.kp)
        if getattr(c, "pos_grid", None) is not None or getattr(c, "time_grid", None) is not None:
            # the position table resampled (ViT) / fitted along time (AST) to this forward's patch grid
            ws.pos_i = f(N, D)
            if full_backward:                             # ... and the gradient eav_embed_bwd leaves for that table
                ws.dpos_i = f(N, D)
        ws.hs = [f(M, D) for _ in range(Lr + 1)] if full_backward else [f(M, D), f(M, D)]
        ws.y1 = [f(M, D) for _ in range(1 if sp else nsave)]     # split mode keeps planes, not fp32 copies
        ws.fused = self._fused_attention()
        # split mode + fused attention: the backward reads the fp16 planes of qkv, the fp32 tensor is transient
        ws.qkv = [f(M, 3 * D) for _ in range(1 if (sp and ws.fused) else nsave)]
        if sp:
            self._alloc_split(ws, dev, nsave)
        if ws.fused:      # flash-style kernels: only the log-sum-exp per (image, head, query) is kept
            ws.lse = [f(B * H, N) for _ in range(nsave)]
            ws.delta = f(B * H, N)
        else:
            ws.P = [torch.zeros(B * H, N, ldn, dtype=torch.float32, device=dev) for _ in range(nsave)]
            if c.attention_dropout > 0.0:     # the dropped probabilities of the current layer (P itself feeds the Jacobian)
                ws.Pd = torch.zeros(B * H, N, ldn, dtype=torch.float32, device=dev)
        ws.ao = [f(M, D) for _ in range(nsave)]
        ws.hmid = [f(M, D) for _ in range(nsave)]
        ws.y2 = [f(M, D) for _ in range(1 if sp else nsave)]
        ws.pre = [f(M, FF) for _ in range(nsave)]
        ws.act = [f(M, FF) for _ in range(1 if sp else nsave)]
        ws.st = [f(4, M) for _ in range(nsave)]           # mean1, rstd1, mean2, rstd2
        R = B * c.nextra
        ws.rows, ws.seqr, ws.stf = f(R, D), f(R, D), f(2, R)
        ws.pooled, ws.hl, ws.sth = f(B, D), f(B, D), f(2, B)
        ws.logits = f(B, c.num_labels)
        ws.head_ws = self._head_scratch(B, f)
        if full_backward:
            ws.dh, ws.dy, ws.dao = f(M, D), f(M, D), f(M, D)
            ws.dact, ws.dqkv = f(M, FF), f(M, 3 * D)
            if c.hidden_dropout > 0.0:        # dh o M / (1 - p): what enters the fc2 / o_proj gradient products
                ws.dhd = f(M, D)
            if not ws.fused:
                ws.dP = torch.zeros(B * H, N, ldn, dtype=torch.float32, device=dev)
            ws.demb = f(B * c.npatch, D)
            ws.np_ln = _lib.plain("eav_layernorm_bwd_nparts", M)
            ws.part_ln = f(ws.np_ln, 2 * D)
            ws.part_ln_pool = [ws.part_ln, f(ws.np_ln, 2 * D)]     # split path: see _part_buf
            ws.part_ln3_pool = [f(ws.np_ln, 3 * D) for _ in range(4)]   # ... with the bias-gradient section (fused_dh)
            ws.np_cs = _lib.plain("eav_colsum_nparts", M)
            ws.part_cs = f(ws.np_cs, max(FF, 3 * D))
            shapes = [(D, FF, M), (FF, D, M), (3 * D, D, M), (D, D, M), (D, c.kp, B * c.npatch)]
            plan = "eav_gemm_sp_splitk_plan" if sp else "eav_gemm_f32_splitk_plan"
            ws.splitk = f(max(_lib.plain(plan, m, n, k) * m * n for m, n, k in shapes))
        ws.drows, ws.dseqr = f(R, D), f(R, D)
        ws.dpooled, ws.dhl = f(B, D), f(B, D)
        ws.np_lnr = _lib.plain("eav_layernorm_bwd_nparts", R)
        ws.part_lnr = f(ws.np_lnr, 2 * D)
        return ws

    # ------------------------------------------------------------------ split-operand (fp16 hi/lo planes) plumbing
    FS, BS = 5, 8   # slots per layer: forward y1, qkv, ao, y2, act; backward dh(fc2), dact, dh(o), dao, dS, dqkv, dy(fc1), dy(qkv)

    def _alloc_split(self, ws, dev, nsave):
        c = self._geo
        D, FF, Lr, M = c.hidden, c.ff, c.layers, ws.M
        MP = ws.B * c.npatch
        kp = lambda k: _lib.plain("eav_sp_kpad", k)  # noqa: E731
        # Row planes only: the weight-gradient products contract over the ROWS (tokens) of the same planes the forward /
        # data-gradient products read (transposing LDS reads in gemm_sp.hip), so no transposed copy of any activation or
        # gradient exists.  Rows are padded to a multiple of 32 with zeros (contracted like real tokens; the conversion
        # never writes them).
        h = lambda r, k: torch.zeros((r + 31) // 32 * 32, 2 * kp(k), dtype=torch.float16, device=dev)  # noqa: E731
        full = ws.full
        ws.colp = h(MP, c.kp)
        ws.y1p = [h(M, D) for _ in range(nsave)]
        ws.aop = [h(M, D) for _ in range(nsave)]
        ws.y2p = [h(M, D) for _ in range(nsave)]
        ws.actp = [h(M, FF) for _ in range(nsave)]
        ws.fslots, ws.fslot = self._slots(1 + self.FS * Lr, dev)
        if ws.fused:   # attention operands: row planes of qkv and per-head transposed planes (csrc/attention_sp.hip)
            ws.qkvrow = [torch.empty(M, 6 * D, dtype=torch.float16, device=dev) for _ in range(nsave)]
        if full:
            # backward operands: one set, reused by every layer.  dh is converted twice per layer (fc2 and o_proj stage)
            # and its weight gradients run on the side stream, so the two uses must not share one buffer
            ws.dhp, ws.dhp2 = h(M, D), h(M, D)
            ws.dactp, ws.dqkvp = h(M, FF), h(M, 3 * D)
            ws.dembp = h(MP, D)
            ws.np_cs2 = _lib.plain("eav_sp_convert_colsum_nparts", M)
            ws.part_cs2 = torch.empty(ws.np_cs2, max(FF, 3 * D), dtype=torch.float32, device=dev)
            ws.part_cs2_pool = [ws.part_cs2] + [torch.empty_like(ws.part_cs2) for _ in range(3)]
            ws.np_attn = ws.B * ((c.ntok + 31) // 32)          # bias-gradient partials of the attention backward: one row per 32-token tile
            ws.part_attn_pool = [torch.zeros(ws.np_attn, 3 * D, dtype=torch.float32, device=dev) for _ in range(4)]
            ws.bslots, ws.bslot = self._slots(2 + self.BS * Lr, dev)
            if c.hidden_dropout > 0.0:        # measured scales of the two gated gradients of every layer
                ws.dslots, ws.dslot = self._slots(2 * Lr, dev)
            if ws.fused:
                ws.dorow = torch.empty(M, 2 * D, dtype=torch.float16, device=dev)

    @staticmethod
    def _slots(n, dev):
        """n zeroed scale slots ([n, SLOT] floats) and the device address of each."""
        table = torch.zeros(n, SLOT, dtype=torch.float32, device=dev)
        return table, [table.data_ptr() + 4 * SLOT * k for k in range(n)]

    def _weight_keys(self):
        """[(cache key, parameter name of the [out, in] matrix, out, in)] of every GEMM weight."""
        c = self.cfg
        keys = [("patch", f"{c.prefix}.embeddings.patch_embeddings.projection.weight", c.hidden, c.kp)]
        for i in range(c.layers):
            L = f"{c.prefix}.layers.{i}"
            keys += [(f"qkv{i}", f"{L}.attention.q_proj.weight", 3 * c.hidden, c.hidden),
                     (f"o{i}", f"{L}.attention.o_proj.weight", c.hidden, c.hidden),
                     (f"fc1{i}", f"{L}.mlp.fc1.weight", c.ff, c.hidden),
                     (f"fc2{i}", f"{L}.mlp.fc2.weight", c.hidden, c.ff)]
        return keys

    def _refresh_weight_planes(self, dev, need_T):
        """(Re)build the fp16 hi/lo planes of the GEMM weights (and of their transposes, for the data-gradient
        products) that changed: FusedAdam records the byte ranges it updated (`_eav_dirty`), any torch in-place write
        to the flat buffer (load_state_dict, .copy_) bumps its version and invalidates everything."""
        flat, offs = self._flat[0], self._flat[2]
        keys = self._weight_keys()
        wp = self._wplanes
        if wp is None or wp.dev != dev or (need_T and not wp.T):
            wp = self._wplanes = WeightPlanes([(k, 4 * offs[pn][0], out, inn) for k, pn, out, inn in keys],
                                              self.cfg.layers, dev, need_T)
            wp.main = self._main
        # Invalidation key: flatten_parameters rebinds p.data to views of the flat buffer, and a rebound .data has its
        # OWN version counter - load_state_dict, p.copy_/add_ under no_grad and torch.optim optimisers bump the
        # parameters' versions, never the flat buffer's.  So the key is the sum of the GEMM weights' versions (host-side,
        # ~50 attribute reads) plus the flat buffer's own version (flat.copy_ / flat.zero_ style writes);
        # load_state_dict / _apply also drop the cache outright.  FusedAdam writes through raw pointers (no version
        # moves): it reports the byte ranges it updated instead (`_eav_dirty`, recorded only because this model asked
        # for it through `_eav_track_dirty`).
        flat._eav_track_dirty = True
        versions = (flat._version, sum(self._pmap[pn]._version for _, pn, _, _ in keys))
        dirty, flat._eav_dirty = getattr(flat, "_eav_dirty", []), []
        stale = wp.stale(flat.data_ptr(), versions, dirty, need_T)
        # (the refresh goes to the side stream - idle during the forward - when this step runs on two streams)
        side = self._side_stream(dev) if (stale and self._two_streams() and self.kernel_events is None) else None
        wp.refresh(stale, flat.data_ptr(), versions, side)

    def _terms(self, kind):
        """MFMA terms of the backward products of `kind` ("dgrad" | "wgrad"): 3 = fp32-grade, 1 = hi.hi only; wgrad also 2 =
        hi.hi + lo_grad.hi_act (the activation operand rounded to fp16, the gradient operand at full split precision -
        the producers' a-priori gradient planes stay on)."""
        t = self.wgrad_terms if kind == "wgrad" else self.dgrad_terms
        return self.grad_terms if t is None else int(t)

    def _bwd_three_terms(self):
        """Every backward product on three terms: the producers may then write gradient planes under loose a-priori
        bounds (a hi.hi-only product needs the tight measured scale of its operands)."""
        return self._terms("dgrad") != 1 and self._terms("wgrad") != 1

    def _two_streams(self):
        """Whether this step runs its weight gradients / final reductions beside the main stream (overlap_wgrad)."""
        o = self.overlap_wgrad
        if o == "auto":
            return self._ws is not None and self._ws.B * self._geo.ntok >= 8192
        return bool(o)

    def _begin(self):
        """Head of every launch sequence (forward, backward, the head functions): look the current stream up once -
        torch.cuda.current_stream() costs tens of microseconds per call, and the step waits on ~50 events."""
        self._main = torch.cuda.current_stream()
        self._st = self._main.cuda_stream
        if self._wplanes is not None:
            self._wplanes.main = self._main
        return self._st

    def _to_planes(self, src, R, C, ld, slot, dst, amax_done=False):
        """fp32 [R, C] -> row planes (one set serves the products that contract over columns AND those over rows)."""
        if not amax_done:
            self._call("eav_sp_absmax", src, R, C, ld, slot, self._st)
        self._call("eav_sp_convert", src, R, C, ld, slot, _lib.ptr(dst), None, self._st)

    def _part_buf(self, pool):
        """Next buffer of a small ring of partial-sum buffers.  The final reductions of bias / LayerNorm parameter gradients
        are gradient OUTPUTS nothing downstream reads, so they run on the side stream (_reduce_async); the main stream
        waits for the reduction that last read a buffer only when the ring comes round to it (a layer later)."""
        ws = self._ws
        ring = getattr(ws, pool)
        i = self._ring_pos.get(pool, -1) + 1
        self._ring_pos[pool] = i = i % len(ring)
        ev = self._part_busy.pop(ring[i].data_ptr(), None)
        if ev is not None:
            self._main.wait_event(ev)
        return ring[i]

    def _reduce_async(self, buf, off_bytes, nparts, stride, n, out):
        """Final fixed-order reduction of a partial-sum buffer into a gradient nothing downstream reads: off the main stream.
        It gets its OWN stream (not the weight-gradient stream): a 24-block kernel queued in order between persistent GEMMs
        waits for a CU whose LDS is not taken by two GEMM workgroups, and held the weight gradients behind it back by
        ~130 us per launch at ViT B=128 (9.6 ms of side-stream time per step)."""
        if not (self._two_streams() and self.kernel_events is None):
            self._call("eav_reduce_partials", _lib.ptr(buf) + off_bytes, nparts, stride, n, 1.0, out, self._st)
            return
        if self._aux is None or self._aux.device != buf.device:
            self._aux = torch.cuda.Stream(device=buf.device)
        aux = self._aux
        ready = torch.cuda.Event()
        ready.record()
        aux.wait_event(ready)
        _lib.call("eav_reduce_partials", _lib.ptr(buf) + off_bytes, nparts, stride, n, 1.0, out, aux.cuda_stream)
        done = torch.cuda.Event()
        done.record(aux)
        self._part_busy[buf.data_ptr()] = done

    def _to_planes_bias(self, src, R, C, slot, dst, bias_grad):
        """Conversion pass that also produces the bias gradient (column sums of src) - src's max|x| is already in slot."""
        ws = self._ws
        self._before_overwrite(dst)
        part = self._part_buf("part_cs2_pool")
        self._call("eav_sp_convert_colsum", src, R, C, C, slot, _lib.ptr(dst), None, _lib.ptr(part), self._st)
        self._reduce_async(part, 0, ws.np_cs2, C, C, bias_grad)

    def _gemm_sp(self, A, slotA, B, slotB, C, M, N, K, ldc, batch=1, sA=0, sC=0, alpha=1.0, bias=None, gelu=0,
                 pre=None, resid=None, ldr=0, acc=0, amax=None, blockmax=True):
        """C[M,N] = epilogue(alpha A[M,K] . B[N,K]^T) on planes."""
        # flags: backward products with grad_terms = 1 run on the hi.hi term alone (see the class attribute); the backward's
        # data gradients share the GPU with the side stream's weight gradients (EAV_GEMM_SHARED_GPU: see csrc/gemm_sp.hip)
        bwd = self._phase == "bwd"
        flags = (1 if (self._terms("dgrad") if bwd else self.fwd_terms) == 1 else 0) | (2 if bwd and self._two_streams() else 0) \
            | (0 if blockmax else 8)
        self._call("eav_gemm_sp_ex", A, B, C, slotA, slotB, M, N, K, ldc, batch, sA, sC, float(alpha), bias, gelu, pre,
                   resid, ldr, acc, amax, None, None, None, flags, self._st)

    def _wgrad_sp(self, AT, slotA, BT, slotB, C, M, N, K):
        """C[M,N] = sum over the K tokens of A[t,m] B[t,n]: ROW planes of A [K,M] and B [K,N] (the contraction runs over the
        rows: eav_gemm_sp_splitk reads the fragments with transposing LDS loads); split-K.

        Weight gradients are off the critical path of the backward (nothing downstream reads them before the optimiser),
        so they run on a side HIP stream: their MFMA work fills the matrix pipe while the main stream is in its
        HBM- / VALU-bound stretches (operand conversions, LayerNorm / GELU backward, the attention backward) and in the
        tails of its own GEMMs.  Ordering: the side stream waits for the event recorded after the conversion that
        produced A; the main stream waits for a weight gradient only before it overwrites that gradient's A planes
        (one layer later) and at the end of the backward."""
        name = {1: "eav_gemm_sp_splitk_x1", 2: "eav_gemm_sp_splitk_x2"}.get(self._terms("wgrad"), "eav_gemm_sp_splitk")
        if not self._two_streams() or (self.kernel_events is not None and name in self.kernel_events):
            self._call(name, _lib.ptr(AT), _lib.ptr(BT), C, _lib.ptr(self._ws.splitk), slotA, slotB, M,
                       N, K, 0, self._st)
            return
        self._side_stream(AT.device)
        ready = torch.cuda.Event()
        ready.record()
        self._side.wait_event(ready)
        _lib.call(name, _lib.ptr(AT), _lib.ptr(BT), C, _lib.ptr(self._ws.splitk), slotA, slotB, M, N, K,
                  0, self._side.cuda_stream)
        done = torch.cuda.Event()
        done.record(self._side)
        self._wgrad_done[AT.data_ptr()] = done

    def _side_stream(self, dev):
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)
        return self._side

    def _before_overwrite(self, buf):
        """Main stream: the weight gradient that still reads `buf` (launched a layer ago on the side stream) must be
        finished before the next conversion overwrites it."""
        ev = self._wgrad_done.pop(buf.data_ptr(), None) if buf is not None else None
        if ev is not None:
            self._main.wait_event(ev)

    def _join_wgrads(self):
        if self._side is not None and self._wgrad_done:
            self._main.wait_stream(self._side)
            self._wgrad_done.clear()
        if self._aux is not None and self._part_busy:
            self._main.wait_stream(self._aux)
            self._part_busy.clear()

    # ------------------------------------------------------------------ classification head (shared by the full path
    # and by Encoder.head on cached features: same kernels, same arguments, hence bit-equal logits and gradients)
    def _head_wide(self):
        """Whether the classification Linear runs on eav_dense_wide_* (head_algo)."""
        algo, n = self.head_algo, self.cfg.num_labels
        if algo not in ("auto", "wide", "narrow"):
            raise ValueError(f"head_algo {algo!r}: expected 'auto', 'wide' or 'narrow'")
        if algo == "narrow" and n > HEAD_NARROW_CLASSES:
            raise NotImplementedError(f"head_algo 'narrow' takes at most {HEAD_NARROW_CLASSES} classes, the head has {n}")
        return algo == "wide" or (algo == "auto" and n > HEAD_NARROW_CLASSES)

    def _head_scratch(self, B, f):
        """The wide backward's class slices of d loss / d feat (None where the head kernels need no scratch)."""
        n = _lib.plain("eav_dense_wide_bwd_ws_floats", B, self.cfg.hidden, self.cfg.num_labels) if self._head_wide() else 0
        return f(n) if n else None

    def _dense_forward(self, feat, weight, bias, hw, B):
        c, P = self.cfg, _lib.ptr
        if self._head_wide():
            self._call("eav_dense_wide_fwd", P(feat), weight, bias, P(hw.logits), B, c.hidden, c.num_labels, self._st)
        else:
            self._call("eav_dense_softmax_fwd", P(feat), weight, bias, P(hw.logits), None, B, c.hidden, c.num_labels,
                       self._st)

    def _dense_backward(self, dlogits, feat, weight, dweight, dbias, dfeat, hw, B):
        c, P = self.cfg, _lib.ptr
        if self._head_wide():
            self._call("eav_dense_wide_bwd", P(dlogits), P(feat), weight, dweight, dbias, P(dfeat), P(hw.head_ws), B,
                       c.hidden, c.num_labels, self._st)
        else:
            self._call("eav_dense_softmax_bwd", P(dlogits), None, P(feat), weight, dweight, dbias, P(dfeat), B, c.hidden,
                       c.num_labels, self._st)

    def _head_forward(self, feat, hw, B):
        """feat [B, D] = the classifier's input (AST: mean of the cls / distillation rows after the final LayerNorm,
        HF modeling_audio_spectrogram_transformer.py ASTMLPHead; ViT: the cls row after the final LayerNorm)."""
        c, P, L, st = self.cfg, _lib.ptr, self._call, self._st
        D = c.hidden
        w = lambda k: P(self._pmap[k])  # noqa: E731
        if c.kind == "ast":
            sh = P(hw.sth)
            L("eav_layernorm_fwd", P(feat), w("classifier.layernorm.weight"), w("classifier.layernorm.bias"),
              P(hw.hl), sh, sh + 4 * B, B, D, c.eps, st)
            self._dense_forward(hw.hl, w("classifier.dense.weight"), w("classifier.dense.bias"), hw, B)
        else:
            self._dense_forward(feat, w("classifier.weight"), w("classifier.bias"), hw, B)

    def _head_backward(self, dlogits, feat, hw, B, need_dfeat):
        """Head gradients into the flat gradient buffer; d loss / d feat into hw.dpooled (AST) / hw.dseqr (ViT)."""
        c, P, L, st = self.cfg, _lib.ptr, self._call, self._st
        D = c.hidden
        gflat, offs = self._flat[1], self._flat[2]
        gp = lambda k: gflat.data_ptr() + 4 * offs[k][0]  # noqa: E731
        w = lambda k: P(self._pmap[k])  # noqa: E731
        if c.kind == "ast":
            self._dense_backward(dlogits, hw.hl, w("classifier.dense.weight"), gp("classifier.dense.weight"),
                                 gp("classifier.dense.bias"), hw.dhl, hw, B)
            sh = P(hw.sth)
            L("eav_layernorm_bwd", P(hw.dhl), P(feat), w("classifier.layernorm.weight"), sh, sh + 4 * B,
              P(hw.dpooled), 0, P(hw.part_lnr), B, D, st)
            self._reduce_gamma_beta(hw.part_lnr, _lib.plain("eav_layernorm_bwd_nparts", B),
                                    gp("classifier.layernorm.weight"), gp("classifier.layernorm.bias"))
        else:
            self._dense_backward(dlogits, feat, w("classifier.weight"), gp("classifier.weight"), gp("classifier.bias"),
                                 hw.dseqr, hw, B)

    def _head_ws(self, B, dev):
        hw = self._hws.get(B)
        if hw is None or hw.feat.device != dev or hw.logits.shape[1] != self.cfg.num_labels \
                or hw.wide != self._head_wide():
            c, D = self.cfg, self.cfg.hidden
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
            hw = self._hws[B] = SimpleNamespace(
                feat=f(B, D), hl=f(B, D), sth=f(2, B), logits=f(B, c.num_labels), dhl=f(B, D), dpooled=f(B, D),
                dseqr=f(B, D), part_lnr=f(_lib.plain("eav_layernorm_bwd_nparts", B * c.nextra), 2 * D), token=-1,
                head_ws=self._head_scratch(B, f), wide=self._head_wide())
        return hw

    def last_features(self):
        """The classifier's input of the most recent forward ([B, hidden], a copy): constant per sample while the backbone
        is frozen AND the model has no dropout (dropout_active() false - every dropout of the reference checkpoints is 0.0),
        which is what the trainers' frozen-phase feature cache stores (finetune.FineTuneBase)."""
        ws = self._ws
        if ws is None:
            raise _lib.EavError("Encoder.last_features: no forward has run")
        return (ws.pooled if self.cfg.kind == "ast" else ws.seqr[:ws.B]).clone()

    def head(self, feat):
        """Classifier on backbone features [B, hidden] (from last_features): logits with the head's autograd graph."""
        if not isinstance(feat, torch.Tensor) or not feat.is_cuda or feat.dim() != 2 or feat.shape[1] != self.cfg.hidden:
            raise _lib.EavError("Encoder.head: features must be a [batch, hidden] tensor on the ROCm device")
        self._ensure_flat()
        return _Out(_HeadFn.apply(feat.contiguous().float(), self, *[self._pmap[k] for k in self._names]))

    def _workspace_for(self, B, dev, full):
        """The workspace of a batch of B.  Three replaceable ones are kept (the full batch, a ragged last batch, an
        evaluation batch): the 5000 % 128 = 8 frames at the end of every vision epoch must not free and re-zero the 19 GB
        of the B = 128 one.  One allocated for a full backward also serves the no_grad forwards of its batch size; one
        without the backward's buffers is replaced when a full backward comes."""
        key = (B, str(dev), self._fused_attention(), self.precision == "split", self._head_wide(),
               (self._geo.H, self._geo.W))
        old = self._wss.get(key)
        if old is not None and full and not old.full:
            del self._wss[key]
            if getattr(old, "pinned", False):       # a captured graph still writes to it
                self._wss[key + ("head only",)] = old

        def make():
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.empty_cache()            # hand an evicted workspace's blocks back before taking new ones
            return self._alloc(B, dev, full)
        return self._workspace(key, make, keep_unpinned=3)

    def _launch_forward(self, x):
        c = self._geo
        P, L = _lib.ptr, self._call
        st = self._begin()
        self._phase = "fwd"
        B = x.shape[0]
        D, N = c.hidden, c.ntok
        full = self._want_full
        ws = self._workspace_for(B, x.device, full)
        sp = ws.sp
        drop = self._begin_dropout(ws, B, x.device)
        if sp:
            self._refresh_weight_planes(x.device, full)
            ws.fslots.zero_()
        pre = c.prefix
        w = lambda k: P(self._pmap[k])  # noqa: E731
        # patch embedding: im2col rows x projection weight -> token rows [nextra:], then cls/dist + positions
        L("eav_im2col", P(x), P(ws.col), B, c.C, c.H, c.W, c.patch, c.sy, c.sx, c.transposed, st)
        h0 = ws.hs[0]
        if sp:
            self._to_planes(P(ws.col), B * c.npatch, c.kp, c.kp, ws.fslot[0], ws.colp)
            wpl, wsl = self._wplanes.get("patch")
            self._gemm_sp(P(ws.colp), ws.fslot[0], wpl, wsl, P(h0) + 4 * c.nextra * D, c.npatch, D, c.kp, D, batch=B,
                          sA=c.npatch * 4 * _lib.plain("eav_sp_kpad", c.kp), sC=N * D,      # (plane row stride in bytes)
                          bias=w(f"{pre}.embeddings.patch_embeddings.projection.bias"))
        else:
            self._gemm(P(ws.col), w(f"{pre}.embeddings.patch_embeddings.projection.weight"),
                       P(h0) + 4 * c.nextra * D, c.npatch, D, c.kp, c.kp, c.kp, D, batch=B,
                       sA=(c.npatch * c.kp, 0), sC=(N * D, 0),
                       bias=w(f"{pre}.embeddings.patch_embeddings.projection.bias"))
        pos = w(f"{pre}.embeddings.position_embeddings")
        g = getattr(c, "pos_grid", None)
        if g is not None:
            tb = pos_interp.device_tables(g, c.ny, c.nx, x.device)
            L("eav_pos_bicubic_fwd", pos, P(ws.pos_i), g, c.ny, c.nx, D, c.nextra, *[P(t) for t in tb["fwd"]], st)
            pos = P(ws.pos_i)
        nx0 = getattr(c, "time_grid", None)
        if nx0 is not None:
            tb = pos_time.device_tables(nx0, c.nx, x.device)
            L("eav_pos_time_fwd", pos, P(ws.pos_i), c.ny, nx0, c.nx, D, c.nextra, *[P(t) for t in tb["fwd"]], st)
            pos = P(ws.pos_i)
        L("eav_embed_finish", P(h0), w(f"{pre}.embeddings.cls_token"),
          w(f"{pre}.embeddings.distillation_token") if c.kind == "ast" else None, pos, B, N, D, c.nextra, st)
        if drop.ph > 0.0:
            self._drop_add(P(h0), None, P(h0), ws.M * D, drop.ph, 0, "emb")
        scale = (D // c.heads) ** -0.5
        if sp and c.layers:
            self._forward_scales()
        layer = self._layer_forward_split if sp else self._layer_forward_f32
        for i in range(c.layers):
            j = i if ws.full else 0
            hin = ws.hs[i] if ws.full else ws.hs[i & 1]
            hout = ws.hs[i + 1] if ws.full else ws.hs[(i + 1) & 1]
            layer(i, j, hin, hout, f"{pre}.layers.{i}", P(ws.st[j]), scale)
        hlast = ws.hs[c.layers] if ws.full else ws.hs[c.layers & 1]
        R = B * c.nextra
        L("eav_token_rows", P(hlast), P(ws.rows), B, N, D, c.nextra, 0, st)
        sf = P(ws.stf)
        L("eav_layernorm_fwd", P(ws.rows), w(f"{pre}.layernorm.weight"), w(f"{pre}.layernorm.bias"), P(ws.seqr), sf,
          sf + 4 * R, R, D, c.eps, st)
        if c.kind == "ast":
            L("eav_pair_mean", P(ws.seqr), P(ws.pooled), B, D, 0, st)
        self._head_forward(ws.pooled if c.kind == "ast" else ws.seqr, ws, B)
        self._token += 1
        self._saved = (self._token, x, full, self._active_geo)
        return self._token

    def _layer_forward_f32(self, i, j, hin, hout, Lk, stp, scale):
        """One encoder layer on the exact-fp32 GEMM and attention kernels (precision "fp32"; _gemm_name: also bf16)."""
        c, ws = self._geo, self._ws
        P, L, st = _lib.ptr, self._call, self._st
        D, FF, N, H, M, B, ldn = c.hidden, c.ff, c.ntok, c.heads, ws.M, ws.B, ws.ldn
        hd = D // H
        drop = ws.drop
        w = lambda k: P(self._pmap[k])  # noqa: E731
        L("eav_layernorm_fwd", P(hin), w(f"{Lk}.layernorm_before.weight"), w(f"{Lk}.layernorm_before.bias"),
          P(ws.y1[j]), stp, stp + 4 * M, M, D, c.eps, st)
        qkv = P(ws.qkv[j])
        self._gemm(P(ws.y1[j]), w(f"{Lk}.attention.q_proj.weight"), qkv, M, 3 * D, D, D, D, 3 * D,
                   bias=w(f"{Lk}.attention.q_proj.bias"))
        if ws.fused and drop.pa > 0.0:
            L("eav_attn_fwd_dropout", qkv, P(ws.ao[j]), P(ws.lse[j]), B, H, N, hd, scale, drop.pa,
              self._site_seed(1 + 3 * i), drop.mk(f"attn.{i}"), drop.cnt, st)
        elif ws.fused:
            L("eav_attn_fwd", qkv, P(ws.ao[j]), P(ws.lse[j]), B, H, N, hd, scale, st)
        else:
            Pm = P(ws.P[j])
            self._gemm(qkv, qkv + 4 * D, Pm, N, N, hd, 3 * D, 3 * D, ldn, batch=B * H, heads=H,
                       sA=(N * 3 * D, hd), sB=(N * 3 * D, hd), sC=(H * N * ldn, N * ldn), alpha=scale)
            Pv = self._softmax_forward(i, Pm, B * H * N, N, ldn)
            self._gemm(Pv, qkv + 8 * D, P(ws.ao[j]), N, hd, N, ldn, 3 * D, D, tB=1, batch=B * H, heads=H,
                       sA=(H * N * ldn, N * ldn), sB=(N * 3 * D, hd), sC=(N * D, hd))
        # (hidden dropout sits between the bias and the residual add: the product leaves without the residual and one
        # element-wise pass forms resid + Dropout(product))
        hd_on = drop.ph > 0.0
        self._gemm(P(ws.ao[j]), w(f"{Lk}.attention.o_proj.weight"), P(ws.hmid[j]), M, D, D, D, D, D,
                   bias=w(f"{Lk}.attention.o_proj.bias"), resid=None if hd_on else P(hin), ldr=0 if hd_on else D)
        if hd_on:
            self._drop_add(P(ws.hmid[j]), P(hin), P(ws.hmid[j]), M * D, drop.ph, 2 + 3 * i, f"attn_out.{i}")
        L("eav_layernorm_fwd", P(ws.hmid[j]), w(f"{Lk}.layernorm_after.weight"), w(f"{Lk}.layernorm_after.bias"),
          P(ws.y2[j]), stp + 8 * M, stp + 12 * M, M, D, c.eps, st)
        self._gemm(P(ws.y2[j]), w(f"{Lk}.mlp.fc1.weight"), P(ws.act[j]), M, FF, D, D, D, FF,
                   bias=w(f"{Lk}.mlp.fc1.bias"), gelu=1, pre=P(ws.pre[j]))
        self._gemm(P(ws.act[j]), w(f"{Lk}.mlp.fc2.weight"), P(hout), M, D, FF, FF, FF, D,
                   bias=w(f"{Lk}.mlp.fc2.bias"), resid=None if hd_on else P(ws.hmid[j]), ldr=0 if hd_on else D)
        if hd_on:
            self._drop_add(P(hout), P(ws.hmid[j]), P(hout), M * D, drop.ph, 3 + 3 * i, f"mlp_out.{i}")

    def _softmax_forward(self, i, Pm, rows, N, ldn):
        """Materialised-score path: softmax in place over the scores of layer i; returns the operand of the P.V product -
        P itself, or with attention dropout the dropped probabilities (P stays undropped for the Jacobian)."""
        ws = self._ws
        d = ws.drop
        if d.pa > 0.0:
            self._call("eav_softmax_dropout_fwd", Pm, _lib.ptr(ws.Pd), rows, N, ldn, d.pa, self._site_seed(1 + 3 * i),
                       d.mk(f"attn.{i}"), d.cnt, self._st)
            return _lib.ptr(ws.Pd)
        self._call("eav_softmax_fwd", Pm, rows, N, ldn, self._st)
        return Pm

    def _attention_backward_scores(self, g, i, qkv, dao, dqkv, scale):
        """Materialised-score path, backward of the attention core of layer i with the batched product `g`: dV = Pd^T dO,
        dP = dO V^T, dS = softmax backward (in place over dP), dQ = s dS K, dK = s dS^T Q.  With attention dropout the
        softmax backward gates dP and regenerates the dropped probabilities Pd, so it runs before the dV product."""
        c, ws = self._geo, self._ws
        D, N, H = c.hidden, c.ntok, c.heads
        hd, ldn, B = D // H, ws.ldn, ws.B
        P, d = _lib.ptr, ws.drop
        Pm, dP = P(ws.P[i]), P(ws.dP)
        sP, sQ, sO = (H * N * ldn, N * ldn), (N * 3 * D, hd), (N * D, hd)
        if d.pa > 0.0:
            g(dao, qkv + 8 * D, dP, N, N, hd, D, 3 * D, ldn, batch=B * H, heads=H, sA=sO, sB=sQ, sC=sP)
            self._call("eav_softmax_dropout_bwd", Pm, dP, P(ws.Pd), B * H * N, N, ldn, d.pa, self._site_seed(1 + 3 * i),
                       d.mk(f"attn.{i}"), d.cnt, self._st)
            g(P(ws.Pd), dao, dqkv + 8 * D, N, hd, N, ldn, D, 3 * D, tA=1, tB=1, batch=B * H, heads=H, sA=sP, sB=sO, sC=sQ)
        else:
            g(Pm, dao, dqkv + 8 * D, N, hd, N, ldn, D, 3 * D, tA=1, tB=1, batch=B * H, heads=H, sA=sP, sB=sO, sC=sQ)
            g(dao, qkv + 8 * D, dP, N, N, hd, D, 3 * D, ldn, batch=B * H, heads=H, sA=sO, sB=sQ, sC=sP)
            self._call("eav_softmax_bwd", Pm, dP, B * H * N, N, ldn, self._st)
        g(dP, qkv + 4 * D, dqkv, N, hd, N, ldn, 3 * D, 3 * D, tB=1, batch=B * H, heads=H, sA=sP, sB=sQ, sC=sQ, alpha=scale)
        g(dP, qkv, dqkv + 4 * D, N, hd, N, ldn, 3 * D, 3 * D, tA=1, tB=1, batch=B * H, heads=H, sA=sP, sB=sQ, sC=sQ,
          alpha=scale)

    _SCALE_PARAMS = ("layernorm_before.weight", "layernorm_before.bias", "layernorm_after.weight", "layernorm_after.bias",
                     "mlp.fc1.bias", "attention.q_proj.bias")

    def _scale_offsets(self, i):
        """(offset of layer i's first parameter in the flat buffer, the offsets relative to it of the parameters
        eav_tf_forward_scales_qkv reads, in its argument order)."""
        offs, Lk = self._flat[2], f"{self.cfg.prefix}.layers.{i}"
        first = offs[f"{Lk}.attention.q_proj.weight"][0]
        return first, tuple(offs[f"{Lk}.{n}"][0] - first for n in self._SCALE_PARAMS)

    def _forward_scales(self):
        """A-priori operand scales (rigorous bounds: eav_tf_forward_scales_qkv) of y1, qkv, y2, act of EVERY layer in one
        launch - the flat parameter buffer lays the layers out identically.  Falls back to one launch per layer (inside
        _layer_forward_split) if it does not."""
        c, ws, wp = self.cfg, self._ws, self._wplanes
        self._scales_all = False
        if not (self.fused_planes and c.hidden % 8 == 0 and c.ff % 8 == 0):
            return
        first, rel = zip(*(self._scale_offsets(i) for i in range(c.layers)))
        stride = first[1] - first[0] if c.layers > 1 else 0
        if any(r != rel[0] for r in rel) or any(first[i] - first[0] != i * stride for i in range(c.layers)):
            return
        if wp.norm_ready is not None:              # the row norms come from the side-stream weight refresh
            self._main.wait_event(wp.norm_ready)
        self._call("eav_tf_forward_scales_qkv", _lib.ptr(self._flat[0]) + 4 * first[0], stride, c.layers, *rel[0],
                   c.hidden, c.ff, wp.wnorm_fc1.data_ptr(), wp.wnorm_qkv.data_ptr(), ws.fslot[1], self.FS * SLOT, 0, 3, 4,
                   1 if (self.fused_qkv and ws.fused) else -1, self._st)
        self._scales_all = True

    def _layer_forward_split(self, i, j, hin, hout, Lk, stp, scale):
        """One encoder layer with every projection on the split-operand GEMM; the attention core stays on the fp32
        kernels.  LayerNorm / attention / GELU outputs are converted to planes once (plus the transposed planes when
        a backward will follow); only the planes are kept per layer."""
        c, ws = self._geo, self._ws
        P, L, st = _lib.ptr, self._call, self._st
        D, FF, N, H, M = c.hidden, c.ff, c.ntok, c.heads, ws.M
        hd = D // H
        w = lambda k: P(self._pmap[k])  # noqa: E731
        s_y1, s_qkv, s_ao, s_y2, s_act = ws.fslot[1 + self.FS * i:1 + self.FS * (i + 1)]
        y, ao, act = ws.y1[0], ws.ao[j], ws.act[0]
        # Producers write the operand planes themselves where a rigorous bound of the tensor exists BEFORE it is computed
        # (LayerNorm outputs, the MLP's GELU output: eav_tf_forward_scales) - no fp32 copy, no measured maximum, no
        # conversion pass for y1, y2, act.  The attention output keeps the measured scale (its kernel emits max|O|).
        fusedp = self.fused_planes and D % 8 == 0 and FF % 8 == 0
        if fusedp:
            self._wplanes.get(f"fc1{i}")        # (waits for the side-stream refresh of this layer's fc1 planes / row norms)
            if not self._scales_all:
                first, rel = self._scale_offsets(i)
                L("eav_tf_forward_scales_qkv", P(self._flat[0]) + 4 * first, 0, 1, *rel, D, FF,
                  self._wplanes.wnorm_fc1.data_ptr() + 4 * i, self._wplanes.wnorm_qkv.data_ptr() + 4 * i, s_y1, 0, 0, 3, 4,
                  1 if (self.fused_qkv and ws.fused) else -1, st)
            L("eav_layernorm_fwd_planes", P(hin), w(f"{Lk}.layernorm_before.weight"), w(f"{Lk}.layernorm_before.bias"),
              None, P(ws.y1p[j]), s_y1, stp, stp + 4 * M, M, D, c.eps, st)
        else:
            L("eav_layernorm_fwd_amax", P(hin), w(f"{Lk}.layernorm_before.weight"), w(f"{Lk}.layernorm_before.bias"),
              P(y), stp, stp + 4 * M, M, D, c.eps, s_y1, st)
            self._to_planes(P(y), M, D, D, s_y1, ws.y1p[j], amax_done=True)
        qkv = P(ws.qkv[0 if ws.fused else j])
        wpl, wsl = self._wplanes.get(f"qkv{i}")
        qkvp = fusedp and self.fused_qkv and ws.fused
        if qkvp:
            # the projection writes the row planes of Q | K | V itself (lo without the 2^11 lift: the attention kernels' format,
            # scale = the bound eav_tf_forward_scales_qkv put into s_qkv); the per-head transposes (V^T for the forward; Q^T,
            # K^T for the backward) are a pure fp16 transposition of those planes
            L("eav_gemm_sp_ex", P(ws.y1p[j]), wpl, None, s_y1, wsl, M, 3 * D, D, 3 * D, 1, 0, 0, 1.0,
              w(f"{Lk}.attention.q_proj.bias"), 0, None, None, 0, 0, s_qkv, P(ws.qkvrow[j]), s_qkv, None,
              4 | 8 | (1 if self.fwd_terms == 1 else 0), st)      # (+ the MEASURED max|qkv| into the slot's shards: the
            #                                                         backward's bound of |dqkv| uses it, eav_attn_dqkv_bound)
        else:
            self._gemm_sp(P(ws.y1p[j]), s_y1, wpl, wsl, qkv, M, 3 * D, D, 3 * D, bias=w(f"{Lk}.attention.q_proj.bias"),
                          amax=s_qkv if ws.fused else None)
        if ws.fused:
            if not qkvp:
                # row planes of Q | K | V and the per-head transposes (V^T for the forward; Q^T, K^T for the backward)
                L("eav_attn_sp_prep", qkv, s_qkv, P(ws.qkvrow[j]), None, ws.B, N, 3 * D, D, 0, st)
            if ws.drop.pa > 0.0:
                # attention dropout: the DROP instantiation, fp32 output and its measured maximum (the o-proj planes come
                # from the conversion pass below) - the plane-writing form's scale |O| <= max|V| assumes rows of P sum to 1
                ws.delta_from_planes = False
                L("eav_attn_fwd_sp_dropout", P(ws.qkvrow[j]), s_qkv, P(ao), P(ws.lse[j]), s_ao, ws.B, H, N, hd, scale,
                  ws.drop.pa, self._site_seed(1 + 3 * i), ws.drop.mk(f"attn.{i}"), ws.drop.cnt, st)
            elif fusedp and self.fused_ao:
                # the attention output leaves as the planes of the o-proj products (scale: qkv's own, |O| <= max|V|); its
                # fp32 copy is written only when a backward will read it
                # (... and only by the unfused gradient flow: the fused one forms delta = dO . O from these planes)
                # (recorded on the workspace: the backward forms delta from ws.aop ONLY if THIS kernel wrote them - its
                # planes carry one tensor-wide scale; eav_sp_convert's planes below have per-row-block boosts)
                ws.delta_from_planes = self.fused_dqkv and self._bwd_three_terms()
                need_ao = ws.full and not ws.delta_from_planes
                L("eav_attn_fwd_sp_planes", P(ws.qkvrow[j]), None, s_qkv, P(ao) if need_ao else None,
                  P(ws.lse[j]), None, P(ws.aop[j]), s_ao, ws.B, H, N, hd, scale, st)
            else:
                ws.delta_from_planes = False
                L("eav_attn_fwd_sp", P(ws.qkvrow[j]), None, s_qkv, P(ao), P(ws.lse[j]), s_ao, ws.B, H, N, hd,
                  scale, st)
        else:
            ldn = ws.ldn
            Pm = P(ws.P[j])
            self._gemm_f32(qkv, qkv + 4 * D, Pm, N, N, hd, 3 * D, 3 * D, ldn, batch=ws.B * H, heads=H,
                           sA=(N * 3 * D, hd), sB=(N * 3 * D, hd), sC=(H * N * ldn, N * ldn), alpha=scale)
            Pv = self._softmax_forward(i, Pm, ws.B * H * N, N, ldn)
            self._gemm_f32(Pv, qkv + 8 * D, P(ao), N, hd, N, ldn, 3 * D, D, tB=1, batch=ws.B * H, heads=H,
                           sA=(H * N * ldn, N * ldn), sB=(N * 3 * D, hd), sC=(N * D, hd))
        if not (ws.fused and fusedp and self.fused_ao) or (ws.fused and ws.drop.pa > 0.0):
            self._to_planes(P(ao), M, D, D, s_ao, ws.aop[j], amax_done=ws.fused)
        wpl, wsl = self._wplanes.get(f"o{i}")
        # (hidden dropout: the product leaves without the residual, one element-wise pass forms resid + Dropout(product) - the
        # split GEMM's epilogue stays as it is)
        drop = ws.drop
        hd_on = drop.ph > 0.0
        self._gemm_sp(P(ws.aop[j]), s_ao, wpl, wsl, P(ws.hmid[j]), M, D, D, D, bias=w(f"{Lk}.attention.o_proj.bias"),
                      resid=None if hd_on else P(hin), ldr=0 if hd_on else D)
        if hd_on:
            self._drop_add(P(ws.hmid[j]), P(hin), P(ws.hmid[j]), M * D, drop.ph, 2 + 3 * i, f"attn_out.{i}")
        if fusedp:
            L("eav_layernorm_fwd_planes", P(ws.hmid[j]), w(f"{Lk}.layernorm_after.weight"),
              w(f"{Lk}.layernorm_after.bias"), None, P(ws.y2p[j]), s_y2, stp + 8 * M, stp + 12 * M, M, D, c.eps, st)
            wpl, wsl = self._wplanes.get(f"fc1{i}")
            # fc1: bias + erf-GELU in the epilogue; the pre-activation is kept (fp32) for the backward only, the
            # activation leaves as planes - it never exists in fp32
            self._call("eav_gemm_sp_ex", P(ws.y2p[j]), wpl, None, s_y2, wsl, M, FF, D, FF, 1, 0, 0, 1.0,
                       w(f"{Lk}.mlp.fc1.bias"), 1, P(ws.pre[j]) if ws.full else None, None, 0, 0, None, P(ws.actp[j]),
                       s_act, None, 1 if self.fwd_terms == 1 else 0, st)
        else:
            L("eav_layernorm_fwd_amax", P(ws.hmid[j]), w(f"{Lk}.layernorm_after.weight"),
              w(f"{Lk}.layernorm_after.bias"), P(y), stp + 8 * M, stp + 12 * M, M, D, c.eps, s_y2, st)
            self._to_planes(P(y), M, D, D, s_y2, ws.y2p[j], amax_done=True)
            wpl, wsl = self._wplanes.get(f"fc1{i}")
            # fc1 stores the PRE-activation only (kept per layer for the backward; a scratch buffer in the frozen phase)
            # and max|GELU|; the conversion applies the GELU while it splits - the activation never exists in fp32
            pre = P(ws.pre[j]) if ws.full else P(act)
            self._gemm_sp(P(ws.y2p[j]), s_y2, wpl, wsl, pre, M, FF, D, FF, bias=w(f"{Lk}.mlp.fc1.bias"), gelu=3,
                          amax=s_act)
            self._call("eav_sp_convert_gelu", pre, M, FF, FF, s_act, P(ws.actp[j]), None, self._st)
        wpl, wsl = self._wplanes.get(f"fc2{i}")
        self._gemm_sp(P(ws.actp[j]), s_act, wpl, wsl, P(hout), M, D, FF, D, bias=w(f"{Lk}.mlp.fc2.bias"),
                      resid=None if hd_on else P(ws.hmid[j]), ldr=0 if hd_on else D)
        if hd_on:
            self._drop_add(P(hout), P(ws.hmid[j]), P(hout), M * D, drop.ph, 3 + 3 * i, f"mlp_out.{i}")

    def _gemm_f32(self, A, B, C, M, N, K, lda, ldb, ldc, tA=0, tB=0, batch=1, heads=1, sA=(0, 0), sB=(0, 0),
                  sC=(0, 0), alpha=1.0):
        self._call("eav_gemm_f32", A, B, C, M, N, K, lda, ldb, ldc, tA, tB, batch, heads, sA[0], sA[1], sB[0], sB[1],
                   sC[0], sC[1], float(alpha), None, 0, None, None, 0, 0, self._st)

    def _layer_backward_split(self, i, Lk, stp, gp, scale):
        """Backward of one layer: dh (gradient w.r.t. the layer output, fp32) in ws.dh on entry, gradient w.r.t. the
        layer input on exit.  Every weight gradient is a split-K GEMM over the transposed planes; data gradients use
        the planes of the transposed weights."""
        c, ws = self._geo, self._ws
        P, L, st = _lib.ptr, self._call, self._st
        D, FF, N, H, M = c.hidden, c.ff, c.ntok, c.heads, ws.M
        hd = D // H
        w = lambda k: P(self._pmap[k])  # noqa: E731
        dh, dy, dao, dact, dqkv = P(ws.dh), P(ws.dy), P(ws.dao), P(ws.dact), P(ws.dqkv)
        s_y1, s_qkv, s_ao, s_y2, s_act = ws.fslot[1 + self.FS * i:1 + self.FS * (i + 1)]
        b_dh2, b_dact, b_dh1, b_dao, b_ds, b_dqkv, b_dy2, b_dy1 = ws.bslot[1 + self.BS * i:1 + self.BS * (i + 1)]
        b_below = ws.bslot[1 + self.BS * (i - 1)] if i > 0 else ws.bslot[0]     # max|dh| of the layer below (the embedding's)
        fdh = self.fused_dh and self._bwd_three_terms()      # (hi.hi-only gradient products need the tight measured scales)
        # Hidden dropout: the gradient entering the fc2 / o_proj products is dh o M / (1 - p) (the residual branch keeps dh).
        # The gate is a pass of its own into ws.dhd; the gated tensor gets its own MEASURED scale slot (s_dh2 / s_dh1) - the
        # producers' slots hold max|dh| of the ungated tensor, up to 1 / (1 - p) too small.  fused_dh is off on such a step:
        # the LayerNorm backward's planes (and their a-priori bound) are those of the ungated dh.
        drop = ws.drop
        hd_on = drop.ph > 0.0
        fdh = fdh and not hd_on
        s_dh2, s_dh1, g_dh = b_dh2, b_dh1, dh
        if hd_on:
            s_dh2, s_dh1, g_dh = ws.dslot[2 * i], ws.dslot[2 * i + 1], P(ws.dhd)
            self._drop_add(dh, None, g_dh, M * D, drop.ph, 3 + 3 * i, f"mlp_out.{i}")
            L("eav_sp_absmax", g_dh, M, D, D, s_dh2, st)
        # fc2: h_out = h_mid + act.W2^T + b2.  max|dh| is already in b_dh2 (left there by the producer of dh); every
        # conversion pass also yields the bias gradient of its tensor.  (fused_dh: the layer above's LayerNorm backward
        # already wrote these planes and the bias-gradient partials - only the top layer's dh comes from the head)
        if not (fdh and i < c.layers - 1):
            self._to_planes_bias(g_dh, M, D, s_dh2, ws.dhp, gp(f"{Lk}.mlp.fc2.bias"))
        self._wgrad_sp(ws.dhp, s_dh2, ws.actp[i], s_act, gp(f"{Lk}.mlp.fc2.weight"), D, FF, M)
        wpl, wsl = self._wplanes.get(f"fc2{i}", transposed=True)
        if self.fused_dact and FF % 8 == 0:
            # data gradient through fc2 and the GELU in one pass, result straight into the planes of dact: its scale comes
            # from |dact| = |(dh W2) gelu'(pre)| <= 1.13 sqrt(D) max|dh| max_j ||W2[:, j]||_2 (max|dh| is in b_dh2, the column
            # norms are refreshed with the weight planes); the epilogue also leaves fc1's bias-gradient partials
            L("eav_sp_bound_scale", b_dact, s_dh2, self._wplanes.wcolnorm_fc2.data_ptr() + 4 * i,
              1.13 * float(np.sqrt(D)), st)
            self._before_overwrite(ws.dactp)
            part = self._part_buf("part_cs2_pool")
            flags = (1 if self._terms("dgrad") == 1 else 0) | (2 if self._two_streams() else 0)
            L("eav_gemm_sp_ex", P(ws.dhp), wpl, None, s_dh2, wsl, M, FF, D, FF, 1, 0, 0, 1.0, None, 2, P(ws.pre[i]), None, 0,
              0, None, P(ws.dactp), b_dact, P(part), flags, st)
            self._reduce_async(part, 0, ws.np_cs2, FF, FF, gp(f"{Lk}.mlp.fc1.bias"))
        else:
            # ... the epilogue multiplies by gelu'(pre) and emits max|dact|; one conversion pass (planes + bias gradient)
            self._gemm_sp(P(ws.dhp), s_dh2, wpl, wsl, dact, M, FF, D, FF, gelu=2, pre=P(ws.pre[i]), amax=b_dact)
            self._to_planes_bias(dact, M, FF, b_dact, ws.dactp, gp(f"{Lk}.mlp.fc1.bias"))
        # fc1
        self._wgrad_sp(ws.dactp, b_dact, ws.y2p[i], s_y2, gp(f"{Lk}.mlp.fc1.weight"), FF, D, M)
        wpl, wsl = self._wplanes.get(f"fc1{i}", transposed=True)
        if fdh:
            self._gemm_sp(P(ws.dactp), b_dact, wpl, wsl, dy, M, D, FF, D, amax=b_dy2, blockmax=False)
            self._ln_bwd_planes(dy, P(ws.hmid[i]), w(f"{Lk}.layernorm_after.weight"), stp + 8 * M, stp + 12 * M, dh, b_dh1,
                                b_dh2, b_dy2, ws.dhp2, gp(f"{Lk}.layernorm_after.weight"), gp(f"{Lk}.layernorm_after.bias"),
                                gp(f"{Lk}.attention.o_proj.bias"), s_y2)
        else:
            self._gemm_sp(P(ws.dactp), b_dact, wpl, wsl, dy, M, D, FF, D)
            part = self._part_buf("part_ln_pool")
            L("eav_layernorm_bwd_amax", dy, P(ws.hmid[i]), w(f"{Lk}.layernorm_after.weight"), stp + 8 * M, stp + 12 * M, dh,
              1, P(part), M, D, b_dh1, st)
            self._reduce_ln(part, gp(f"{Lk}.layernorm_after.weight"), gp(f"{Lk}.layernorm_after.bias"))
            # o_proj
            if hd_on:
                self._drop_add(dh, None, g_dh, M * D, drop.ph, 2 + 3 * i, f"attn_out.{i}")
                L("eav_sp_absmax", g_dh, M, D, D, s_dh1, st)
            self._to_planes_bias(g_dh, M, D, s_dh1, ws.dhp2, gp(f"{Lk}.attention.o_proj.bias"))
        self._wgrad_sp(ws.dhp2, s_dh1, ws.aop[i], s_ao, gp(f"{Lk}.attention.o_proj.weight"), D, D, M)
        wpl, wsl = self._wplanes.get(f"o{i}", transposed=True)
        # (dao goes to the attention operand preparation: one scale per tensor, no row-block maxima needed)
        self._gemm_sp(P(ws.dhp2), s_dh1, wpl, wsl, dao, M, D, D, D, amax=b_dao if ws.fused else None, blockmax=False)
        # attention core
        if ws.fused:
            L("eav_attn_sp_prep", dao, b_dao, P(ws.dorow), None, ws.B, N, D, D, 0, st)
            # dqkv as planes straight from the attention backward, delta = dO . O from the planes of O - only when the
            # forward of THIS step wrote those planes with eav_attn_fwd_sp_planes (EAV_FUSED_AO=0 / EAV_FUSED_PLANES=0 runs
            # convert a fp32 O with per-row-block boosts the planes-delta kernel does not read); hi.hi-only gradient
            # products need the tight measured scale
            fused_bwd = bool(getattr(ws, "delta_from_planes", False)) and self.fused_dqkv and self._bwd_three_terms()
            if fused_bwd:
                self._before_overwrite(ws.dqkvp)
                part = self._part_buf("part_attn_pool")
                # (delta = dO . O from the planes of dO and of the attention output: no fp32 attention output in the step)
                L("eav_attn_bwd_sp_planes", P(ws.qkvrow[i]), None, P(ws.dorow), None, s_qkv, b_dao, b_ds,
                  None, None, P(ws.lse[i]), P(ws.delta), None, None, P(ws.dqkvp), b_dqkv, P(part), P(ws.aop[i]), s_ao,
                  ws.B, H, N, hd, scale, st)
                self._reduce_async(part, 0, ws.np_attn, 3 * D, 3 * D, gp(f"{Lk}.attention.q_proj.bias"))
            elif drop.pa > 0.0:
                # (fused_dqkv is off on such a step - delta_from_planes is false: fp32 dqkv, the conversion pass measures it)
                L("eav_attn_bwd_sp_dropout", P(ws.qkvrow[i]), P(ws.dorow), s_qkv, b_dao, b_ds, P(ws.ao[i]), dao,
                  P(ws.lse[i]), P(ws.delta), dqkv, b_dqkv, ws.B, H, N, hd, scale, drop.pa, self._site_seed(1 + 3 * i),
                  drop.mk(f"attn.{i}"), drop.cnt, st)
            else:
                L("eav_attn_bwd_sp", P(ws.qkvrow[i]), None, P(ws.dorow), None, s_qkv, b_dao, b_ds,
                  P(ws.ao[i]), dao, P(ws.lse[i]), P(ws.delta), dqkv, b_dqkv, ws.B, H, N, hd, scale, st)
        else:
            self._attention_backward_scores(self._gemm_f32, i, P(ws.qkv[i]), dao, dqkv, scale)
        # fused q/k/v projection
        if not ws.fused:
            self._call("eav_sp_absmax", dqkv, M, 3 * D, 3 * D, b_dqkv, st)
        if not (ws.fused and fused_bwd):
            self._to_planes_bias(dqkv, M, 3 * D, b_dqkv, ws.dqkvp, gp(f"{Lk}.attention.q_proj.bias"))
        self._wgrad_sp(ws.dqkvp, b_dqkv, ws.y1p[i], s_y1, gp(f"{Lk}.attention.q_proj.weight"), 3 * D, D, M)
        wpl, wsl = self._wplanes.get(f"qkv{i}", transposed=True)
        # the gradient w.r.t. this layer's input is the next (lower) layer's dh: leave its max in that layer's slot
        if fdh and i > 0:
            self._gemm_sp(P(ws.dqkvp), b_dqkv, wpl, wsl, dy, M, D, 3 * D, D, amax=b_dy1, blockmax=False)
            below = Lk.rsplit(".", 1)[0] + f".{i - 1}"
            self._ln_bwd_planes(dy, P(ws.hs[i]), w(f"{Lk}.layernorm_before.weight"), stp, stp + 4 * M, dh,
                                b_below, b_dh1, b_dy1, ws.dhp, gp(f"{Lk}.layernorm_before.weight"),
                                gp(f"{Lk}.layernorm_before.bias"), gp(f"{below}.mlp.fc2.bias"), s_y1)
        else:
            self._gemm_sp(P(ws.dqkvp), b_dqkv, wpl, wsl, dy, M, D, 3 * D, D)
            part = self._part_buf("part_ln_pool")
            L("eav_layernorm_bwd_amax", dy, P(ws.hs[i]), w(f"{Lk}.layernorm_before.weight"), stp, stp + 4 * M, dh, 1,
              P(part), M, D, b_below, st)
            self._reduce_ln(part, gp(f"{Lk}.layernorm_before.weight"), gp(f"{Lk}.layernorm_before.bias"))

    def _ln_bwd_planes(self, dy, x, gamma, mean, rstd, dh, slot_out, slot_old, slot_dy, planes, g_gamma, g_beta, g_bias,
                       slot_fwd):
        """LayerNorm backward, accumulated into dh, whose result ALSO leaves as the operand planes of the next gradient
        products (scale: the bound of eav_layernorm_bwd_bound - measured max|dh| before, max|dy|, max|gamma|, the forward's max
        rstd - formed inside the launch), with the bias-gradient partials of the linear layer that consumes dh: no conversion pass."""
        ws, D, M = self._ws, self.cfg.hidden, self._ws.M
        L, P = self._call, _lib.ptr
        self._before_overwrite(planes)
        part = self._part_buf("part_ln3_pool")
        L("eav_layernorm_bwd_planes", dy, x, gamma, mean, rstd, dh, 1, P(part), M, D, slot_out, P(planes), slot_old, slot_dy,
          slot_fwd, self._st)
        if g_beta == g_gamma + 4 * D:
            self._reduce_async(part, 0, ws.np_ln, 3 * D, 2 * D, g_gamma)
        else:
            self._reduce_async(part, 0, ws.np_ln, 3 * D, D, g_gamma)
            self._reduce_async(part, 4 * D, ws.np_ln, 3 * D, D, g_beta)
        self._reduce_async(part, 8 * D, ws.np_ln, 3 * D, D, g_bias)

    def _wgrad(self, A, B, C, M, N, K, lda, ldb):
        """C[M,N] = A^T.B for A stored [K,M], B stored [K,N] (weight gradient: contraction over tokens)."""
        self._call(self._gemm_name() + "_splitk", A, B, C, _lib.ptr(self._ws.splitk), M, N, K, lda, ldb, 1, 1, self._st)

    def _reduce_gamma_beta(self, part, nparts, g_gamma, g_beta):
        """LayerNorm weight / bias gradients from `part` ([nparts][2 D]: dgamma | dbeta partials), one launch each."""
        D = self.cfg.hidden
        self._call("eav_reduce_partials", _lib.ptr(part), nparts, 2 * D, D, 1.0, g_gamma, self._st)
        self._call("eav_reduce_partials", _lib.ptr(part) + 4 * D, nparts, 2 * D, D, 1.0, g_beta, self._st)

    def _reduce_ln(self, part, gw, gb):
        """LayerNorm weight / bias gradients from `part` ([np_ln][2 D]: dgamma | dbeta partials): one launch when the
        two gradients are neighbours in the flat buffer (they are: weight, then bias, D floats each)."""
        ws, D = self._ws, self.cfg.hidden
        if gb == gw + 4 * D:
            self._reduce_async(part, 0, ws.np_ln, 2 * D, 2 * D, gw)
        else:
            self._reduce_gamma_beta(part, ws.np_ln, gw, gb)

    def _bias_grad(self, dy_ptr, M, N, ld, out):
        ws = self._ws
        self._call("eav_colsum", dy_ptr, _lib.ptr(ws.part_cs), M, N, ld, self._st)
        self._call("eav_reduce_partials", _lib.ptr(ws.part_cs), ws.np_cs, N, N, 1.0, out, self._st)

    def _layer_backward_f32(self, i, Lk, stp, gp, scale):
        """Backward of one layer on the exact-fp32 kernels: ws.dh holds the gradient w.r.t. the layer output on entry, the
        gradient w.r.t. the layer input on exit."""
        c, ws = self._geo, self._ws
        P, L, st = _lib.ptr, self._call, self._st
        D, FF, N, H, M, B = c.hidden, c.ff, c.ntok, c.heads, ws.M, ws.B
        hd = D // H
        drop = ws.drop
        w = lambda k: P(self._pmap[k])  # noqa: E731
        dh, dy, dao, dact, dqkv = P(ws.dh), P(ws.dy), P(ws.dao), P(ws.dact), P(ws.dqkv)
        # fc2: h_out = h_mid + Dropout(act.W2^T + b2): the products see dh o M / (1 - p), the residual branch dh
        g_dh = dh
        if drop.ph > 0.0:
            g_dh = P(ws.dhd)
            self._drop_add(dh, None, g_dh, M * D, drop.ph, 3 + 3 * i, f"mlp_out.{i}")
        self._wgrad(g_dh, P(ws.act[i]), gp(f"{Lk}.mlp.fc2.weight"), D, FF, M, D, FF)
        self._bias_grad(g_dh, M, D, D, gp(f"{Lk}.mlp.fc2.bias"))
        self._gemm(g_dh, w(f"{Lk}.mlp.fc2.weight"), dact, M, FF, D, D, FF, FF, tB=1)
        L("eav_gelu_bwd", dact, P(ws.pre[i]), M * FF, st)
        # fc1
        self._wgrad(dact, P(ws.y2[i]), gp(f"{Lk}.mlp.fc1.weight"), FF, D, M, FF, D)
        self._bias_grad(dact, M, FF, FF, gp(f"{Lk}.mlp.fc1.bias"))
        self._gemm(dact, w(f"{Lk}.mlp.fc1.weight"), dy, M, D, FF, FF, D, D, tB=1)
        # layernorm_after: dh (now gradient w.r.t. h_mid) += LN backward
        L("eav_layernorm_bwd", dy, P(ws.hmid[i]), w(f"{Lk}.layernorm_after.weight"), stp + 8 * M,
          stp + 12 * M, dh, 1, P(ws.part_ln), M, D, st)
        self._reduce_gamma_beta(ws.part_ln, ws.np_ln, gp(f"{Lk}.layernorm_after.weight"), gp(f"{Lk}.layernorm_after.bias"))
        # o_proj
        if drop.ph > 0.0:
            self._drop_add(dh, None, g_dh, M * D, drop.ph, 2 + 3 * i, f"attn_out.{i}")
        self._wgrad(g_dh, P(ws.ao[i]), gp(f"{Lk}.attention.o_proj.weight"), D, D, M, D, D)
        self._bias_grad(g_dh, M, D, D, gp(f"{Lk}.attention.o_proj.bias"))
        self._gemm(g_dh, w(f"{Lk}.attention.o_proj.weight"), dao, M, D, D, D, D, D, tB=1)
        # attention core
        qkv = P(ws.qkv[i])
        if ws.fused and drop.pa > 0.0:
            L("eav_attn_bwd_dropout", qkv, P(ws.ao[i]), dao, P(ws.lse[i]), P(ws.delta), dqkv, B, H, N, hd, scale,
              drop.pa, self._site_seed(1 + 3 * i), drop.mk(f"attn.{i}"), drop.cnt, st)
        elif ws.fused:
            L("eav_attn_bwd", qkv, P(ws.ao[i]), dao, P(ws.lse[i]), P(ws.delta), dqkv, B, H, N, hd, scale, st)
        else:     # materialised scores, batched over (image, head)
            self._attention_backward_scores(self._gemm, i, qkv, dao, dqkv, scale)
        # fused q/k/v projection
        self._wgrad(dqkv, P(ws.y1[i]), gp(f"{Lk}.attention.q_proj.weight"), 3 * D, D, M, 3 * D, D)
        self._bias_grad(dqkv, M, 3 * D, 3 * D, gp(f"{Lk}.attention.q_proj.bias"))
        self._gemm(dqkv, w(f"{Lk}.attention.q_proj.weight"), dy, M, D, 3 * D, 3 * D, D, D, tB=1)
        L("eav_layernorm_bwd", dy, P(ws.hs[i]), w(f"{Lk}.layernorm_before.weight"), stp, stp + 4 * M, dh, 1,
          P(ws.part_ln), M, D, st)
        self._reduce_gamma_beta(ws.part_ln, ws.np_ln, gp(f"{Lk}.layernorm_before.weight"), gp(f"{Lk}.layernorm_before.bias"))

    def _trained_grads(self, full):
        """What a backward hands to autograd, in the order of the parameters the forward took: views of the flat
        gradient buffer for the trained parameters (the classifier alone unless `full`), None for the others."""
        g, pm = self._grad_views(), self._pmap
        return [g[k].view(pm[k].shape) if pm[k].requires_grad and (full or k.startswith("classifier.")) else None
                for k in self._names]

    def _launch_backward(self, dlogits, token):
        self._check_token(token)
        full, self._active_geo = self._saved[2], self._saved[3]       # the geometry of the forward this backward belongs to
        c = self._geo
        P, L = _lib.ptr, self._call
        st = self._begin()
        self._phase = "bwd"
        ws = self._ws
        B, M, sp = ws.B, ws.M, ws.sp
        D, N = c.hidden, c.ntok
        _, gflat, offs = self._flat
        gp = lambda k: gflat.data_ptr() + 4 * offs[k][0]  # noqa: E731
        pre = c.prefix
        R = B * c.nextra
        # ---- head
        self._head_backward(dlogits, ws.pooled if c.kind == "ast" else ws.seqr, ws, B, full)
        if c.kind == "ast" and full:
            L("eav_pair_mean", P(ws.dseqr), P(ws.dpooled), B, D, 1, st)
        if full:
            sf = P(ws.stf)
            L("eav_layernorm_bwd", P(ws.dseqr), P(ws.rows), P(self._pmap[f"{pre}.layernorm.weight"]), sf, sf + 4 * R,
              P(ws.drows), 0, P(ws.part_lnr), R, D, st)
            self._reduce_gamma_beta(ws.part_lnr, ws.np_lnr, gp(f"{pre}.layernorm.weight"), gp(f"{pre}.layernorm.bias"))
            ws.dh.zero_()
            L("eav_token_rows", P(ws.dh), P(ws.drows), B, N, D, c.nextra, 1, st)
            scale = (D // c.heads) ** -0.5
            dh = P(ws.dh)
            drop = ws.drop
            if sp and drop.ph > 0.0:
                ws.dslots.zero_()
            if sp:
                ws.bslots.zero_()
                # dh of the top layer comes from the head (token-row scatter): one pass for its maximum; every other dh
                # gets its maximum from the LayerNorm backward that produces it
                self._call("eav_sp_absmax", dh, M, D, D, ws.bslot[1 + self.BS * (c.layers - 1)], st)
            # ---- layers
            layer = self._layer_backward_split if sp else self._layer_backward_f32
            for i in reversed(range(c.layers)):
                Lk = f"{pre}.layers.{i}"
                layer(i, Lk, P(ws.st[i]), gp, scale)
                if self.grad_ready_hook is not None:   # layer i's parameters are one contiguous slice
                    self._join_wgrads()         # the layer's weight gradients must be complete before they travel
                    last = offs[f"{Lk}.mlp.fc2.bias"]
                    self.grad_ready_hook(offs[f"{Lk}.attention.q_proj.weight"][0], last[0] + last[1])
            # ---- embeddings ("emb" dropout: dh is final here, so its gate runs in place)
            if drop.ph > 0.0:
                self._drop_add(dh, None, dh, M * D, drop.ph, 0, "emb")
            g, nx0 = getattr(c, "pos_grid", None), getattr(c, "time_grid", None)
            if nx0 is not None:
                # AST at another length: the fitted table's gradient, then the adjoint of the fit (rows 0 and 1, the cls and
                # distillation positions, are copied - the token gradients below read the same values as ever)
                L("eav_embed_bwd", dh, P(ws.dpos_i), P(ws.demb), B, N, D, c.nextra, st)
                tb = pos_time.device_tables(nx0, c.nx, ws.dpos_i.device)
                L("eav_pos_time_bwd", P(ws.dpos_i), gp(f"{pre}.embeddings.position_embeddings"), c.ny, nx0, c.nx, D,
                  c.nextra, *[P(t) for t in tb["bwd"]], tb["nnz"], st)
            elif g is None:
                L("eav_embed_bwd", dh, gp(f"{pre}.embeddings.position_embeddings"), P(ws.demb), B, N, D, c.nextra, st)
            else:
                # the gradient of the RESAMPLED table first; the stored table's is its image under the adjoint operator
                # (row 0, the cls position, is copied - the cls-token gradient below reads the same values as ever)
                L("eav_embed_bwd", dh, P(ws.dpos_i), P(ws.demb), B, N, D, c.nextra, st)
                tb = pos_interp.device_tables(g, c.ny, c.nx, ws.dpos_i.device)
                L("eav_pos_bicubic_bwd", P(ws.dpos_i), gp(f"{pre}.embeddings.position_embeddings"), g, c.ny, c.nx, D,
                  c.nextra, *[P(t) for t in tb["bwd_y"]], tb["nnzy"], *[P(t) for t in tb["bwd_x"]], tb["nnzx"], st)
            gpos = gflat[offs[f"{pre}.embeddings.position_embeddings"][0]:]
            gflat[offs[f"{pre}.embeddings.cls_token"][0]:][:D].copy_(gpos[:D])
            if c.kind == "ast":
                gflat[offs[f"{pre}.embeddings.distillation_token"][0]:][:D].copy_(gpos[D:2 * D])
            MP = B * c.npatch
            if sp:
                # demb (the patch rows of dh) gets its own maximum pass: the slot layer 0's LayerNorm backward filled is
                # indexed by the rows of dh (cls / distillation rows included), and the per-row-block maxima must be the
                # converted tensor's own
                s_demb = ws.bslot[1 + self.BS * c.layers]
                self._to_planes(P(ws.demb), MP, D, D, s_demb, ws.dembp)
                self._wgrad_sp(ws.dembp, s_demb, ws.colp, ws.fslot[0],
                               gp(f"{pre}.embeddings.patch_embeddings.projection.weight"), D, c.kp, MP)
            else:
                self._wgrad(P(ws.demb), P(ws.col), gp(f"{pre}.embeddings.patch_embeddings.projection.weight"), D, c.kp,
                            MP, D, c.kp)
            self._call("eav_colsum", P(ws.demb), P(ws.part_cs), MP, D, D, st)
            self._call("eav_reduce_partials", P(ws.part_cs), _lib.plain("eav_colsum_nparts", MP), D, D, 1.0,
                       gp(f"{pre}.embeddings.patch_embeddings.projection.bias"), st)
        self._join_wgrads()          # side-stream weight gradients complete before autograd / the optimiser see them
        return self._trained_grads(full)


def ASTForAudioClassification(cfg=None, weights=None):
    return Encoder(cfg or make_config("ast"), weights)


def ViTForImageClassification(cfg=None, weights=None):
    return Encoder(cfg or make_config("vit"), weights)
