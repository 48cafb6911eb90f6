"""The AST / ViT encoder's configuration, free of any device: the HF config.json round trip, the parameter layout and key
names, the geometry of a forward at another image size / clip length, the problem type and the per-rank dropout seed.
Imports torch only (transformer.py re-exports every name)."""
from __future__ import annotations

from types import SimpleNamespace

import torch

# Classes the classification head takes: up to HEAD_NARROW_CLASSES (16, criteria.py) on eav_dense_softmax_* (the classes in
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


def patch_dropout_keep(npatch, p):
    """The number of patches a sample keeps of `npatch` under patch dropout `p`: timm.layers.PatchDropout's
    max(1, int(L * (1 - p)))."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"patch_dropout must satisfy 0 <= p < 1, got {p!r}")
    return max(1, int(int(npatch) * (1.0 - p)))


def patch_dropout_geometry(geo, p):
    """The geometry of a training forward under patch dropout `p` (timm.layers.PatchDropout), derived from the one it would
    have had - cfg itself, or what interpolated_geometry / ast_length_geometry made of it: a copy whose npatch is the kept
    count K = patch_dropout_keep(P, p) and whose ntok is nextra + K, which is what everything below the embeddings reads.
    The full grid stays beside them: H, W, ny, nx, pos_grid / time_grid are untouched (im2col and the position table are
    those of the full grid) and grid_npatch = P.  Pure: needs no device.  ValueError unless 0 <= p < 1,
    NotImplementedError for a full grid beyond MAX_TOKENS tokens."""
    P = int(geo.npatch)
    K = patch_dropout_keep(P, p)
    if P + geo.nextra > MAX_TOKENS:
        raise NotImplementedError(f"at most {MAX_TOKENS} tokens: the full grid gives {P + geo.nextra}")
    out = SimpleNamespace(**vars(geo))
    out.grid_npatch, out.npatch, out.ntok = P, K, geo.nextra + K
    return out


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
