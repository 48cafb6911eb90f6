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

This module is the public model, its loading and saving, the workspace and the two launch sequences.  The rest of the encoder:
encoder_config (what needs no device), encoder_layers (the two layer schedules), encoder_head (the classification head and
Encoder.head), encoder_dropout (the dropout sites and generator), encoder_outputs (output_attentions / output_hidden_states /
attention rollout), patch_keep (patch dropout: the plan of who is kept and its tables), encoder_drop_path (stochastic depth: the
rates and the per-sample scale table).
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import _lib, pos_interp, pos_time
from .criteria import BCEWithLogitsLoss, CrossEntropyLoss, MSELoss
from .encoder_config import (HEAD_MAX_CLASSES, MAX_TOKENS, PROBLEM_TYPES, _check_single_label,  # noqa: F401 (re-exported)
                             ast_length_geometry, config_from_hf, config_to_hf, interpolated_geometry, make_config,
                             normalise_key, param_shapes, patch_dropout_geometry, rank_dropout_seed, resolve_problem_type)
from .encoder_drop_path import EncoderDropPath
from .encoder_dropout import EncoderDropout
from .encoder_head import EncoderHead, _HeadFn
from .encoder_layers import Fp32Layers, SplitLayers
from .encoder_outputs import EncoderOutputs
from .optim import flatten_parameters
from .patch_keep import EncoderPatchKeep
from .runtime import KernelFn, KernelModule, gather_batch

DEFAULT_PRECISION = "split"


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
    def __init__(self, logits, loss=None, hidden_states=None, attentions=None):
        self.logits, self.loss = logits, loss
        self.hidden_states, self.attentions = hidden_states, attentions


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
        # it is not worse than the exact-fp32 kernels and it passes the same parity bounds) or "fp32" (exact-fp32 MFMA).
        # Comparison only, and only with the extras library: "bf16" (bf16 MFMA operands everywhere, fp32 accumulate: ~5e-3
        # logit drift) and "bf16_bwd" (fp32 forward - logits unchanged - and bf16 operands for the backward products only).
        # EAV_ENCODER_PRECISION overrides.
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
        # the two layer schedules (encoder_layers.py); a forward takes the one of `precision`, its backward the same one
        self._fp32, self._split = Fp32Layers(self), SplitLayers(self)
        # ... and the head, the dropout generator and the extra outputs (encoder_head.py, encoder_dropout.py, encoder_outputs.py)
        self._head, self._dropgen, self._outputs = EncoderHead(self), EncoderDropout(self), EncoderOutputs(self)
        self._wplanes = None          # split mode: the WeightPlanes of the GEMM weights
        self._phase = "fwd"
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
        # Patch dropout (timm.layers.PatchDropout), 0 <= p < 1: in training mode every sample keeps a random
        # K = max(1, int(P (1 - p))) of the P patches of the forward's grid, chosen after the position embedding; the readout
        # tokens always stay, evaluation sees every token.  The forward then runs at patch_dropout_geometry of the geometry
        # it would have had - the dropped patches leave before the projection (patch_keep.py, csrc/patch_keep.hip).  0 (the
        # default) and eval mode launch exactly what they always did.
        self.patch_dropout = 0.0
        self._patch_keep = EncoderPatchKeep(self)
        # Stochastic depth (timm.layers.DropPath, scale_by_keep), 0 <= r < 1: in training mode sample b drops the whole residual
        # branch of layer i with probability p_i = r i / (layers - 1), both branches with independent draws, the kept ones
        # scaled by 1 / (1 - p_i) (encoder_drop_path.py, csrc/drop_path.hip).  A per-sample mask has no token layout: it runs at
        # every geometry, with patch dropout too.  0 (the default), eval mode and every layer with p_i = 0 (always layer 0)
        # launch exactly what they always did.
        self.drop_path_rate = 0.0
        self._droppath = EncoderDropPath(self)
        # HF's model(..., output_attentions=, output_hidden_states=): these attributes are the defaults of those two keywords
        # of __call__ (HF: config.output_attentions / config.output_hidden_states; from_pretrained copies them from config.json)
        self.output_attentions = False
        self.output_hidden_states = False
        self._out_flags = (None, None)    # the two keywords of the call in flight (__call__)
        self._outs = None             # the forward in flight: what it is to collect beside the logits (encoder_outputs.Outputs)
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
        hf = json.load(open(os.path.join(model_path, "config.json")))
        cfg = config_from_hf(hf)
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
        model.output_attentions = bool(hf.get("output_attentions", False))
        model.output_hidden_states = bool(hf.get("output_hidden_states", False))
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
        self._drop_workspaces()

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

    def _drop_workspaces(self):
        self._ws = None
        self._wss, self._hws = {}, {}

    def _apply(self, fn, *args, **kwargs):
        self._wplanes = None
        self._drop_workspaces()
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

    def __call__(self, *args, output_attentions=None, output_hidden_states=None, **kwargs):
        """model(x, ..., output_attentions=None, output_hidden_states=None): forward()'s arguments plus HF's two output
        keywords (forward's own parameter list stays as it is: the two travel beside it; None: the attributes of the same
        names).  They add `hidden_states` - layers + 1 tensors [B, N, hidden]: the embedding output (after embedding dropout when active), then
        every layer's output, the last one WITHOUT the final LayerNorm, as HF returns them - and `attentions` - layers tensors
        [B, heads, N, N], the softmax probabilities - to the result; N is the token count of this forward.  Both are fresh
        fp32 allocations (one buffer each, returned as per-layer views), written on the model's stream inside the layer loop,
        and DETACHED from autograd: HF's versions carry gradients, these do not.  The logits, and a backward that follows,
        are bit for bit those of a forward without the flags.  With head_dim 64 the probabilities come from
        csrc/attn_probs.hip (the fused attention never stores them), otherwise they are copied out of the softmax buffer."""
        self._out_flags = (output_attentions, output_hidden_states)
        try:
            return super().__call__(*args, **kwargs)
        finally:
            self._out_flags, self._outs = (None, None), None

    def forward(self, x=None, labels=None, pixel_values=None, input_values=None, interpolate_pos_encoding=None):
        x = x if x is not None else (pixel_values if pixel_values is not None else input_values)
        self._require_gpu(x)
        c = self.cfg
        outs = self._outputs.request(*self._out_flags)
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
        pd = float(self.patch_dropout)
        if not 0.0 <= pd < 1.0:
            raise ValueError(f"patch_dropout must satisfy 0 <= p < 1, got {self.patch_dropout!r}")
        if self.training and pd > 0.0:
            if self.dropout_active():
                raise NotImplementedError("dropout together with patch dropout is not implemented (DESIGN.md section 11): the "
                                          "dropout sites are laid out for cfg.ntok tokens")
            geo = patch_dropout_geometry(geo if geo is not None else c, pd)
        if self._droppath.active() and self.dropout_active():       # (validates drop_path_rate whatever the mode)
            raise NotImplementedError("dropout together with drop path is not implemented (DESIGN.md section 11): stock "
                                      "checkpoints have hidden_dropout_prob = attention_probs_dropout_prob = 0")
        self._active_geo = geo
        x = x.contiguous().float()
        self._ensure_flat()
        self._want_full = torch.is_grad_enabled() and any(
            p.requires_grad for k, p in self._pmap.items() if not k.startswith("classifier."))
        self._outs = outs             # (_launch_forward allocates and fills what it asks for)
        logits = KernelFn.apply(x, self, *[self._pmap[k] for k in self._names])
        self._outs = None
        loss = None
        if labels is not None:
            loss = self.criterion(labels)(logits, labels)
        return _Out(logits, loss) if outs is None else _Out(logits, loss, *outs.result())

    def attention_rollout(self, x, as_grid=False, interpolate_pos_encoding=None):
        """Attention rollout (Abnar & Zuidema 2020) of the readout tokens, [B, N]: how much of each input token reaches the
        classifier through the attention layers, heads averaged, the residual stream counted as half of every layer.  From
        the top layer down r <- r (0.5 A_l + 0.5 I), A_l the head mean of layer l (head_dim 64: written by the
        attention-probability kernels themselves, no [B, heads, N, N] buffer exists; otherwise summed over the heads' slices
        of the softmax buffer), starting from the one-hot readout row - CLS for a ViT; CLS and the distillation token for
        AST, averaged at the end as the pooled feature is their mean.  Runs under no_grad in eval mode (the mode is
        restored).  as_grid: the patch tokens only, as the forward's patch grid [B, gy, gx]."""
        return self._outputs.rollout(x, as_grid, interpolate_pos_encoding)

    def criterion(self, labels=None):
        """The criterion of cfg.problem_type, held on the encoder: CrossEntropyLoss, BCEWithLogitsLoss or MSELoss
        (criteria.py).  While the type is unset, `labels` resolve it as HF does (resolve_problem_type) and it is written into
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
        return self._dropgen.sites(B)

    def mix_dropout_rank(self, rank):
        """Data parallelism: give replica `rank` its own dropout stream (rank_dropout_seed)."""
        self.dropout_seed = rank_dropout_seed(self.dropout_seed, rank)

    def forward_counter(self):
        """Number of generator-mode dropout forwards so far (reads the device counter back)."""
        return 0 if self._fwd_counter is None else int(self._fwd_counter.item())

    def generated_dropout_masks(self, B, counter, seed=None):
        """The keep-masks the generator draws in the forward whose counter value is `counter` (the value
        forward_counter() returns after that forward), as set_dropout_masks takes them."""
        return self._dropgen.generated_masks(B, counter, seed)

    def set_patch_keep(self, idx):
        """Testing hook, the twin of set_dropout_masks: explicit kept patches [B, K] (integers, every row ascending and
        unique, in [0, P) of the forward that uses them; K that forward's kept count) instead of the generated plan; None
        returns to generated plans.  Validated here, once - it reads the table back, so call it outside a capture."""
        self._patch_keep.set_table(idx)

    def generated_patch_keep(self, B, counter, seed=None):
        """The keep table [B, K] (int32) the plan draws in the forward whose counter value is `counter` (the value
        forward_counter() returns after that forward), at the geometry of the most recent patch-dropped forward - before
        any: cfg's under patch_dropout."""
        return self._patch_keep.generated(B, counter, seed)

    def last_patch_keep(self):
        """The keep table [B, K] (int32, a copy) of the most recent forward, which must have dropped patches."""
        ws = self._ws
        if ws is None or getattr(ws, "keep", None) is None:
            raise _lib.EavError("Encoder.last_patch_keep: the most recent forward dropped no patches")
        return ws.keep.clone()

    def drop_path_rates(self):
        """The drop probability of every layer's two residual branches under drop_path_rate: float32 [layers],
        torch.linspace(0, r, layers) formed in float64 and rounded once."""
        return self._droppath.rates()

    def set_drop_path_masks(self, mask):
        """Testing hook, the twin of set_dropout_masks: an explicit keep table uint8 [layers, 2, B] on the model's device
        ([i, 0] the attention branch of layer i, [i, 1] its MLP branch; rows of layers with p_i = 0 are not read) instead of
        the generated draws; None returns to them.  Validated here, once - call it outside a capture."""
        self._droppath.set_masks(mask)

    def generated_drop_path(self, B, counter, seed=None):
        """The keep table uint8 [layers, 2, B] the generator draws in the forward whose counter value is `counter` (the
        value forward_counter() returns after that forward); rows of layers with p_i = 0 are all ones."""
        return self._droppath.generated(B, counter, seed)

    def last_drop_path(self):
        """The scale table float32 [layers, 2, B] (a copy) of the most recent forward, which must have run with drop path:
        0 where a branch was dropped, 1 / (1 - p_i) where it was kept, 1 in the rows of layers with p_i = 0."""
        ws = self._ws
        if ws is None or getattr(ws, "dpath", None) is None:
            raise _lib.EavError("Encoder.last_drop_path: the most recent forward ran without drop path")
        return ws.dpath.table.clone()

    def _path_add(self, y, resid, out, layer, branch):
        """out = resid + s o y with the per-sample scales of (layer, branch); resid None: the gate alone, the site's backward."""
        ws = self._ws
        self._call("eav_drop_path_add", y, resid, out, ws.dpath.row(layer, branch), ws.B, self._geo.ntok * self._geo.hidden,
                   self._st)

    def _drop_add(self, y, resid, out, n, kind, layer=0):
        """out = resid + Dropout(y) at the hidden-dropout site (kind, layer); resid None: the gate alone, the site's backward."""
        self._call("eav_tf_dropout_add", y, resid, out, n, *self._ws.drop.site(kind, layer), self._st)

    @staticmethod
    def _fitted(c):
        """(pos_grid, time_grid) of a geometry: what its position table is fitted from (ViT: interpolated_geometry; AST:
        ast_length_geometry); None, None for cfg itself and wherever the stored table serves as it is."""
        return getattr(c, "pos_grid", None), getattr(c, "time_grid", None)

    @staticmethod
    def _grid(c):
        """The patch count of the full grid of a patch-dropped geometry (patch_dropout_geometry: c.npatch of them are
        kept); None for every other geometry."""
        return getattr(c, "grid_npatch", None)

    def _alloc(self, B, dev, full_backward, lay):
        c = self._geo
        D, FF, N, H, Lr = c.hidden, c.ff, c.ntok, c.heads, c.layers
        M = B * N
        ldn = (N + 3) // 4 * 4
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        ws = SimpleNamespace(B=B, M=M, ldn=ldn, full=full_backward, layers=lay, fused=self._fused_attention())
        nsave = Lr if full_backward else 1
        ws.col = f(B * c.npatch, c.kp)
        grid = self._grid(c)
        ws.keep = None                        # patch dropout: the forward's keep table (its own buffer or an explicit one)
        if grid is not None:
            ws.keep_own, ws.inv = self._patch_keep.buffers(c, B, dev)
        if self._fitted(c) != (None, None):
            # the position table resampled (ViT) / fitted along time (AST) to this forward's patch grid
            Np = N if grid is None else c.nextra + grid
            ws.pos_i = f(Np, D)
            if full_backward:                             # ... and the gradient eav_embed_bwd leaves for that table
                ws.dpos_i = f(Np, D)
        ws.hs = [f(M, D) for _ in range(Lr + 1)] if full_backward else [f(M, D), f(M, D)]
        keep = lay.fp32_copies(nsave)         # of y1, y2, act (and qkv under the fused attention): split mode keeps planes
        ws.y1 = [f(M, D) for _ in range(keep)]
        ws.qkv = [f(M, 3 * D) for _ in range(keep if ws.fused else nsave)]
        lay.alloc(ws, dev, nsave)             # the split path's planes and slots
        if ws.fused:      # flash-style kernels: only the log-sum-exp per (image, head, query) is kept
            ws.lse = [f(B * H, N) for _ in range(nsave)]
            ws.delta = f(B * H, N)
        else:
            ws.P = [torch.zeros(B * H, N, ldn, dtype=torch.float32, device=dev) for _ in range(nsave)]
            if c.attention_dropout > 0.0:     # the dropped probabilities of the current layer (P itself feeds the Jacobian)
                ws.Pd = torch.zeros(B * H, N, ldn, dtype=torch.float32, device=dev)
        ws.ao = [f(M, D) for _ in range(nsave)]
        ws.hmid = [f(M, D) for _ in range(nsave)]
        ws.y2 = [f(M, D) for _ in range(keep)]
        ws.pre = [f(M, FF) for _ in range(nsave)]
        ws.act = [f(M, FF) for _ in range(keep)]
        ws.st = [f(4, M) for _ in range(nsave)]           # mean1, rstd1, mean2, rstd2
        R = B * c.nextra
        ws.rows, ws.seqr, ws.stf = f(R, D), f(R, D), f(2, R)
        ws.pooled = f(B, D)
        vars(ws).update(self._head.buffers(B, f, False))  # hl, sth, logits, head_ws
        if full_backward:
            ws.dh, ws.dy, ws.dao = f(M, D), f(M, D), f(M, D)
            ws.dact, ws.dqkv = f(M, FF), f(M, 3 * D)
            # dh o M / (1 - p): what enters the fc2 / o_proj gradient products (drop path allocates its own on first use)
            ws.dhd = f(M, D) if c.hidden_dropout > 0.0 else None
            if not ws.fused:
                ws.dP = torch.zeros(B * H, N, ldn, dtype=torch.float32, device=dev)
            ws.demb = f(B * c.npatch, D)
            ws.np_ln = _lib.plain("eav_layernorm_bwd_nparts", M)
            ws.part_ln = f(ws.np_ln, 2 * D)
            ws.part_ln_pool = [ws.part_ln, f(ws.np_ln, 2 * D)]     # split path: rings of partial sums, SideStreams.part_buf
            ws.part_ln3_pool = [f(ws.np_ln, 3 * D) for _ in range(4)]   # ... with the bias-gradient section (fused_dh)
            ws.np_cs = _lib.plain("eav_colsum_nparts", M)
            ws.part_cs = f(ws.np_cs, max(FF, 3 * D))
            shapes = [(D, FF, M), (FF, D, M), (3 * D, D, M), (D, D, M), (D, c.kp, B * c.npatch)]
            ws.splitk = f(max(_lib.plain(lay.SPLITK_PLAN, m, n, k) * m * n for m, n, k in shapes))
        ws.drows = f(R, D)
        vars(ws).update(self._head.buffers(B, f, True))   # dseqr, dpooled, dhl, part_lnr
        ws.np_lnr = _lib.plain("eav_layernorm_bwd_nparts", R)
        return ws

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

    def _two_streams(self):
        """Whether this step runs its weight gradients / final reductions beside the main stream (overlap_wgrad)."""
        o = self.overlap_wgrad
        if o == "auto":
            return self._ws is not None and self._ws.B * self._geo.ntok >= 8192
        return bool(o)

    def _join_wgrads(self):
        """Main stream: wait for what the split path put on its side streams."""
        self._split.streams.join()

    def _w(self, k):
        """Device address of parameter k."""
        return self._pmap[k].data_ptr()

    def _gp(self, k):
        """Device address of parameter k's gradient in the flat gradient buffer (whose address _begin looked up)."""
        return self._gbase + 4 * self._goffs[k][0]

    def _reduce_ln(self, part, nparts, g_gamma, g_beta, joint=None):
        """LayerNorm weight / bias gradients from `part` ([nparts][2 D]: dgamma | dbeta partials), one launch each - or,
        given the split path's `joint` reduction (SideStreams.reduce), ONE launch beside the main stream when the two
        gradients are neighbours in the flat buffer (they are: weight, then bias, D floats each)."""
        D = self.cfg.hidden
        if joint is not None and g_beta == g_gamma + 4 * D:
            joint(part, 0, nparts, 2 * D, 2 * D, g_gamma)
            return
        self._call("eav_reduce_partials", _lib.ptr(part), nparts, 2 * D, D, 1.0, g_gamma, self._st)
        self._call("eav_reduce_partials", _lib.ptr(part) + 4 * D, nparts, 2 * D, D, 1.0, g_beta, self._st)

    def _begin(self):
        """Head of every launch sequence (forward, backward, the head functions): look the current stream up once -
        torch.cuda.current_stream() costs tens of microseconds per call, and the step waits on ~50 events."""
        self._main = torch.cuda.current_stream()
        self._st = self._main.cuda_stream
        self._gbase, self._goffs = self._flat[1].data_ptr(), self._flat[2]
        if self._wplanes is not None:
            self._wplanes.main = self._main
        return self._st

    # ------------------------------------------------------------------ classification head (encoder_head.py)
    def _head_wide(self):
        """Whether the classification Linear runs on eav_dense_wide_* (head_algo)."""
        return self._head.wide()

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

    def _workspace_for(self, B, dev, full, lay):
        """The workspace of a batch of B.  Three replaceable ones are kept (the full batch, a ragged last batch, an
        evaluation batch): the 5000 % 128 = 8 frames at the end of every vision epoch must not free and re-zero the 19 GB
        of the B = 128 one.  One allocated for a full backward also serves the no_grad forwards of its batch size; one
        without the backward's buffers is replaced when a full backward comes."""
        key = (B, str(dev), self._fused_attention(), lay.split, self._head_wide(),
               (self._geo.H, self._geo.W), self._geo.npatch if self._grid(self._geo) is not None else None)
        old = self._wss.get(key)
        if old is not None and full and not old.full:
            del self._wss[key]
            if getattr(old, "pinned", False):       # a captured graph still writes to it
                self._wss[key + ("head only",)] = old

        def make():
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.empty_cache()            # hand an evicted workspace's blocks back before taking new ones
            return self._alloc(B, dev, full, lay)
        return self._workspace(key, make, keep_unpinned=3)

    def _fit_positions(self, pos, ws):
        """The position table this forward adds, given the stored one (device addresses): the stored table itself, or
        ws.pos_i after resampling it to the forward's patch grid (ViT, pos_grid: bicubic, pos_interp) / fitting it along
        time (AST, time_grid: pos_time)."""
        c, P = self._geo, _lib.ptr
        g, nx0 = self._fitted(c)
        if g is not None:
            tb = pos_interp.device_tables(g, c.ny, c.nx, ws.pos_i.device)
            self._call("eav_pos_bicubic_fwd", pos, P(ws.pos_i), g, c.ny, c.nx, c.hidden, c.nextra,
                       *[P(t) for t in tb["fwd"]], self._st)
        elif nx0 is not None:
            tb = pos_time.device_tables(nx0, c.nx, ws.pos_i.device)
            self._call("eav_pos_time_fwd", pos, P(ws.pos_i), c.ny, nx0, c.nx, c.hidden, c.nextra,
                       *[P(t) for t in tb["fwd"]], self._st)
        else:
            return pos
        return P(ws.pos_i)

    def _fit_positions_backward(self, ws, gpos):
        """The adjoint of _fit_positions: the gradient of the fitted table (ws.dpos_i, left by eav_embed_bwd) into the stored
        table's gradient `gpos`.  The rows of the extra tokens are copied (ViT: row 0, the cls position; AST: rows 0 and 1,
        cls and distillation) - the token gradients read the same values as at the native size."""
        c, P = self._geo, _lib.ptr
        g, nx0 = self._fitted(c)
        if nx0 is not None:
            tb = pos_time.device_tables(nx0, c.nx, ws.dpos_i.device)
            self._call("eav_pos_time_bwd", P(ws.dpos_i), gpos, c.ny, nx0, c.nx, c.hidden, c.nextra,
                       *[P(t) for t in tb["bwd"]], tb["nnz"], self._st)
        else:
            tb = pos_interp.device_tables(g, c.ny, c.nx, ws.dpos_i.device)
            self._call("eav_pos_bicubic_bwd", P(ws.dpos_i), gpos, g, c.ny, c.nx, c.hidden, c.nextra,
                       *[P(t) for t in tb["bwd_y"]], tb["nnzy"], *[P(t) for t in tb["bwd_x"]], tb["nnzx"], self._st)

    def _launch_forward(self, x):
        c = self._geo
        P, L, w = _lib.ptr, self._call, self._w
        st = self._begin()
        self._phase = "fwd"
        B = x.shape[0]
        D, N = c.hidden, c.ntok
        full = self._want_full
        lay = self._split if self.precision == "split" else self._fp32     # (an unknown precision: Fp32Layers.gemm_name raises)
        ws = self._workspace_for(B, x.device, full, lay)
        dropped = self._grid(c) is not None      # patch dropout: the three embedding launches in their _keep forms
        # the device forward counter advances once per forward, whichever generators read it (config dropout, the
        # patch-dropout plan, drop path)
        if self._dropgen.generates() or (dropped and self._patch_keep.table is None) or self._droppath.generates():
            L("eav_counter_inc", self._counter(x.device).data_ptr(), st)
        drop = self._dropgen.begin(ws, B, x.device)
        self._droppath.begin(ws, B, x.device)
        lay.begin_forward(ws, x.device, full)
        pre = c.prefix
        # patch embedding: im2col rows x projection weight -> token rows [nextra:], then cls/dist + positions
        if dropped:
            self._patch_keep.begin(ws, B, x.device)
            L("eav_im2col_keep", P(x), P(ws.col), P(ws.keep), B, c.C, c.H, c.W, c.patch, c.sy, c.sx, c.transposed, c.npatch, st)
        else:
            L("eav_im2col", P(x), P(ws.col), B, c.C, c.H, c.W, c.patch, c.sy, c.sx, c.transposed, st)
        h0 = ws.hs[0]
        lay.patch_embed(ws, h0, w(f"{pre}.embeddings.patch_embeddings.projection.bias"))
        pos = self._fit_positions(w(f"{pre}.embeddings.position_embeddings"), ws)
        tokens = (w(f"{pre}.embeddings.cls_token"), w(f"{pre}.embeddings.distillation_token") if c.kind == "ast" else None)
        if dropped:
            L("eav_embed_finish_keep", P(h0), *tokens, pos, P(ws.keep), B, c.npatch, D, c.nextra, st)
        else:
            L("eav_embed_finish", P(h0), *tokens, pos, B, N, D, c.nextra, st)
        if drop.ph > 0.0:
            self._drop_add(P(h0), None, P(h0), ws.M * D, "emb")
        outs = self._outs
        if outs is not None:
            outs.allocate(c, B, x.device)
            if outs.hidden is not None:
                outs.hidden[0].view(ws.M, D).copy_(h0)
        scale = (D // c.heads) ** -0.5
        layer = lay.layer_forward
        for i in range(c.layers):
            j = i if ws.full else 0
            hin = ws.hs[i] if ws.full else ws.hs[i & 1]
            hout = ws.hs[i + 1] if ws.full else ws.hs[(i + 1) & 1]
            layer(i, j, hin, hout, f"{pre}.layers.{i}", P(ws.st[j]), scale)
            if outs is not None and outs.hidden is not None:      # (the workspace's copy is the next layer's, or forward's, to reuse)
                outs.hidden[i + 1].view(ws.M, D).copy_(hout)
        hlast = ws.hs[c.layers] if ws.full else ws.hs[c.layers & 1]
        R = B * c.nextra
        L("eav_token_rows", P(hlast), P(ws.rows), B, N, D, c.nextra, 0, st)
        sf = P(ws.stf)
        L("eav_layernorm_fwd", P(ws.rows), w(f"{pre}.layernorm.weight"), w(f"{pre}.layernorm.bias"), P(ws.seqr), sf,
          sf + 4 * R, R, D, c.eps, st)
        if c.kind == "ast":
            L("eav_pair_mean", P(ws.seqr), P(ws.pooled), B, D, 0, st)
        self._head.forward(ws.pooled if c.kind == "ast" else ws.seqr, ws, B)
        self._token += 1
        self._saved = (self._token, x, full, self._active_geo)
        return self._token

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
        P, L, gp = _lib.ptr, self._call, self._gp
        st = self._begin()
        self._phase = "bwd"
        ws = self._ws
        B, M, lay = ws.B, ws.M, ws.layers
        D, N = c.hidden, c.ntok
        _, gflat, offs = self._flat
        pre = c.prefix
        R = B * c.nextra
        # ---- head
        self._head.backward(dlogits, ws.pooled if c.kind == "ast" else ws.seqr, ws, B)
        if c.kind == "ast" and full:
            L("eav_pair_mean", P(ws.dseqr), P(ws.dpooled), B, D, 1, st)
        if full:
            sf = P(ws.stf)
            L("eav_layernorm_bwd", P(ws.dseqr), P(ws.rows), P(self._pmap[f"{pre}.layernorm.weight"]), sf, sf + 4 * R,
              P(ws.drows), 0, P(ws.part_lnr), R, D, st)
            self._reduce_ln(ws.part_lnr, ws.np_lnr, gp(f"{pre}.layernorm.weight"), gp(f"{pre}.layernorm.bias"))
            ws.dh.zero_()
            L("eav_token_rows", P(ws.dh), P(ws.drows), B, N, D, c.nextra, 1, st)
            scale = (D // c.heads) ** -0.5
            dh = P(ws.dh)
            drop = ws.drop
            lay.begin_backward(ws)
            # ---- layers
            layer = lay.layer_backward
            for i in reversed(range(c.layers)):
                Lk = f"{pre}.layers.{i}"
                layer(i, Lk, P(ws.st[i]), scale)
                if self.grad_ready_hook is not None:   # layer i's parameters are one contiguous slice
                    self._join_wgrads()         # the layer's weight gradients must be complete before they travel
                    last = offs[f"{Lk}.mlp.fc2.bias"]
                    self.grad_ready_hook(offs[f"{Lk}.attention.q_proj.weight"][0], last[0] + last[1])
            # ---- embeddings ("emb" dropout: dh is final here, so its gate runs in place)
            if drop.ph > 0.0:
                self._drop_add(dh, None, dh, M * D, "emb")
            # the position table's gradient: straight into the stored table's, or - the table fitted to this forward's patch
            # grid - into ws.dpos_i and through the adjoint of the fit
            fitted = self._fitted(c) != (None, None)
            dpos = P(ws.dpos_i) if fitted else gp(f"{pre}.embeddings.position_embeddings")
            if self._grid(c) is not None:      # patch dropout: the full grid's rows, +0.0 where nobody kept
                L("eav_embed_bwd_keep", dh, dpos, P(ws.demb), P(ws.inv), B, c.grid_npatch, c.npatch, D, c.nextra, st)
            else:
                L("eav_embed_bwd", dh, dpos, P(ws.demb), B, N, D, c.nextra, st)
            if fitted:
                self._fit_positions_backward(ws, gp(f"{pre}.embeddings.position_embeddings"))
            gpos = gflat[offs[f"{pre}.embeddings.position_embeddings"][0]:]
            gflat[offs[f"{pre}.embeddings.cls_token"][0]:][:D].copy_(gpos[:D])
            if c.kind == "ast":
                gflat[offs[f"{pre}.embeddings.distillation_token"][0]:][:D].copy_(gpos[D:2 * D])
            MP = B * c.npatch
            lay.patch_wgrad(ws, gp(f"{pre}.embeddings.patch_embeddings.projection.weight"), MP)
            self._call("eav_colsum", P(ws.demb), P(ws.part_cs), MP, D, D, st)
            self._call("eav_reduce_partials", P(ws.part_cs), _lib.plain("eav_colsum_nparts", MP), D, D, 1.0,
                       gp(f"{pre}.embeddings.patch_embeddings.projection.bias"), st)
        self._join_wgrads()          # side-stream weight gradients complete before autograd / the optimiser see them
        return self._trained_grads(full)


def ASTForAudioClassification(cfg=None, weights=None):
    return Encoder(cfg or make_config("ast"), weights)


def ViTForImageClassification(cfg=None, weights=None):
    return Encoder(cfg or make_config("vit"), weights)
