"""The classification head of transformer.Encoder: [LayerNorm (AST) +] Linear, narrow or wide (head_algo), forward and backward.

The full step runs it on the model's workspace, Encoder.head runs it alone on cached backbone features with a head-only
workspace: the same methods, the same buffers (EncoderHead.buffers), hence bit-equal logits and gradients.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import _lib
from .criteria import head_is_wide


class _HeadFn(torch.autograd.Function):
    """The classification head alone on cached backbone features (Encoder.head): the same kernels, in the same order and
    with the same arguments, as the tail of _launch_forward / the start of _launch_backward."""

    @staticmethod
    def forward(ctx, feat, model, *params):
        ctx.model, ctx.B = model, feat.shape[0]
        hw = model._head.workspace(feat.shape[0], feat.device)
        hw.feat.copy_(feat)
        model._begin()
        model._head.forward(hw.feat, hw, feat.shape[0])
        hw.token = model._token = model._token + 1
        ctx.token = hw.token
        return hw.logits.clone()

    @staticmethod
    def backward(ctx, dlogits):
        model = ctx.model
        hw = model._head.workspace(ctx.B, dlogits.device)
        if hw.token != ctx.token:
            raise _lib.EavError("Encoder.head backward: activations were overwritten by a later head forward")
        model._begin()
        model._head.backward(dlogits.contiguous(), hw.feat, hw, ctx.B)
        return (None, None, *model._trained_grads(False))


class EncoderHead:
    """The head's launches and buffers; `m` is the encoder."""

    def __init__(self, m):
        self.m = m

    def wide(self):
        """Whether the classification Linear runs on eav_dense_wide_* (head_algo)."""
        return head_is_wide(self.m.head_algo, self.m.cfg.num_labels, "the head has")

    def buffers(self, B, f, backward):
        """{name: buffer} of what the head kernels touch beside their input, for a batch of B; f(*shape) allocates.  In two
        halves, so that the full workspace keeps its allocation order (and with it every buffer's address): what the forward
        writes - head_ws is the wide backward's class slices of d loss / d feat, None where no scratch is needed - and,
        `backward`, the gradients."""
        c, D = self.m.cfg, self.m.cfg.hidden
        if backward:
            return dict(dseqr=f(B * c.nextra, D), dpooled=f(B, D), dhl=f(B, D),
                        part_lnr=f(_lib.plain("eav_layernorm_bwd_nparts", B * c.nextra), 2 * D))
        n = _lib.plain("eav_dense_wide_bwd_ws_floats", B, D, c.num_labels) if self.wide() else 0
        return dict(hl=f(B, D), sth=f(2, B), logits=f(B, c.num_labels), head_ws=f(n) if n else None)

    def workspace(self, B, dev):
        """The head-only workspace of Encoder.head: the head's buffers, its input `feat`, the token of the forward that
        filled it and the routing it was sized for."""
        m = self.m
        hw = m._hws.get(B)
        if hw is None or hw.feat.device != dev or hw.logits.shape[1] != m.cfg.num_labels or hw.wide != self.wide():
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
            hw = m._hws[B] = SimpleNamespace(feat=f(B, m.cfg.hidden), token=-1, wide=self.wide(), **self.buffers(B, f, False),
                                             **self.buffers(B, f, True))
        return hw

    def dense_forward(self, feat, weight, bias, hw, B):
        m, c, P = self.m, self.m.cfg, _lib.ptr
        if self.wide():
            m._call("eav_dense_wide_fwd", P(feat), weight, bias, P(hw.logits), B, c.hidden, c.num_labels, m._st)
        else:
            m._call("eav_dense_softmax_fwd", P(feat), weight, bias, P(hw.logits), None, B, c.hidden, c.num_labels, m._st)

    def dense_backward(self, dlogits, feat, weight, dweight, dbias, dfeat, hw, B):
        m, c, P = self.m, self.m.cfg, _lib.ptr
        if self.wide():
            m._call("eav_dense_wide_bwd", P(dlogits), P(feat), weight, dweight, dbias, P(dfeat), P(hw.head_ws), B,
                    c.hidden, c.num_labels, m._st)
        else:
            m._call("eav_dense_softmax_bwd", P(dlogits), None, P(feat), weight, dweight, dbias, P(dfeat), B, c.hidden,
                    c.num_labels, m._st)

    def forward(self, feat, hw, B):
        """feat [B, D] = the classifier's input (AST: mean of the cls / distillation rows after the final LayerNorm,
        HF modeling_audio_spectrogram_transformer.py ASTMLPHead; ViT: the cls row after the final LayerNorm)."""
        m = self.m
        c, P, w = m.cfg, _lib.ptr, m._w
        if c.kind == "ast":
            sh = P(hw.sth)
            m._call("eav_layernorm_fwd", P(feat), w("classifier.layernorm.weight"), w("classifier.layernorm.bias"),
                    P(hw.hl), sh, sh + 4 * B, B, c.hidden, c.eps, m._st)
            self.dense_forward(hw.hl, w("classifier.dense.weight"), w("classifier.dense.bias"), hw, B)
        else:
            self.dense_forward(feat, w("classifier.weight"), w("classifier.bias"), hw, B)

    def backward(self, dlogits, feat, hw, B):
        """Head gradients into the flat gradient buffer; d loss / d feat into hw.dpooled (AST) / hw.dseqr (ViT)."""
        m = self.m
        c, P, w, gp = m.cfg, _lib.ptr, m._w, m._gp
        if c.kind == "ast":
            self.dense_backward(dlogits, hw.hl, w("classifier.dense.weight"), gp("classifier.dense.weight"),
                                gp("classifier.dense.bias"), hw.dhl, hw, B)
            sh = P(hw.sth)
            m._call("eav_layernorm_bwd", P(hw.dhl), P(feat), w("classifier.layernorm.weight"), sh, sh + 4 * B,
                    P(hw.dpooled), 0, P(hw.part_lnr), B, c.hidden, m._st)
            m._reduce_ln(hw.part_lnr, _lib.plain("eav_layernorm_bwd_nparts", B), gp("classifier.layernorm.weight"),
                         gp("classifier.layernorm.bias"))
        else:
            self.dense_backward(dlogits, feat, w("classifier.weight"), gp("classifier.weight"), gp("classifier.bias"),
                                hw.dseqr, hw, B)
