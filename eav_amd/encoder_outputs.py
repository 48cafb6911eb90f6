"""What a forward of transformer.Encoder returns beside the logits: hidden states, attention probabilities, and the head means
attention_rollout is made of.

One Outputs object carries a forward's request (Encoder._outs, made by EncoderOutputs.request from the two keywords of the
call) and, once _launch_forward has run, the buffers: fresh fp32 allocations, detached from autograd.
"""
from __future__ import annotations

import torch

from . import _lib

HEAD_MEANS = object()       # output_attentions=HEAD_MEANS: the head means instead of the probabilities (attention_rollout)


class Outputs:
    """want_hidden, attn ("probs" | "mean" | None): the request; hidden [layers + 1, B, N, D], probs [layers, B, H, N, N],
    mean [layers, B, N, N]: the buffers, each None unless asked for and allocated."""

    def __init__(self, want_hidden, attn):
        self.want_hidden, self.attn = want_hidden, attn
        self.hidden = self.probs = self.mean = None

    def allocate(self, c, B, dev):
        """Fresh for every forward - the workspace is the next forward's to overwrite."""
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.hidden = f(c.layers + 1, B, c.ntok, c.hidden) if self.want_hidden else None
        self.probs = f(c.layers, B, c.heads, c.ntok, c.ntok) if self.attn == "probs" else None
        self.mean = f(c.layers, B, c.ntok, c.ntok) if self.attn == "mean" else None

    def result(self):
        """(hidden_states, attentions) as the model returns them: per-layer views."""
        attn = self.probs if self.probs is not None else self.mean
        return (None if self.hidden is None else tuple(self.hidden.unbind(0)),
                None if attn is None else tuple(attn.unbind(0)))


class EncoderOutputs:
    """The request of a call, the attention probabilities of a layer, and attention rollout; `m` is the encoder."""

    def __init__(self, m):
        self.m = m

    def request(self, output_attentions, output_hidden_states):
        """The Outputs of a call with these two keywords (None: the encoder's attributes of the same names), None when
        it wants nothing beside the logits."""
        m = self.m
        means = output_attentions is HEAD_MEANS
        want_attn = m.output_attentions if output_attentions is None else bool(output_attentions) and not means
        want_hidden = m.output_hidden_states if output_hidden_states is None else bool(output_hidden_states)
        if want_attn or want_hidden:
            if torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("output_attentions / output_hidden_states allocate their results: not available "
                                          "while the stream is capturing")
            if want_attn and m.training and m.cfg.attention_dropout > 0.0:
                raise NotImplementedError("output_attentions in training mode with attention_probs_dropout_prob > 0 is not "
                                          "implemented: HF returns the dropped probabilities there")
        elif not means:
            return None
        return Outputs(bool(want_hidden), "mean" if means else ("probs" if want_attn else None))

    def attention(self, i, j, scale, qkv=None, rowp=None, slot=None):
        """Layer i's attention probabilities into the forward's outputs, right after its attention kernel (workspace index
        j): the fused path launches csrc/attn_probs.hip on the operands that kernel consumed - fp32 `qkv`, or the row planes
        `rowp` with their scale `slot` - and the lse it wrote; the materialised path copies the softmax output out of ws.P[j]
        (row stride ldn).  A no-op unless the forward asked for them."""
        m = self.m
        o = m._outs
        if o is None or o.attn is None:
            return
        c, ws, P = m._geo, m._ws, _lib.ptr
        N, H = c.ntok, c.heads
        probs = None if o.probs is None else P(o.probs[i])
        mean = None if o.mean is None else P(o.mean[i])
        if not ws.fused:
            if o.probs is not None:
                o.probs[i].view(ws.B * H, N, N).copy_(ws.P[j][:, :, :N])
            if o.mean is not None:      # the heads of an image are H slices of ws.P[j], N ldn floats apart: summed in head order
                pad = torch.empty(ws.B, N, ws.ldn, dtype=torch.float32, device=ws.P[j].device)
                for b in range(ws.B):
                    m._call("eav_reduce_partials", P(ws.P[j][b * H]), H, N * ws.ldn, N * ws.ldn, 1.0 / H, P(pad[b]), m._st)
                o.mean[i].copy_(pad[:, :, :N])
        elif rowp is not None:
            m._call("eav_attn_probs_sp", rowp, slot, P(ws.lse[j]), probs, mean, ws.B, H, N, c.hidden // H, scale, m._st)
        else:
            m._call("eav_attn_probs", qkv, P(ws.lse[j]), probs, mean, ws.B, H, N, c.hidden // H, scale, m._st)

    def rollout(self, x, as_grid, interpolate_pos_encoding):
        m = self.m
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("attention_rollout allocates its result: not available while the stream is capturing")
        training = m.training
        m.eval()
        try:
            with torch.no_grad():
                mean = m(x, interpolate_pos_encoding=interpolate_pos_encoding, output_attentions=HEAD_MEANS,
                         output_hidden_states=False).attentions
                c = m._geo
                B, N, R = x.shape[0], c.ntok, c.nextra
                r, r_next = torch.zeros(B, R, N, dtype=torch.float32, device=x.device), torch.empty(B, R, N, device=x.device)
                for k in range(R):
                    r[:, k, k].fill_(1.0)
                st = m._begin()
                for i in reversed(range(c.layers)):
                    m._call("eav_rollout_step", _lib.ptr(r), _lib.ptr(mean[i]), _lib.ptr(r_next), B, R, N, st)
                    r, r_next = r_next, r
                out = torch.empty(B, N, dtype=torch.float32, device=x.device)
                if R == 2:
                    m._call("eav_pair_mean", _lib.ptr(r), _lib.ptr(out), B, N, 0, st)
                else:
                    out.copy_(r[:, 0])
        finally:
            m.train(training)
        return out[:, c.nextra:].reshape(B, c.ny, c.nx) if as_grid else out
