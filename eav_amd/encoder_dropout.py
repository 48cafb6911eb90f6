"""The dropout of transformer.Encoder: the one table of its sites, the generator, and the state of one forward.

Every keep decision is a hash of (site seed, device-resident forward counter, element index); the site seed derives from
Encoder.dropout_seed and the site's id, the id from SITES.  A launch names its site as (kind, layer) and takes the kernel
arguments from DropState.site, so a forward and its backward regenerate the same mask by construction.
"""
from __future__ import annotations

import torch

from . import _lib

# kind -> (id at layer 0, id stride per layer, attention rate?), in HF's call order; the name is "emb" / "<kind>.<layer>"
# "patch_keep" is no dropout site but the seed stream of the patch-dropout plan (patch_keep.py): an id no layer count
# reaches (3 * layers < 2^23), still inside the 24 bits site_seed has room for.
SITES = {"emb": (0, 0, False), "attn": (1, 3, True), "attn_out": (2, 3, False), "mlp_out": (3, 3, False),
         "patch_keep": (1 << 23, 0, False)}


def site_id(kind, layer=0):
    first, stride, _ = SITES[kind]
    return first + stride * layer


def site_name(kind, layer=0):
    return kind if kind == "emb" else f"{kind}.{layer}"


def site_seed(seed, sid):
    return (int(seed) + ((sid + 1) << 40)) & 0xFFFFFFFFFFFFFFFF


class DropState:
    """Dropout of one forward, kept on its workspace for the backward: the probabilities (0 in eval mode), the model's seed,
    and the explicit masks {site name: uint8 tensor} or the device counter's address."""

    def __init__(self, seed, ph, pa, masks=None, cnt=None):
        self.seed, self.ph, self.pa, self.masks, self.cnt = seed, float(ph), float(pa), masks, cnt

    def site(self, kind, layer=0):
        """(p, seed, mask pointer, counter pointer): the kernel arguments of the site (kind, layer)."""
        first, stride, attention = SITES[kind]
        mask = None if self.masks is None else self.masks[site_name(kind, layer)].data_ptr()
        return (self.pa if attention else self.ph, site_seed(self.seed, first + stride * layer), mask, self.cnt)


class EncoderDropout:
    """What Encoder's public dropout surface delegates to; `m` is the encoder."""

    def __init__(self, m):
        self.m = m

    def sites(self, B):
        c = self.m.cfg
        # (indexed by SITES' "attention rate?")
        shape = ((B, c.ntok, c.hidden), (B, c.heads, c.ntok, c.ntok))
        rate = (c.hidden_dropout, c.attention_dropout)
        where = [("emb", 0)] + [(kind, i) for i in range(c.layers) for kind in SITES if SITES[kind][1]]      # (the per-layer kinds)
        return {site_name(kind, i): (site_id(kind, i), shape[SITES[kind][2]], rate[SITES[kind][2]])
                for kind, i in where if rate[SITES[kind][2]] > 0.0}

    def generated_masks(self, B, counter, seed=None):
        m = self.m
        dev = next(m.parameters()).device
        cnt = torch.tensor(int(counter), dtype=torch.int64, device=dev)
        seed = m.dropout_seed if seed is None else seed
        out = {}
        for name, (sid, shape, p) in self.sites(B).items():
            mask = out[name] = torch.empty(shape, dtype=torch.uint8, device=dev)
            _lib.call("eav_tf_dropout_mask", mask.data_ptr(), mask.numel(), float(p), site_seed(seed, sid), cnt.data_ptr(),
                      _lib.stream_ptr())
        return out

    def generates(self):
        """Whether the forward about to run draws its masks from the device forward counter."""
        m, c = self.m, self.m.cfg
        return m.training and (c.hidden_dropout > 0.0 or c.attention_dropout > 0.0) and m._dropout_masks is None

    def begin(self, ws, B, dev):
        """The DropState of this forward, left on the workspace: explicit masks are validated, else it reads the device
        forward counter (which the encoder advances, once per forward, for all its generators)."""
        m, c = self.m, self.m.cfg
        ph, pa = (c.hidden_dropout, c.attention_dropout) if m.training else (0.0, 0.0)
        d = ws.drop = DropState(m.dropout_seed, ph, pa)
        if ph > 0.0 or pa > 0.0:
            if m._dropout_masks is not None:
                d.masks = dict(m._dropout_masks)
                for name, (_, shape, _) in self.sites(B).items():
                    k = d.masks.get(name)
                    if not (isinstance(k, torch.Tensor) and k.dtype == torch.uint8 and k.device == dev
                            and tuple(k.shape) == shape and k.is_contiguous()):
                        raise _lib.EavError(f"set_dropout_masks: site {name!r} needs a contiguous uint8 mask {shape} on {dev}")
            else:
                d.cnt = m._counter(dev).data_ptr()
        return d
