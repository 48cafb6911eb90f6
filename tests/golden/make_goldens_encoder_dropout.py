"""Goldens for the encoders' dropout (tests/golden/encoder_dropout_{ast,vit}.npz), produced by the installed Hugging Face
classes - ASTForAudioClassification / ViTForImageClassification with attn_implementation="eager" (the sdpa path never
calls F.dropout) - in training mode.  torch.nn.functional.dropout is patched for the duration of a forward so that it
consumes explicit keep-masks in call order (emb, then per layer attn, attn_out, mlp_out); the masks come from the repo's
deterministic generator at a recorded seed (tests/encoder_dropout_ref.site_masks), so the fixtures store seeds, not masks.
Development container only; data-only output: per case logits and loss in full, gradients and post-step parameters as a
strided sample, sum |.| and max |.| per tensor."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vit_oracle as vo  # noqa: E402
from tests import encoder_dropout_ref as R  # noqa: E402
from tests.golden_util import tf_weights  # noqa: E402


def hf_model(cfg, ph, pa):
    from transformers import ASTConfig, ASTForAudioClassification, ViTConfig, ViTForImageClassification
    common = dict(hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                  intermediate_size=cfg["ff"], patch_size=cfg["patch"], layer_norm_eps=cfg["eps"],
                  num_labels=cfg["num_labels"], hidden_dropout_prob=ph, attention_probs_dropout_prob=pa,
                  attn_implementation="eager")
    if cfg["kind"] == "ast":
        return ASTForAudioClassification(ASTConfig(frequency_stride=cfg["fstride"], time_stride=cfg["tstride"],
                                                   max_length=cfg["frames"], num_mel_bins=cfg["mel"], **common))
    return ViTForImageClassification(ViTConfig(image_size=cfg["image"], num_channels=cfg["channels"], **common))


class MaskedDropout:
    """Context manager: F.dropout(x, p, training) returns x * mask / (1 - p) with the next mask of `order`."""

    def __init__(self, masks, order):
        self.queue = [(n, masks[n]) for n in order]
        self.used = []

    def __enter__(self):
        self.orig = torch.nn.functional.dropout

        def dropout(x, p=0.5, training=True, inplace=False):
            if not training or p == 0.0:
                return x
            name, m = self.queue.pop(0)
            assert tuple(m.shape) == tuple(x.shape), (name, m.shape, x.shape)
            self.used.append((name, float(p)))
            return x * torch.from_numpy(m).to(x.dtype) * (1.0 / (1.0 - p))
        torch.nn.functional.dropout = dropout
        return self

    def __exit__(self, *exc):
        torch.nn.functional.dropout = self.orig
        if exc[0] is None:
            assert not self.queue, f"masks never consumed: {[n for n, _ in self.queue]}"


def make(kind):
    cfg = R.oracle_cfg(kind)
    W = tf_weights(R.WSEED[kind], vo.param_shapes(cfg), std=R.STD)
    hk = set(vo.head_keys(cfg))
    out = {"kind": kind, "wseed": R.WSEED[kind], "xseed": R.XSEED, "mseed": R.MSEED, "std": R.STD, "lr": R.LR,
           "B": R.BATCH, "ntok": cfg["ntok"]}
    for case, (ph, pa) in R.CASES.items():
        torch.manual_seed(0)
        model = hf_model(cfg, ph, pa)
        sd = model.state_dict()
        assert set(sd) == set(W), set(sd) ^ set(W)
        model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in W.items()})
        model.train()
        opt = torch.optim.AdamW(model.parameters(), lr=R.LR)
        for s, freeze in enumerate((False, True)):
            x, y = R.batch(kind, cfg, R.XSEED + s, R.BATCH)
            masks = R.site_masks(R.MSEED, s, R.BATCH, cfg["ntok"], cfg["hidden"], cfg["heads"], cfg["layers"], ph, pa)
            for k, p in model.named_parameters():
                p.requires_grad = (not freeze) or (k in hk)
            opt.zero_grad()
            with MaskedDropout(masks, R.site_names(cfg["layers"], ph, pa)) as md:
                logits = model(torch.from_numpy(x)).logits
            assert [n for n, _ in md.used] == R.site_names(cfg["layers"], ph, pa)
            loss = torch.nn.CrossEntropyLoss()(logits, torch.from_numpy(y))
            loss.backward()
            out[f"{case}.logits{s}"] = logits.detach().numpy().copy()
            out[f"{case}.loss{s}"] = np.float32(loss.item())
            grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            opt.step()
            for k, p in model.named_parameters():
                if k in grads:
                    for tag, t in (("grad", grads[k]), ("post", p)):
                        smp, sa, mx = R.summarise(t)
                        out[f"{case}.{tag}{s}.{k}"] = smp
                        out[f"{case}.{tag}{s}.{k}#sumabs"] = sa
                        out[f"{case}.{tag}{s}.{k}#maxabs"] = mx
        print("case", kind, case, out[f"{case}.logits0"][0], float(out[f"{case}.loss0"]))
    path = os.path.join(HERE, f"encoder_dropout_{kind}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for kind in (sys.argv[1:] or ["ast", "vit"]):
        make(kind)
