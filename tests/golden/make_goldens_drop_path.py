"""Goldens of stochastic depth (timm.layers.DropPath, scale_by_keep) for the encoders (tests/golden/drop_path_{ast,vit}.npz),
produced by the installed Hugging Face classes - ASTForAudioClassification / ViTForImageClassification - in training mode on
the CPU.  In this version of transformers every encoder layer owns ONE `dropout` module (p = 0 here: the identity), called
first on the attention branch and then on the MLP branch, each time right before the residual add.  A counting forward hook on
layers[i].dropout that multiplies the output by s[i, call][:, None, None] therefore restates drop path exactly; the hook
asserts the two calls per layer.  The keep tables are tests/drop_path_ref.golden_keep, the scales float32 1 / (1 - p_i).
One unfrozen AdamW step, then one frozen step (classifier only).  Development container only; data-only output: logits and
loss in full, gradients and post-step parameters as a strided sample, sum |.| and max |.| per tensor
(tests/encoder_dropout_ref.summarise)."""
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
from tests import drop_path_ref as R  # noqa: E402
from tests.encoder_dropout_ref import summarise  # noqa: E402
from tests.golden.make_goldens_encoder_dropout import hf_model  # noqa: E402
from tests.golden_util import tf_weights  # noqa: E402


class PathHooks:
    """Forward hooks on every layer's `dropout`: call k (0: attention branch, 1: MLP branch) of layer i returns
    output * scale[i, k][:, None, None]."""

    def __init__(self, model, layers):
        mods = {n: m for n, m in model.named_modules()}
        names = [n for n in mods if n.endswith(".dropout") and ".layers." in n]
        self.drops = []
        for i in range(layers):
            hit = [n for n in names if n.endswith(f".layers.{i}.dropout")]
            assert len(hit) == 1, (i, hit)
            self.drops.append(mods[hit[0]])
        self.scale, self.calls, self.handles = None, None, []

    def __enter__(self):
        self.calls = [0] * len(self.drops)
        for i, d in enumerate(self.drops):
            self.handles.append(d.register_forward_hook(lambda mod, inp, out, i=i: self.gate(i, out)))
        return self

    def gate(self, i, out):
        k = self.calls[i]
        self.calls[i] += 1
        assert k < 2, f"layer {i}: a third dropout call"
        return out * self.scale[i, k][:, None, None]

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        self.handles = []
        if exc[0] is None:
            assert self.calls == [2] * len(self.drops), self.calls


def make(kind):
    cfg = R.oracle_cfg(kind)
    W = tf_weights(R.WSEED[kind], vo.param_shapes(cfg), std=R.STD)
    hk = set(vo.head_keys(cfg))
    out = {"kind": kind, "wseed": R.WSEED[kind], "xseed": R.XSEED, "std": R.STD, "lr": R.LR, "B": R.BATCH, "rate": R.RATE,
           "ntok": cfg["ntok"]}
    torch.manual_seed(0)
    model = hf_model(cfg, 0.0, 0.0)
    assert set(model.state_dict()) == set(W), set(model.state_dict()) ^ set(W)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in W.items()})
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=R.LR)
    hooks = PathHooks(model, cfg["layers"])
    for s, freeze in enumerate((False, True)):
        x, y = R.batch(kind, cfg, R.XSEED + s, R.BATCH)
        keep = R.golden_keep(s)
        out[f"keep{s}"] = keep
        hooks.scale = torch.from_numpy(R.scales_of(keep, R.RATE).astype(np.float32))
        for k, p in model.named_parameters():
            p.requires_grad = (not freeze) or (k in hk)
        opt.zero_grad()
        with hooks:
            logits = model(torch.from_numpy(x)).logits
        loss = torch.nn.CrossEntropyLoss()(logits, torch.from_numpy(y))
        loss.backward()
        out[f"logits{s}"] = logits.detach().numpy().copy()
        out[f"loss{s}"] = np.float32(loss.item())
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        for k, p in model.named_parameters():
            if k in grads:
                for tag, t in (("grad", grads[k]), ("post", p)):
                    smp, sa, mx = summarise(t)
                    out[f"{tag}{s}.{k}"] = smp
                    out[f"{tag}{s}.{k}#sumabs"] = sa
                    out[f"{tag}{s}.{k}#maxabs"] = mx
        print("step", kind, s, out[f"logits{s}"][0], float(out[f"loss{s}"]))
    path = os.path.join(HERE, f"drop_path_{kind}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for kind in (sys.argv[1:] or ["ast", "vit"]):
        make(kind)
