"""Goldens of patch dropout (timm.layers.PatchDropout), produced by the Hugging Face classes the reference instantiates
(Transformer_Audio.py:22, Transformer_Vision.py:29) on the CPU: the model's own `embeddings(x)` - tokens plus position
embeddings - then the kept rows of every sample gathered (the readout tokens always), then HF's encoder, final LayerNorm
and head, by wrapping the embeddings module's forward and calling the model as ever.  Weights from tests/golden_util.tf_weights,
keep tables from the numpy plan (tests/patch_keep_ref.model_keep), cases patch_keep_ref.MODEL_CASES.  An AST at another
length than its checkpoint's gets its table fitted by make_goldens_ast_length.torch_fit, so the table's gradient has the
stored shape.  Development container only; data-only fixtures.

    patch_dropout.npz       vit64 (16 patches, 7 kept), ast96 (256-frame checkpoint at 96 frames, 54 of 108 kept)
    patch_dropout_256.npz   ast256 (150 of 300 kept), ast256w (hidden 128, 2 heads: 107 of 300 kept, embedding gradients only)
Per case: <name>.keep, <name>.logits, <name>.loss, <name>.grad.<parameter>.  (Two files: one would exceed 1 MiB.)"""
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
from tests import patch_keep_ref as R  # noqa: E402
from tests.golden.make_goldens_ast_length import torch_fit  # noqa: E402
from tests.golden.make_goldens_tf import hf_model  # noqa: E402
from tests.golden_util import tf_weights  # noqa: E402


def oracle_cfg(c, size):
    return vo.cfg_ast(**c["kw"], frames=size) if c["kind"] == "ast" else vo.cfg_vit(**c["kw"], image=size)


def run(name):
    c = R.MODEL_CASES[name]
    W = tf_weights(R.MODEL_WSEED, vo.param_shapes(oracle_cfg(c, c["native"])), std=R.MODEL_STD)
    cfg = oracle_cfg(c, c["size"])
    torch.manual_seed(0)
    model = hf_model(cfg)
    params = {k: torch.from_numpy(np.ascontiguousarray(v)).requires_grad_(True) for k, v in W.items()}
    assert set(params) == set(model.state_dict())
    fitted = dict(params)
    if c["size"] != c["native"]:
        key = f"{cfg['prefix']}.embeddings.position_embeddings"
        fitted[key] = torch_fit(params[key], 12, (c["native"] - 16) // 10 + 1, (c["size"] - 16) // 10 + 1)
    keep = R.model_keep(name)
    nextra = cfg["nextra"]
    rows = torch.from_numpy(np.concatenate([np.tile(np.arange(nextra), (R.MODEL_B, 1)), nextra + keep], 1).astype(np.int64))
    emb = getattr(model, cfg["prefix"]).embeddings
    plain = emb.forward

    def kept(*a, **k):
        h = plain(*a, **k)
        assert h.shape[1] == nextra + c["P"], h.shape
        return torch.gather(h, 1, rows[:, :, None].expand(-1, -1, h.shape[-1]))

    emb.forward = kept
    model.train()
    x, y = R.model_batch(name)
    o = torch.func.functional_call(model, fitted, (torch.from_numpy(x),), {"labels": torch.from_numpy(y)})
    o.loss.backward()
    out = {f"{name}.keep": keep, f"{name}.logits": o.logits.detach().numpy().copy(), f"{name}.loss": np.float32(o.loss.item())}
    for k, p in params.items():
        if c["grads"] == "all" or ".embeddings." in k:
            out[f"{name}.grad.{k}"] = p.grad.numpy().copy()
    return out


def main():
    files = {}
    for name, c in R.MODEL_CASES.items():
        files.setdefault(c["file"], {}).update(run(name))
    for fn, out in files.items():
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), {k: v for k, v in out.items() if k.endswith(".logits")})


if __name__ == "__main__":
    main()
