"""Goldens of ViT's interpolate_pos_encoding, produced by the Hugging Face class the reference instantiates
(Transformer_Vision.py:29) called with interpolate_pos_encoding=True: the reduced model of make_goldens_tf.reduced_case
(2 layers, hidden 64, 4 heads, ff 128, native 224 x 224) on smaller frames.  Development container only; data-only fixture.

    vit_interp.npz   112 x 112: logits, loss and every gradient of one unfrozen step;  64 x 144: logits and loss."""
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
from tests.golden.make_goldens_tf import hf_model, load  # noqa: E402
from tests.golden_util import tf_weights  # noqa: E402
from tests.vit_interp_ref import frames  # noqa: E402

WSEED, XSEED, STD, B = 12, 120, 0.08, 3


def main():
    cfg = vo.cfg_vit(hidden=64, layers=2, heads=4, ff=128)
    W = tf_weights(WSEED, vo.param_shapes(cfg), std=STD)
    torch.manual_seed(0)
    model = hf_model(cfg)
    load(model, W)
    model.train()
    out = {"wseed": WSEED, "xseed": XSEED, "std": STD, "B": B}
    x, y = frames(XSEED, B, 112, 112)
    o = model(torch.from_numpy(x), labels=torch.from_numpy(y), interpolate_pos_encoding=True)
    o.loss.backward()
    out["logits112"] = o.logits.detach().numpy().copy()
    out["loss112"] = np.float32(o.loss.item())
    for k, p in model.named_parameters():
        out[f"grad112.{k}"] = p.grad.numpy().copy()
    x, y = frames(XSEED + 1, B, 64, 144)
    with torch.no_grad():
        o = model(torch.from_numpy(x), labels=torch.from_numpy(y), interpolate_pos_encoding=True)
    out["logits64x144"] = o.logits.numpy().copy()
    out["loss64x144"] = np.float32(o.loss.item())
    path = os.path.join(HERE, "vit_interp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), out["logits112"], out["logits64x144"])


if __name__ == "__main__":
    main()
