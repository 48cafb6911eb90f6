"""Goldens of the AST at another clip length, produced by the Hugging Face class the reference instantiates
(Transformer_Audio.py:22): ASTForAudioClassification(ASTConfig(max_length=T')) is a stock model at any T'; with its
position_embeddings set to the stored table fitted to T' by torch's own operations - a slice of the centre window for a
shorter input, F.interpolate(mode="bilinear", align_corners=False) for a longer one - it defines the expected logits, loss
and gradients.  The reduced model of make_goldens_tf.reduced_case (2 layers, hidden 64, 4 heads, ff 128) with native frames
256, i.e. a stored grid of 12 x 25.  Development container only; data-only fixture.

    ast_length.npz   T' = 96 (cut, 9 time patches): logits, loss and every gradient of one unfrozen step, the table's in the
                     stored 302-row shape, through the fit;  T' = 336 (linear, 33 time patches): logits and loss."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vit_oracle as vo  # noqa: E402
from tests.ast_length_ref import clips  # noqa: E402
from tests.golden.make_goldens_tf import hf_model  # noqa: E402
from tests.golden_util import tf_weights  # noqa: E402

WSEED, XSEED, STD, B, NATIVE = 21, 210, 0.08, 3, 256
KEY = "audio_spectrogram_transformer.embeddings.position_embeddings"


def torch_fit(pos, ny, nx0, nx):
    """[1, 2 + ny nx0, D] -> [1, 2 + ny nx, D], differentiable."""
    D = pos.shape[-1]
    grid = pos[:, 2:].reshape(1, ny, nx0, D).permute(0, 3, 1, 2)
    if nx < nx0:
        s = nx0 // 2 - nx // 2
        grid = grid[:, :, :, s:s + nx]
    else:
        grid = F.interpolate(grid, size=(ny, nx), mode="bilinear", align_corners=False)
    return torch.cat([pos[:, :2], grid.permute(0, 2, 3, 1).reshape(1, ny * nx, D)], 1)


def run(W, T, train):
    cfg = vo.cfg_ast(hidden=64, layers=2, heads=4, ff=128, frames=T)
    nx0, nx = (NATIVE - 16) // 10 + 1, (T - 16) // 10 + 1
    torch.manual_seed(0)
    model = hf_model(cfg)
    params = {k: torch.from_numpy(np.ascontiguousarray(v)).requires_grad_(train) for k, v in W.items()}
    assert set(params) == set(model.state_dict())
    fitted = dict(params)
    fitted[KEY] = torch_fit(params[KEY], 12, nx0, nx)
    assert tuple(fitted[KEY].shape) == tuple(model.state_dict()[KEY].shape)
    model.train(train)
    x, y = clips(XSEED + T, B, T)
    o = torch.func.functional_call(model, fitted, (torch.from_numpy(x),), {"labels": torch.from_numpy(y)})
    if train:
        o.loss.backward()
    return o, params


def main():
    W = tf_weights(WSEED, vo.param_shapes(vo.cfg_ast(hidden=64, layers=2, heads=4, ff=128, frames=NATIVE)), std=STD)
    out = {"wseed": WSEED, "xseed": XSEED, "std": STD, "B": B, "native": NATIVE}
    o, params = run(W, 96, True)
    out["logits96"] = o.logits.detach().numpy().copy()
    out["loss96"] = np.float32(o.loss.item())
    for k, p in params.items():
        out[f"grad96.{k}"] = p.grad.numpy().copy()
    with torch.no_grad():
        o, _ = run(W, 336, False)
    out["logits336"] = o.logits.numpy().copy()
    out["loss336"] = np.float32(o.loss.item())
    path = os.path.join(HERE, "ast_length.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), out["logits96"], out["logits336"])


if __name__ == "__main__":
    main()
