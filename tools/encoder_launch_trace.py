#!/usr/bin/env python3
"""What an Encoder training step launches, and what it computes, as one JSON - to compare two commits that should issue the same
step (a refactor of the host code): run it on both with the same built library (EAV_LIB_PATH) and diff the files.
    python tools/encoder_launch_trace.py out.json
Every configuration trains for two steps (B = 3, torch.manual_seed(0), FusedAdam).  Per configuration the JSON holds `step`,
the ordered launches of the second step, and `sha256` of that step's logits and loss, of its gradients and of the parameters
after its optimiser step (one digest over every gradient / every parameter, in named_parameters() order); launch_trace.py has
the recorder and the file format.  Only the public surface of the package is used."""
import sys

import torch

from launch_trace import digest, recording, write      # (puts the repository root on sys.path)
from eav_amd import synth, transformer as T  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam  # noqa: E402

B = 3
SHAPES = {"128": dict(hidden=128, layers=2, heads=2, ff=256),      # head dimension 64: the fused attention kernels
          "64": dict(hidden=64, layers=2, heads=4, ff=128)}        # head dimension 16: materialised scores
FUSED = ("fused_planes", "fused_ao", "fused_qkv", "fused_dqkv", "fused_dh", "fused_dact")


def configurations():
    """[(name, kind, make_config arguments, Encoder attributes, classifier only, input size or None)]"""
    out = []
    for kind in ("vit", "ast"):
        for sn, shape in SHAPES.items():
            for prec in ("fp32", "split"):
                base = f"{kind}-{sn}-{prec}"
                for frozen in (False, True):
                    out.append((base + ("-classifier" if frozen else ""), kind, shape, dict(precision=prec), frozen, None))
                out.append((base + "-dropout", kind, dict(shape, hidden_dropout=0.1, attention_dropout=0.1),
                            dict(precision=prec), False, None))
        split = dict(precision="split")
        variants = [("grad_terms1", dict(grad_terms=1)), ("wgrad_terms2", dict(wgrad_terms=2))]
        variants += [(f"{f}-off", {f: False}) for f in FUSED]
        variants += [(f"overlap-{o}", dict(overlap_wgrad=o)) for o in (True, False)]
        for vn, attrs in variants:
            out.append((f"{kind}-128-split-{vn}", kind, SHAPES["128"], dict(split, **attrs), False, None))
    for prec in ("fp32", "split"):
        out.append((f"vit-64-{prec}-64x144", "vit", SHAPES["64"], dict(precision=prec, interpolate_pos_encoding=True), False,
                    (64, 144)))
        for frames in (96, 336):
            out.append((f"ast-64-{prec}-{frames}of256", "ast", dict(SHAPES["64"], frames=256),
                        dict(precision=prec, variable_length=True), False, frames))
    return out


def run(kind, cfg_args, attrs, frozen, size, dev):
    torch.manual_seed(0)
    model = T.Encoder(T.make_config(kind, **cfg_args)).to(dev).train()
    for k, v in attrs.items():
        setattr(model, k, v)
    if frozen:
        for k, p in model.named_parameters():
            p.requires_grad = k.startswith("classifier.")
    if kind == "ast":
        x, y = synth.mel_batch(5, B, size or model.cfg.W)
    elif size is None:
        x, y = synth.frame_batch(5, B, model.cfg.H)
    else:
        x, y = synth.frame_batch(5, B, max(size))
        x = x[:, :, :size[0], :size[1]].copy()
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=5e-6, weight_decay=0.01, decoupled=True)
    crit = CrossEntropyLoss()
    launches = []
    for step in range(2):
        with recording(launches, on=step == 1):
            opt.zero_grad()
            logits = model(x).logits
            loss = crit(logits, y)
            loss.backward()
            if step == 1:
                sha = {"logits": digest(logits), "loss": digest(loss),
                       "gradients": digest(*[p.grad for p in model.parameters() if p.grad is not None])}
            opt.step()
    torch.cuda.synchronize()
    sha["parameters"] = digest(*model.parameters())
    return {"launches": launches, "sha256": sha}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "encoder_launch_trace.json"
    dev = torch.device("cuda", 0)
    result = {}
    for name, kind, cfg_args, attrs, frozen, size in configurations():
        result[name] = run(kind, cfg_args, attrs, frozen, size, dev)
        print(f"{name}: {len(result[name]['launches'])} launches", flush=True)
    write(result, out_path)


if __name__ == "__main__":
    main()
