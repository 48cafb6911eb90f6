#!/usr/bin/env python3
"""What an Encoder training step launches, and what it computes, as one JSON - to compare two commits that should issue the same
step (a refactor of the host code): run it on both with the same built library (EAV_LIB_PATH) and diff the files.
    python tools/encoder_launch_trace.py out.json
Every configuration trains for two steps (B = 3, torch.manual_seed(0), FusedAdam).  Per configuration the JSON holds `step`,
the ordered launches of the second step, and `sha256` of that step's logits and loss, of its gradients and of the parameters
after its optimiser step (one digest over every gradient / every parameter, in named_parameters() order); launch_trace.py has
the recorder and the file format.  A configuration's `mode` picks the step: "step" model(x) and a CrossEntropyLoss; "head" a
no_grad forward, then Encoder.head on last_features() (the trainers' frozen-phase feature cache); "labels" model(x, labels=y)
and its own loss; "masks" a dropout step under set_dropout_masks(generated_dropout_masks(...)); "outputs" no training - one eval
forward with output_hidden_states / output_attentions and attention_rollout, plain and as_grid, all four results digested.
Only the public surface of the package is used."""
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
    """[(name, kind, make_config arguments, Encoder attributes, classifier only, input size or None, mode)]"""
    out = []
    dropout = dict(hidden_dropout=0.1, attention_dropout=0.1)
    for kind in ("vit", "ast"):
        for sn, shape in SHAPES.items():
            for prec in ("fp32", "split"):
                base = f"{kind}-{sn}-{prec}"
                for frozen in (False, True):
                    out.append((base + ("-classifier" if frozen else ""), kind, shape, dict(precision=prec), frozen, None))
                out.append((base + "-dropout", kind, dict(shape, **dropout), dict(precision=prec), False, None))
                out.append((base + "-dropout-masks", kind, dict(shape, **dropout), dict(precision=prec), False, None, "masks"))
                out.append((base + "-head", kind, shape, dict(precision=prec), True, None, "head"))
                out.append((base + "-head-40", kind, dict(shape, num_labels=40), dict(precision=prec), True, None, "head"))
                out.append((base + "-40", kind, dict(shape, num_labels=40), dict(precision=prec), False, None))
                out.append((base + "-wide", kind, shape, dict(precision=prec, head_algo="wide"), False, None))
                for pt, n in (("regression", 1), ("regression", 3), ("multi_label_classification", 4)):
                    out.append((f"{base}-{pt}-{n}", kind, dict(shape, num_labels=n, problem_type=pt), dict(precision=prec),
                                False, None, "labels"))
                out.append((base + "-outputs", kind, shape, dict(precision=prec), False, None, "outputs"))
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
    return [c if len(c) == 7 else c + ("step",) for c in out]


def outputs(model, x):
    """mode "outputs": the launches and digests of an eval forward with both output flags and of attention_rollout."""
    launches = []
    model.eval()
    with recording(launches), torch.no_grad():
        out = model(x, output_hidden_states=True, output_attentions=True)
        roll, grid = model.attention_rollout(x), model.attention_rollout(x, as_grid=True)
    torch.cuda.synchronize()
    return {"launches": launches, "sha256": {"logits": digest(out.logits), "hidden_states": digest(*out.hidden_states),
                                             "attentions": digest(*out.attentions), "rollout": digest(roll),
                                             "rollout_grid": digest(grid)}}


def run(kind, cfg_args, attrs, frozen, size, mode, dev):
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
    if mode == "outputs":
        return outputs(model, x)
    if mode == "labels":        # float targets [B, classes]; a one-output regression also takes them flat
        y = torch.from_numpy(synth.normal(7, (B, model.cfg.num_labels)).astype("float32")).to(dev)
        if model.cfg.problem_type == "multi_label_classification":
            y = (y > 1.0).float()
        elif model.cfg.num_labels == 1:
            y = y[:, 0].contiguous()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=5e-6, weight_decay=0.01, decoupled=True)
    crit = CrossEntropyLoss()
    launches = []
    for step in range(2):
        with recording(launches, on=step == 1):
            opt.zero_grad()
            if mode == "masks":     # the masks the generator would draw in its forward number step + 1, handed back explicitly
                model.set_dropout_masks(model.generated_dropout_masks(B, step + 1))
            if mode == "head":
                with torch.no_grad():
                    model(x)
                logits = model.head(model.last_features()).logits
            elif mode == "labels":
                out = model(x, labels=y)
                logits, loss = out.logits, out.loss
            else:
                logits = model(x).logits
            if mode != "labels":
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
    for name, kind, cfg_args, attrs, frozen, size, mode in configurations():
        result[name] = run(kind, cfg_args, attrs, frozen, size, mode, dev)
        print(f"{name}: {len(result[name]['launches'])} launches", flush=True)
    write(result, out_path)


if __name__ == "__main__":
    main()
