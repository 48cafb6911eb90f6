#!/usr/bin/env python3
"""Encoder train step at small per-rank batches: eager two-stream (default) vs eager single-stream vs ONE hipGraph replay of
the single-stream step (forward, CE, backward, AdamW).  Prints ms per step and checks that the replayed losses equal the
eager single-stream ones bit for bit.
    python tools/encoder_graph_step.py vit 16 [steps] [--image-size N] [--freeze]
    python tools/encoder_graph_step.py ast 8 [steps] [--max-length N] [--freeze]
--image-size N (ViT): N x N frames with interpolate_pos_encoding on - the position table resampled to (N // 16)^2 patches.
--max-length N (AST): clips of N frames with variable_length on - the position table fitted to (N - 16) // 10 + 1 time patches
(N = 1024: the flag on at the native length, the same launches as without it).
--freeze: the backbone frozen (forward, head backward, AdamW on the head) - the trainers' first frozen epoch, before the
feature cache takes over.  One JSON line with the three step times and samples / s closes the output."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from eav_amd import synth, transformer as T  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam, unit_gradient  # noqa: E402


def build(kind, B, dev, overlap, capturable, image_size=None, freeze=False, max_length=None):
    torch.manual_seed(0)
    model = T.Encoder(T.make_config(kind)).to(dev).train()
    model.overlap_wgrad = overlap
    if image_size is not None:
        model.interpolate_pos_encoding = True
    if max_length is not None:
        model.variable_length = True
    if freeze:
        for k, p in model.named_parameters():
            p.requires_grad = k.startswith("classifier.")
    x, y = (synth.mel_batch(5, B, max_length or 1024) if kind == "ast" else synth.frame_batch(5, B, image_size or 224))
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=5e-6, weight_decay=0.01, decoupled=True, capturable=capturable)
    crit = CrossEntropyLoss()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = crit(model(x).logits, y)
        loss.backward(gradient=unit_gradient(dev))
        opt.step()
        return loss.detach()
    return model, step


def timeit(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=("ast", "vit"))
    ap.add_argument("batch", type=int)
    ap.add_argument("steps", type=int, nargs="?", default=12)
    ap.add_argument("--image-size", type=int, default=None)
    ap.add_argument("--max-length", type=int, default=None)
    ap.add_argument("--freeze", action="store_true")
    args = ap.parse_args()
    if args.image_size is not None and args.kind != "vit":
        ap.error("--image-size is a ViT option")
    if args.max_length is not None and args.kind != "ast":
        ap.error("--max-length is an AST option")
    kind, B, steps = args.kind, args.batch, args.steps
    dev = torch.device("cuda", 0)
    geo = (args.image_size, args.freeze, args.max_length)
    _, s2 = build(kind, B, dev, True, False, *geo)
    for _ in range(4):
        s2()
    t2 = timeit(s2, steps)
    del s2
    torch.cuda.empty_cache()
    _, s1 = build(kind, B, dev, False, True, *geo)
    ref = [float(s1()) for _ in range(4)]
    t1 = timeit(s1, steps)
    ref += [float(s1()) for _ in range(3)]
    del s1
    torch.cuda.empty_cache()
    mg, sg = build(kind, B, dev, False, True, *geo)
    got = [float(sg()) for _ in range(4)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = sg()
    mg._pin_workspace()

    def replay():
        g.replay()
        return loss
    tg = timeit(replay, steps)
    # (capture does not execute: `steps` replays = steps 5 .. 4 + steps of the trajectory)
    after = [float(replay()) for _ in range(3)]
    print(f"{kind} B={B}: eager two-stream {t2:.3f} ms, eager single-stream {t1:.3f} ms, graph replay (single stream) {tg:.3f} ms")
    print("  losses eager single-stream:", [f"{v:.6f}" for v in ref])
    print("  losses graph             :", [f"{v:.6f}" for v in got + after])
    ok = ref[:4] == got and ref[4:] == after
    print("  trajectories bit-equal:", ok)
    best = min(t2, t1, tg)
    print(json.dumps({"kind": kind, "batch": B, "image_size": args.image_size, "max_length": args.max_length, "freeze": args.freeze,
                      "eager_two_stream_ms": round(t2, 3), "eager_single_stream_ms": round(t1, 3),
                      "graph_replay_ms": round(tg, 3), "samples_per_s": round(B / best * 1e3, 1), "bit_equal": ok}))


if __name__ == "__main__":
    main()
