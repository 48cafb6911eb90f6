#!/usr/bin/env python3
"""Encoder training step (AST B = 8, 1 214 tokens / ViT B = 128, 197 tokens; split precision) with Encoder.patch_dropout
alternated inside ONE process between 0, 0.25 and 0.5 - the box-to-box spread (3-4 %) is larger than some of the differences
looked for, and the p = 0 column launches what a model without the attribute launches.  Also times the plan kernel alone at
the step's own (B, P, K).  Prints the device clock next to the numbers.
usage: patch_dropout_step.py ast|vit [B] [reps] [p,p,...]"""
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from eav_amd import _lib, patch_keep, synth, transformer as T  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam  # noqa: E402

kind = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else (8 if kind == "ast" else 128)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rates = [float(p) for p in (sys.argv[4].split(",") if len(sys.argv) > 4 else ("0", "0.25", "0.5"))]
_lib.load()
model = T.Encoder(T.make_config(kind)).cuda().train()
model.precision = "split"
x, y = (synth.mel_batch(5, B) if kind == "ast" else synth.frame_batch(5, B))
x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
opt, crit = FusedAdam(model.parameters(), lr=5e-6, weight_decay=0.01, decoupled=True), CrossEntropyLoss()


def step():
    opt.zero_grad()
    crit(model(x).logits, y).backward()
    opt.step()


for p in rates:                 # every rate's workspace exists before anything is timed
    model.patch_dropout = p
    for _ in range(3):
        step()
ts = {p: [] for p in rates}
for r in range(reps):
    for p in rates[r % len(rates):] + rates[:r % len(rates)]:
        model.patch_dropout = p
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(6):
            step()
        torch.cuda.synchronize()
        ts[p].append((time.perf_counter() - t0) / 6 * 1e3)


def clock_text():
    """sclk / mclk as rocm-smi shows them right after the timed loops (a query only)."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        got = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(got) if got else "clock: not available"
    except Exception as e:          # noqa: BLE001 - the tool is optional on a box
        return f"clock: not available ({type(e).__name__})"


clock = clock_text()
base = statistics.median(ts[rates[0]])
for p, v in ts.items():
    m = statistics.median(v)
    K = T.patch_dropout_geometry(model.cfg, p).npatch
    print(f"{kind} B={B} patch_dropout={p:<5g} K={K:5d} tokens={K + model.cfg.nextra:5d} {m:7.2f} ms/step  {B / m * 1e3:8.1f} samples/s  "
          f"({m / base - 1:+.1%} vs p={rates[0]:g})  " + " ".join(f"{t:.2f}" for t in v), flush=True)
print(f"{kind} {clock}", flush=True)

# the plan kernel alone
P = model.cfg.npatch
K = T.patch_dropout_geometry(model.cfg, 0.5).npatch
keep = torch.empty(B, K, dtype=torch.int32, device="cuda")
inv = torch.empty(B, P, dtype=torch.int32, device="cuda")
cnt = torch.ones((), dtype=torch.int64, device="cuda")
for _ in range(3):
    patch_keep.keep_plan(keep, inv, P, patch_keep.plan_seed(1), cnt)
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(100):
    patch_keep.keep_plan(keep, inv, P, patch_keep.plan_seed(1), cnt)
b.record()
torch.cuda.synchronize()
print(f"{kind} eav_patch_keep_plan B={B} P={P} K={K}: {a.elapsed_time(b) * 10:.2f} us per launch (100 back to back)", flush=True)
