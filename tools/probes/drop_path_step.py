#!/usr/bin/env python3
"""Encoder training step (AST B = 8, 1 214 tokens / ViT B = 128, 197 tokens; split precision) with Encoder.drop_path_rate
alternated inside ONE process between 0, 0.1 and 0.2 - the box-to-box spread (3-4 %) is larger than the differences looked
for, and the r = 0 column launches what a model without the attribute launches.  Layers with p_i > 0 (all but layer 0) pay two
element-wise passes in the forward, two gates, two eav_sp_absmax and the unfused LayerNorm-backward / conversion path in the
backward.  Also times eav_drop_path_add alone at the step's own (B, tokens x hidden) and the plan kernel.  Prints the device
clock next to the numbers.
usage: drop_path_step.py ast|vit [B] [reps] [r,r,...]"""
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from eav_amd import _lib, synth, transformer as T  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam  # noqa: E402

kind = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else (8 if kind == "ast" else 128)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rates = [float(p) for p in (sys.argv[4].split(",") if len(sys.argv) > 4 else ("0", "0.1", "0.2"))]
_lib.load()
model = T.Encoder(T.make_config(kind)).cuda().train()
model.precision = "split"
has_feature = hasattr(model, "drop_path_rate")        # (the same file measures the r = 0 column on a tree without the feature)
if not has_feature:
    rates = [0.0]
x, y = (synth.mel_batch(5, B) if kind == "ast" else synth.frame_batch(5, B))
x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
opt, crit = FusedAdam(model.parameters(), lr=5e-6, weight_decay=0.01, decoupled=True), CrossEntropyLoss()


def step():
    opt.zero_grad()
    crit(model(x).logits, y).backward()
    opt.step()


def set_rate(r):
    if has_feature:
        model.drop_path_rate = r


for r in rates:                 # every rate's buffers exist before anything is timed
    set_rate(r)
    for _ in range(3):
        step()
ts = {r: [] for r in rates}
for k in range(reps):
    for r in rates[k % len(rates):] + rates[:k % len(rates)]:
        set_rate(r)
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(6):
            step()
        torch.cuda.synchronize()
        ts[r].append((time.perf_counter() - t0) / 6 * 1e3)


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
for r, v in ts.items():
    m = statistics.median(v)
    print(f"{kind} B={B} drop_path_rate={r:<5g} {m:7.2f} ms/step  {B / m * 1e3:8.1f} samples/s  "
          f"({m / base - 1:+.1%} vs r={rates[0]:g})  " + " ".join(f"{t:.2f}" for t in v), flush=True)
print(f"{kind} {clock}", flush=True)

if has_feature:                 # the two kernels alone
    from eav_amd import encoder_drop_path as dp
    c = model.cfg
    per = c.ntok * c.hidden
    scale = torch.empty(c.layers, 2, B, dtype=torch.float32, device="cuda")
    cnt = torch.ones((), dtype=torch.int64, device="cuda")
    yb, rb = torch.randn(B, per, device="cuda"), torch.randn(B, per, device="cuda")
    st = _lib.stream_ptr()
    row = scale.data_ptr() + 4 * B * (2 * c.layers - 1)

    def timed(fn, n=100):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    t_plan = timed(lambda: dp.plan(scale, 0.2, dp.plan_seed(1), cnt))
    t_add = timed(lambda: _lib.call("eav_drop_path_add", yb.data_ptr(), rb.data_ptr(), yb.data_ptr(), row, B, per, st))
    t_gate = timed(lambda: _lib.call("eav_drop_path_add", yb.data_ptr(), None, rb.data_ptr(), row, B, per, st))
    gb = B * per * 4 / 1e9
    print(f"{kind} eav_drop_path_plan L={c.layers} B={B}: {t_plan:.2f} us per launch (100 back to back)", flush=True)
    print(f"{kind} eav_drop_path_add B={B} per_sample={per}: {t_add:.2f} us in place with resid ({3 * gb / t_add * 1e3:.2f} TB/s), "
          f"{t_gate:.2f} us gate ({2 * gb / t_gate * 1e3:.2f} TB/s)", flush=True)
