#!/usr/bin/env python3
"""The optimiser step over an AST-sized flat buffer (run on the GPU): what the bias / LayerNorm no-decay split costs on
the one-launch-per-run path and on the job-table path (csrc/adam_jobs.hip).

  (a) one group                 FusedAdam: a single eav_adam_step launch over the 86.2 M parameters
  (b) no-decay split            FusedAdam with two param groups: one eav_adam_step launch per contiguous run
  (c) no-decay split, table     FusedAdam(multi_tensor=True), the same two groups: eav_adam_jobs_begin + eav_adam_step_jobs

Every step is bracketed by HIP events; after 10 warm-up steps the median of 30 is reported (with the fastest and the
slowest), the variants taken in turn so that drift hits them alike, with the launches per step (counted at _lib.call) and
GB/s over the 28 bytes per parameter AdamW must move (16 read, 12 written), and the host wall time of the step() call
itself (nothing synchronises inside it) over the same steps.  The parameters keep changing, the gradient
is constant.  `--encoder` adds whole training steps of the reduced (2 layers, 64 wide) and the full ViT at B = 128 with
the trainers' learning-rate options off and on (layer decay 0.75, no-decay split, linear schedule).

`--avg` times weight averaging (FusedAdam.set_averaging) on the same layout, one group, the job-table path:
  (a) the step without averaging            eav_adam_jobs_begin + eav_adam_step_jobs                 28 B/param
  (b) the fused averaging step              eav_adam_jobs_begin_avg + eav_adam_step_jobs_avg (EMA)   36 B/param
  (c) (a), then torch._foreach_lerp_        the average as a separate pass over the same tensors     40 B/param
All timed steps of (b) are lerp steps (the copy falls into the warm-up).  The spread is reported as min / max and as the
median absolute deviation.

usage: adam_jobs_bench.py [--encoder | --avg] [--out FILE]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eav_amd import _lib, synth, transformer as T  # noqa: E402
from eav_amd.encoder_config import param_shapes  # noqa: E402
from eav_amd.finetune import encoder_no_decay, encoder_param_groups  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam, LRSchedule, WeightAveraging, flatten_parameters  # noqa: E402

WARMUP, TIMED = 10, 30
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def clock_text():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        got = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(got) if got else "clock: not available"
    except Exception as e:          # noqa: BLE001 - the tool is optional on a box
        return f"clock: not available ({type(e).__name__})"


def ast_sized_module():
    """A module with the parameters of AST-base (names and shapes of param_shapes) on the device."""
    cfg = T.make_config("ast")
    module = torch.nn.Module()
    names = []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for i, (name, shape) in enumerate(param_shapes(cfg).items()):
        p = torch.nn.Parameter(torch.randn(shape, device="cuda", generator=gen) * 0.02)
        module.register_parameter(f"p{i}", p)
        names.append(name)
    return module, names


def timed_steps(variants):
    """variants: {label: step function}.  Returns ({label: [ms] * TIMED}, {label: [host ms] * TIMED}), the variants
    interleaved step by step; the host time is the wall time of the call itself, which synchronises with nothing."""
    for _ in range(WARMUP):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times, host = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(TIMED):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            fn()
            host[k].append(1e3 * (time.perf_counter() - t0))
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return times, host


def launches_of(fn):
    names, real = [], _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        fn()
    finally:
        _lib.call = real
    torch.cuda.synchronize()
    return names


def optimiser_bench():
    opts = {}
    for label in ("a", "b", "c"):
        module, names = ast_sized_module()
        flat, gflat, _ = flatten_parameters(module)
        gflat.copy_(torch.randn(gflat.numel(), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 1e-3)
        params = list(module.parameters())
        for p in params:
            off = p._eav_flat[2]
            p.grad = gflat[off:off + p.numel()].view(p.shape)
        if label == "a":
            groups = [{"params": params}]
        else:
            groups = [{"params": [p for p, n in zip(params, names) if not encoder_no_decay(n)]},
                      {"params": [p for p, n in zip(params, names) if encoder_no_decay(n)], "weight_decay": 0.0}]
        opts[label] = (FusedAdam(groups, lr=5e-6, weight_decay=0.01, decoupled=True, multi_tensor=label == "c"),
                       sum(p.numel() for p in params), flat.numel(), len(params))
    n, nflat, ntensors = opts["a"][1:]
    say(f"AST-base layout: {ntensors} tensors, {n} parameters ({nflat} floats in the flat buffer), fp32 p / g / m / v")
    times, host = timed_steps({k: v[0].step for k, v in opts.items()})
    what = {"a": "one group, single eav_adam_step", "b": "no-decay split, one eav_adam_step per run",
            "c": "no-decay split, job table (begin + step_jobs)"}
    for k in ("a", "b", "c"):
        names = launches_of(opts[k][0].step)
        ms = statistics.median(times[k])
        say(f"({k}) {what[k]}: median {ms:.3f} ms per step (min {min(times[k]):.3f}, max {max(times[k]):.3f}, {TIMED} steps), "
            f"{len(names)} launches per step, {28 * n / ms / 1e6:.0f} GB/s over 28 B/param; host time of step() median "
            f"{statistics.median(host[k]):.3f} ms (min {min(host[k]):.3f}, max {max(host[k]):.3f})")


def averaging_bench():
    decay = 0.999
    opts = {}
    for label in ("a", "b", "c"):
        module, _ = ast_sized_module()
        flat, gflat, _ = flatten_parameters(module)
        gflat.copy_(torch.randn(gflat.numel(), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 1e-3)
        params = list(module.parameters())
        for p in params:
            off = p._eav_flat[2]
            p.grad = gflat[off:off + p.numel()].view(p.shape)
        opt = FusedAdam(params, lr=5e-6, weight_decay=0.01, decoupled=True, multi_tensor=True)
        step = opt.step
        if label == "b":
            opt.set_averaging(WeightAveraging("ema", decay))
        elif label == "c":
            data = [p.data for p in params]
            avgs = [d.clone() for d in data]

            def step(opt=opt, data=data, avgs=avgs):
                opt.step()
                torch._foreach_lerp_(avgs, data, 1.0 - decay)
        opts[label] = (step, sum(p.numel() for p in params), len(params))
    n, ntensors = opts["a"][1:]
    say(f"AST-base layout: {ntensors} tensors, {n} parameters, one group, FusedAdam(multi_tensor=True), EMA decay {decay}")
    times, host = timed_steps({k: v[0] for k, v in opts.items()})
    what = {"a": ("step without averaging", 28), "b": ("fused averaging step", 36),
            "c": ("step without averaging + torch._foreach_lerp_", 40)}
    for k in ("a", "b", "c"):
        torch_launches = []
        if k == "c":            # the lerp's own kernels are not library calls: count them with the profiler
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                torch._foreach_lerp_(avgs, data, 1.0 - decay)
                torch.cuda.synchronize()
            torch_launches = [e for e in prof.events() if e.device_type.name != "CPU"]
        names = launches_of(opts[k][0])
        ms = statistics.median(times[k])
        mad = statistics.median(abs(t - ms) for t in times[k])
        label, nbytes = what[k]
        say(f"({k}) {label}: median {ms:.3f} ms per step (min {min(times[k]):.3f}, max {max(times[k]):.3f}, MAD {mad:.4f}, "
            f"{TIMED} steps), {len(names)} library launches per step"
            + (f" + {len(torch_launches)} of torch's" if k == "c" else "")
            + f", {nbytes * n / ms / 1e6:.0f} GB/s over {nbytes} B/param; host time median "
            f"{statistics.median(host[k]):.3f} ms (min {min(host[k]):.3f}, max {max(host[k]):.3f})")


def encoder_bench(label, cfg, B):
    x, y = synth.frame_batch(5, B, cfg.H)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    crit = CrossEntropyLoss()
    runs = {}
    for on in (False, True):
        torch.manual_seed(0)
        model = T.Encoder(cfg).cuda().train()
        opt = FusedAdam(model.parameters(), lr=5e-6, weight_decay=0.01, decoupled=True)
        if on:
            template = {k: v for k, v in opt.param_groups[0].items() if k != "params"}
            opt.param_groups = [dict(template, **g) for g in encoder_param_groups(model, 5e-6, 0.01, 0.75, False)]
            opt.set_schedule(LRSchedule("linear", 4, 10 ** 6))

        def step(model=model, opt=opt):
            opt.zero_grad()
            crit(model(x).logits, y).backward()
            opt.step()
        runs["options on" if on else "options off"] = step
    times, _ = timed_steps(runs)
    for k, fn in runs.items():
        names = launches_of(fn)
        adam = [n for n in names if n.startswith("eav_adam") or n.startswith("eav_counter")]
        say(f"{label} B={B} training step, {k}: median {statistics.median(times[k]):.3f} ms (min {min(times[k]):.3f}, max "
            f"{max(times[k]):.3f}), {len(names)} launches per step, {len(adam)} of them the optimiser's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", action="store_true")
    ap.add_argument("--avg", action="store_true", help="time the weight-averaging step instead (module docstring)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    global TIMED
    if not torch.cuda.is_available():
        sys.exit("adam_jobs_bench.py measures on the GPU: no device found")
    say(f"{torch.cuda.get_device_name(0)}; {clock_text()}; HIP events around every step, {WARMUP} warm-up, median of {TIMED}")
    if args.avg:
        averaging_bench()
    else:
        optimiser_bench()
    if args.encoder:
        encoder_bench("reduced ViT (2 layers, 64 wide, 56 x 56)",
                      T.make_config("vit", hidden=64, layers=2, heads=4, ff=128, image=56), 128)
        TIMED = 20
        encoder_bench("ViT-base", T.make_config("vit"), 128)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
