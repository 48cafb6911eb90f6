"""Time eav_augment_gather against eav_gather_rows on the batches the benchmark's trainers assemble.

    python tools/augment_bench.py [--iters 200] [--repeats 5]

Shapes: AST, 8 clips of [1024, 128] out of a 280-clip split; ViT, 128 frames of [3 x 224, 224] out of 1024 frames.  Per
shape three launches are timed, alternating, each alone on the card between device events over `--iters` launches
(launch i assembles batch i % K of one shuffled epoch of K batches, so the sources change from launch to launch):
    gather   eav_gather_rows (what DeviceLoader.gather launches)
    plain    eav_augment_gather with lambda = 1, no flip, empty bands: the same bytes as the gather
    mixup    eav_augment_gather with lambda = 0.7 and a partner per sample, two row and two column bands, flips
Bytes are counted from the shapes: the gather reads one sample and writes one, mixup reads two and writes one (cells inside
a band are written but not read: the count is the upper bound).  One JSON line per shape; the fraction is of the 8 TB/s
HBM3E peak."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eav_amd import _lib  # noqa: E402
from eav_amd.augment import BatchAugment  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = {"ast": (280, 8, 1024, 128), "vit": (1024, 128, 3 * 224, 224)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the MI355X: a CPU run measures nothing")
    st = torch.cuda.current_stream().cuda_stream
    for kind, (N, B, R, C) in SHAPES.items():
        x = torch.randn(N, R, C, device="cuda")
        y = torch.randint(0, 5, (N,), device="cuda")
        # one shuffled epoch: launch i takes the epoch's batch i % K, so the sources change from launch to launch
        order = np.random.default_rng(0).permutation(N)
        batches = [order[k:k + B].tolist() for k in range(0, N - B + 1, B)]
        K = len(batches)
        idx_dev = torch.as_tensor(batches, dtype=torch.long, device="cuda")                     # [K, B]
        plain = torch.from_numpy(BatchAugment().plan_epoch(batches, 0)).cuda()                  # [K B, record]
        mix = BatchAugment(mixup_alpha=0.4, time_mask=48, freq_mask=24, hflip=True).plan_epoch(batches, 0, (R, C))
        mix[:, 2] = np.array([0.7], dtype=np.float32).view(np.int32)[0]
        mix = torch.from_numpy(mix).cuda()
        rec = 4 * B * plain.shape[1]                                                            # bytes of a batch's records
        out = torch.empty(B, R, C, device="cuda")
        tout = torch.empty(B, 5, device="cuda")
        runs = {
            "gather": lambda k: _lib.call("eav_gather_rows", x.data_ptr(), idx_dev.data_ptr() + 8 * B * k, out.data_ptr(), B,
                                          R * C, st),
            "plain": lambda k: _lib.call("eav_augment_gather", x.data_ptr(), None, plain.data_ptr() + rec * k, 0.0,
                                         out.data_ptr(), None, B, R, C, 0, st),
            "mixup": lambda k: _lib.call("eav_augment_gather", x.data_ptr(), y.data_ptr(), mix.data_ptr() + rec * k, 0.0,
                                         out.data_ptr(), tout.data_ptr(), B, R, C, 5, st),
        }
        times = {k: [] for k in runs}
        for fn in runs.values():                    # warm up every launch
            for i in range(10):
                fn(i % K)
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, fn in runs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(args.iters):
                    fn(i % K)
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3 / args.iters)
        sample = B * R * C * 4
        nbytes = {"gather": 2 * sample, "plain": 2 * sample, "mixup": 3 * sample}
        rep = {"shape": kind, "batch": [B, R, C], "iters": args.iters}
        for k in runs:
            us = float(np.median(times[k]))
            rep[k] = {"us": round(us, 2), "us_min": round(min(times[k]), 2), "us_max": round(max(times[k]), 2),
                      "MB": round(nbytes[k] / 1e6, 2), "TB_per_s": round(nbytes[k] / us / 1e6, 3),
                      "of_hbm_peak": round(nbytes[k] / (us * 1e-6) / HBM_PEAK, 3)}
        rep["mixup_over_gather"] = round(rep["mixup"]["us"] / rep["gather"]["us"], 3)
        print(json.dumps(rep))


if __name__ == "__main__":
    main()
