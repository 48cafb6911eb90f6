"""Video CNN (eav_amd/cnn_vision.py) training-step timing at 224 x 224: ms/step and images/s at B = 32 (the reference
driver's batch) and B = 128, frozen (backbone forward in training mode + head forward / backward) and unfrozen (full
step), against the same network built from plain torch.nn layers on torch-ROCm (eager, same process, same device).

    python tools/video_cnn_step_bench.py [--steps 10] [--warmup 3] [--batches 32,128] [--out FILE] [--only-ours]

A step is forward + cross-entropy + backward + AdamW (weight decay 0.01) on a resident batch; times are host clocks around
work that ends in a device synchronise.  The FLOP count is computed from the shapes (forward 2 x MACs of every conv and
Linear; a full step 3 x forward, a frozen step the forward plus the head's backward)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eav_amd import synth  # noqa: E402
from eav_amd.cnn_vision import VideoModel, _plan  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam  # noqa: E402
from tests.video_cnn_ref import TvVideoModel  # noqa: E402

NC, HW = 5, 224
PEAK_TFLOPS = 157.3       # MI355X dense fp32 matrix peak


def flops_per_image(model):
    stem, _, blocks, (fh, fw) = _plan(model, HW, HW)
    units = [stem] + [u for b in blocks for u in b if u is not None]
    conv = sum(2 * u.OH * u.OW * u.Co * u.Ci * u.k * u.k for u in units)
    head = 2 * (2 * 2 * 2048 * 2048 + 2048 * 1024 + 1024 * NC)
    return conv, head


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench(B, steps, warmup, only_ours):
    x = torch.from_numpy(synth.normal(1, (B, 3, HW, HW))).cuda()
    y = torch.from_numpy(synth.labels(2, B, NC)).cuda()
    res = {"B": B, "image": HW}
    for freeze in (True, False):
        tag = "frozen" if freeze else "unfrozen"
        torch.manual_seed(0)
        model = VideoModel(NC).cuda().train()
        for p in model.feature_extractor.parameters():
            p.requires_grad = not freeze
        crit, opt = CrossEntropyLoss(), FusedAdam(model.parameters(), lr=1e-4, weight_decay=0.01, decoupled=True)

        def ours():
            opt.zero_grad()
            crit(model(x), y).backward()
            opt.step()
        res[f"{tag}_ms"] = timed(ours, steps, warmup)
        if not only_ours:
            torch.manual_seed(0)
            net = TvVideoModel(NC).cuda().train()
            for p in net.feature_extractor.parameters():
                p.requires_grad = not freeze
            tcrit, topt = nn.CrossEntropyLoss(), torch.optim.AdamW(net.parameters(), lr=1e-4)

            def ref():
                topt.zero_grad()
                tcrit(net(x), y).backward()
                topt.step()
            res[f"{tag}_torch_nn_ms"] = timed(ref, steps, warmup)
            res[f"{tag}_speedup_vs_torch_nn"] = res[f"{tag}_torch_nn_ms"] / res[f"{tag}_ms"]
        del model, opt
        torch.cuda.empty_cache()
    conv, head = flops_per_image(VideoModel(NC))
    step_flop = B * 3 * (conv + head)
    res["fwd_gflop_per_image"] = (conv + head) / 1e9
    res["unfrozen_step_gflop"] = step_flop / 1e9
    res["unfrozen_floor_ms_at_peak"] = step_flop / (PEAK_TFLOPS * 1e12) * 1e3
    res["unfrozen_fraction_of_peak"] = res["unfrozen_floor_ms_at_peak"] / res["unfrozen_ms"]
    res["images_per_s_unfrozen"] = B / res["unfrozen_ms"] * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-ours", action="store_true")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "results": []}
    for B in [int(b) for b in a.batches.split(",")]:
        r = bench(B, a.steps, a.warmup, a.only_ours)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
