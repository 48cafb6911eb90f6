"""Audio CNN (eav_amd/cnn_audio.py) training-step timing at T = 180: eager and hipGraph-replayed (GraphStep) ms/step and
samples/s at B = 64 and B = 512, against the same network built from plain torch.nn layers on torch-ROCm (eager, in the
same process on the same device) as the stated comparison.

    python tools/audio_cnn_step_bench.py [--steps 50] [--warmup 10] [--batches 64,512] [--out FILE] [--only-ours]

A step is gather + forward + cross-entropy + backward + Adam; times are host clocks around work that ends in a device
synchronise.  --only-ours skips the torch.nn comparison (kernel-trace runs)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eav_amd import synth  # noqa: E402
from eav_amd.cnn_audio import AudioModel  # noqa: E402
from eav_amd.eegnet import GraphStep, gather_batch  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam  # noqa: E402

T, NC = 180, 5


def torch_net():
    """The same layers as plain torch.nn modules (generic ROCm kernels)."""
    return nn.Sequential(
        nn.Conv1d(1, 256, 5, padding=2), nn.ReLU(), nn.Conv1d(256, 128, 5, padding=2), nn.ReLU(), nn.Dropout(0.1),
        nn.MaxPool1d(8), nn.Conv1d(128, 128, 5, padding=2), nn.ReLU(), nn.Conv1d(128, 128, 5, padding=2), nn.ReLU(),
        nn.Dropout(0.5), nn.Flatten(), nn.Linear(128 * 22, NC))


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
    N = 4 * B
    xs = torch.from_numpy(synth.normal(1, (N, T, 1))).cuda()
    ys = torch.from_numpy(synth.labels(2, N, NC)).cuda()
    orders = [torch.randperm(N)[:B].tolist() for _ in range(8)]
    res = {"B": B, "T": T}
    k = [0]

    def nxt():
        k[0] += 1
        return orders[k[0] % len(orders)]

    torch.manual_seed(0)
    model = AudioModel(NC).cuda().train()
    crit, opt = CrossEntropyLoss(), FusedAdam(model.parameters(), lr=1e-3, capturable=True)

    def eager():
        data, targets = gather_batch(xs, ys, torch.as_tensor(nxt(), device="cuda"))
        opt.zero_grad()
        crit(model(data), targets).backward()
        opt.step()
    res["eager_ms"] = timed(eager, steps, warmup)
    step = GraphStep(model, opt, crit, xs, ys, B)
    res["graph_ms"] = timed(lambda: step.run(nxt()), steps, warmup + 3)
    if not only_ours:
        torch.manual_seed(0)
        net = torch_net().cuda().train()
        tcrit, topt = nn.CrossEntropyLoss(), torch.optim.Adam(net.parameters(), lr=1e-3)

        def ref():
            i = torch.as_tensor(nxt(), device="cuda")
            topt.zero_grad()
            tcrit(net(xs[i].permute(0, 2, 1)), ys[i]).backward()
            topt.step()
        res["torch_nn_eager_ms"] = timed(ref, steps, warmup)
    for key in [k_ for k_ in res if k_.endswith("_ms")]:
        res[key.replace("_ms", "_samples_per_s")] = B / res[key] * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="64,512")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-ours", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("audio_cnn_step_bench: needs the MI355X (no CPU timing)")
    rows = [bench(int(b), a.steps, a.warmup, a.only_ours) for b in a.batches.split(",")]
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "rows": rows}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
