#!/usr/bin/env python3
"""What an EEGNet_tor training step launches, and what it computes, as one JSON - to compare two commits that should issue the
same step (a refactor of the host code): run it on both with the same built library (EAV_LIB_PATH) and diff the files.
    python tools/eegnet_launch_trace.py out.json
Every configuration runs two steps (B = 4, nb_classes = 5, torch.manual_seed(0), FusedAdam(capturable=True); train mode,
dropout 0.5, Chans = 30, kernLength = 64 unless its name says otherwise).  Per configuration the JSON holds `step`, the ordered
launches of the second step, and `sha256` of that step's scores and loss, of its gradients and of the parameters after its
optimiser step; launch_trace.py has the recorder and the file format.  The configurations: every branch of the fast path's
step (FIR and separableConv algorithm, conv_fuse, eval-mode step, dropout kinds, max-norm, the fused no-grad forward), the
indexed input of GraphStep with and without the eav_step_begin merge (its two eager warm-up steps: nothing is captured), the
generic widths, and one step of each other model that runs the shared BatchNorm / dropout glue.  Only the public surface of the
package is used."""
import sys

import numpy as np
import torch

from launch_trace import digest, recording, write      # (puts the repository root on sys.path)
from eav_amd import synth  # noqa: E402
from eav_amd.eegnet import EEGNet_tor, GraphStep  # noqa: E402
from eav_amd.optim import CrossEntropyLoss, FusedAdam  # noqa: E402

B, NB = 4, 5
FAST = dict(Chans=30, kernLength=64)
GENERIC = dict(F1=4, D=2, F2=16, kernLength=32, Chans=5, Samples=128)
IDX = [6, 1, 4, 3]          # of 8 samples: not contiguous, so the gather is real


def configurations():
    """[(name, EEGNet_tor arguments, attributes, mode)]: mode "train" / "eval" = an eager step in that mode, "graph-train" /
    "graph-eval" = through GraphStep.run, "infer" / "infer-indexed" = a no-grad eval-mode forward, "masks" = explicit masks."""
    out = []
    algos = [("S500", 500, {}), ("S1408", 1408, {}),
             ("S1408-convfft-fused", 1408, dict(conv_algo="fft", conv_fuse=True)),
             ("S1408-convfft-unfused", 1408, dict(conv_algo="fft", conv_fuse=False))]
    for name, S, attrs in algos:
        for mode in ("train", "eval"):
            out.append((f"{name}-{mode}", dict(FAST, Samples=S), attrs, mode))
    out.append(("S502-eval", dict(FAST, Samples=502), {}, "eval"))
    out.append(("S500-spatial-dropout", dict(FAST, Samples=500, dropoutType="SpatialDropout2D"), {}, "train"))
    out.append(("S500-masks", dict(FAST, Samples=500), {}, "masks"))
    out.append(("S500-no-max-norm", dict(FAST, Samples=500), dict(apply_max_norm=False), "train"))
    out.append(("S500-fused-eval", dict(FAST, Samples=500), dict(fused_eval=True), "infer"))
    out.append(("S500-fused-eval-indexed", dict(FAST, Samples=500), dict(fused_eval=True), "infer-indexed"))
    for conv in ("fft", "mfma"):
        for mode in ("train", "eval"):
            out.append((f"S1408-graphstep-conv{conv}-{mode}", dict(FAST, Samples=1408), dict(conv_algo=conv), "graph-" + mode))
    # (a train-mode GraphStep on the FFT FIR path takes the weight gradient from the input tables; this one reads y1)
    out.append(("S1408-graphstep-convfft-train-xtab-off", dict(FAST, Samples=1408), dict(conv_algo="fft", fir_xtab=False),
                "graph-train"))
    for mode in ("train", "eval"):       # the MFMA FIR pair's indexed entry points
        out.append((f"S500-graphstep-{mode}", dict(FAST, Samples=500), {}, "graph-" + mode))
    out.append(("generic-train", GENERIC, {}, "train"))
    out.append(("generic-graphstep-train", GENERIC, {}, "graph-train"))
    return out


def traced_steps(model, step):
    """Two calls of step() -> (scores, loss or None); the second recorded."""
    launches = []
    for k in range(2):
        with recording(launches, on=k == 1):
            scores, loss = step()
    torch.cuda.synchronize()
    sha = {"scores": digest(scores)}
    if loss is not None:
        sha.update(loss=digest(loss), gradients=digest(*[p.grad for p in model.parameters() if p.grad is not None]),
                   parameters=digest(*model.parameters()))
    return {"launches": launches, "sha256": sha}


def eager(model, x, y, before=None):
    opt, crit = FusedAdam(model.parameters(), lr=1e-3, capturable=True), CrossEntropyLoss()

    def step():
        if before is not None:
            before()
        opt.zero_grad()
        scores = model(x)
        loss = crit(scores, y)
        loss.backward()
        opt.step()
        return scores, loss

    return traced_steps(model, step)


def run_eegnet(args, attrs, mode, dev):
    torch.manual_seed(0)
    model = EEGNet_tor(NB, **args).to(dev)
    for k, v in attrs.items():
        setattr(model, k, v)
    C, S = args["Chans"], args["Samples"]
    x, y = synth.eeg_batch(5, 8, C, S)
    xs, ys = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    model.train(mode in ("train", "masks", "graph-train"))
    if mode.startswith("graph-"):
        gs = GraphStep(model, FusedAdam(model.parameters(), lr=1e-3, capturable=True), CrossEntropyLoss(), xs, ys, B)
        return traced_steps(model, lambda: gs.run(IDX))
    if mode.startswith("infer"):
        idx = torch.tensor(IDX, dtype=torch.long, device=dev)

        def forward():
            with torch.no_grad():
                return (model.forward_indexed(xs, idx) if mode == "infer-indexed" else model(xs[:B])), None

        return traced_steps(model, forward)
    before = None
    if mode == "masks":
        bits = lambda seed, n: torch.from_numpy((synth.splitmix64(seed, B * 64 * n) & np.uint64(1)).astype(np.uint8)  # noqa: E731
                                                .reshape(B, 64, n)).to(dev)
        masks = (bits(11, S // 4), bits(12, S // 32))
        before = lambda: model.set_dropout_masks(masks)  # noqa: E731
    return eager(model, xs[:B], ys[:B], before)


def run_shared(name, dev):
    """One other model each that runs KernelModule's BatchNorm launches and the saved-forward record."""
    torch.manual_seed(0)
    if name == "cnn_eeg":
        from eav_amd.cnn_eeg import EEGNet
        model = EEGNet(NB, Chans=8, Samples=128).to(dev).train()
        x, y = synth.eeg_batch(5, B, 8, 128)
    elif name == "shallow":
        from eav_amd.transformer_eeg import ShallowConvNet
        model = ShallowConvNet(nb_classes=NB, num_layers=2).to(dev).train()
        x, y = synth.eeg_batch(5, B, 30, 500)
    else:
        from eav_amd.cnn_vision import VideoModel
        model = VideoModel(NB).to(dev).train()
        x, y = synth.normal(5, (2, 3, 64, 64)), synth.labels(6, 2, NB)
    return eager(model, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "eegnet_launch_trace.json"
    dev = torch.device("cuda", 0)
    result = {}
    for name, args, attrs, mode in configurations():
        result[name] = run_eegnet(args, attrs, mode, dev)
        print(f"{name}: {len(result[name]['launches'])} launches", flush=True)
    for name in ("cnn_eeg", "shallow", "video"):
        result[name] = run_shared(name, dev)
        print(f"{name}: {len(result[name]['launches'])} launches", flush=True)
    write(result, out_path)


if __name__ == "__main__":
    main()
