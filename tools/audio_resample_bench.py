#!/usr/bin/env python3
"""One subject's worth of audio through the resampler: 100 files x 20 s at 44.1 kHz -> 16 kHz, resident on the device.

    python tools/audio_resample_bench.py [--out profiles/audio_resample_bench.json]

Two legs, each a child process under its own time limit (a leg that fails ends the run): `kernel` times
eav_resample_sinc_f32 (one launch for the 100 rows), `conv1d` the same job in torchaudio's own form, F.conv1d of the padded
batch with every stored tap at stride orig.  20 timed launches after 5 warm-up launches, device events around each launch
(around the library call itself in the kernel leg),
the median reported (the conv1d leg times the convolution alone, not the transpose that puts its phases back into sample
order).  GB/s are over the algorithmic bytes - the input read once, the output written once - and the
fraction is of the 6.3 TB/s a tuned streaming copy reaches on the MI355X (8 TB/s peak)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILES, SECONDS, RATE, TARGET = 100, 20, 44100, 16000
WARMUP, TIMED = 5, 20
HBM_COPY_TBPS = 6.3


def leg(name):
    import numpy as np
    import torch
    from eav_amd import _lib, synth
    from eav_amd.preprocess import resample_waveforms, resampled_length, sinc_resample_design
    n = SECONDS * RATE
    taps, width, orig, new = sinc_resample_design(RATE, TARGET)
    n_out = resampled_length(n, orig, new)
    x = torch.from_numpy(synth.normal(7, (FILES, n), 0.0, 0.1)).cuda()
    if name == "kernel":
        run, finish = (lambda: resample_waveforms(x, RATE, TARGET)), (lambda o: o)
    else:
        xp = torch.nn.functional.pad(x[:, None], (width, width + orig))
        w = torch.from_numpy(taps).cuda()[:, None, :]
        # timed: the convolution alone; its [file, phase, frame] result still needs a transpose to sample order
        run = lambda: torch.nn.functional.conv1d(xp, w, stride=orig)  # noqa: E731
        finish = lambda o: o.transpose(1, 2).reshape(FILES, -1)[:, :n_out]  # noqa: E731
    ms = []
    _lib.TRACE = {}                         # events directly around the library call: no allocator / wrapper time in the kernel leg
    for i in range(WARMUP + TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = run()
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
    if name == "kernel":
        ms = [a.elapsed_time(b) for a, b in _lib.TRACE["eav_resample_sinc_f32"][WARMUP:]]
    y = finish(y)
    assert y.shape == (FILES, n_out)
    med = float(np.median(ms))
    nbytes = 4 * FILES * (n + n_out)
    print(json.dumps({"leg": name, "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "algorithmic_bytes": nbytes, "gbps": round(nbytes / med / 1e6, 1),
                      "frac_of_copy_rate": round(nbytes / med / 1e9 / HBM_COPY_TBPS, 3),
                      "checksum": float(y.double().abs().sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("kernel", "conv1d"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_resample_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg)
    res = {"job": f"{FILES} files x {SECONDS} s, {RATE} -> {TARGET} Hz, fp32, device resident",
           "launches": {"warmup": WARMUP, "timed": TIMED, "statistic": "median of device-event times"}}
    for name in ("kernel", "conv1d"):
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"leg {name} ended with status {r.returncode}; nothing further is started\n{r.stderr[-3000:]}")
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    res["conv1d_over_kernel"] = round(res["conv1d"]["ms"] / res["kernel"]["ms"], 2)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
