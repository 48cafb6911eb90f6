#!/usr/bin/env python3
"""One subject's recording through the rational-rate resampler: [30, 2 000 000] float64 at 500 Hz -> 128 Hz (32 / 125),
resident on the device.

    python tools/eeg_resample_bench.py [--out profiles/eeg_resample_bench.json]

The `kernel` leg is a child process under its own time limit (if it fails the run ends): eav_resample_poly_f64 through
eeg_data.resample, 20 timed launches after 5 warm-up launches, device events around the library call itself, the median
reported.  `scipy` is scipy.signal.resample_poly of the same array on the host in the same run (one warm-up call, the
median of 3).  GB/s are over the algorithmic bytes - the input read once, the output written once - and the fraction is
of the 6.3 TB/s a tuned streaming copy reaches on the MI355X (8 TB/s peak); fma/s counts one fma per tap and output."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS, SAMPLES, UP, DOWN = 30, 2_000_000, 32, 125
WARMUP, TIMED = 5, 20
HBM_COPY_TBPS = 6.3


def recording():
    import numpy as np
    from eav_amd import synth
    return synth.normal(11, (CHANNELS, SAMPLES), 0.0, 1.0).astype(np.float64)


def kernel_leg():
    import numpy as np
    import torch
    from eav_amd import _lib
    from eav_amd.eeg_data import resample, resample_poly_design
    x = torch.from_numpy(recording()).cuda()
    n_out = -(-SAMPLES * UP // DOWN)
    _lib.TRACE = {}                          # events directly around the library call: no allocator / wrapper time
    for _ in range(WARMUP + TIMED):
        y = resample(x, UP, DOWN)
    torch.cuda.synchronize()
    assert y.shape == (CHANNELS, n_out)
    ms = [a.elapsed_time(b) for a, b in _lib.TRACE["eav_resample_poly_f64"][WARMUP:]]
    med = float(np.median(ms))
    ntaps = len(resample_poly_design(UP, DOWN)[0])
    nbytes = 8 * CHANNELS * (SAMPLES + n_out)
    fmas = CHANNELS * n_out * ntaps / UP      # every output meets ntaps / up taps (to within one)
    print(json.dumps({"leg": "kernel", "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "algorithmic_bytes": nbytes, "gbps": round(nbytes / med / 1e6, 1),
                      "frac_of_copy_rate": round(nbytes / med / 1e9 / HBM_COPY_TBPS, 3),
                      "gfma_per_s": round(fmas / med / 1e6, 1), "checksum": float(y.abs().sum())}))


def scipy_leg():
    import numpy as np
    from scipy.signal import resample_poly
    x = recording()
    s = []
    for _ in range(4):
        t0 = time.perf_counter()
        y = resample_poly(x, UP, DOWN, axis=1)
        s.append((time.perf_counter() - t0) * 1e3)
    return {"leg": "scipy", "ms": round(float(np.median(s[1:])), 1), "ms_min": round(min(s[1:]), 1), "ms_max": round(max(s[1:]), 1),
            "checksum": float(np.abs(y).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("kernel",))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_resample_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for the kernel leg")
    args = ap.parse_args()
    if args.leg:
        return kernel_leg()
    res = {"job": f"[{CHANNELS}, {SAMPLES}] float64, resample_poly {UP} / {DOWN} (500 -> 128 Hz), device resident",
           "launches": {"warmup": WARMUP, "timed": TIMED, "statistic": "median of device-event times"}}
    r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", "kernel"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"leg kernel ended with status {r.returncode}; nothing further is started\n{r.stderr[-3000:]}")
    res["kernel"] = json.loads(r.stdout.strip().splitlines()[-1])
    res["scipy"] = scipy_leg()
    res["scipy_over_kernel"] = round(res["scipy"]["ms"] / res["kernel"]["ms"], 1)
    res["checksum_gap"] = abs(res["scipy"]["checksum"] - res["kernel"]["checksum"]) / res["scipy"]["checksum"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
