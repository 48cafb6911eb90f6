"""Eval forward of the full-size encoders with output_attentions against without (precision "split"): ViT B = 128 (197
tokens) and AST B = 8 (1214 tokens), randomly initialised.  Informational - DESIGN.md section 4.9.

    python tools/probes/attn_outputs_time.py                 device-event times, the two forms alternated (profiler off)
    rocprofv3 --kernel-trace --stats -d DIR -o attn -- python tools/probes/attn_outputs_time.py --trace
                                                             a short run for the per-kernel times (attn_probs_kernel<true>)
"""
import sys

import torch

sys.path.insert(0, ".")
from eav_amd import synth, transformer as T  # noqa: E402

TRACE = "--trace" in sys.argv
WARM, REPS = (1, 3) if TRACE else (3, 10)


def forward_ms(model, x, attn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = model(x, output_attentions=attn)
    b.record()
    torch.cuda.synchronize()
    del out                      # (the 2.9 / 6.8 GB of probabilities go back to the allocator before the next forward)
    return a.elapsed_time(b)


for kind, B in (("vit", 128), ("ast", 8)):
    torch.manual_seed(0)
    model = T.Encoder(T.make_config(kind)).cuda().eval()
    model.precision = "split"
    x = torch.from_numpy((synth.frame_batch(1, B) if kind == "vit" else synth.mel_batch(1, B))[0]).cuda()
    times = {False: [], True: []}
    with torch.no_grad():
        for i in range(WARM + REPS):
            for attn in (False, True):
                t = forward_ms(model, x, attn)
                if i >= WARM:
                    times[attn].append(t)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    c = model.cfg
    gb = c.layers * B * c.heads * c.ntok ** 2 * 4 / 1e9
    print(f"{kind} B={B} N={c.ntok} split eval forward: {med[False]:.2f} ms without, {med[True]:.2f} ms with "
          f"output_attentions ({gb:.2f} GB of probabilities; median of {REPS}, min {min(times[False]):.2f} / "
          f"{min(times[True]):.2f}, max {max(times[False]):.2f} / {max(times[True]):.2f})", flush=True)
    del model, x
    torch.cuda.empty_cache()
