#!/usr/bin/env python3
"""The encoder's wide classification head alone: forward + cross-entropy + backward at three shapes.

    python tools/head_wide_bench.py [--out profiles/head_wide_bench.json]

(B, hidden, classes) = (8, 768, 527) the stock AST checkpoint at the audio trainer's ragged last batch, (128, 768, 1000) a
stock ViT-B at the vision trainer's batch, (128, 1024, 21843) an ImageNet-21k head on a ViT-L width.

Two legs, each a child process under its own time limit (a leg that fails ends the run):

`head` times the head-only step - and, separately, its dense products (`dense_only`, the figure the choice between the
two rests on) and its loss (`loss_only`) - two ways, alternating them launch by launch in one process: `wide` =
eav_dense_wide_fwd, eav_ce_wide_fwd_bwd, eav_dense_wide_bwd (csrc/head_wide.hip), and `composition` = the same products from the kernels the
library had before: eav_gemm_f32 with the bias epilogue for the logits, eav_ce_fwd_bwd for the loss, eav_gemm_f32 with
transposed operands for dw and din, eav_colsum + eav_reduce_partials for dbias.  eav_gemm_f32 takes leading dimensions
that are multiples of 4, so the composition runs with the class count rounded UP to one (528, 1000, 21844) - at 527 or
21843 classes it could not run at all.  Each way is captured once as a hipGraph and replayed: 20 timed replays after 5
warm-up replays, device events around each replay, the median reported (`eager_ms`: the same with plain launches, where
the host's enqueue time shows).  GB/s = the bytes of w read once plus dw written once over the wide time.

`step` times one unfrozen training step (forward, loss, backward; no optimiser) of a 2-layer encoder of that width with
that head, so that the head's share of it can be stated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 768, 527), (128, 768, 1000), (128, 1024, 21843)]
STEP_MODELS = [("ast", dict(heads=12, ff=3072)), ("vit", dict(heads=12, ff=3072)), ("vit", dict(heads=16, ff=4096))]
WARMUP, TIMED = 5, 20
STEP_WARMUP, STEP_TIMED = 2, 5


def _median_ms(fns, warmup, timed):
    """Median device-event time of each callable, the callables alternating launch by launch."""
    import numpy as np
    import torch
    ms = [[] for _ in fns]
    for i in range(warmup + timed):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[j].append(a.elapsed_time(b))
    return [dict(ms=round(float(np.median(m)), 4), ms_min=round(min(m), 4), ms_max=round(max(m), 4)) for m in ms]


def head_leg():
    import torch
    from eav_amd import _lib, synth
    P = _lib.ptr
    out = []
    for B, NF, NC in SHAPES:
        NCp = (NC + 3) // 4 * 4
        dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")  # noqa: E731
        x, w, bias = dev(synth.normal(1, (B, NF))), dev(synth.normal(2, (NCp, NF), 0.0, 0.02)), dev(synth.normal(3, (NCp,), 0.0, 0.02))
        y = torch.from_numpy(synth.labels(4, B)).cuda()
        flag, loss = torch.zeros((), dtype=torch.int32, device="cuda"), f(())
        # wide: NC classes (the first NC rows of w)
        lg, dl, dw, db, din = f(B, NC), f(B, NC), f(NC, NF), f(NC), f(B, NF)
        ws = f(max(1, _lib.plain("eav_dense_wide_bwd_ws_floats", B, NF, NC)))
        cws = f(_lib.plain("eav_ce_wide_ws_floats", B))

        def wide(dense=True, ce=True):
            st = _lib.stream_ptr()
            if dense:
                _lib.call("eav_dense_wide_fwd", P(x), P(w), P(bias), P(lg), B, NF, NC, st)
            if ce:
                _lib.call("eav_ce_wide_fwd_bwd", P(lg), P(y), P(loss), P(dl), None, P(flag), P(cws), B, NC, st)
            if dense:
                _lib.call("eav_dense_wide_bwd", P(dl), P(x), P(w), P(dw), P(db), P(din), P(ws), B, NF, NC, st)

        # composition: NCp classes
        lg2, dl2, dw2, db2, din2, loss2 = f(B, NCp), f(B, NCp), f(NCp, NF), f(NCp), f(B, NF), f(())
        npart = _lib.plain("eav_colsum_nparts", B)
        part = f(npart, NCp)

        def composition(dense=True, ce=True):
            st = _lib.stream_ptr()
            g = lambda A, Bm, C, M, N, K, lda, ldb, ldc, tA, tB, bs: _lib.call(  # noqa: E731
                "eav_gemm_f32", A, Bm, C, M, N, K, lda, ldb, ldc, tA, tB, 1, 1, 0, 0, 0, 0, 0, 0, 1.0, bs, 0, None, None, 0, 0, st)
            if dense:
                g(P(x), P(w), P(lg2), B, NCp, NF, NF, NF, NCp, 0, 0, P(bias))
            if ce:
                _lib.call("eav_ce_fwd_bwd", P(lg2), P(y), P(loss2), P(dl2), None, P(flag), B, NCp, st)
            if dense:
                g(P(dl2), P(x), P(dw2), NCp, NF, B, NCp, NF, NF, 1, 1, None)
                _lib.call("eav_colsum", P(dl2), P(part), B, NCp, NCp, st)
                _lib.call("eav_reduce_partials", P(part), npart, NCp, NCp, 1.0, P(db2), st)
                g(P(dl2), P(w), P(din2), B, NF, NCp, NCp, NF, NF, 0, 1, None)

        wide()
        composition()
        torch.cuda.synchronize()
        # same seeded inputs: the two ways agree (the composition's extra classes move the softmax a little)
        gap = {"logits": float((lg - lg2[:, :NC]).abs().max()), "dw_rel": float((dw - dw2[:NC]).abs().max() / dw.abs().max()),
               "loss": [float(loss), float(loss2)]}
        eager = _median_ms([wide, composition], WARMUP, TIMED)
        # the whole step, then its dense products (logits, dw, dbias, din) and its loss alone, each way
        graphs = []
        for kw in ({}, {"ce": False}, {"dense": False}):
            for fn in (wide, composition):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    fn(**kw)
                graphs.append(gr.replay)
        timed = _median_ms(graphs, WARMUP, TIMED)
        nbytes = 2 * 4 * NC * NF
        r = {"B": B, "hidden": NF, "classes": NC, "composition_classes": NCp,
             "wide": dict(timed[0], eager_ms=eager[0]["ms"]), "composition": dict(timed[1], eager_ms=eager[1]["ms"]),
             "wide_over_composition": round(timed[0]["ms"] / timed[1]["ms"], 3),
             "dense_only": {"wide": timed[2], "composition": timed[3],
                            "wide_over_composition": round(timed[2]["ms"] / timed[3]["ms"], 3)},
             "loss_only": {"wide": timed[4], "composition": timed[5],
                           "wide_over_composition": round(timed[4]["ms"] / timed[5]["ms"], 3)},
             "w_read_plus_dw_written_bytes": nbytes, "gbps": round(nbytes / timed[0]["ms"] / 1e6, 1), "agreement": gap}
        out.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(out))


def step_leg():
    import numpy as np
    import torch
    from eav_amd import synth, transformer as T
    from eav_amd.optim import CrossEntropyLoss
    out = []
    for (B, NF, NC), (kind, kw) in zip(SHAPES, STEP_MODELS):
        torch.manual_seed(0)
        model = T.Encoder(T.make_config(kind, hidden=NF, layers=2, num_labels=NC, **kw)).cuda().train()
        x = torch.from_numpy(synth.mel_batch(5, B, 1024, 128)[0] if kind == "ast" else synth.frame_batch(5, B, 224)[0]).cuda()
        y = torch.from_numpy((synth.splitmix64(6, B) % np.uint64(NC)).astype(np.int64)).cuda()
        crit = CrossEntropyLoss()

        def step():
            for p in model.parameters():
                p.grad = None
            crit(model(x).logits, y).backward()
        r = _median_ms([step], STEP_WARMUP, STEP_TIMED)[0]
        r.update(B=B, hidden=NF, classes=NC, model=f"{kind}, 2 layers, precision {model.precision}")
        out.append(r)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("head", "step"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_wide_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        return head_leg() if args.leg == "head" else step_leg()
    res = {"job": "classification head alone: forward + cross-entropy + backward, fp32",
           "launches": {"warmup": WARMUP, "timed": TIMED, "statistic": "median of device-event times around hipGraph replays"}}
    legs = {}
    for name in ("head", "step"):
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"leg {name} ended with status {r.returncode}; nothing further is started\n{r.stderr[-3000:]}")
        legs[name] = json.loads(r.stdout.strip().splitlines()[-1])
    res["shapes"] = legs["head"]
    for h, s in zip(res["shapes"], legs["step"]):
        h["unfrozen_step"] = s
        h["head_share_of_step"] = round(h["wide"]["ms"] / s["ms"], 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
