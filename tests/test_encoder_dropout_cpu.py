"""Encoder dropout without a GPU: the configuration surface, the trainers' cache gate, the replicas' seeds, and the
fixtures themselves - the pure-torch restatement of the four sites (tests/encoder_dropout_ref.py) reproduces what the
Hugging Face classes produced with the same explicit masks (tests/golden/encoder_dropout_{ast,vit}.npz), which pins the
fixtures and the mask order."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import encoder_dropout_ref as R

AST_JSON = {"model_type": "audio-spectrogram-transformer", "hidden_size": 128, "num_hidden_layers": 2,
            "num_attention_heads": 2, "intermediate_size": 256, "num_mel_bins": 128, "max_length": 256,
            "id2label": {str(i): str(i) for i in range(5)}}
VIT_JSON = {"model_type": "vit", "hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 2,
            "intermediate_size": 256, "image_size": 224, "id2label": {str(i): str(i) for i in range(5)}}


@pytest.mark.parametrize("cfg_json", [AST_JSON, VIT_JSON], ids=["ast", "vit"])
def test_config_from_hf_carries_both_dropout_fields(cfg_json):
    from eav_amd import transformer as T
    c = T.config_from_hf(dict(cfg_json, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.3))
    assert c.hidden_dropout == pytest.approx(0.1) and c.attention_dropout == pytest.approx(0.3)
    c0 = T.config_from_hf(cfg_json)                               # absent fields: HF's defaults, 0.0
    assert c0.hidden_dropout == 0.0 and c0.attention_dropout == 0.0
    assert T.make_config(c.kind).hidden_dropout == 0.0 and T.make_config(c.kind).attention_dropout == 0.0


@pytest.mark.parametrize("field", ["hidden_dropout", "attention_dropout"])
@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5])
def test_make_config_rejects_probabilities_outside_0_1(field, p):
    from eav_amd import transformer as T
    with pytest.raises(ValueError, match=field):
        T.make_config("vit", **{field: p})
    with pytest.raises(ValueError, match=field):
        T.config_from_hf(dict(VIT_JSON, **{{"hidden_dropout": "hidden_dropout_prob",
                                            "attention_dropout": "attention_probs_dropout_prob"}[field]: p}))
    assert getattr(T.make_config("vit", **{field: 0.999}), field) == pytest.approx(0.999)


def test_dropout_sites_follow_the_hf_call_order_and_shapes():
    from eav_amd import transformer as T
    m = T.Encoder(T.make_config("vit", hidden_dropout=0.1, attention_dropout=0.2, **R.MODEL))
    sites = m.dropout_sites(3)
    assert list(sites) == R.site_names(2, 0.1, 0.2)
    assert sites["emb"][1] == (3, 197, 128) and sites["attn.1"][1] == (3, 2, 197, 197) and sites["mlp_out.0"][1] == (3, 197, 128)
    assert len({sid for sid, _, _ in sites.values()}) == len(sites)            # one stream per site
    assert sites["attn.0"][2] == pytest.approx(0.2) and sites["attn_out.0"][2] == pytest.approx(0.1)
    m0 = T.Encoder(T.make_config("vit", attention_dropout=0.2, **R.MODEL))
    assert list(m0.dropout_sites(1)) == ["attn.0", "attn.1"] and m0.dropout_active()
    assert not T.Encoder(T.make_config("vit", **R.MODEL)).dropout_active()


def test_dropout_seed_follows_the_torch_seed_and_ranks_get_their_own():
    from eav_amd import transformer as T
    cfg = T.make_config("vit", hidden_dropout=0.1, **R.MODEL)
    torch.manual_seed(11)
    a = T.Encoder(cfg).dropout_seed
    torch.manual_seed(11)
    b = T.Encoder(cfg).dropout_seed
    torch.manual_seed(12)
    c = T.Encoder(cfg).dropout_seed
    assert isinstance(a, int) and a == b == 11 and c == 12
    seeds = {T.rank_dropout_seed(a, r) for r in range(8)}
    assert len(seeds) == 8 and T.rank_dropout_seed(a, 0) == a and all(0 <= s < 2 ** 64 for s in seeds)
    m = T.Encoder(cfg)
    m.mix_dropout_rank(3)
    assert m.dropout_seed == T.rank_dropout_seed(12, 3)


def test_no_two_streams_are_shifted_copies_of_each_other():
    """eav_hash32(seed, idx) finalises seed + (idx + 1) G, G = 0x9E3779B97F4A7C15: two streams whose seeds differ by k G are
    the same stream shifted by k elements.  The seed offsets between ranks (rank_dropout_seed), forward counters (2 c) and
    sites ((site + 1) << 40) must therefore not be k G (mod 2^64) for any |k| a tensor can hold (< 2^40 elements)."""
    from eav_amd import transformer as T
    G, M = 0x9E3779B97F4A7C15, (1 << 64) - 1
    inv = pow(G, -1, 1 << 64)

    def shift(offset):                       # the |k| with k G == offset (mod 2^64)
        k = (offset * inv) & M
        return min(k, (-k) & M)
    ranks = [T.rank_dropout_seed(0, r) for r in range(1, 1025)]
    offsets = ranks + [(a - b) & M for a in ranks[:64] for b in ranks[:64] if a != b]
    offsets += [2 * c for c in range(1, 1 << 16)] + [s << 40 for s in range(1, 3 * 64 + 2)]
    offsets += [(r + 2 * c) & M for r in ranks[:8] for c in range(1, 64)]
    assert min(shift(o) for o in offsets) > 1 << 40


@pytest.mark.parametrize("ph,pa,cached", [(0.0, 0.0, True), (0.1, 0.0, False), (0.0, 0.2, False), (0.1, 0.1, False)])
def test_trainers_bypass_the_frozen_feature_cache_under_dropout(capsys, ph, pa, cached):
    from eav_amd import transformer as T
    from eav_amd.finetune import FineTuneBase
    tr = FineTuneBase()
    tr.model = SimpleNamespace(cfg=T.make_config("vit", hidden_dropout=ph, attention_dropout=pa, **R.MODEL))
    tr.device, tr.grad_sync = torch.device("cpu"), None
    tr.train_dataloader = SimpleNamespace(dataset=range(6))
    tr.test_dataloader = SimpleNamespace(dataset=range(4))
    tr._begin_phase_cache(True)
    said = capsys.readouterr().out
    assert (tr._feat_cache is not None) == cached
    assert ("cache bypassed" in said) == (not cached) and said.count("\n") == (0 if cached else 1)
    tr._begin_phase_cache(False)                                   # the unfrozen phase never caches and says nothing
    assert tr._feat_cache is None and capsys.readouterr().out == ""


@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_torch_restatement_reproduces_the_hf_goldens(golden_dir, kind, case):
    """fp32 CPU torch against fp32 CPU HF with the same masks: the two differ by the order of a few fp32 operations (HF's
    fused linear / layer-norm calls against the restated ones), i.e. by rounding - logits and loss within 2e-5, gradients
    within 1e-4 of the tensor's maximum (a hundredth of the GPU tests' bound), AdamW's post-step parameters by the rule of
    test_reduced_model_training_steps_match_hf.  A wrong mask order or a misplaced site moves the logits by 1e-1."""
    g = np.load(os.path.join(golden_dir, f"encoder_dropout_{kind}.npz"))
    assert (int(g["wseed"]), int(g["xseed"]), int(g["mseed"]), int(g["B"])) == (R.WSEED[kind], R.XSEED, R.MSEED, R.BATCH)
    others = [os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir)
              if f.endswith(".npz") and not f.startswith("encoder_dropout_")]
    assert os.path.getsize(os.path.join(golden_dir, f"encoder_dropout_{kind}.npz")) <= max(others)   # no larger than the largest
    out = R.run_case(kind, case)
    lr = float(g["lr"])
    for s in (0, 1):
        assert np.abs(out[f"logits{s}"].numpy() - g[f"{case}.logits{s}"]).max() <= 2e-5
        assert abs(float(out[f"loss{s}"]) - float(g[f"{case}.loss{s}"])) <= 2e-5
        gkeys = sorted(k[len(f"{case}.grad{s}."):] for k in g.files if k.startswith(f"{case}.grad{s}.") and "#" not in k)
        assert gkeys == sorted(k[len(f"grad{s}."):] for k in out if k.startswith(f"grad{s}."))
        assert len(gkeys) == (4 if kind == "ast" else 2) if s == 1 else len(gkeys) > 30
        for k in gkeys:
            smp, sa, mx = R.summarise(out[f"grad{s}.{k}"])
            ref, rmax = g[f"{case}.grad{s}.{k}"], float(g[f"{case}.grad{s}.{k}#maxabs"])
            tol = max(1e-4 * rmax, 1e-6)      # (floor of the GPU test: k_proj.bias gradients are rounding noise around 0)
            assert np.abs(smp - ref).max() <= tol, (k, np.abs(smp - ref).max(), rmax)
            assert abs(mx - rmax) <= tol and abs(sa - float(g[f"{case}.grad{s}.{k}#sumabs"])) <= tol * out[f"grad{s}.{k}"].numel() + 1e-4 * sa
            err = np.abs(R.summarise(out[f"post{s}.{k}"])[0].astype(np.float64) - g[f"{case}.post{s}.{k}"])
            assert err.max() <= 2.1 * lr, (k, err.max())
            if not k.endswith("k_proj.bias"):
                assert (err <= 0.05 * lr).mean() >= 0.97, (k, (err <= 0.05 * lr).mean())
    # the cases differ from the control by far more than any bound above: the masks took effect
    if case != "d":
        assert np.abs(g[f"{case}.logits0"] - g["d.logits0"]).max() > 1e-2


def test_dropout_kernel_instantiations_are_scratch_free():
    """Every dropout instantiation on the default dropout path compiles for gfx950 without scratch: the DROP forms of the three
    fused fp32 attention kernels keep the occupancy of the forms without dropout (3 / 2 / 2 waves per SIMD) - the dK,dV
    kernel sits at 229 VGPRs without dropout and forms its keep bits in a rolled loop to stay there - and the element-wise /
    softmax kernels of csrc/tf_dropout.hip.  The DROP = false forms are what they were.  hipcc cross-compiles: no GPU needed."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.resources(os.path.join(root, "eav_amd", "csrc", "attention.hip"))
    occ = {"attn_fwd_kernel": 3, "attn_bwd_q_kernel": 2, "attn_bwd_kv_kernel": 2}
    seen = set()
    for r in rows:
        assert int(r["ScratchSize"]) == 0, (r["demangled"], r["ScratchSize"])
        for name, o in occ.items():
            if name + "<" in r["demangled"]:
                seen.add((name, "<true>" in r["demangled"]))
                assert int(r["Occupancy"]) == o and int(r["AGPRs"]) == 0, r
    assert seen == {(n, d) for n in occ for d in (True, False)}, seen
    # split-precision fused attention: the DROP forms that are launched - forward <4> / <2>, dQ <4>, dK,dV <4> - without scratch
    # at the occupancy of the forms without dropout (the 2-wave dQ form would need 12 bytes of scratch and is not built)
    rows = kr.resources(os.path.join(root, "eav_amd", "csrc", "attention_sp.hip"), ["-fno-slp-vectorize"])
    drop = [r for r in rows if ", true>" in r["demangled"]]
    names = sorted(r["demangled"].split("(")[0] for r in drop)
    assert names == ["void attn_bwd_kv_sp_kernel<4, true>", "void attn_bwd_q_sp_kernel<4, true>",
                     "void attn_fwd_sp_kernel<2, true>", "void attn_fwd_sp_kernel<4, true>"], names
    for r in rows:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs"]) <= 256 and int(r["AGPRs"]) == 0, r
    for r in drop:
        assert int(r["Occupancy"]) == (3 if "attn_fwd" in r["demangled"] else 2), r
    rows = kr.resources(os.path.join(root, "eav_amd", "csrc", "tf_dropout.hip"))
    assert len(rows) == 8, [r["demangled"] for r in rows]
    for r in rows:
        assert int(r["ScratchSize"]) == 0, (r["demangled"], r["ScratchSize"])
