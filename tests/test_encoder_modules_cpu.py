"""The encoder's modules: encoder_config is free of any device and re-exported by transformer, encoder_layers names the
eav_gemm_sp_ex flags as the header does, and Encoder keeps the attribute surface tests, bench.py and tools/ use.  No device."""
import copy
import os
import re

import pytest

from eav_amd import (encoder_config as EC, encoder_dropout as ED, encoder_head as EH, encoder_layers as EL,
                     encoder_outputs as EO, optim, transformer as T)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("HEAD_MAX_CLASSES", "MAX_TOKENS", "PROBLEM_TYPES", "make_config", "config_from_hf", "config_to_hf", "_check_single_label",
         "resolve_problem_type", "param_shapes", "normalise_key", "rank_dropout_seed", "interpolated_geometry",
         "ast_length_geometry")
ENV = ("EAV_ENCODER_PRECISION", "EAV_HEAD_ALGO", "EAV_GRAD_TERMS", "EAV_WGRAD_TERMS", "EAV_DGRAD_TERMS", "EAV_FWD_TERMS",
       "EAV_FUSED_PLANES", "EAV_FUSED_DACT", "EAV_FUSED_AO", "EAV_FUSED_QKV", "EAV_FUSED_DQKV", "EAV_FUSED_DH")


def test_encoder_config_is_device_free_and_reexported_by_transformer():
    src = open(EC.__file__).read()
    assert set(re.findall(r"^from \.(\w*) import", src, flags=re.M)) == set() and "\nimport eav_amd" not in src
    imports = "\n".join(re.findall(r"^\s*(?:from|import)\s.*$", src, flags=re.M))
    for forbidden in ("_lib", "runtime", "weight_planes", "pos_interp", "pos_time", "eav_amd"):
        assert forbidden not in imports, (forbidden, imports)
    for name in MOVED:
        assert getattr(T, name) is getattr(EC, name), name
        if callable(getattr(EC, name)):
            assert getattr(EC, name).__module__ == "eav_amd.encoder_config", name


def test_gemm_flag_constants_are_the_headers():
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define EAV_GEMM_(\w+)\s+(\d+)\b", header, flags=re.M)}
    assert set(defines) == {"ONE_TERM", "SHARED_GPU", "PLANES_NOLIFT", "NO_BLOCKMAX"}, defines
    for name, value in defines.items():
        assert getattr(EL, f"GEMM_{name}") == value, name
    assert EL.SLOT == int(re.search(r"^#define EAV_SP_SLOT\s+(\d+)", header, flags=re.M).group(1))
    # the slot indices eav_tf_forward_scales_qkv is given, and the order the layer functions unpack
    assert (EL.F_Y1, EL.F_QKV, EL.F_AO, EL.F_Y2, EL.F_ACT, EL.FS) == (0, 1, 2, 3, 4, 5)
    assert (EL.B_DH2, EL.B_DACT, EL.B_DH1, EL.B_DAO, EL.B_DS, EL.B_DQKV, EL.B_DY2, EL.B_DY1, EL.BS) == (0, 1, 2, 3, 4, 5, 6, 7, 8)


def test_encoder_keeps_its_attribute_surface_and_deepcopies_its_schedules(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    model = T.Encoder(T.make_config("vit", hidden=32, layers=1, heads=2, ff=64, image=32))
    defaults = dict(precision=T.DEFAULT_PRECISION, head_algo="auto", overlap_wgrad="auto", grad_terms=3, wgrad_terms=None,
                    dgrad_terms=None, fwd_terms=3, fused_planes=True, fused_dact=True, fused_ao=True, fused_qkv=True,
                    fused_dqkv=True, fused_dh=True, kernel_events=None, grad_ready_hook=None, interpolate_pos_encoding=False,
                    variable_length=False, _flat=None, _ws=None, _wss={}, _hws={}, _wplanes=None, _active_geo=None,
                    _fwd_counter=None)
    for name, value in defaults.items():
        assert getattr(model, name) == value and type(getattr(model, name)) is type(value), name
    assert T.DEFAULT_PRECISION == "split" and isinstance(model.dropout_seed, int)
    assert not hasattr(model, "use_fused_attention") and model._fused_attention() is False      # (head_dim 16)
    assert model._names == list(T.param_shapes(model.cfg)) and not hasattr(model, "_pmap")    # (_pmap: made by _ensure_flat)
    for name in ("_ensure_flat", "_weight_keys", "_head_wide", "_fused_attention", "_join_wgrads", "_two_streams",
                 "_pin_workspace", "_check_token", "_require_gpu"):
        assert callable(getattr(model, name)), name
    assert model._head_wide() is False and model._two_streams() is False
    model._join_wgrads()                                    # nothing is in flight: touches no stream
    model._ensure_flat()
    assert set(model._pmap) == set(model._names)
    # both schedules exist from construction on, the precision picks one per forward
    assert isinstance(model._fp32, EL.Fp32Layers) and isinstance(model._split, EL.SplitLayers)
    assert model._fp32.m is model and model._split.m is model and model._split.streams.m is model
    # ... and so do the head, the dropout generator and the extra outputs
    assert isinstance(model._head, EH.EncoderHead) and isinstance(model._dropgen, ED.EncoderDropout)
    assert isinstance(model._outputs, EO.EncoderOutputs)
    assert model._head.m is model and model._dropgen.m is model and model._outputs.m is model
    assert model._outs is None and model._out_flags == (None, None)
    assert not hasattr(model, "_want_outs") and not hasattr(model, "_rollout")
    model.precision = "no such precision"
    with pytest.raises(ValueError, match="unknown precision 'no such precision'"):
        model._fp32.gemm_name()
    model.precision = "bf16_bwd"
    assert model._fp32.gemm_name() == "eav_gemm_f32"
    model._phase = "bwd"
    assert model._fp32.gemm_name() == "eav_gemm_bf16"
    model.grad_terms, model.wgrad_terms = 1, 2
    assert (model._split.terms("dgrad"), model._split.terms("wgrad"), model._split.bwd_three_terms()) == (1, 2, False)
    fresh = T.Encoder(model.cfg)
    twin = copy.deepcopy(fresh)
    assert twin._fp32.m is twin and twin._split.m is twin and twin._split.streams.m is twin
    assert twin._split is not fresh._split and twin._fp32 is not fresh._fp32 and fresh._split.m is fresh
    assert twin._head.m is twin and twin._dropgen.m is twin and twin._outputs.m is twin
    assert twin._head is not fresh._head and twin._dropgen is not fresh._dropgen and twin._outputs is not fresh._outputs
    assert fresh._head.m is fresh and fresh._dropgen.m is fresh and fresh._outputs.m is fresh
    assert twin._wplanes is None and twin._wss == {} and twin._wss is not fresh._wss
    model._wplanes = sentinel = object()
    model.reset_head(model.classifier.weight.detach()[:3], model.classifier.bias.detach()[:3])
    assert model._wplanes is sentinel and model._flat is None and model._ws is None and model._hws == {}


def test_dropout_sites_come_from_one_table():
    cfg = T.make_config("vit", hidden=32, layers=2, heads=2, ff=64, image=32, hidden_dropout=0.1, attention_dropout=0.2)
    model = T.Encoder(cfg)
    B, N, D, H = 3, cfg.ntok, 32, 2
    hid, att = (B, N, D), (B, H, N, N)
    table = {"emb": (0, hid, 0.1),
             "attn.0": (1, att, 0.2), "attn_out.0": (2, hid, 0.1), "mlp_out.0": (3, hid, 0.1),
             "attn.1": (4, att, 0.2), "attn_out.1": (5, hid, 0.1), "mlp_out.1": (6, hid, 0.1)}
    sites = model.dropout_sites(B)
    assert sites == table and list(sites) == list(table)                 # (HF's call order)
    model.cfg.attention_dropout = 0.0
    assert model.dropout_sites(B) == {k: v for k, v in table.items() if not k.startswith("attn.")}
    model.cfg.attention_dropout, model.cfg.hidden_dropout = 0.2, 0.0
    assert model.dropout_sites(B) == {k: v for k, v in table.items() if k.startswith("attn.")}
    # the kernel arguments of a site: its probability, the seed of its id, no mask, the counter's address
    for seed in (0, 12345, (1 << 64) - 1):
        d = ED.DropState(seed, 0.1, 0.2, cnt=4242)
        for name, (sid, _, p) in table.items():
            kind, _, layer = name.partition(".")
            assert ED.site_id(kind, int(layer or 0)) == sid and ED.site_name(kind, int(layer or 0)) == name
            assert d.site(kind, int(layer or 0)) == (p, (seed + ((sid + 1) << 40)) % (1 << 64), None, 4242), name
    assert d.site("emb") == d.site("emb", 0)


def test_head_routing_is_one_function():
    """optim.head_is_wide answers, and refuses, as Encoder._head_wide and CrossEntropyLoss._wide did each on their own."""
    def old(algo, n, last):
        if algo not in ("auto", "wide", "narrow"):
            raise ValueError(f"head_algo {algo!r}: expected 'auto', 'wide' or 'narrow'")
        if algo == "narrow" and n > 16:
            raise NotImplementedError(f"head_algo 'narrow' takes at most 16 classes, {last} {n}")
        return algo == "wide" or (algo == "auto" and n > 16)

    def outcome(fn):
        try:
            return fn()
        except (ValueError, NotImplementedError) as e:
            return type(e), str(e)

    crit = optim.CrossEntropyLoss()
    for n in (16, 17):
        enc = T.Encoder(T.make_config("vit", hidden=32, layers=1, heads=2, ff=64, image=32, num_labels=n))
        for algo in ("auto", "wide", "narrow", "mfma"):
            enc.head_algo = crit.head_algo = algo
            for last, caller in (("the head has", enc._head_wide), ("the scores have", lambda: crit._wide(n))):
                want = outcome(lambda: old(algo, n, last))
                assert outcome(lambda: optim.head_is_wide(algo, n, last)) == want, (algo, n, last)
                assert outcome(caller) == want, (algo, n, last)
    assert optim.head_is_wide("auto", 16, "") is False and optim.head_is_wide("auto", 17, "") is True
    assert outcome(lambda: optim.head_is_wide("narrow", 17, "the head has")) == (
        NotImplementedError, "head_algo 'narrow' takes at most 16 classes, the head has 17")
    assert outcome(lambda: optim.head_is_wide("mfma", 16, "the head has"))[0] is ValueError
