"""The encoder's modules: encoder_config is free of any device and re-exported by transformer, encoder_layers names the
eav_gemm_sp_ex flags as the header does, and Encoder keeps the attribute surface tests, bench.py and tools/ use.  No device."""
import copy
import os
import re

import pytest

from eav_amd import encoder_config as EC, encoder_layers as EL, transformer as T

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
    assert twin._wplanes is None and twin._wss == {} and twin._wss is not fresh._wss
    model._wplanes = sentinel = object()
    model.reset_head(model.classifier.weight.detach()[:3], model.classifier.bias.detach()[:3])
    assert model._wplanes is sentinel and model._flat is None and model._ws is None and model._hws == {}
