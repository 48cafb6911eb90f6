"""Patch dropout without a device: the numpy plan (tests/patch_keep_ref.py), timm's keep count, the geometry, the seed
stream, the declarations and the trainer / command-line surface."""
import os
import re

import numpy as np
import pytest

from eav_amd import encoder_config as EC, encoder_dropout as ED, transformer as T
from tests import patch_keep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("eav_patch_keep_plan", "eav_patch_keep_invert", "eav_im2col_keep", "eav_embed_finish_keep", "eav_embed_bwd_keep")


@pytest.mark.parametrize("B,P,K", R.PLAN_CASES)
def test_plan_rows_are_ascending_unique_and_inverted(B, P, K):
    keep, inv = R.plan(B, P, K, R.plan_seed(99), 3)
    assert keep.shape == (B, K) and inv.shape == (B, P) and keep.dtype == inv.dtype == np.int32
    assert (keep >= 0).all() and (keep < P).all() and (np.diff(keep, axis=1) > 0).all()
    for b in range(B):
        assert np.array_equal(inv[b, keep[b]], np.arange(K))
        assert (inv[b] >= 0).sum() == K and set(inv[b][inv[b] < 0]) <= {-1}
        # the kept set is the K smallest of (key, p)
        key = R.hash32(R.plan_seed(99), B * P, 3).reshape(B, P)[b].astype(np.int64) * 4096 + np.arange(P)
        assert set(keep[b]) == set(np.argsort(key, kind="stable")[:K])
    assert np.array_equal(R.invert(keep, P), inv)


def test_planted_ties_fall_to_the_smaller_index():
    for P, K in ((10, 4), (3, 1), (300, 150), (2046, 1023)):
        for name, keys, want in R.tie_cases(P, K):
            keep, inv = R.plan(1, P, K, 0, keys=keys)
            assert np.array_equal(keep[0], want), (P, K, name)
            assert np.array_equal(inv, R.invert(keep, P))
    # the largest 32-bit key is a key like any other
    keys = np.array([[0xFFFFFFFF, 0, 0xFFFFFFFF, 1]], np.uint32)
    assert np.array_equal(R.plan(1, 4, 3, 0, keys=keys)[0], [[0, 1, 3]])


def test_keep_count_is_timms_rule():
    for P in (1, 16, 196, 300, 1212, 2046):
        assert EC.patch_dropout_keep(P, 0.0) == P
        assert EC.patch_dropout_keep(P, 0.5) == max(1, P // 2)
        assert EC.patch_dropout_keep(P, 0.999) == max(1, int(P * (1.0 - 0.999)))
        for p in (0.0, 0.25, 0.5, 0.643, 0.999):
            assert EC.patch_dropout_keep(P, p) == R.keep_count(P, p) == max(1, int(P * (1.0 - p)))
    assert EC.patch_dropout_keep(196, 0.999) == 1 and EC.patch_dropout_keep(1212, 0.999) == 1 and EC.patch_dropout_keep(2046, 0.999) == 2
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            EC.patch_dropout_keep(196, bad)
    for name, c in R.MODEL_CASES.items():
        assert EC.patch_dropout_keep(c["P"], c["p"]) == c["K"], name


def test_geometry_composes_with_the_other_geometries():
    vit = T.make_config("vit", hidden=64, layers=2, heads=4, ff=128)
    g = EC.patch_dropout_geometry(vit, 0.5)
    assert (g.grid_npatch, g.npatch, g.ntok, g.ny, g.nx, g.H, g.W) == (196, 98, 99, 14, 14, 224, 224)
    assert (vit.npatch, vit.ntok) == (196, 197) and not hasattr(vit, "grid_npatch")          # pure: cfg is untouched
    gi = EC.patch_dropout_geometry(EC.interpolated_geometry(vit, 112, 64), 0.25)
    assert (gi.grid_npatch, gi.npatch, gi.ntok, gi.ny, gi.nx, gi.pos_grid) == (28, 21, 22, 7, 4, 14)
    ast = T.make_config("ast", hidden=64, layers=2, heads=4, ff=128, frames=256)
    ga = EC.patch_dropout_geometry(EC.ast_length_geometry(ast, 96), 0.5)
    assert (ga.grid_npatch, ga.npatch, ga.ntok, ga.nx, ga.W, ga.time_grid) == (108, 54, 56, 9, 96, 25)
    gn = EC.patch_dropout_geometry(ast, 0.999)
    assert (gn.grid_npatch, gn.npatch, gn.ntok) == (300, 1, 3)
    assert EC.patch_dropout_geometry(ast, 0.0).npatch == 300
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError):
            EC.patch_dropout_geometry(ast, bad)
    # the FULL grid has to fit the position kernels and the plan: dropping does not make an oversized grid legal
    big = T.make_config("vit", hidden=64, layers=1, heads=4, ff=128)
    big.npatch, big.ntok = EC.MAX_TOKENS, EC.MAX_TOKENS + 1
    with pytest.raises(NotImplementedError):
        EC.patch_dropout_geometry(big, 0.9)
    assert T.patch_dropout_geometry is EC.patch_dropout_geometry


def test_counter_and_rank_give_other_subsets():
    B, P, K = 4, 300, 150
    seed = 1234
    a = R.plan(B, P, K, R.plan_seed(seed), 1)[0]
    assert not np.array_equal(a, R.plan(B, P, K, R.plan_seed(seed), 2)[0])
    assert np.array_equal(a, R.plan(B, P, K, R.plan_seed(seed), 1)[0])
    seen = [a]
    for rank in (1, 2, 3):
        k = R.plan(B, P, K, R.plan_seed(EC.rank_dropout_seed(seed, rank)), 1)[0]
        assert all(not np.array_equal(k, s) for s in seen), rank
        # ... and not rank 0's table shifted by a few samples either
        assert all(not np.array_equal(k[0], s[b]) for s in seen for b in range(B)), rank
        seen.append(k)
    assert EC.rank_dropout_seed(seed, 0) == seed


def test_seed_stream_is_a_site_of_its_own():
    from eav_amd import patch_keep
    sid = ED.site_id("patch_keep")
    assert sid == R.PATCH_KEEP_SITE == ED.site_id("patch_keep", 7)              # (no per-layer stride)
    assert sid > ED.site_id("mlp_out", 100000) and sid + 1 < (1 << 24)          # no layer count reaches it; 24 bits hold it
    for seed in (0, 12345, (1 << 64) - 1):
        assert patch_keep.plan_seed(seed) == R.plan_seed(seed) == ED.site_seed(seed, sid)
    # the dropout sites of a model are what they were
    cfg = T.make_config("vit", hidden=32, layers=2, heads=2, ff=64, image=32, hidden_dropout=0.1, attention_dropout=0.2)
    assert list(T.Encoder(cfg).dropout_sites(2)) == ["emb", "attn.0", "attn_out.0", "mlp_out.0", "attn.1", "attn_out.1", "mlp_out.1"]


def test_entry_points_are_declared_bound_and_exported():
    from eav_amd import _lib
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    assert int(re.search(r"^#define EAV_MAX_TOKENS\s+(\d+)", header, flags=re.M).group(1)) == EC.MAX_TOKENS
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in KERNELS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name)
    src = open(os.path.join(ROOT, "eav_amd", "csrc", "patch_keep.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")
    # refused before any launch
    for args in ((1, 1, 1, 0, 1), (1, 1, 1, 5, 6), (1, 1, 1, EC.MAX_TOKENS, 1), (1, 1, 0, 4, 2)):
        with pytest.raises(_lib.EavError, match="eav_patch_keep_plan"):
            _lib.call("eav_patch_keep_plan", *args, 0, None, None, None)


def test_encoder_surface_and_refusals_without_a_device():
    import torch
    model = T.Encoder(T.make_config("vit", hidden=32, layers=1, heads=2, ff=64, image=32))
    assert model.patch_dropout == 0.0
    for name in ("set_patch_keep", "generated_patch_keep", "last_patch_keep"):
        assert callable(getattr(model, name))
    model.set_patch_keep(torch.tensor([[0, 2], [1, 3]]))
    model.set_patch_keep(None)
    for bad in ([[2, 0]], [[1, 1]], [[-1, 2]], [0, 1], [[0.5, 1.5]]):
        with pytest.raises(ValueError):
            model.set_patch_keep(torch.tensor(bad))
    from eav_amd import _lib
    with pytest.raises(_lib.EavError):
        model.last_patch_keep()


def test_trainer_attribute_and_command_line_flag():
    from eav_amd.finetune import FineTuneBase
    assert FineTuneBase.patch_dropout == 0.0
    tool = open(os.path.join(ROOT, "tools", "run_finetune_subjects.py")).read()
    assert '"--patch-dropout"' in tool and "tr.patch_dropout = args.patch_dropout" in tool
    # the flag as the tool declares it: parsed as a float, default 0
    import argparse
    decl = re.search(r'ap\.add_argument\("--patch-dropout".*?\)\n', tool, flags=re.S).group(0)
    ap = argparse.ArgumentParser()
    exec(decl, {"ap": ap})
    assert ap.parse_args([]).patch_dropout == 0.0 and ap.parse_args(["--patch-dropout", "0.25"]).patch_dropout == 0.25
    # ... and reaches the model through the phase set-up: unfrozen phases only

    class Stub(FineTuneBase):
        def __init__(self):
            self.model = T.Encoder(T.make_config("vit", hidden=32, layers=1, heads=2, ff=64, image=32))

    tr = Stub()
    tr.patch_dropout = 0.25
    tr._apply_regularisers(freeze=False)
    assert tr.model.patch_dropout == 0.25
    tr._apply_regularisers(freeze=True)
    assert tr.model.patch_dropout == 0.0
    tr.patch_dropout = 1.0
    with pytest.raises(ValueError):
        tr._apply_regularisers(freeze=False)
