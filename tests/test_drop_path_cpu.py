"""Stochastic depth of the AST / ViT encoders, what needs no device: the rates against torch.linspace, the site ids against
every id the dropout sites and the patch-dropout plan use, the restatement's own keep fraction (tests/drop_path_ref.py), and
the refusals of the library and of the model's surface that run before anything is launched."""
import math

import numpy as np
import pytest
import torch

from tests import drop_path_ref as R


@pytest.mark.parametrize("r", [0.1, 0.5])
@pytest.mark.parametrize("L", [1, 2, 3, 12])
def test_rates_are_linspace_rounded_once(L, r):
    from eav_amd import encoder_drop_path as dp, transformer as T
    want = torch.linspace(0, r, L, dtype=torch.float64).to(torch.float32).numpy()
    got = dp.rates(r, L)
    assert got.dtype == np.float32 and got.shape == (L,)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(R.rates(r, L).view(np.uint32), want.view(np.uint32))
    assert got[0] == 0.0 and (L == 1 or got[-1] == np.float32(r))
    model = T.Encoder(T.make_config("vit", hidden=32, layers=L, heads=2, ff=64, image=32))
    assert model.drop_path_rate == 0.0 and not model.drop_path_rates().any()
    model.drop_path_rate = r
    assert np.array_equal(model.drop_path_rates().view(np.uint32), want.view(np.uint32))


def test_site_ids_are_disjoint_from_every_other_site():
    from eav_amd import encoder_drop_path as dp, encoder_dropout as ed, patch_keep
    layers = 12
    taken = {ed.site_id(kind, i) for kind, (_, stride, _) in ed.SITES.items() for i in range(layers if stride else 1)}
    assert ed.site_id("patch_keep") in taken and len(taken) == 1 + 3 * layers + 1
    mine = [s for i in range(layers) for s in dp.site_ids(i)]
    assert mine == [(1 << 23) + 1 + r for r in range(2 * layers)] == [s for i in range(layers) for s in R.site_ids(i)]
    assert len(set(mine)) == 2 * layers and not set(mine) & taken and min(mine) > ed.site_id("patch_keep")
    # the seeds: site_seed has room for 24 bits of id, and the plan's rule "row r adds r << 40" is site_seed of consecutive ids
    assert max(mine) + 1 < 1 << 24
    for seed in (0, 12345, (1 << 64) - 5):
        assert dp.plan_seed(seed) == R.site_seed(seed, mine[0]) != patch_keep.plan_seed(seed)
        for r, sid in enumerate(mine):
            assert (dp.plan_seed(seed) + (r << 40)) & R.M64 == ed.site_seed(seed, sid) == R.site_seed(seed, sid)
    # ... and the ids stay out of the per-layer iteration over SITES
    assert sorted(ed.SITES) == ["attn", "attn_out", "emb", "mlp_out", "patch_keep"]


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_the_restatements_keep_fraction(p):
    """A condition on the reference alone: over 2^16 draws the kept fraction lies within 4 binomial sigmas of 1 - p."""
    n = 1 << 16
    for seed, sid, counter in ((1, R.site_ids(1)[0], 1), (987654321, R.site_ids(11)[1], 77)):
        kept = int((R.draws(seed, sid, n, counter) >= np.float32(p)).sum())
        assert abs(kept - n * (1 - p)) <= 4 * math.sqrt(n * p * (1 - p)), (p, kept)
    # the plan: two branches of a layer draw independently, another counter draws another table
    k1, s1 = R.plan(3, 4096, 0.5, 5, 1)
    k2, _ = R.plan(3, 4096, 0.5, 5, 2)
    assert k1[0].all() and (s1[0] == 1).all()
    assert 0.4 < (k1[1, 0] == k1[1, 1]).mean() < 0.7 and not np.array_equal(k1[1:], k2[1:])
    assert set(np.unique(s1[2])) == {np.float32(0), np.float32(2)}


def test_argument_refusals_without_a_device():
    from eav_amd import _lib
    ok = 4096                                                       # (an aligned address; nothing is launched)
    for args in ((None, 2, 2, 0.1, 1, None, None, None), (ok, 0, 2, 0.1, 1, None, None, None),
                 (ok, 2, 0, 0.1, 1, None, None, None), (ok, 2, 2, 1.0, 1, None, None, None),
                 (ok, 2, 2, -0.1, 1, None, None, None), (ok, 2, 2, float("nan"), 1, None, None, None)):
        with pytest.raises(_lib.EavError, match="eav_drop_path_plan"):
            _lib.call("eav_drop_path_plan", *args)
    for args in ((None, ok, ok, ok, 1, 4, None), (ok, ok, None, ok, 1, 4, None), (ok, ok, 2 * ok, None, 1, 4, None),
                 (ok, ok, 2 * ok, ok, 0, 4, None), (ok, ok, 2 * ok, ok, 1, 6, None), (ok, ok, 2 * ok, ok, 1, 0, None),
                 (ok, ok, ok, ok, 1, 4, None)):                     # (the last one: out is resid)
        with pytest.raises(_lib.EavError, match="eav_drop_path_add"):
            _lib.call("eav_drop_path_add", *args)
    for args in ((ok + 4, ok, 2 * ok, ok, 1, 4, None), (ok, ok + 8, 2 * ok, ok, 1, 4, None), (ok, None, 2 * ok + 4, ok, 1, 4, None)):
        with pytest.raises(_lib.EavError, match="16-byte aligned"):
            _lib.call("eav_drop_path_add", *args)


def test_model_surface_refusals_without_a_device():
    from eav_amd import _lib, transformer as T
    model = T.Encoder(T.make_config("vit", hidden=32, layers=3, heads=2, ff=64, image=32))
    for bad in (1.0, -0.1, 1.5, float("nan")):
        model.drop_path_rate = bad
        with pytest.raises(ValueError, match="drop_path_rate"):
            model.drop_path_rates()
    model.drop_path_rate = 0.2
    for bad in (torch.ones(3, 2, 4), torch.ones(3, 2, 4, dtype=torch.int32), torch.ones(2, 2, 4, dtype=torch.uint8),
                torch.ones(3, 4, dtype=torch.uint8), torch.ones(3, 2, 0, dtype=torch.uint8), np.ones((3, 2, 4), np.uint8)):
        with pytest.raises(ValueError, match="set_drop_path_masks"):
            model.set_drop_path_masks(bad)
    model.set_drop_path_masks(torch.ones(3, 2, 4, dtype=torch.uint8))
    model.set_drop_path_masks(None)
    with pytest.raises(_lib.EavError, match="last_drop_path"):
        model.last_drop_path()
    # the surface of the config dropout does not know the new sites
    assert model.dropout_sites(2) == {}
    dropping = T.Encoder(T.make_config("vit", hidden=32, layers=3, heads=2, ff=64, image=32, hidden_dropout=0.1))
    dropping.drop_path_rate = 0.2
    assert sorted(dropping.dropout_sites(2)) == sorted(["emb"] + [f"{k}.{i}" for k in ("attn_out", "mlp_out") for i in range(3)])
