"""Host side of the fine-tuning regularisers: BatchAugment.plan_epoch's table (the contract the GPU tests replay),
CrossEntropyLoss's argument validation, the "balanced" class weights, and the two new entry points in the ABI."""
import os
import re

import numpy as np
import pytest
import torch

from tests import augment_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [[5, 2, 9, 0], [7, 1, 3, 8], [4, 6]]


def _plan(epoch=0, seed=3, shape=(40, 16), **kw):
    from eav_amd.augment import BatchAugment
    opts = dict(mixup_alpha=0.4, time_mask=8, freq_mask=6, hflip=True)
    opts.update(kw)
    return BatchAugment(seed=seed, **opts).plan_epoch(BATCHES, epoch, shape)


def test_plan_is_a_function_of_seed_and_epoch():
    from eav_amd.augment import RECORD_INTS
    a, b = _plan(), _plan()
    assert a.dtype == np.int32 and a.shape == (10, RECORD_INTS) and RECORD_INTS == ar.RECORD_INTS
    assert np.array_equal(a, b)
    assert not np.array_equal(a, _plan(epoch=1)) and not np.array_equal(a, _plan(seed=4))
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    assert int(re.search(r"#define EAV_AUGMENT_RECORD_INTS (\d+)", header).group(1)) == RECORD_INTS


def test_plan_draws_stay_inside_their_ranges():
    R, C = 40, 16
    seen_flip, seen_mixed_partner, widths = set(), False, []
    for epoch in range(20):
        t = _plan(epoch=epoch, shape=(R, C))
        lam = ar.lam_of(t)
        assert ((lam >= 0.5) & (lam <= 1.0)).all()
        pos = 0
        for idx in BATCHES:
            part = t[pos:pos + len(idx)]
            pos += len(idx)
            assert part[:, 0].tolist() == idx                              # the sources in the loader's order
            assert sorted(part[:, 1].tolist()) == sorted(idx)              # partners: a permutation of the micro-batch
            assert len(set(ar.lam_of(part).tolist())) == 1                 # one lambda per micro-batch
            seen_mixed_partner |= part[:, 1].tolist() != idx
        seen_flip |= set(t[:, 3].tolist())
        for lo, size, param in ((4, R, 8), (6, R, 8), (8, C, 6), (10, C, 6)):
            a, b = t[:, lo], t[:, lo + 1]
            assert ((a >= 0) & (a <= b) & (b <= size) & (b - a < param)).all()
            widths += (b - a).tolist()
    assert seen_flip == {0, 1} and seen_mixed_partner and max(widths) > 0 and min(widths) == 0


def test_plan_with_a_mask_wider_than_the_axis():
    t = _plan(shape=(3, 2), time_mask=50, freq_mask=50)
    for lo, size in ((4, 3), (6, 3), (8, 2), (10, 2)):
        assert ((t[:, lo] >= 0) & (t[:, lo] <= t[:, lo + 1]) & (t[:, lo + 1] <= size)).all()


def test_plan_with_every_option_off_is_a_plain_gather():
    from eav_amd.augment import BatchAugment
    aug = BatchAugment()
    assert not aug.active
    t = aug.plan_epoch(BATCHES, 0)
    flat = [i for idx in BATCHES for i in idx]
    assert t[:, 0].tolist() == flat and t[:, 1].tolist() == flat
    assert (ar.lam_of(t) == 1.0).all() and not t[:, 3:].any()
    # each option alone leaves the others' words untouched
    t = _plan(mixup_alpha=0.0, hflip=False, freq_mask=0)
    assert (ar.lam_of(t) == 1.0).all() and t[:, 1].tolist() == flat and not t[:, 3].any() and not t[:, 8:].any()
    with pytest.raises(ValueError, match="shape"):
        BatchAugment(time_mask=4).plan_epoch(BATCHES, 0)
    for bad in (dict(mixup_alpha=-0.1), dict(time_mask=-1), dict(freq_mask=1.5)):
        with pytest.raises(ValueError):
            BatchAugment(**bad)


def test_cross_entropy_loss_argument_validation():
    from eav_amd.optim import CrossEntropyLoss
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            CrossEntropyLoss(label_smoothing=eps)
    with pytest.raises(TypeError):
        CrossEntropyLoss(None, 0.1)                                       # keyword arguments only
    crit = CrossEntropyLoss(weight=np.array([1.0, 2.0, 0.5]), label_smoothing=1.0)
    assert crit.label_smoothing == 1.0 and crit.weight.dtype == torch.float32 and crit.weight.tolist() == [1.0, 2.0, 0.5]
    for name in ("weight", "label_smoothing"):
        with pytest.raises(AttributeError):
            setattr(crit, name, 0.0)
    scores = torch.zeros(4, 3)
    for dtype in (torch.int64, torch.int32, torch.bool):
        with pytest.raises(TypeError, match="class probabilities"):
            crit(scores, torch.zeros(4, 3, dtype=dtype))
    d = CrossEntropyLoss()
    assert d.weight is None and d.label_smoothing == 0.0


def test_balanced_class_weights_are_sklearns():
    from sklearn.utils.class_weight import compute_class_weight
    from eav_amd.finetune import balanced_class_weights
    y = np.array([0, 0, 0, 1, 2, 2, 4, 4, 4, 4, 3, 0])
    want = compute_class_weight("balanced", classes=np.arange(5), y=y)
    assert np.allclose(balanced_class_weights(y, 5), want, rtol=1e-15, atol=0.0)
    w = balanced_class_weights(np.array([0, 0, 2, -100]), 4)               # ignored labels do not count; absent classes: 0
    assert np.allclose(w, [3 / (4 * 2), 0.0, 3 / (4 * 1), 0.0])


def test_trainer_options_need_single_label_classification():
    """FineTuneBase._apply_regularisers refuses the criterion options in the other problem types; masks and flip pass."""
    from eav_amd.finetune import FineTuneBase

    class _Cfg:
        num_labels = 3

    class _Model:
        cfg = _Cfg()

    tr = FineTuneBase()
    tr.model, tr.problem_type, tr._criterion_key = _Model(), "regression", (0.0, None)
    for name, value in (("label_smoothing", 0.1), ("class_weights", [1.0, 1.0, 1.0]), ("mixup_alpha", 0.2)):
        setattr(tr, name, value)
        with pytest.raises(ValueError, match="single-label"):
            tr._apply_regularisers(False)
        delattr(tr, name)
    tr.time_mask, tr.hflip = 4, True
    tr._apply_regularisers(False)
    assert tr._augment is not None and tr._augment.time_mask == 4 and tr._augment.hflip
    tr._apply_regularisers(True)                                          # a frozen phase never augments
    assert tr._augment is None
    tr.problem_type, tr.class_weights = None, [1.0, 2.0]
    with pytest.raises(ValueError, match="2 weights for 3 classes"):
        tr._apply_regularisers(False)


def test_new_entry_points_are_declared_and_typed():
    from eav_amd import _lib
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    lib = _lib.load()
    for name, nargs in (("eav_ce_general_fwd_bwd", 13), ("eav_augment_gather", 11)):
        assert re.search(rf"\bint {name}\(", header)
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
    assert re.search(r"\bint64_t eav_ce_general_ws_floats\(", header) and "eav_ce_general_ws_floats" in _lib.PLAIN
    # bad arguments are refused before anything is launched
    with pytest.raises(_lib.EavError, match="eav_ce_general_fwd_bwd"):
        _lib.call("eav_ce_general_fwd_bwd", None, None, None, None, 0.0, None, None, None, None, None, 1, 1, None)
    with pytest.raises(_lib.EavError, match="eav_augment_gather"):
        _lib.call("eav_augment_gather", None, None, None, 0.0, None, None, 1, 1, 1, 0, None)
