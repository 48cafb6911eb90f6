"""config.problem_type on the CPU side: the configuration round trip, the resolution rule against the Hugging Face classes,
the reference loss of tests/problem_type_ref.py against their `.loss` (which pins the reference of the GPU tests), the
criteria's refusal of host tensors, float labels in DeviceLoader, and the resources of csrc/head_loss.hip."""
import os

import pytest
import torch

from tests import problem_type_ref as ptr

TINY = dict(hidden=32, layers=1, heads=2, ff=64, image=32)


def test_config_reads_problem_type():
    from eav_amd import transformer as T
    base = {"model_type": "vit", "hidden_size": 32, "num_hidden_layers": 1, "num_attention_heads": 2,
            "intermediate_size": 64, "image_size": 32, "id2label": {"0": "a", "1": "b"}}
    assert T.config_from_hf(base).problem_type is None
    for pt in T.PROBLEM_TYPES:
        assert T.config_from_hf(dict(base, problem_type=pt)).problem_type == pt
    assert T.config_from_hf(dict(base, problem_type=None)).problem_type is None
    with pytest.raises(ValueError, match="problem_type"):
        T.config_from_hf(dict(base, problem_type="ranking"))
    with pytest.raises(ValueError, match="problem_type"):
        T.make_config("vit", problem_type="multi_label")
    assert T.make_config("vit").problem_type is None and T.make_config("ast").problem_type is None
    assert sorted(T.PROBLEM_TYPES) == sorted(ptr.PROBLEM_TYPES)


def _hf_tiny(num_labels, problem_type=None):
    from oracle import vit_oracle as vo
    torch.manual_seed(num_labels)
    return ptr.hf_model(vo.cfg_vit(num_labels=num_labels, **TINY), problem_type).eval()


@pytest.mark.parametrize("num_labels,shape,dtype,expected", [
    (3, (4, 3), torch.float32, "multi_label_classification"),
    (3, (4,), torch.int64, "single_label_classification"),
    (1, (4,), torch.float32, "regression"),
    (1, (4, 1), torch.float32, "regression"),
])
def test_resolution_rule_is_hugging_faces(num_labels, shape, dtype, expected):
    from eav_amd import transformer as T
    model = _hf_tiny(num_labels)
    assert model.config.problem_type is None
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, num_labels, shape, generator=g) if dtype == torch.int64 else torch.rand(shape, generator=g)
    model(torch.randn(4, 3, 32, 32, generator=g), labels=labels)
    assert model.config.problem_type == expected                  # HF wrote its choice back
    assert T.resolve_problem_type(num_labels, labels) == expected
    enc = T.Encoder(T.make_config("vit", num_labels=num_labels, **TINY))
    assert enc.cfg.problem_type is None
    assert type(enc.criterion(labels)).__name__ == {"regression": "MSELoss", "single_label_classification": "CrossEntropyLoss",
                                                    "multi_label_classification": "BCEWithLogitsLoss"}[expected]
    assert enc.cfg.problem_type == expected                       # sticky, like HF's
    assert enc.criterion(labels) is enc.criterion()               # held on the encoder, not rebuilt
    other = torch.zeros(4, dtype=torch.int64)
    assert enc.criterion(other) is enc.criterion() and enc.cfg.problem_type == expected


def test_reset_head_forgets_an_inferred_problem_type_only():
    from eav_amd import transformer as T
    enc = T.Encoder(T.make_config("vit", num_labels=1, **TINY))
    enc.criterion(torch.zeros(4))
    assert enc.cfg.problem_type == "regression"
    enc.reset_head(torch.zeros(3, 32), torch.zeros(3))
    assert enc.cfg.problem_type is None
    enc.cfg.problem_type = "multi_label_classification"           # set by the caller
    enc.reset_head(torch.zeros(2, 32), torch.zeros(2))
    assert enc.cfg.problem_type == "multi_label_classification"
    enc = T.Encoder(T.make_config("vit", num_labels=4, problem_type="regression", **TINY))      # set in the config
    enc.criterion(torch.zeros(4, 4))
    enc.reset_head(torch.zeros(2, 32), torch.zeros(2))
    assert enc.cfg.problem_type == "regression"


@pytest.mark.parametrize("num_labels", [1, 2, 527])
@pytest.mark.parametrize("problem_type", ptr.PROBLEM_TYPES)
def test_reference_loss_is_hugging_faces(problem_type, num_labels):
    """tests/problem_type_ref.loss in float64 on HF's own logits against HF's .loss: 1e-5 relative, the bound of
    test_oracle_matches_hf_at_wide_heads - an fp32 mean of at most ~2000 O(1) terms sits two orders below it."""
    if problem_type == "single_label_classification" and num_labels == 1:
        # no such Hugging Face model exists: its configuration refuses the pair, and so does ours
        from eav_amd import transformer as T
        with pytest.raises(ValueError, match="num_labels > 1"):
            _hf_tiny(num_labels, problem_type)
        with pytest.raises(ValueError, match="num_labels > 1"):
            T.make_config("vit", num_labels=1, problem_type=problem_type)
        enc = T.Encoder(T.make_config("vit", num_labels=1, **TINY))
        enc.cfg.problem_type = problem_type
        with pytest.raises(ValueError, match="num_labels > 1"):
            enc.criterion(torch.zeros(4, dtype=torch.int64))
        return
    model = _hf_tiny(num_labels, problem_type)
    g = torch.Generator().manual_seed(11 + num_labels)
    if problem_type == "single_label_classification":
        labels = torch.randint(0, num_labels, (4,), generator=g)
    elif problem_type == "regression":
        labels = torch.randn(4, num_labels, generator=g)
    else:
        labels = (torch.rand(4, num_labels, generator=g) < 0.3).float()
    with torch.no_grad():
        out = model(torch.randn(4, 3, 32, 32, generator=g), labels=labels)
    ref, got = float(out.loss.double()), float(ptr.loss(out.logits.double(), labels, problem_type))
    print(f"{problem_type} x {num_labels}: HF {ref:.9g}, reference {got:.9g}, relative gap {abs(got - ref) / max(abs(ref), 1e-300):.2e}")
    assert abs(got - ref) <= 1e-5 * abs(ref)
    if problem_type == "regression" and num_labels == 1:          # HF's squeeze(): [B] and [B, 1] are one thing
        assert float(ptr.loss(out.logits.double(), labels[:, 0], problem_type)) == got


def test_criteria_refuse_host_tensors():
    from eav_amd import _lib
    from eav_amd.optim import BCEWithLogitsLoss, MSELoss
    s, t = torch.zeros(4, 3), torch.zeros(4, 3)
    for crit in (BCEWithLogitsLoss(), MSELoss()):
        with pytest.raises(_lib.EavError, match="device"):
            crit(s, t)
        crit.check()                                              # nothing to report: a no-op
    with pytest.raises(_lib.EavError, match="device"):
        BCEWithLogitsLoss().accumulate(s, t, torch.zeros(()), torch.zeros((), dtype=torch.int32))
    with pytest.raises(_lib.EavError, match="device"):
        MSELoss().accumulate(s, t, torch.zeros(()))


def test_device_loader_keeps_float_label_rows():
    """The host branch of gather_batch / DeviceLoader with label_dtype=torch.float32: [N, NC] rows stay fp32 and follow
    their samples, through the gather and through the contiguous-slice fast path; the default stays int64 [N]."""
    from eav_amd.runtime import DeviceLoader
    x = torch.arange(7 * 3, dtype=torch.float32).view(7, 3)
    y = torch.arange(7 * 2, dtype=torch.float32).view(7, 2) / 4
    dl = DeviceLoader(x, y.numpy(), 3, False, "cpu", label_dtype=torch.float32)
    assert dl.y.dtype == torch.float32 and tuple(dl.y.shape) == (7, 2)
    for idx in ([5, 0, 3], [2, 3, 4], [6]):
        xb, yb = dl.gather(idx)
        assert torch.equal(xb, x[idx]) and torch.equal(yb, y[idx]) and yb.dtype == torch.float32
        assert torch.equal(dl.gather_labels(idx), y[idx])
    batches = list(dl)
    assert [tuple(b[1].shape) for b in batches] == [(3, 2), (3, 2), (1, 2)]
    one = DeviceLoader(x, y[:, 0], 3, False, "cpu", label_dtype=torch.float32)
    assert tuple(one.y.shape) == (7,) and torch.equal(one.gather([4, 1])[1], y[[4, 1], 0])
    dflt = DeviceLoader(x, [0, 1, 2, 3, 4, 0, 1], 3, False, "cpu")
    assert dflt.y.dtype == torch.int64 and torch.equal(dflt.gather([6, 2])[1], torch.tensor([1, 2]))
    with pytest.raises(ValueError):
        DeviceLoader(x, y, 3, False, "cpu", label_dtype=torch.float16)


def test_head_loss_kernels_are_scratch_free():
    """Every kernel of csrc/head_loss.hip compiles for gfx950 without scratch and without LDS (hipcc cross-compiles
    here: no GPU needed)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.resources(os.path.join(root, "eav_amd", "csrc", "head_loss.hip"))
    names = " ".join(r["demangled"] for r in rows)
    assert "head_loss_rows_kernel<true>" in names and "head_loss_rows_kernel<false>" in names, names
    assert "head_loss_finish_kernel" in names, names
    for r in rows:
        assert int(r["ScratchSize"]) == 0, (r["demangled"], r["ScratchSize"])
        assert int(r["LDS Size"]) == 0, r
