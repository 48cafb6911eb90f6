"""EEGNet_tor's modules: the model builds one schedule of eegnet_paths (FastPath / GenericPath) from its constructor arguments
and keeps the attribute surface tests, bench.py, __graft_entry__ and tools/ use; runtime names the fields of a BatchNorm
parameter block as the header documents them; the saved forward is a record.  No device."""
import copy
import os
import re

import pytest
import torch

from eav_amd import cnn_eeg, eegnet as E, eegnet_canon, eegnet_paths as EP, runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("EAV_FIR_ALGO", "EAV_CONV_ALGO", "EAV_CONV_FUSE")
GENERIC = dict(F1=4, D=2, F2=16, kernLength=32, Chans=5, Samples=128)
STATE_DICT = [
    "firstConv.weight",
    "firstBN.weight", "firstBN.bias", "firstBN.running_mean", "firstBN.running_var", "firstBN.num_batches_tracked",
    "depthwiseConv.weight",
    "depthwiseBN.weight", "depthwiseBN.bias", "depthwiseBN.running_mean", "depthwiseBN.running_var",
    "depthwiseBN.num_batches_tracked",
    "separableConv.weight",
    "separableBN.weight", "separableBN.bias", "separableBN.running_mean", "separableBN.running_var",
    "separableBN.num_batches_tracked",
    "dense.weight", "dense.bias",
]


@pytest.mark.parametrize("args,generic,path", [({}, False, EP.FastPath), (GENERIC, True, EP.GenericPath)])
def test_attribute_surface_and_path_selection(args, generic, path, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    model = E.EEGNet_tor(5, **args)
    defaults = dict(_generic=generic, _infer=False, fir_algo="auto", conv_algo="auto", conv_fuse=True, fused_eval=False,
                    apply_max_norm=True, dropout_seed=0x0EA5EED, spatial_dropout=False, _ws=None, _wss={}, _saved=None,
                    _flat=None, _token=0)
    for name, value in defaults.items():
        assert getattr(model, name) == value and type(getattr(model, name)) is type(value), name
    for name in ("forward", "forward_indexed", "forward_batch", "set_dropout_masks", "_use_fft", "_launch_forward",
                 "_launch_backward", "_forward_output", "_pin_workspace", "_check_token"):
        assert callable(getattr(model, name)), name
    assert type(model._path) is path and model._path.m is model
    assert not hasattr(model, "fir_precision") and not hasattr(model, "_step_begin")
    assert E.EEGNet_tor(5, dropoutType="SpatialDropout2D", **args).spatial_dropout is True
    # bench.py, tools/ and the tests import these from eav_amd.eegnet
    assert (E.GraphStep, E.gather_batch, E.DeviceLoader) == (R.GraphStep, R.gather_batch, R.DeviceLoader)
    assert E.IndexedBatch is EP.IndexedBatch and callable(E.Trainer_uni)
    assert E.EEGNet_tor._PARAM_ORDER == [k for k in STATE_DICT if "running" not in k and "tracked" not in k]


def test_environment_sets_the_algorithm_switches(monkeypatch):
    monkeypatch.setenv("EAV_FIR_ALGO", "mfma")
    monkeypatch.setenv("EAV_CONV_ALGO", "fft")
    monkeypatch.setenv("EAV_CONV_FUSE", "0")
    model = E.EEGNet_tor(5)
    assert (model.fir_algo, model.conv_algo, model.conv_fuse) == ("mfma", "fft", False)
    assert model._use_fft() is False and model._path.use_conv_fft(1) is True
    model.fir_algo = model.conv_algo = "no such algorithm"
    with pytest.raises(ValueError, match="fir_algo 'no such algorithm'"):
        model._use_fft()
    with pytest.raises(ValueError, match="conv_algo 'no such algorithm'"):
        model._path.use_conv_fft(1)
    assert E.EEGNet_tor(5, **GENERIC)._use_fft() is False


@pytest.mark.parametrize("args", [{}, GENERIC])
def test_deepcopy_gives_the_copy_a_path_of_its_own(args):
    model = E.EEGNet_tor(5, **args)
    twin = copy.deepcopy(model)
    assert type(twin._path) is type(model._path) and twin._path is not model._path
    assert twin._path.m is twin and model._path.m is model
    assert twin._wss == {} and twin._wss is not model._wss


@pytest.mark.parametrize("args", [{}, GENERIC])
def test_path_registers_nothing_with_the_module(args):
    model = E.EEGNet_tor(5, **args)
    assert list(model.state_dict()) == STATE_DICT
    assert [k for k, _ in model.named_parameters()] == E.EEGNet_tor._PARAM_ORDER
    assert "_path" not in model._modules and "_path" not in model._parameters and "_path" not in model._buffers
    assert not isinstance(model._path, torch.nn.Module)
    assert [k for k, _ in model.named_children()] == [
        "dropout", "firstConv", "firstBN", "elu", "depthwiseConv", "depthwiseBN", "depthwisePool", "separableConv",
        "separableBN", "separablePool", "flatten", "dense", "softmax"]


def test_bn_field_constants_are_the_headers_order():
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    doc = re.search(r"bn_params = ([\w, ]+?) \(8 floats each\); part \[nparts\]\[8\]\[klen\]", header).group(1)
    assert doc == "mean, invstd, scale, shift, m1, m2"
    names = [f"BN_{k.upper()}" for k in doc.split(", ")]
    assert [getattr(R, k) for k in names] == [0, 1, 2, 3, 4, 5]
    buf = torch.zeros(6 * 64)
    for n in (8, 64):
        for k in range(6):
            assert R.bn_field(buf, n, k) == buf.data_ptr() + 4 * n * k
    assert R.bn_field(buf, 64, R.BN_M1) - buf.data_ptr() == 4 * 256 and R.bn_field(buf, 8, R.BN_M2) - buf.data_ptr() == 4 * 40


def test_saved_forward_is_a_record_with_the_token_first():
    Saved = eegnet_canon.Saved
    assert EP.Saved is Saved and Saved._fields == ("token", "x", "training", "drop1", "drop2", "mk", "ws", "probs")
    ws, mk = object(), (lambda i: None)
    s = Saved(7, "x", True, (0.5, 1, None, None), (0.5, 2, None, None), mk, ws)
    assert s[0] == 7 == s.token and s.ws is ws and s.mk is mk and s.probs is None and s.training is True
    assert Saved(8, "x", False, (), (), mk, ws, "p").probs == "p"
    # KernelModule._check_token reads _saved[0]
    model = cnn_eeg.EEGNet(5, Chans=8, Samples=128)
    model._saved = s
    model._check_token(7)
    with pytest.raises(Exception, match="overwritten by a later forward"):
        model._check_token(6)


def test_absent_bn_job_is_spelled_once():
    assert tuple(EP.BnBwdJob()) == (None, 0, 0, 0.0, 0, None, None, None, None)
    assert [type(v) for v in EP.BnBwdJob()] == [type(v) for v in (None, 0, 0, 0.0, 0, None, None, None, None)]


def test_one_input_view_and_indexed_batch_carries_the_step_begin():
    assert open(EP.__file__).read().count("isinstance(x, IndexedBatch)") == 1
    assert "isinstance(x, IndexedBatch)" not in open(E.__file__).read()
    data, idx = torch.zeros(6, 1, 30, 500), torch.tensor([4, 1, 3])
    b = EP.IndexedBatch(data, idx)
    assert b.shape == (3, 1, 30, 500) and b.device == data.device and b.step_begin is None and b.merged is False
    assert EP.FastPath.input_view(b) == (data.data_ptr(), idx.data_ptr(), 3)
    assert EP.FastPath.input_view(data[:2]) == (data.data_ptr(), None, 2)
    begin = (1, 2, 3, 4, 3)
    assert EP.IndexedBatch(data, idx, begin).step_begin == begin
    # the generic path has no launch that could take it: forward_batch gathers the labels itself
    assert E.EEGNet_tor(5, **GENERIC)._path.step_begin_args(None, idx, idx, idx) is None
