"""CPU-side checks of the audio CNN (eav_amd/cnn_audio.py, csrc/audio_cnn.hip): the reference's signatures and defaults,
state_dict keys and seeded default initialisation (against the golden's fresh weights), the input-length range, the
C ABI's argument validation without a device, and a scratch-free gfx950 compile of every kernel."""
import hashlib
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["features.0.weight", "features.0.bias", "features.2.weight", "features.2.bias", "features.6.weight",
        "features.6.bias", "features.8.weight", "features.8.bias", "classifier.weight", "classifier.bias"]


def test_signatures_and_defaults_match_reference():
    from eav_amd import cnn_audio as ca
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]  # noqa: E731
    assert sig(ca.AudioModel.__init__) == [("self", inspect.Parameter.empty), ("num_classes", 5)]
    assert sig(ca.create_dataloader) == [("x", inspect.Parameter.empty), ("y", inspect.Parameter.empty),
                                         ("batch_size", 64), ("shuffle", True)]
    assert [p for p, _ in sig(ca.ActivationSaver.__init__)] == ["self", "model", "val_loader", "save_dir"]
    assert sig(ca.train_model) == [("model", inspect.Parameter.empty), ("train_loader", inspect.Parameter.empty),
                                   ("val_loader", inspect.Parameter.empty), ("epochs", 100), ("lr", 1e-3),
                                   ("save_dir", "activations"), ("subject_id", None), ("device", None)]
    assert ca.MODEL_DIR == r"D:\.spyder-py3\finetuned_cnn_7030"


def test_modules_state_dict_and_seeded_init(golden_dir):
    from eav_amd.cnn_audio import AudioModel
    g = np.load(os.path.join(golden_dir, "audio_cnn_train_model.npz"))
    torch.manual_seed(int(g["wseed"]))
    m = AudioModel(num_classes=5)
    sd = m.state_dict()
    assert list(sd) == KEYS == list(g["fresh_keys"])
    assert [type(m.features[i]).__name__ for i in range(11)] == [
        "Conv1d", "ReLU", "Conv1d", "ReLU", "Dropout", "MaxPool1d", "Conv1d", "ReLU", "Conv1d", "ReLU", "Dropout"]
    assert (m.features[4].p, m.features[10].p, m.features[5].kernel_size) == (0.1, 0.5, 8)
    assert tuple(m.classifier.weight.shape) == (5, 128 * 22)
    for k, h in zip(KEYS, g["fresh_sha256"]):
        assert hashlib.sha256(np.ascontiguousarray(sd[k].numpy()).tobytes()).hexdigest() == str(h), k
    for k in ("features.0.weight", "features.0.bias", "classifier.bias"):
        assert np.array_equal(sd[k].numpy(), g[f"fresh.{k}"])


@pytest.mark.parametrize("T", [175, 184, 100])
def test_input_length_outside_the_classifier_range_raises(T):
    from eav_amd.cnn_audio import AudioModel
    with pytest.raises(NotImplementedError, match="176 <= T <= 183"):
        AudioModel()(torch.zeros(2, 1, T))
    with pytest.raises(NotImplementedError, match="176 <= T <= 183"):
        AudioModel()(torch.zeros(2, T, 1))


def test_no_cpu_fallback():
    from eav_amd import _lib
    from eav_amd.cnn_audio import AudioModel
    with pytest.raises(_lib.EavError, match="no CPU fallback"):
        AudioModel()(torch.zeros(2, 1, 180))


def test_abi_argument_validation_without_gpu():
    """Bad sizes, lengths and pointers return an error string and launch nothing."""
    from eav_amd import _lib
    call = _lib.call
    with pytest.raises(_lib.EavError, match=r"T = 184 gives 23 pooled positions.*176\.\.\.183"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, 8, 4, 256, 128, 184, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="T = 175"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, 8, 4, 256, 128, 175, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="null tensor"):
        call("eav_audio_conv5_fwd", None, 8, 8, 8, 8, 4, 256, 128, 180, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="argmax"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, None, 4, 256, 128, 180, 176, 1, 0.1, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="dropout probability"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, None, 4, 128, 128, 22, 22, 0, 1.0, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="input channels"):
        call("eav_audio_conv5_fwd", 8, 8, 8, 8, None, 4, 24, 128, 22, 22, 0, 0.0, 0, None, None, None)
    with pytest.raises(_lib.EavError, match="pool scatter"):
        call("eav_audio_conv5_dgrad", 8, None, 1.0, 8, 8, None, None, 1.0, 4, 128, 128, 22, 22, 1, None)
    with pytest.raises(_lib.EavError, match="null tensor"):
        call("eav_audio_conv5_dgrad", None, None, 1.0, 8, 8, None, None, 1.0, 4, 128, 128, 22, 22, 0, None)
    n = _lib.plain("eav_audio_wgrad_nparts", 64, 256, 128, 176)
    assert 1 <= n <= 64 * 6
    with pytest.raises(_lib.EavError, match="nparts"):
        call("eav_audio_conv5_wgrad", 8, None, 1.0, 8, 8, 64, 256, 128, 180, 176, n + 1, None)
    with pytest.raises(_lib.EavError, match="null tensor"):
        call("eav_audio_conv5_wgrad", 8, None, 1.0, None, 8, 64, 256, 128, 180, 176, n, None)
    assert _lib.plain("eav_audio_wgrad_nparts", 0, 256, 128, 176) == 0


def test_kernels_compile_for_gfx950_without_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.resources(os.path.join(ROOT, "eav_amd", "csrc", "audio_cnn.hip"))
    names = [r["demangled"] for r in rows]
    assert len(rows) == 6 and sum("conv5_kernel" in n for n in names) == 5 and any("wgrad" in n for n in names), names
    for r in rows:
        assert int(r["ScratchSize"]) == 0, (r["demangled"], r["ScratchSize"])
        assert int(r["LDS Size"]) <= 64 * 1024 and int(r["Occupancy"]) >= 3, r
