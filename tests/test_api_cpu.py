"""CPU-side checks: the C-ABI library loads and exports every symbol declared in
include/eav_hip.h, the host classes keep the reference's names / signatures /
state_dict keys, and the product path fails loudly without a device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols(header="eav_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eav_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from eav_amd import _lib
    lib = _lib.load()
    names = _declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/eav_hip.h but not exported"
    assert sorted(_lib.EXPORTS) == names, set(_lib.EXPORTS) ^ set(names)
    assert lib.eav_abi_version() == 3
    # the process-global test / tuning overrides live in their own header, apart from the product ABI
    tuning = _declared_symbols("eav_hip_tuning.h")
    assert tuning == sorted(_lib.TUNING) and not set(tuning) & set(names)
    for n in tuning:
        assert hasattr(lib, n)
    # every exported eav_* symbol is declared in one of the two headers
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if " T eav_" in ln})
    assert exported == sorted(names + tuning), set(exported) ^ set(names + tuning)


def test_argument_validation_without_gpu():
    """Status/err-string path of the ABI (no kernel is launched for bad arguments)."""
    from eav_amd import _lib
    with pytest.raises(_lib.EavError, match="kernLength"):
        _lib.call("eav_eegnet_fir_fwd", 1, 1, 1, 1, 1, 30, 500, 301, None)
    with pytest.raises(_lib.EavError, match="pool"):
        _lib.call("eav_bn_elu_pool_fwd", 1, 1, 1, 1, 64, 100, 3, 0.0, 0, None, None, None)
    assert _lib.plain("eav_conv64_ntiles", 2500) == 20
    assert _lib.plain("eav_eegnet_fir_fwd_nparts", 64, 30, 10000) == 512


def test_eegnet_class_surface_matches_reference(golden_dir):
    from eav_amd.eegnet import EEGNet_tor, Trainer_uni
    sig = inspect.signature(EEGNet_tor.__init__)
    assert list(sig.parameters)[1:] == ["nb_classes", "Chans", "Samples", "dropoutRate", "kernLength", "F1", "D",
                                        "F2", "norm_rate", "dropoutType"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["Chans"], d["Samples"], d["dropoutRate"], d["kernLength"], d["F1"], d["D"], d["F2"], d["norm_rate"]) == \
        (30, 500, 0.5, 300, 8, 8, 64, 1.0)
    tsig = inspect.signature(Trainer_uni.__init__)
    assert list(tsig.parameters)[1:] == ["model", "data", "lr", "batch_size", "num_epochs", "device"]
    assert tsig.parameters["lr"].default == 1e-4 and tsig.parameters["batch_size"].default == 32
    m = EEGNet_tor(nb_classes=5, Samples=500)
    g = np.load(os.path.join(golden_dir, "eegnet_s500_train.npz"))
    ref_keys = sorted(k[len("post0."):] for k in g.files if k.startswith("post0."))
    mine = sorted(k for k in m.state_dict() if not k.endswith("num_batches_tracked"))
    assert mine == ref_keys
    for k in ref_keys:
        assert tuple(m.state_dict()[k].shape) == g[f"post0.{k}"].shape
    assert sum(p.numel() for p in m.parameters()) == 74933          # SURVEY 2.1 (S=500)
    assert sum(p.numel() for p in EEGNet_tor(5, Samples=10000).parameters()) == 169973


def test_default_init_consumes_torch_rng_like_reference():
    """Same sub-modules in the same order => torch.manual_seed gives the same initial weights as
    the reference's nn.Module would draw (checked against plain torch layers built in that order)."""
    from eav_amd.eegnet import EEGNet_tor
    torch.manual_seed(7)
    m = EEGNet_tor(nb_classes=5, Samples=500)
    torch.manual_seed(7)
    torch.nn.Dropout(0.5)
    c1 = torch.nn.Conv2d(1, 8, (1, 300), padding='same', bias=False)
    torch.nn.BatchNorm2d(8)
    c2 = torch.nn.Conv2d(8, 64, (30, 1), groups=8, bias=False)
    torch.nn.BatchNorm2d(64)
    c3 = torch.nn.Conv2d(64, 64, (1, 16), padding='same', bias=False)
    torch.nn.BatchNorm2d(64)
    d = torch.nn.Linear(64 * 15, 5)
    assert torch.equal(m.firstConv.weight, c1.weight) and torch.equal(m.depthwiseConv.weight, c2.weight)
    assert torch.equal(m.separableConv.weight, c3.weight) and torch.equal(m.dense.weight, d.weight)


def test_no_cpu_fallback():
    from eav_amd import _lib
    from eav_amd.eegnet import EEGNet_tor, Trainer_uni
    m = EEGNet_tor(nb_classes=5, Samples=500)
    with pytest.raises(_lib.EavError):
        m(torch.zeros(2, 1, 30, 500))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.EavError):
            Trainer_uni(m, [np.zeros((4, 1, 30, 500), np.float32), np.zeros(4, np.int64)] * 2)
    with pytest.raises(NotImplementedError):
        EEGNet_tor(nb_classes=5, F1=32)          # beyond the LDS tiles of the generic kernels


def test_device_loader_visits_batches_like_dataloader():
    """Index order == torch DataLoader's for the same torch.manual_seed (CPU tensors here)."""
    from torch.utils.data import DataLoader, TensorDataset
    from eav_amd.eegnet import DeviceLoader
    x = torch.arange(23, dtype=torch.float32).view(23, 1)
    y = torch.arange(23)
    torch.manual_seed(3)
    ref = [b[1].tolist() for _ in range(2) for b in DataLoader(TensorDataset(x, y), batch_size=5, shuffle=True)]
    torch.manual_seed(3)
    dl = DeviceLoader(x, y, 5, True, torch.device("cpu"))
    got = [b[1].tolist() for _ in range(2) for b in dl]
    assert got == ref and len(dl) == 5


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "eav_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", text, flags=re.M), f


def test_encoder_reads_real_hf_directories(tmp_path):
    """Encoder.from_pretrained on directories written by Hugging Face's own save_pretrained (the model_path the
    reference trainers receive): config fields, safetensors keys and the 5-class head line up."""
    from transformers import ASTConfig, ASTForAudioClassification, ViTConfig, ViTForImageClassification
    from eav_amd import transformer as T
    for kind, model in (
        ("ast", ASTForAudioClassification(ASTConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=2,
                                                    intermediate_size=64, num_labels=5))),
        ("vit", ViTForImageClassification(ViTConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=2,
                                                    intermediate_size=64, num_labels=7, image_size=32))),
    ):
        d = tmp_path / kind
        model.save_pretrained(str(d))
        enc = T.Encoder.from_pretrained(str(d))
        sd, ref = enc.state_dict(), model.state_dict()
        assert sorted(sd) == sorted(ref)
        for k in ref:
            assert torch.equal(sd[k].reshape(ref[k].shape), ref[k]), k
        assert enc.cfg.kind == kind and enc.cfg.num_labels == (5 if kind == "ast" else 7)
        w = torch.zeros(5, 32)
        enc.reset_head(w, torch.zeros(5))                     # the reference swaps in a 5-class head
        assert enc.cfg.num_labels == 5 and len(enc.head_parameters()) == (4 if kind == "ast" else 2)
        with pytest.raises(Exception):
            enc(torch.zeros(1, 1024, 128) if kind == "ast" else torch.zeros(1, 3, 32, 32))   # no CPU fallback


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No silent fallback: if libeav_hip.so is absent every entry into the product path raises EavError."""
    from eav_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libeav_hip.so"))
    with pytest.raises(_lib.EavError, match="not built"):
        _lib.load()
    with pytest.raises(_lib.EavError):
        _lib.call("eav_renorm_rows", 1, 1, 1, 1.0, None)


def test_canonical_eegnet_constructor_state_matches_reference(golden_dir):
    """eav_amd.cnn_eeg.EEGNet: same constructor signature as CNN_torch/CNN_EEG.py:12-13, same state_dict keys, and a
    freshly constructed model is in the reference's state - default init drawn from the torch RNG in the same order,
    BatchNorm buffers touched by the reference's train-mode shape probe (CNN_EEG.py:48-54)."""
    from eav_amd.cnn_eeg import EEGNet, EEGNetTrainer
    assert list(inspect.signature(EEGNet.__init__).parameters)[1:] == [
        "nb_classes", "Chans", "Samples", "dropoutRate", "kernLength", "F1", "D", "F2", "norm_rate"]
    assert list(inspect.signature(EEGNetTrainer.__init__).parameters)[1:] == [
        "model", "train_dataset", "val_dataset", "batch_size", "epochs", "lr"]
    for name in ("train_epoch", "validate_epoch", "train", "predict"):
        assert callable(getattr(EEGNetTrainer, name))
    g = np.load(os.path.join(golden_dir, "cnn_eeg_trainer.npz"))
    torch.manual_seed(0)
    m = EEGNet(nb_classes=int(g["nb"]), Chans=int(g["chans"]), Samples=int(g["S"]), dropoutRate=0.0)
    sd = m.state_dict()
    fresh = [k[len("fresh."):] for k in g.files if k.startswith("fresh.")]
    assert len(fresh) == 7
    for k in fresh:
        assert np.array_equal(sd[k].numpy(), g["fresh." + k]), k
    assert [k for k in sd if "num_batches" not in k and "running" not in k] == [
        "block1.0.weight", "block1.1.weight", "block1.1.bias", "block1.2.weight", "block1.3.weight", "block1.3.bias",
        "block2.0.weight", "block2.1.weight", "block2.2.weight", "block2.2.bias", "classifier.weight",
        "classifier.bias"]
    with pytest.raises(NotImplementedError):
        EEGNet(nb_classes=4, F1=32)


def test_shallow_convnet_class_surface_and_default_init():
    """eav_amd.transformer_eeg mirrors Transformer_torch/Transformer_EEG.py: class names, constructor signatures and the
    176 parameter names in the reference's order (oracle.shallow_tf_oracle.param_names is pinned to the reference by
    the golden tests)."""
    from eav_amd import _lib, transformer_eeg as te
    from oracle.shallow_tf_oracle import param_names
    for name in ("PatchEmbedding", "MultiHeadAttention", "FeedForwardBlock", "TransformerLayer", "ShallowConvNet",
                 "TrainerUni"):
        assert hasattr(te, name)
    assert list(inspect.signature(te.ShallowConvNet.__init__).parameters)[1:] == [
        "nb_classes", "chans", "samples", "dropout", "num_layers"]
    assert list(inspect.signature(te.TrainerUni.__init__).parameters)[1:] == [
        "model", "data", "lr", "batch_size", "epochs", "subject", "device"]
    torch.manual_seed(0)
    m = te.ShallowConvNet(5)
    assert [n for n, _ in m.named_parameters()] == param_names(12)
    assert m.fc.weight.shape == (5, 2600) and m.fc.bias is None
    with pytest.raises(_lib.EavError):
        te.TrainerUni(m, data=[torch.zeros(4, 1, 30, 500), torch.zeros(4, dtype=torch.long)] * 2, device="cpu")


def test_calculate_accuracy_and_trial_vote():
    """Transformer_Vision.py:8-11 (argmax == labels, mean) and :174-185 (mean over 25 frames -> argmax)."""
    import numpy as np
    import torch
    from eav_amd.vision import calculate_accuracy, trial_vote
    from types import SimpleNamespace
    logits = torch.tensor([[2.0, 1.0, 0.0], [0.0, 3.0, 1.0], [0.1, 0.2, 0.3], [1.0, 0.0, 0.0]])
    # the reference passes the HF output object (outputs.logits)
    assert abs(calculate_accuracy(SimpleNamespace(logits=logits), torch.tensor([0, 1, 0, 0])) - 0.75) < 1e-7
    frames = np.zeros((2 * 25, 5), np.float32)
    frames[:25, 3] = 1.0
    frames[25:, 1] = np.linspace(0, 2, 25)
    frames[25:, 4] = 0.9
    pred, acc, f1 = trial_vote(frames, np.array([3, 1]))
    assert list(pred) == [3, 1] and acc == 1.0 and f1 == 1.0


def test_unsupported_configurations_raise_not_silently_differ():
    """EEGNet_tor.py:16-17,21 accepts any F1 / D / F2 / kernLength / Chans / dropoutType.  The reference configuration
    runs the specialised fp32-MFMA kernels, other widths the run-time-parametrised kernels (`_generic`) with the same
    sub-modules / state_dict; only sizes beyond those kernels' LDS tiles fail - loudly, at construction."""
    from eav_amd.eegnet import EEGNet_tor
    ref = __import__("torch").nn
    assert not EEGNet_tor(5)._generic
    for kw in (dict(F1=4), dict(D=2), dict(F2=32), dict(kernLength=301), dict(Chans=33),
               dict(F1=4, D=2, F2=16, kernLength=64, Chans=64, Samples=256), dict(kernLength=1024, Samples=2048),
               dict(Chans=256)):
        m = EEGNet_tor(5, **kw)
        assert m._generic
        full = dict(F1=8, D=8, F2=64, kernLength=300, Chans=30, Samples=500)
        full.update(kw)
        assert tuple(m.firstConv.weight.shape) == (full["F1"], 1, 1, full["kernLength"])
        assert tuple(m.depthwiseConv.weight.shape) == (full["F1"] * full["D"], 1, full["Chans"], 1)
        assert tuple(m.separableConv.weight.shape) == (full["F2"], full["F1"] * full["D"], 1, 16)
        assert tuple(m.dense.weight.shape) == (5, full["F2"] * (full["Samples"] // 32))
        assert isinstance(m.separableBN, ref.BatchNorm2d)
    for kw in (dict(F1=32), dict(D=16), dict(F1=16, D=8), dict(F2=128), dict(kernLength=1025), dict(Chans=257)):
        with pytest.raises(NotImplementedError):
            EEGNet_tor(5, **kw)
    # every dropoutType other than 'Dropout' is nn.Dropout2d in the reference (:21) - supported (per-map masks)
    m = EEGNet_tor(5, dropoutType="SpatialDropout2D", dropoutRate=0.5)
    assert m.spatial_dropout and isinstance(m.dropout, torch.nn.Dropout2d)
    assert not EEGNet_tor(5).spatial_dropout


def test_bench_headline_is_compact_and_complete():
    """bench.py's LAST stdout line must stay small enough for the driver's parser (round 3's 27 KB line was not parsed):
    the compact headline built from a full round-3 detail record is < 4 KB and carries roofline + cpu_baseline + one short
    record per modality."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    detail = json.load(open(os.path.join(root, "profiles", "r03_bench_line.json")))
    line = json.dumps(bench.compact_headline(detail), separators=(",", ":"))
    assert len(line) < 4096, len(line)
    head = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "modalities"):
        assert k in head, k
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(head["roofline"])
    assert {"value", "unit", "cores", "kind", "sample"} <= set(head["cpu_baseline"])
    assert set(head["modalities"]) == {"eegnet", "ast", "vit"} and "workload" in head["config"]
    for m in head["modalities"].values():
        assert {"value", "ms_per_step", "batch", "roofline", "cpu_baseline"} <= set(m)


def test_bench_plain_headline_and_output_dump(tmp_path):
    """A plain bench.py run (no --full) prints the headline fields only - metric, value, unit, ms_per_step of ONE timed
    step, higher_is_better, dtype - and --dump-outputs writes float32 / float64 .npy files named after the outputs."""
    import argparse
    import importlib.util
    import json
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    args = argparse.Namespace(steps=20, warmup=5)
    rec = bench.headline_record(args, 1, 64, "single", 20 * 1.25e-3, None)
    head = json.loads(json.dumps(bench.compact_headline(rec), separators=(",", ":")))
    assert abs(head["ms_per_step"] - 1.25) < 1e-9 and abs(head["value"] - 64 / 1.25e-3) < 0.01
    assert head["unit"] == "samples/s" and head["higher_is_better"] is True and head["dtype"] == "f32"
    assert head["steps"] == 20 and head["warmup"] == 5 and head["scaling"] == "none"
    assert not {"roofline", "cpu_baseline", "modalities", "detail"} & set(head)

    class Run:
        def outputs(self, step=True):
            out = {"param.w": np.ones((3, 4), np.float32), "buffer.n": np.array(7.0)}
            if step:
                out.update(scores=np.full((64, 5), 0.2, np.float32), loss=np.ones(1, np.float32))
            return out
    bench.dump_outputs(str(tmp_path / "one"), Run(), None)
    bench.dump_outputs(str(tmp_path / "job"), Run(), {"final_losses": [1.5] * 42})
    assert sorted(os.listdir(tmp_path / "one")) == ["buffer.n.npy", "loss.npy", "param.w.npy", "scores.npy"]
    assert sorted(os.listdir(tmp_path / "job")) == ["buffer.n.npy", "param.w.npy", "subject_final_losses.npy"]
    for d in ("one", "job"):
        for f in os.listdir(tmp_path / d):
            assert np.load(tmp_path / d / f).dtype in (np.float32, np.float64), f


def test_bench_subject_job_record_and_multi_gpu_headline():
    """The N > 1 headline of bench.py: a fixed-total-work (42 subjects) rate comparable with the N = 1 step rate.  The record
    arithmetic on CPU: value = subjects x steps x batch / seconds (doubling the time of the busiest rank halves it), the
    ideal speed-up of the hybrid schedule at 8 ranks is 8.0 (7.0 for plain round-robin), speed-up against this run's own
    one-GPU step rate; the compact line says `scaling: strong` and carries the ideal and the measured fraction of it."""
    import importlib.util
    import json
    import torch
    from eav_amd.dist import subject_schedule
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    have = torch.ones(42)
    s1 = subject_schedule(1)
    r1 = bench._subject_job_record(s1, 1, 42, 50, 64, [42 * 50 * 1.5e-3, 42 * 50 * 1.5e-3, 0.0], have, torch.device("cpu"), True)
    assert abs(r1["value"] - 64 / 1.5e-3) < 1 and r1["ideal_speedup"] == 1.0 and r1["all_subjects_reported"]
    assert abs(r1["speedup_vs_one_gpu_rate_of_this_run"] - 1.0) < 1e-3
    r2 = bench._subject_job_record(s1, 1, 42, 50, 64, [2 * 42 * 50 * 1.5e-3, 2 * 42 * 50 * 1.5e-3, 0.0], have,
                                   torch.device("cpu"), True)
    assert abs(r2["value"] - r1["value"] / 2) < 1                      # one rank doing twice the work: half the rate
    # an 8-rank record as rank 0 would assemble it (world = 1 here: no process group on CPU; the schedule is the 8-rank one)
    s8 = subject_schedule(8)
    t_solo, t_tail = 5 * 50 * 1.5e-3, 50 * 0.6e-3
    r8 = bench._subject_job_record(s8, 1, 42, 50, 64, [t_solo + t_tail, t_solo, t_tail], have, torch.device("cpu"), True)
    assert r8["ideal_speedup"] == 8.0 and r8["ideal_speedup_round_robin"] == 7.0 and r8["schedule"]["group_size"] == 4
    assert 7.6 < r8["speedup_vs_one_gpu_rate_of_this_run"] < 8.0 and 0.95 < r8["speedup_vs_ideal"] < 1.0
    assert r8["scaling"].startswith("strong")
    detail = json.load(open(os.path.join(root, "profiles", "r03_bench_line.json")))
    detail.update({"n_gpus": 8, "scaling": "strong", "value": r8["value"], "ideal_speedup": r8["ideal_speedup"],
                   "speedup_vs_ideal": r8["speedup_vs_ideal"],
                   "multi_gpu": {"backend": "nccl", "rccl_ranks": 8, "subject_sharded": r8,
                                 "strong": {"value": 1.0}, "weak": {"value": 2.0}}})
    detail.pop("predicted_strong_scaling", None)
    head = bench.compact_headline(detail)
    line = json.dumps(head, separators=(",", ":"))
    assert len(line) < 4096, len(line)
    assert head["scaling"] == "strong" and head["ideal_speedup"] == 8.0 and head["speedup_vs_ideal"] == r8["speedup_vs_ideal"]
    mg = head["multi_gpu"]
    assert mg["eegnet_subject_sharded"] == r8["value"] and mg["eegnet_strong"] == 1.0 and mg["eegnet_weak"] == 2.0
    assert mg["eegnet_subjects_ideal_speedup"] == 8.0 and "predicted_strong_scaling_at_8" not in head


def test_runtime_module_is_shared_by_the_models_and_reexported_by_eegnet():
    """eav_amd.runtime holds the training runtime and the models' base class: it imports no model module, eegnet keeps the
    old import path alive with the same objects, the models (the AST / ViT Encoder among them) derive from KernelModule,
    and GraphStep refuses anything else."""
    import copy
    import eav_amd.eegnet as eg
    import eav_amd.runtime as rt
    from eav_amd import _lib, transformer as T
    from eav_amd.cnn_audio import AudioModel
    from eav_amd.cnn_eeg import EEGNet
    from eav_amd.optim import FusedAdam
    from eav_amd.transformer_eeg import ShallowConvNet
    src = open(rt.__file__).read()
    assert sorted(set(re.findall(r"^from \.(\w*) import", src, flags=re.M))) == ["", "optim"] and "\nimport eav_amd" not in src
    for name in ("cached_workspace", "gather_batch", "GraphStep", "DeviceLoader"):
        assert getattr(eg, name) is getattr(rt, name) and getattr(rt, name).__module__ == "eav_amd.runtime"
    for model in (eg.EEGNet_tor(5), EEGNet(5), ShallowConvNet(5, num_layers=1), AudioModel(),
                  T.Encoder(T.make_config("vit", hidden=32, layers=1, heads=2, ff=64, image=32))):
        assert isinstance(model, rt.KernelModule) and model._wss == {} and model._flat is None
        twin = copy.deepcopy(model)
        assert list(twin.state_dict()) == list(model.state_dict()) and twin._wss is not model._wss
        with pytest.raises(_lib.EavError, match=f"eav_amd.{type(model).__name__} runs on an MI355X only"):
            model._require_gpu(torch.zeros(1))
        with pytest.raises(_lib.EavError, match=f"{type(model).__name__}.backward: the activations of this forward"):
            model._check_token(1)
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(_lib.EavError, match="KernelModule"):
        rt.GraphStep(lin, FusedAdam(lin.parameters(), capturable=True), None, torch.zeros(4, 2), torch.zeros(4), 2)


def test_gradient_views_alias_the_flat_gradient_buffer():
    """KernelModule._grad_views() are the parameters' slices of the flat gradient buffer; _grads_out() hands autograd those
    slices in the parameters' shapes, in named_parameters() order, and None exactly for the frozen parameters."""
    import eav_amd.eegnet as eg
    from eav_amd.cnn_audio import AudioModel
    from eav_amd.cnn_eeg import EEGNet
    from eav_amd.transformer_eeg import ShallowConvNet
    generic = eg.EEGNet_tor(5, F1=4, D=2, F2=8, kernLength=32, Chans=6, Samples=64)
    assert generic._generic
    for model in (eg.EEGNet_tor(5), generic, EEGNet(5), ShallowConvNet(5, num_layers=1), AudioModel()):
        named = list(model.named_parameters())
        frozen = {named[1][0], named[-1][0]}
        for k, p in named:
            p.requires_grad_(k not in frozen)
        model._ensure_flat()
        gflat, offs = model._flat[1], model._flat[2]
        views = model._grad_views()
        assert list(views) == [k for k, _ in named]
        for k, v in views.items():
            assert v.dim() == 1 and v.data_ptr() == gflat.data_ptr() + 4 * offs[k][0] and v.numel() == offs[k][1], k
        out = model._grads_out(views)
        assert len(out) == len(named)
        for (k, p), g in zip(named, out):
            assert (g is None) == (k in frozen), k
            if g is not None:
                assert g.shape == p.shape and g.data_ptr() == views[k].data_ptr(), k
                assert g.untyped_storage().data_ptr() == gflat.untyped_storage().data_ptr(), k


@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_encoder_flat_layout_is_the_param_shapes_order(kind):
    """The Encoder's flat buffer follows param_shapes (q, k, v weights adjacent, then their biases - the fused q/k/v GEMM,
    _forward_scales, head_grad_ranges and grad_ready_hook rely on it), every tensor rounded up to 4 floats; that is not the
    named_parameters() order."""
    from eav_amd import transformer as T
    cfg = T.make_config(kind, hidden=32, layers=1, heads=2, ff=64, image=32)
    model = T.Encoder(cfg)
    model._ensure_flat()
    want, total = {}, 0
    for k, shp in T.param_shapes(cfg).items():
        want[k] = (total, int(np.prod(shp)))
        total += (want[k][1] + 3) // 4 * 4
    assert model._flat[2] == want and list(model._flat[2]) == list(want) and model._flat[0].numel() == total
    assert model._names == list(want) and model._names != [n for n, _ in model.named_parameters()]
    for k, p in model.named_parameters():
        assert p.data_ptr() == model._flat[0].data_ptr() + 4 * want[k][0], k


def test_weight_planes_staleness_is_decided_without_a_launch():
    """WeightPlanes.stale: which matrices' planes must be rebuilt, from the flat buffer's address, the version counters,
    the byte ranges the optimiser reported and whether transposes are needed - host arithmetic only."""
    from eav_amd import transformer as T
    from eav_amd.weight_planes import WeightPlanes
    cfg = T.make_config("vit", hidden=32, layers=2, heads=2, ff=64, image=32)
    model = T.Encoder(cfg)
    model._ensure_flat()
    offs = model._flat[2]
    mats = [(k, 4 * offs[pn][0], out, inn) for k, pn, out, inn in model._weight_keys()]
    every = [k for k, _, _, _ in mats]
    assert every == ["patch", "qkv0", "o0", "fc10", "fc20", "qkv1", "o1", "fc11", "fc21"]
    wp = WeightPlanes(mats, cfg.layers, torch.device("cpu"), False)
    base, versions = 1 << 20, (0, 7)
    assert wp.stale(base, versions, [], False) == every            # never refreshed
    wp.key = (base, versions)                                      # (what refresh() leaves behind)
    assert wp.stale(base, versions, [], False) == []
    at = {k: (base + off, base + off + 4 * out * inn) for k, off, out, inn in mats}
    lo, hi = at["fc11"]
    assert wp.stale(base, versions, [(lo + 8, lo + 12)], False) == ["fc11"]
    assert wp.stale(base, versions, [(hi - 4, hi)], False) == ["fc11"] and wp.stale(base, versions, [(hi, hi + 4)], False) == []
    assert wp.stale(base, versions, [(at["o1"][1] - 4, lo + 4)], False) == ["o1", "fc11"]     # a range over two matrices
    assert wp.stale(base, versions, [(at["qkv0"][0], at["qkv0"][0] + 4), (at["fc21"][1] - 4, at["fc21"][1])],
                    False) == ["qkv0", "fc21"]
    assert wp.stale(base, (0, 8), [], False) == every              # a parameter's version moved
    assert wp.stale(base, (1, 7), [], False) == every              # the flat buffer's version moved
    assert wp.stale(base + 64, versions, [], False) == every       # the flat buffer was rebuilt
    assert wp.stale(base, versions, [], True) == every             # transposes needed, none held
    wp.invalidate()
    assert wp.stale(base, versions, [], False) == every


def test_split_gemm_instantiations_are_scratch_free():
    """Every instantiation of gemm_sp_kernel `dispatch` can pick compiles for gfx950 without scratch (round 5: 36-196 bytes per
    lane in all the default forms - the epilogue's tile-invariant index arithmetic, hoisted out of the persistent tile loop
    and spilled around the K loop) and with the register budget of two waves per SIMD; the two-stage forms stay at the 80 KB
    of LDS that let two workgroups share a CU.  hipcc cross-compiles here: no GPU needed (about a minute)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [r for r in kr.resources(os.path.join(root, "eav_amd", "csrc", "gemm_sp.hip")) if "gemm_sp_kernel" in r["demangled"]]
    assert len(rows) >= 12, [r["demangled"] for r in rows]
    for r in rows:
        assert int(r["ScratchSize"]) == 0, (r["demangled"], r["ScratchSize"])
        assert int(r["VGPRs"]) <= 256 and int(r["AGPRs"]) == 0 and int(r["Occupancy"]) == 2, r
        three_stage = r["demangled"].rstrip(">(SpArgs) ").endswith(", 3")
        assert int(r["LDS Size"]) <= (160 if three_stage else 80) * 1024, r
