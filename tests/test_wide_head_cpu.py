"""The encoder's head beyond 16 classes, CPU side: the stock AST config (527 AudioSet labels) constructs, Hugging Face
directories with 527 / 1000 labels load, the class limit is HEAD_MAX_CLASSES, and oracle/vit_oracle.py - the reference of
tests/test_wide_head_gpu.py - equals the Hugging Face classes at those widths."""
import json
import os

import numpy as np
import pytest
import torch

from tests.wide_head_util import wide_batch, wide_case

def _hf_model(ocfg):
    from transformers import ASTConfig, ASTForAudioClassification, ViTConfig, ViTForImageClassification
    common = dict(hidden_size=ocfg["hidden"], num_hidden_layers=ocfg["layers"], num_attention_heads=ocfg["heads"],
                  intermediate_size=ocfg["ff"], patch_size=ocfg["patch"], layer_norm_eps=ocfg["eps"],
                  num_labels=ocfg["num_labels"])
    if ocfg["kind"] == "ast":
        return ASTForAudioClassification(ASTConfig(frequency_stride=ocfg["fstride"], time_stride=ocfg["tstride"],
                                                   max_length=ocfg["frames"], num_mel_bins=ocfg["mel"], **common))
    return ViTForImageClassification(ViTConfig(image_size=ocfg["image"], num_channels=ocfg["channels"], **common))


def test_stock_audioset_config_constructs(golden_dir):
    """config.json of ast-finetuned-audioset, the checkpoint Transformer_Audio.py:22 names: 527 labels."""
    from eav_amd import transformer as T
    cfg = T.config_from_hf(json.load(open(os.path.join(golden_dir, "ast_audioset_config.json"))))
    assert (cfg.kind, cfg.hidden, cfg.layers, cfg.num_labels, cfg.ntok) == ("ast", 768, 12, 527, 1214)
    assert len(cfg.id2label) == 527 and cfg.id2label[0] == "Speech" and cfg.id2label[137] == "Music"
    cfg.layers = 1
    enc = T.Encoder(cfg)
    assert tuple(enc.classifier.dense.weight.shape) == (527, 768) and tuple(enc.classifier.dense.bias.shape) == (527,)
    assert enc.head_algo == "auto" and enc._head_wide()
    enc.reset_head(torch.zeros(5, 768), torch.zeros(5))           # Transformer_Audio.py:24
    assert enc.cfg.num_labels == 5 and enc.cfg.id2label is None and not enc._head_wide()
    assert tuple(enc.classifier.dense.weight.shape) == (5, 768)
    assert T.make_config("vit").id2label is None


def test_encoder_reads_hf_directories_with_wide_heads(tmp_path):
    from transformers import ASTConfig, ASTForAudioClassification, ViTConfig, ViTForImageClassification
    from eav_amd import transformer as T
    for kind, labels, model in (
        ("ast", 527, ASTForAudioClassification(ASTConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=2,
                                                         intermediate_size=64, num_labels=527))),
        ("vit", 1000, ViTForImageClassification(ViTConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=2,
                                                          intermediate_size=64, num_labels=1000, image_size=32))),
    ):
        d = tmp_path / kind
        model.save_pretrained(str(d))
        enc = T.Encoder.from_pretrained(str(d))
        sd, ref = enc.state_dict(), model.state_dict()
        assert sorted(sd) == sorted(ref)
        for k in ref:
            assert torch.equal(sd[k].reshape(ref[k].shape), ref[k]), k
        assert enc.cfg.kind == kind and enc.cfg.num_labels == labels
        assert enc.cfg.id2label == [f"LABEL_{i}" for i in range(labels)]
        enc.reset_head(torch.zeros(5, 32), torch.zeros(5))
        assert enc.cfg.num_labels == 5 and enc.cfg.id2label is None


def test_class_limits():
    from eav_amd import transformer as T
    small = dict(hidden=32, layers=1, heads=2, ff=64, image=32)
    assert T.HEAD_MAX_CLASSES >= 32768
    T.Encoder(T.make_config("vit", num_labels=21843, **small))          # ImageNet-21k
    with pytest.raises(NotImplementedError, match=str(T.HEAD_MAX_CLASSES)):
        T.Encoder(T.make_config("vit", num_labels=T.HEAD_MAX_CLASSES + 1, **small))
    enc = T.Encoder(T.make_config("vit", num_labels=5, **small))
    with pytest.raises(NotImplementedError, match=str(T.HEAD_MAX_CLASSES)):
        enc.reset_head(torch.zeros(T.HEAD_MAX_CLASSES + 1, 32), torch.zeros(T.HEAD_MAX_CLASSES + 1))
    assert tuple(enc.classifier.weight.shape) == (5, 32) and enc.cfg.num_labels == 5      # refused before anything changed
    enc = T.Encoder(T.make_config("vit", num_labels=17, **small))
    assert enc._head_wide()
    enc.head_algo = "narrow"
    with pytest.raises(NotImplementedError, match="narrow"):
        enc._head_wide()
    enc.head_algo = "wide"
    assert enc._head_wide()
    enc.head_algo = "mfma"
    with pytest.raises(ValueError):
        enc._head_wide()
    enc = T.Encoder(T.make_config("vit", num_labels=16, **small))
    assert not enc._head_wide()
    enc.head_algo = "wide"
    assert enc._head_wide()


@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_oracle_matches_hf_at_wide_heads(kind):
    """Pins the reference of the GPU tests: oracle.vit_oracle.forward against the Hugging Face class, 527 / 1000 labels.
    Bound 1e-5: HF fp32 differs from HF fp64 by 5e-7 .. 7e-7 at these shapes, the oracle from HF fp32 by 7e-7."""
    from oracle import vit_oracle as vo
    ocfg, W = wide_case(kind, 41 if kind == "ast" else 42)
    x, _ = wide_batch(kind, 43, 3)
    model = _hf_model(ocfg).eval()
    assert set(model.state_dict()) == set(W)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in W.items()})
    with torch.no_grad():
        ref = model(torch.from_numpy(x)).logits
        got = vo.forward({k: torch.from_numpy(v) for k, v in W.items()}, torch.from_numpy(x), ocfg)
    assert tuple(got.shape) == (3, ocfg["num_labels"])
    err = float((got.double() - ref.double()).abs().max())
    print(f"{kind}: oracle against HF, max |dlogits| = {err:.2e}")
    assert err <= 1e-5


def test_wide_head_kernels_are_scratch_free():
    """Every kernel of csrc/head_wide.hip compiles for gfx950 without scratch, the tile kernel within the 64 KB of static
    LDS (hipcc cross-compiles here: no GPU needed)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.resources(os.path.join(root, "eav_amd", "csrc", "head_wide.hip"))
    names = " ".join(r["demangled"] for r in rows)
    assert "wide_gemm_kernel" in names and "ce_wide_rows_kernel" in names and "ce_wide_finish_kernel" in names, names
    for r in rows:
        assert int(r["ScratchSize"]) == 0, (r["demangled"], r["ScratchSize"])
        assert int(r["LDS Size"]) <= 64 * 1024, r
