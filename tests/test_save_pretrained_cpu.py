"""Encoder.save_pretrained: the directory it writes loads into the Hugging Face classes without a missing, unexpected or
mismatched key and with equal tensors, carries problem_type, label names and geometry, and round-trips through
Encoder.from_pretrained bit for bit."""
import json

import pytest
import torch


def _cases():
    from eav_amd import transformer as T
    names = [f"sound {i}" for i in range(527)]
    return {
        "ast": (T.make_config("ast", hidden=32, layers=1, heads=2, ff=64, frames=64, fstride=8, tstride=12, num_labels=527,
                              id2label=names, hidden_dropout=0.1), names),
        "vit": (T.make_config("vit", hidden=32, layers=1, heads=2, ff=64, image=48, channels=2, num_labels=2,
                              problem_type="regression", attention_dropout=0.25, eps=1e-6), ["LABEL_0", "LABEL_1"]),
    }


@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_saved_directory_loads_into_hugging_face_and_back(kind, tmp_path):
    from transformers import ASTForAudioClassification, ViTForImageClassification
    from eav_amd import transformer as T
    cfg, names = _cases()[kind]
    torch.manual_seed(3)
    enc = T.Encoder(cfg)
    with torch.no_grad():
        for p in enc.parameters():                                # no tensor left at its constant initial value
            p.add_(torch.randn_like(p) * 0.02)
    d = str(tmp_path / kind)
    enc.save_pretrained(d)
    from safetensors import safe_open
    with safe_open(d + "/model.safetensors", "np") as f:
        assert f.metadata() == {"format": "pt"}
        shapes = T.param_shapes(cfg)
        assert sorted(f.keys()) == sorted(shapes)
        assert all(f.get_tensor(k).dtype.name == "float32" and f.get_tensor(k).shape == tuple(shapes[k]) for k in shapes)
    cj = json.load(open(d + "/config.json"))
    assert ("problem_type" in cj) == (kind == "vit")               # omitted while unset

    hf_cls = ASTForAudioClassification if kind == "ast" else ViTForImageClassification
    model, info = hf_cls.from_pretrained(d, output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"] and not info["error_msgs"]
    sd, ref = enc.state_dict(), model.state_dict()
    assert sorted(sd) == sorted(ref)
    for k in ref:
        assert ref[k].dtype == torch.float32 and torch.equal(sd[k], ref[k]), k
    hc = model.config
    assert hc.problem_type == cfg.problem_type and hc.num_labels == cfg.num_labels
    assert [hc.id2label[i] for i in range(cfg.num_labels)] == names and hc.label2id == {n: i for i, n in enumerate(names)}
    assert (hc.hidden_size, hc.num_hidden_layers, hc.num_attention_heads, hc.intermediate_size, hc.patch_size) == \
        (cfg.hidden, cfg.layers, cfg.heads, cfg.ff, cfg.patch)
    assert (hc.hidden_act, hc.layer_norm_eps, hc.qkv_bias) == ("gelu", cfg.eps, True)
    assert (hc.hidden_dropout_prob, hc.attention_probs_dropout_prob) == (cfg.hidden_dropout, cfg.attention_dropout)
    if kind == "ast":
        assert (hc.num_mel_bins, hc.max_length, hc.frequency_stride, hc.time_stride) == (128, 64, 8, 12)
    else:
        assert (hc.image_size, hc.num_channels) == (48, 2)

    back = T.Encoder.from_pretrained(d)
    assert back.source_dir == d and enc.source_dir is None
    assert vars(back.cfg) == dict(vars(cfg), id2label=names)      # LABEL_i is what an unnamed head is called on disk
    sb = back.state_dict()
    assert list(sb) == list(sd) and all(torch.equal(sb[k], sd[k]) for k in sd)


def test_unset_problem_type_and_resolved_one_on_disk(tmp_path):
    """The resolved type of a labelled forward is what the next save writes."""
    from eav_amd import transformer as T
    enc = T.Encoder(T.make_config("vit", hidden=32, layers=1, heads=2, ff=64, image=32, num_labels=3))
    enc.save_pretrained(str(tmp_path / "a"))
    assert "problem_type" not in json.load(open(tmp_path / "a" / "config.json"))
    enc.criterion(torch.zeros(4, 3))
    enc.save_pretrained(str(tmp_path / "a"))                       # an existing directory is overwritten
    assert json.load(open(tmp_path / "a" / "config.json"))["problem_type"] == "multi_label_classification"
    assert T.Encoder.from_pretrained(str(tmp_path / "a")).cfg.problem_type == "multi_label_classification"
