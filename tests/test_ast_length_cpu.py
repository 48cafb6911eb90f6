"""AST clips at their own length, without a device: the geometry rule, the host tables of eav_amd.pos_time against the float64
restatement (tests/ast_length_ref.py) and against torch's own interpolation, the host fit, and the exported checkpoint as
Hugging Face reads it (tests/golden/ast_length.npz)."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ast_length_ref as R
from tests.golden_util import tf_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCED = dict(hidden=64, layers=2, heads=4, ff=128)
KEY = "audio_spectrogram_transformer.embeddings.position_embeddings"


def _pairs():
    return sorted({(nx0, nx) for _, nx0, nx in R.GRIDS})


def test_geometry():
    from eav_amd import transformer as T
    cfg = T.make_config("ast", **REDUCED)
    before = dict(vars(cfg))

    def geo(t):
        g = T.ast_length_geometry(cfg, t)
        return g.nx, g.ntok

    assert (cfg.nx, cfg.ntok) == (101, 1214)
    assert geo(1024) == (101, 1214) and T.ast_length_geometry(cfg, 1024).time_grid is None
    assert geo(506) == (50, 602)
    assert geo(498)[0] == 49
    assert geo(16) == (1, 14)
    g = T.ast_length_geometry(cfg, 506)
    assert (g.W, g.H, g.ny, g.npatch, g.time_grid) == (506, 128, 12, 600, 101)
    for k, v in before.items():                       # the rest of cfg, unchanged - and cfg itself untouched
        if k not in ("W", "nx", "npatch", "ntok"):
            assert getattr(g, k) == v, k
    assert vars(cfg) == before
    with pytest.raises(ValueError):
        T.ast_length_geometry(cfg, 15)
    assert geo(1715) == (170, 2042)
    with pytest.raises(NotImplementedError):
        T.ast_length_geometry(cfg, 1726)              # 172 time patches: 2066 tokens
    with pytest.raises(NotImplementedError):
        T.ast_length_geometry(T.make_config("vit", **REDUCED), 512)


def test_auto_length():
    from eav_amd.audio import auto_max_length
    assert auto_max_length(80000) == 506              # EAV's 5 s clips: 498 frames
    assert auto_max_length(8000) == 56                # 48 frames
    assert auto_max_length(400) == 16                 # one frame: one patch


@pytest.mark.parametrize("nx0,nx", _pairs())
def test_host_tables_equal_the_restatement(nx0, nx):
    from eav_amd import pos_time as pt
    idx, w = pt.time_tables(nx0, nx)
    assert idx.shape == (nx, 2) and idx.dtype == np.int32 and w.shape == (nx, 2) and w.dtype == np.float32
    assert idx.min() >= 0 and idx.max() <= nx0 - 1
    ref = R.time_matrix(nx0, nx)
    dense = pt.dense_time_matrix(idx, w, nx0)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(dense - ref) <= ulp).all(), np.abs(dense - ref).max()
    if nx <= nx0:
        assert np.array_equal(dense, ref)                                  # a cut: zeros and ones
    assert (np.abs(dense.sum(1) - 1.0) <= 2 * 2.0 ** -24).all()           # the weights of each output sum to 1
    for o in range(nx):                                                    # coincident taps are folded
        assert idx[o, 0] != idx[o, 1] or w[o, 1] == 0.0
    ptr, out, wt = pt.time_tables_transposed(idx, w, nx0)
    assert ptr.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == len(out) == len(wt) and (np.diff(ptr) >= 0).all()
    assert len(out) <= 2 * nx and (len(out) == 0 or (out.min() >= 0 and out.max() <= nx - 1))
    assert np.array_equal(pt.dense_time_matrix_transposed(ptr, out, wt, nx), dense)
    for src in range(nx0):                                                 # fixed order: ascending outputs, no pair twice
        assert (np.diff(out[ptr[src]:ptr[src + 1]]) > 0).all()


def test_cut_start_for_odd_and_even_lengths():
    from eav_amd import pos_time as pt
    assert pt.cut_start(25, 9) == 8 and pt.cut_start(25, 10) == 7
    assert R.cut_window(25, 9) == (8, 17) and R.cut_window(25, 10) == (7, 17)
    assert pt.time_tables(25, 9)[0][:, 0].tolist() == list(range(8, 17))
    assert pt.time_tables(25, 10)[0][:, 0].tolist() == list(range(7, 17))
    assert pt.cut_start(101, 50) == 25


@pytest.mark.parametrize("ny,nx0,nx", R.GRIDS)
def test_fit_time_equals_torch(ny, nx0, nx):
    """Longer: F.interpolate(mode="bilinear", align_corners=False) on the [ny, nx0] grid to 1e-6; shorter: a slice, exactly.
    The table is drawn as golden_util.tf_weights draws position embeddings, N(0, 0.02^2): torch forms its weights in fp32
    (lam carries about nx0 2^-24), so the absolute difference scales with the table's magnitude."""
    from eav_amd import pos_time as pt
    from eav_amd import synth
    D = 8
    pos = synth.normal(41 + nx0 + nx, (2 + ny * nx0, D), 0.0, 0.02)
    got = pt.fit_time(pos, ny, nx0, nx, 2)
    assert got.dtype == np.float64 and got.shape == (2 + ny * nx, D)
    assert np.array_equal(got[:2], pos[:2])
    grid = pos[2:].reshape(ny, nx0, D)
    if nx <= nx0:
        s = nx0 // 2 - nx // 2
        assert np.array_equal(got[2:].astype(np.float32), grid[:, s:s + nx].reshape(ny * nx, D))
    else:
        ref = F.interpolate(torch.from_numpy(grid).permute(2, 0, 1)[None], size=(ny, nx), mode="bilinear", align_corners=False)
        ref = ref[0].permute(1, 2, 0).reshape(ny * nx, D).numpy().astype(np.float64)
        assert np.abs(got[2:] - ref).max() <= 1e-6
    assert np.abs(got - R.fit(pos, ny, nx0, nx)).max() <= 4 * 2.0 ** -24 * np.abs(pos).max()
    with pytest.raises(ValueError):
        pt.fit_time(pos[1:], ny, nx0, nx, 2)


def test_attributes_signatures_and_symbols():
    from eav_amd import _lib
    from eav_amd import transformer as T
    from eav_amd.audio import AudioModelTrainer
    model = T.Encoder(T.make_config("ast", hidden=64, layers=1, heads=4, ff=128, frames=64))
    assert model.variable_length is False
    p = inspect.signature(T.Encoder.save_pretrained).parameters
    assert list(p) == ["self", "save_directory", "max_length"] and p["max_length"].default is None
    p = inspect.signature(AudioModelTrainer.__init__).parameters
    assert list(p) == ["self", "DATA", "model_path", "sub", "num_classes", "weight_decay", "lr", "batch_size", "problem_type",
                       "max_length"]
    assert p["max_length"].kind is inspect.Parameter.KEYWORD_ONLY and p["max_length"].default is None
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("eav_pos_time_fwd", "eav_pos_time_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert _lib.plain("eav_abi_version") == 3


def test_bad_arguments_return_a_status_without_a_launch():
    from eav_amd import _lib
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data
    a16 = a + (-a % 16)
    with pytest.raises(_lib.EavError, match="eav_pos_time_fwd"):
        _lib.call("eav_pos_time_fwd", a16, a16 + 64, 1, 2, 3, 6, 2, a, a, None)               # D % 4 != 0
    with pytest.raises(_lib.EavError, match="eav_pos_time_fwd"):
        _lib.call("eav_pos_time_fwd", a16, a16 + 64, 1, 2, 3, 4, 2, None, a, None)            # a table is missing
    with pytest.raises(_lib.EavError, match="eav_pos_time_fwd"):
        _lib.call("eav_pos_time_fwd", a16, a16 + 4, 1, 2, 3, 4, 2, a, a, None)                # out not 16-byte aligned
    with pytest.raises(_lib.EavError, match="eav_pos_time_fwd"):
        _lib.call("eav_pos_time_fwd", a16, a16 + 64, 1, 2, 3, 4, 3, a, a, None)               # nextra = 3
    with pytest.raises(_lib.EavError, match="eav_pos_time_bwd"):
        _lib.call("eav_pos_time_bwd", a16, a16, 1, 2, 3, 4, 2, a, a, a, 4, None)              # in place
    with pytest.raises(_lib.EavError, match="eav_pos_time_bwd"):
        _lib.call("eav_pos_time_bwd", a16, a16 + 64, 1, 0, 3, 4, 2, a, a, a, 4, None)         # nx0 = 0
    with pytest.raises(_lib.EavError, match="eav_pos_time_bwd"):
        _lib.call("eav_pos_time_bwd", a16, a16 + 64, 1, 2, 2049, 4, 2, a, a, a, 4, None)      # nx beyond 2048


# ============================================================================================ export
def _reduced_model(g):
    from eav_amd import transformer as T
    from oracle import vit_oracle as vo
    shapes = vo.param_shapes(vo.cfg_ast(**REDUCED, frames=int(g["native"])))        # (the order the golden drew them in)
    return T.Encoder(T.make_config("ast", **REDUCED, frames=int(g["native"])),
                     tf_weights(int(g["wseed"]), shapes, std=float(g["std"])))


def test_save_pretrained_at_another_length_is_a_stock_hf_model(golden_dir, tmp_path):
    """save_pretrained(dir, max_length=96): HF's ASTForAudioClassification loads the directory with no missing or
    mismatched key, and its CPU logits on the golden's clips are the golden's (HF on the torch-fitted table) within 1e-5."""
    from transformers import ASTForAudioClassification
    g = np.load(os.path.join(golden_dir, "ast_length.npz"))
    model = _reduced_model(g)
    model.save_pretrained(str(tmp_path), max_length=96)
    cfg = json.load(open(tmp_path / "config.json"))
    assert cfg["max_length"] == 96 and cfg["num_mel_bins"] == 128
    hf, info = ASTForAudioClassification.from_pretrained(str(tmp_path), output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
    table = hf.state_dict()[KEY]
    assert tuple(table.shape) == (1, 2 + 12 * 9, 64)
    stored = model.state_dict()[KEY][0, 2:].reshape(12, 25, 64)
    assert torch.equal(table[0, 2:].reshape(12, 9, 64), stored[:, 8:17])          # the centre window, bit for bit
    assert torch.equal(table[0, :2], model.state_dict()[KEY][0, :2])
    x, _ = R.clips(int(g["xseed"]) + 96, int(g["B"]), 96)
    hf.eval()
    with torch.no_grad():
        logits = hf(torch.from_numpy(x)).logits.numpy()
    assert np.abs(logits - g["logits96"]).max() <= 1e-5
    # the model itself keeps the checkpoint's shapes
    assert model.cfg.W == 256 and tuple(model.state_dict()[KEY].shape) == (1, 302, 64)


def test_default_save_pretrained_keeps_the_checkpoint_length(tmp_path):
    from safetensors.numpy import load_file
    from eav_amd import transformer as T
    model = T.Encoder(T.make_config("ast", hidden=64, layers=1, heads=4, ff=128))
    model.save_pretrained(str(tmp_path))
    assert json.load(open(tmp_path / "config.json"))["max_length"] == 1024
    assert load_file(str(tmp_path / "model.safetensors"))[KEY].shape == (1, 1214, 64)
    with pytest.raises(ValueError):
        model.save_pretrained(str(tmp_path / "short"), max_length=8)
    assert not (tmp_path / "short").exists()
    vit = T.Encoder(T.make_config("vit", hidden=64, layers=1, heads=4, ff=128, image=32))
    with pytest.raises(NotImplementedError):
        vit.save_pretrained(str(tmp_path / "vit"), max_length=96)
