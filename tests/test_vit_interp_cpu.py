"""interpolate_pos_encoding without a device: the host tables of eav_amd.pos_interp against the float64 reference
(tests/vit_interp_ref.py) and against torch's own bicubic interpolation, the geometry rule, and the public signatures."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vit_interp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _axes():
    return sorted({(g, n) for g, ny, nx in R.GRIDS for n in (ny, nx)})


@pytest.mark.parametrize("n_in,n_out", _axes())
def test_host_tables_equal_the_float64_matrices_to_one_ulp(n_in, n_out):
    from eav_amd import pos_interp as pi
    idx, w = pi.bicubic_axis_tables(n_in, n_out)
    assert idx.shape == (n_out, 4) and idx.dtype == np.int32 and w.shape == (n_out, 4) and w.dtype == np.float32
    assert idx.min() >= 0 and idx.max() <= n_in - 1
    ref = R.axis_matrix(n_in, n_out)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    dense = pi.dense_axis_matrix(idx, w, n_in)
    assert (np.abs(dense - ref) <= ulp).all(), np.abs(dense - ref).max()
    # the transposed lists hold the same operator: every (output, source) weight once, border taps summed - not dropped
    ptr, out, wt = pi.bicubic_axis_transposed(idx, w, n_in)
    assert ptr.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == len(out) == len(wt) and (np.diff(ptr) >= 0).all()
    assert len(out) == 0 or (out.min() >= 0 and out.max() <= n_out - 1)
    assert np.array_equal(pi.dense_axis_matrix_transposed(ptr, out, wt, n_out), dense)
    assert (np.abs(dense.sum(1) - 1.0) <= 4 * 2.0 ** -24).all()          # a cubic-convolution row sums to 1
    for src in range(n_in):                                               # fixed order: ascending outputs, no pair twice
        o = out[ptr[src]:ptr[src + 1]]
        assert (np.diff(o) > 0).all()


@pytest.mark.parametrize("g,ny,nx", R.GRIDS)
def test_tables_reproduce_torch_bicubic_and_its_adjoint(g, ny, nx):
    """The product's tables applied in float64 against F.interpolate (fp32, CPU) and its autograd adjoint: 4e-6 of the largest
    value - torch rounds its coefficients to fp32 (measured worst case 1.1e-6 forward, 1.0e-6 backward)."""
    from eav_amd import pos_interp as pi
    from eav_amd import synth
    D = 8
    Wy = pi.dense_axis_matrix(*pi.bicubic_axis_tables(g, ny), g)
    Wx = pi.dense_axis_matrix(*pi.bicubic_axis_tables(g, nx), g)
    x = torch.from_numpy(synth.normal(31 + g + ny, (1, D, g, g))).requires_grad_(True)
    y = F.interpolate(x, size=(ny, nx), mode="bicubic", align_corners=False)
    gy = torch.from_numpy(synth.normal(32 + g + nx, (1, D, ny, nx)))
    y.backward(gy)
    fwd = np.einsum("ab,cd,kbd->kac", Wy, Wx, x.detach().numpy()[0].astype(np.float64))
    ref = y.detach().numpy()[0].astype(np.float64)
    assert np.abs(fwd - ref).max() <= 4e-6 * np.abs(ref).max()
    bwd = np.einsum("ab,cd,kac->kbd", Wy, Wx, gy.numpy()[0].astype(np.float64))
    refb = x.grad.numpy()[0].astype(np.float64)
    assert np.abs(bwd - refb).max() <= 4e-6 * np.abs(refb).max()
    # ... and the reference's own resample / adjoint say the same (they are what the GPU tests compare against)
    pos = np.concatenate([np.zeros((1, D)), x.detach().numpy()[0].transpose(1, 2, 0).reshape(g * g, D)], 0)
    assert np.abs(R.resample(pos, g, ny, nx)[1:].reshape(ny, nx, D).transpose(2, 0, 1) - ref).max() <= 4e-6 * np.abs(ref).max()


def test_interpolated_geometry():
    from eav_amd import transformer as T
    cfg = T.make_config("vit", hidden=64, layers=2, heads=4, ff=128)
    before = dict(vars(cfg))

    def geo(h, w):
        g = T.interpolated_geometry(cfg, h, w)
        return g.ny, g.nx, g.ntok

    assert geo(112, 112) == (7, 7, 50)
    assert geo(56, 56) == (3, 3, 10)
    assert geo(64, 144) == (4, 9, 37)
    g = T.interpolated_geometry(cfg, 64, 144)
    assert (g.H, g.W, g.npatch, g.pos_grid) == (64, 144, 36, 14)
    for k, v in before.items():                       # the rest of cfg, unchanged - and cfg itself untouched
        if k not in ("H", "W", "ny", "nx", "npatch", "ntok"):
            assert getattr(g, k) == v, k
    assert vars(cfg) == before
    # HF's shortcut, literally: the stored table whenever the patch COUNT matches and the image is square
    assert T.interpolated_geometry(cfg, 224, 224).pos_grid is None
    assert T.interpolated_geometry(cfg, 230, 230).pos_grid is None and geo(230, 230) == (14, 14, 197)
    assert T.interpolated_geometry(cfg, 224, 225).pos_grid == 14
    with pytest.raises(ValueError):
        T.interpolated_geometry(cfg, 15, 224)
    with pytest.raises(ValueError):
        T.interpolated_geometry(cfg, 224, 8)
    with pytest.raises(NotImplementedError):
        T.interpolated_geometry(cfg, 46 * 16, 46 * 16)          # 2117 tokens
    assert geo(45 * 16, 45 * 16) == (45, 45, 2026)
    with pytest.raises(NotImplementedError):
        T.interpolated_geometry(T.make_config("ast", hidden=64, layers=1, heads=4, ff=128), 128, 1024)


def test_signatures_and_symbols():
    from eav_amd import _lib
    from eav_amd import transformer as T
    from eav_amd.vision import ImageClassifierTrainer
    p = inspect.signature(T.Encoder.forward).parameters
    assert list(p) == ["self", "x", "labels", "pixel_values", "input_values", "interpolate_pos_encoding"]
    assert p["interpolate_pos_encoding"].default is None
    model = T.Encoder(T.make_config("vit", hidden=64, layers=1, heads=4, ff=128, image=32))
    assert model.interpolate_pos_encoding is False
    p = inspect.signature(ImageClassifierTrainer.__init__).parameters
    assert list(p) == ["self", "DATA", "model_path", "sub", "num_labels", "lr", "batch_size", "problem_type", "image_size"]
    assert p["image_size"].kind is inspect.Parameter.KEYWORD_ONLY and p["image_size"].default is None
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("eav_pos_bicubic_fwd", "eav_pos_bicubic_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert _lib.plain("eav_abi_version") == 3


def test_bad_arguments_return_a_status_without_a_launch():
    """The entry points refuse bad arguments on the host (status + message), as every other one does."""
    from eav_amd import _lib
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data
    a16 = a + (-a % 16)
    with pytest.raises(_lib.EavError, match="eav_pos_bicubic_fwd"):
        _lib.call("eav_pos_bicubic_fwd", a16, a16 + 64, 2, 3, 3, 6, 1, a, a, a, a, None)          # D % 4 != 0
    with pytest.raises(_lib.EavError, match="eav_pos_bicubic_fwd"):
        _lib.call("eav_pos_bicubic_fwd", a16, a16 + 64, 2, 3, 3, 4, 1, None, a, a, a, None)       # a table is missing
    with pytest.raises(_lib.EavError, match="eav_pos_bicubic_bwd"):
        _lib.call("eav_pos_bicubic_bwd", a16, a16, 2, 3, 3, 4, 1, a, a, a, 6, a, a, a, 6, None)   # in place
    with pytest.raises(_lib.EavError, match="eav_pos_bicubic_bwd"):
        _lib.call("eav_pos_bicubic_bwd", a16, a16 + 64, 0, 3, 3, 4, 1, a, a, a, 6, a, a, a, 6, None)   # g = 0
