"""A ViT position table at another patch grid: host tables and launches of csrc/pos_interp.hip.

HF's ViTEmbeddings.interpolate_pos_encoding resamples the [g, g, D] patch rows of the position table with
F.interpolate(mode="bicubic", align_corners=False) - no antialiasing - and keeps the cls row.  Per axis, with
scale = n_in / n_out and A = -0.75: s = (o + 0.5) scale - 0.5 (not clamped), i = floor(s), t = s - i, taps at i-1 .. i+2, each
index clamped to [0, n_in - 1], with the cubic-convolution coefficients of bicubic_axis_tables.  The operator is separable,
out = (Wy (x) Wx) pos, and linear in the table, so its backward is the transposed operator.

Tables are built in float64 and rounded to fp32 once.  Taps that the clamp folds onto one source index are SUMMED in
float64 before the rounding (the first of them keeps the sum, the others get weight 0, which the kernels skip): the fp32 entry
of the dense operator is then the rounded float64 entry, whatever cancels between the folded taps.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

CUBIC_A = -0.75


def _cubic_coefficients(t):
    """[len(t), 4] float64 cubic-convolution weights of the taps i-1, i, i+1, i+2 at fraction t."""
    A = CUBIC_A
    outer = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A      # noqa: E731   1 <= x <= 2
    inner = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0            # noqa: E731   0 <= x <= 1
    return np.stack([outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)], 1)


def bicubic_axis_tables(n_in: int, n_out: int):
    """(idx int32 [n_out, 4], w float32 [n_out, 4]) of one axis: the clamped source index and the weight of each tap;
    duplicates of an index within a row carry weight 0 (their float64 weights are folded into its first occurrence)."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"bicubic_axis_tables: sizes must be positive, got {n_in} -> {n_out}")
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5
    i = np.floor(s)
    w = _cubic_coefficients(s - i)
    idx = np.clip(i[:, None].astype(np.int64) + np.arange(-1, 3)[None, :], 0, n_in - 1)
    for o in range(n_out):
        for a in range(1, 4):
            first = int(np.argmax(idx[o] == idx[o, a]))
            if first < a:
                w[o, first] += w[o, a]
                w[o, a] = 0.0
    return idx.astype(np.int32), w.astype(np.float32)


def bicubic_axis_transposed(idx, w, n_in: int):
    """The transposed (CSR) form of one axis: (ptr int32 [n_in + 1], out int32 [nnz], w float32 [nnz]) - for every source
    index the outputs that read it, ascending, with their weights.  Zero weights (the folded duplicates) are left out."""
    rows = [[] for _ in range(n_in)]
    for o in range(idx.shape[0]):
        for a in range(4):
            if w[o, a] != 0.0:
                rows[int(idx[o, a])].append((o, w[o, a]))
    ptr = np.zeros(n_in + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    flat = [e for r in rows for e in r]
    return (ptr, np.asarray([e[0] for e in flat], np.int32).reshape(-1),
            np.asarray([e[1] for e in flat], np.float32).reshape(-1))


def dense_axis_matrix(idx, w, n_in: int):
    """[n_out, n_in] float64 dense form of bicubic_axis_tables' output (tests, documentation)."""
    m = np.zeros((idx.shape[0], n_in), np.float64)
    for o in range(idx.shape[0]):
        for a in range(4):
            m[o, idx[o, a]] += np.float64(w[o, a])
    return m


def dense_axis_matrix_transposed(ptr, out, w, n_out: int):
    """[n_out, n_in] float64 dense form of bicubic_axis_transposed's output."""
    m = np.zeros((n_out, len(ptr) - 1), np.float64)
    for src in range(len(ptr) - 1):
        for k in range(ptr[src], ptr[src + 1]):
            m[out[k], src] += np.float64(w[k])
    return m


_TABLES = {}        # (g, ny, nx, device) -> device tables; they stay alive for every later (possibly captured) launch


def device_tables(g, ny, nx, dev):
    """The device-resident tables of a (g, ny, nx) resampling: built once (a host-to-device copy - not inside a graph
    capture), then reused by every launch."""
    key = (int(g), int(ny), int(nx), str(dev))
    t = _TABLES.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EavError("pos_interp.device_tables: the first use of a grid must not happen inside a graph capture")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        iy, wy = bicubic_axis_tables(g, ny)
        ix, wx = bicubic_axis_tables(g, nx)
        ty, tx = bicubic_axis_transposed(iy, wy, g), bicubic_axis_transposed(ix, wx, g)
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)  # noqa: E731     (no empty device array: a pointer is needed)
        t = _TABLES[key] = dict(fwd=tuple(up(a) for a in (iy, wy, ix, wx)),
                                bwd_y=tuple(up(pad(a)) for a in ty), nnzy=int(ty[1].size),
                                bwd_x=tuple(up(pad(a)) for a in tx), nnzx=int(tx[1].size))
        torch.cuda.current_stream().synchronize()
    return t


def _check(t, rows, D, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            and t.numel() == rows * D):
        raise _lib.EavError(f"{name}: expected a contiguous fp32 device tensor of {rows} x {D} elements")


def pos_bicubic_fwd(pos, out, g, ny, nx, nextra=1, stream=None):
    """out [nextra + ny nx, D] = the table pos [nextra + g g, D] resampled to a ny x nx grid (eav_pos_bicubic_fwd)."""
    D = pos.shape[-1]
    _check(pos, nextra + g * g, D, "pos_bicubic_fwd: pos")
    _check(out, nextra + ny * nx, D, "pos_bicubic_fwd: out")
    t = device_tables(g, ny, nx, pos.device)
    _lib.call("eav_pos_bicubic_fwd", pos.data_ptr(), out.data_ptr(), g, ny, nx, D, nextra,
              *[a.data_ptr() for a in t["fwd"]], _lib.stream_ptr() if stream is None else stream)


def pos_bicubic_bwd(dout, dpos, g, ny, nx, nextra=1, stream=None):
    """dpos [nextra + g g, D] = the adjoint of pos_bicubic_fwd applied to dout [nextra + ny nx, D] (eav_pos_bicubic_bwd);
    dpos may be a raw device address (the parameter's slice of a flat gradient buffer)."""
    D = dout.shape[-1]
    _check(dout, nextra + ny * nx, D, "pos_bicubic_bwd: dout")
    if isinstance(dpos, torch.Tensor):
        _check(dpos, nextra + g * g, D, "pos_bicubic_bwd: dpos")
        dpos = dpos.data_ptr()
    t = device_tables(g, ny, nx, dout.device)
    _lib.call("eav_pos_bicubic_bwd", dout.data_ptr(), dpos, g, ny, nx, D, nextra,
              *[a.data_ptr() for a in t["bwd_y"]], t["nnzy"], *[a.data_ptr() for a in t["bwd_x"]], t["nnzx"],
              _lib.stream_ptr() if stream is None else stream)
