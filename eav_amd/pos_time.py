"""An AST position table at another clip length: host tables and launches of csrc/pos_time.hip.

The checkpoint fixes one thing about the input length: its position table, [nextra + ny nx0, D] with nextra = 2 (cls,
distillation), ny = (mel - patch) // fstride + 1 frequency patches and nx0 = (cfg.W - patch) // tstride + 1 time patches, token
rows frequency-major (row nextra + f nx0 + t).  A forward on [B, T', mel] has nx = (T' - patch) // tstride + 1 time patches and
needs a [nextra + ny nx, D] table.  Hugging Face's AST has no argument for this; the rule is the one the AST authors' own
fine-tuning code uses for inputs of another length.  The nextra rows are copied, the frequency axis is untouched (the mel
bins are the checkpoint's), and the patch rows, seen as [ny, nx0, D] -> [ny, nx, D], follow the length alone:

    nx == nx0   the stored table as it is.
    nx <  nx0   CUT: the centre window, out[f, t] = pos[f, s + t] with s = nx0 // 2 - nx // 2 - one tap of weight 1, so the rows
                come out bit-equal to the source rows.
    nx >  nx0   LINEAR: F.interpolate(mode="bilinear", align_corners=False), which is linear along time because the frequency
                size is equal.  Per output o: scale = nx0 / nx, src = max((o + 0.5) scale - 0.5, 0), i0 = floor(src),
                i1 = min(i0 + 1, nx0 - 1), lam = src - i0, weights (1 - lam, lam) on (i0, i1).

There is no option to choose between cut and linear.  The fit is linear in the table, so its backward is the transposed
operator: for a cut, the window's rows of the gradient copied and exact zeros outside it.

Weights are computed in float64 and rounded to fp32 once.  Taps that coincide (i1 clamped onto i0) are SUMMED in float64
before the rounding: the first keeps the sum, the other gets weight 0, which the kernels skip.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def cut_start(nx0: int, nx: int) -> int:
    """First source time index of the centre window of nx out of nx0 time patches."""
    return nx0 // 2 - nx // 2


def time_tables(nx0: int, nx: int):
    """(idx int32 [nx, 2], w float32 [nx, 2]): the source time index and the weight of the two taps of every output time
    index; an unused or coincident second tap carries weight 0."""
    if nx0 < 1 or nx < 1:
        raise ValueError(f"time_tables: sizes must be positive, got {nx0} -> {nx}")
    o = np.arange(nx, dtype=np.float64)
    if nx <= nx0:                                  # cut (nx == nx0: the identity, s = 0)
        i0 = (cut_start(nx0, nx) + o).astype(np.int64)
        i1, lam = i0.copy(), np.zeros(nx, np.float64)
    else:
        src = np.maximum((o + 0.5) * (np.float64(nx0) / np.float64(nx)) - 0.5, 0.0)
        i0 = np.floor(src).astype(np.int64)
        i1 = np.minimum(i0 + 1, nx0 - 1)
        lam = src - i0
    w = np.stack([1.0 - lam, lam], 1)
    same = i0 == i1
    w[same, 0] += w[same, 1]
    w[same, 1] = 0.0
    return np.stack([i0, i1], 1).astype(np.int32), w.astype(np.float32)


def time_tables_transposed(idx, w, nx0: int):
    """The transposed (CSR) form: (ptr int32 [nx0 + 1], out int32 [nnz], w float32 [nnz]) - for every source time index the
    outputs that read it, ascending, with their weights.  Zero weights are left out."""
    rows = [[] for _ in range(nx0)]
    for o in range(idx.shape[0]):
        for a in range(2):
            if w[o, a] != 0.0:
                rows[int(idx[o, a])].append((o, w[o, a]))
    ptr = np.zeros(nx0 + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    flat = [e for r in rows for e in r]
    return (ptr, np.asarray([e[0] for e in flat], np.int32).reshape(-1),
            np.asarray([e[1] for e in flat], np.float32).reshape(-1))


def dense_time_matrix(idx, w, nx0: int):
    """[nx, nx0] float64 dense form of time_tables' output (fit_time, tests, documentation)."""
    m = np.zeros((idx.shape[0], nx0), np.float64)
    for o in range(idx.shape[0]):
        for a in range(2):
            m[o, idx[o, a]] += np.float64(w[o, a])
    return m


def dense_time_matrix_transposed(ptr, out, w, nx: int):
    """[nx, nx0] float64 dense form of time_tables_transposed's output."""
    m = np.zeros((nx, len(ptr) - 1), np.float64)
    for src in range(len(ptr) - 1):
        for k in range(ptr[src], ptr[src + 1]):
            m[out[k], src] += np.float64(w[k])
    return m


def fit_time(pos, ny: int, nx0: int, nx: int, nextra: int = 2):
    """pos [nextra + ny nx0, D] -> float64 [nextra + ny nx, D]: the table fitted to nx time patches on the host, with the
    tables the kernels use, in float64 arithmetic (Encoder.save_pretrained(max_length=...) writes this, cast to fp32: for a
    cut the source rows themselves)."""
    pos = np.asarray(pos, np.float64)
    if pos.ndim != 2 or pos.shape[0] != nextra + ny * nx0:
        raise ValueError(f"fit_time: expected a [{nextra + ny * nx0}, D] table, got {pos.shape}")
    D = pos.shape[1]
    grid = pos[nextra:].reshape(ny, nx0, D)
    if nx <= nx0:
        s = cut_start(nx0, nx)
        out = grid[:, s:s + nx]
    else:
        out = np.einsum("ts,fsd->ftd", dense_time_matrix(*time_tables(nx0, nx), nx0), grid)
    return np.concatenate([pos[:nextra], out.reshape(ny * nx, D)], 0)


_TABLES = {}        # (nx0, nx, device) -> device tables; they stay alive for every later (possibly captured) launch


def device_tables(nx0, nx, dev):
    """The device-resident tables of an nx0 -> nx fit: built once (a host-to-device copy - not inside a graph capture), then
    reused by every launch."""
    key = (int(nx0), int(nx), str(dev))
    t = _TABLES.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EavError("pos_time.device_tables: the first use of a length must not happen inside a graph capture")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        idx, w = time_tables(nx0, nx)
        tr = time_tables_transposed(idx, w, nx0)
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)  # noqa: E731     (no empty device array: a pointer is needed)
        t = _TABLES[key] = dict(fwd=(up(idx), up(w)), bwd=tuple(up(pad(a)) for a in tr), nnz=int(tr[1].size))
        torch.cuda.current_stream().synchronize()
    return t


def _check(t, rows, D, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            and t.numel() == rows * D):
        raise _lib.EavError(f"{name}: expected a contiguous fp32 device tensor of {rows} x {D} elements")


def pos_time_fwd(pos, out, ny, nx0, nx, nextra=2, stream=None):
    """out [nextra + ny nx, D] = the table pos [nextra + ny nx0, D] fitted to nx time patches (eav_pos_time_fwd)."""
    D = pos.shape[-1]
    _check(pos, nextra + ny * nx0, D, "pos_time_fwd: pos")
    _check(out, nextra + ny * nx, D, "pos_time_fwd: out")
    t = device_tables(nx0, nx, pos.device)
    _lib.call("eav_pos_time_fwd", pos.data_ptr(), out.data_ptr(), ny, nx0, nx, D, nextra,
              *[a.data_ptr() for a in t["fwd"]], _lib.stream_ptr() if stream is None else stream)


def pos_time_bwd(dout, dpos, ny, nx0, nx, nextra=2, stream=None):
    """dpos [nextra + ny nx0, D] = the adjoint of pos_time_fwd applied to dout [nextra + ny nx, D] (eav_pos_time_bwd); dpos
    may be a raw device address (the parameter's slice of a flat gradient buffer)."""
    D = dout.shape[-1]
    _check(dout, nextra + ny * nx, D, "pos_time_bwd: dout")
    if isinstance(dpos, torch.Tensor):
        _check(dpos, nextra + ny * nx0, D, "pos_time_bwd: dpos")
        dpos = dpos.data_ptr()
    t = device_tables(nx0, nx, dout.device)
    _lib.call("eav_pos_time_bwd", dout.data_ptr(), dpos, ny, nx0, nx, D, nextra, *[a.data_ptr() for a in t["bwd"]], t["nnz"],
              _lib.stream_ptr() if stream is None else stream)
