"""The two layer schedules of transformer.Encoder, one class each, and the side streams of the split one.

    Fp32Layers    every product on the exact-fp32 MFMA (gemm_f32.hip, attention.hip; precision "fp32", and through
                  gemm_name "bf16" / "bf16_bwd")
    SplitLayers   every product on the fp16 matrix cores with fp16 hi + lo operand planes (gemm_sp.hip, attention_sp.hip;
                  precision "split"), weight gradients and final reductions beside the main stream (SideStreams)

Each owns its path's share of the workspace, what a forward / a backward prepares, the patch-embedding product and its
weight gradient, and one layer forward / backward.  The encoder (`m`) keeps what both read: the stream of the launch
sequence, the workspace, the geometry, the dropout state, the parameter and gradient pointers.  The materialised-score
attention (head_dim != 64) is the same fp32 kernels on both paths: softmax_forward / attention_backward_scores.
"""
from __future__ import annotations

from functools import partial

import numpy as np
import torch

from . import _lib
from .weight_planes import SLOT, WeightPlanes

# eav_gemm_sp_ex flags (include/eav_hip.h EAV_GEMM_*)
GEMM_ONE_TERM, GEMM_SHARED_GPU, GEMM_PLANES_NOLIFT, GEMM_NO_BLOCKMAX = 1, 2, 4, 8
# Scale slots of the split path.  ws.fslot: [0] the im2col rows, then FS per layer; ws.bslot: [0] max|dh| below layer 0, then
# BS per layer, then the patch rows of dh.
F_Y1, F_QKV, F_AO, F_Y2, F_ACT = FWD_SLOTS = range(5)
B_DH2, B_DACT, B_DH1, B_DAO, B_DS, B_DQKV, B_DY2, B_DY1 = BWD_SLOTS = range(8)     # dh(fc2), dact, dh(o), dao, dS, dqkv, dy(fc1), dy(qkv)
FS, BS = len(FWD_SLOTS), len(BWD_SLOTS)


def path_on(ws, i):
    """Whether layer i of the forward on this workspace drops paths (encoder_drop_path: p_i > 0 in training mode)."""
    dp = ws.dpath
    return dp is not None and 0 <= i < len(dp.p) and dp.on(i)


def gemm_f32(m, A, B, C, M, N, K, lda, ldb, ldc, tA=0, tB=0, batch=1, heads=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), alpha=1.0):
    m._call("eav_gemm_f32", A, B, C, M, N, K, lda, ldb, ldc, tA, tB, batch, heads, sA[0], sA[1], sB[0], sB[1],
            sC[0], sC[1], float(alpha), None, 0, None, None, 0, 0, m._st)


def softmax_forward(m, i, Pm, rows, N, ldn):
    """Materialised-score path: softmax in place over the scores of layer i; returns the operand of the P.V product -
    P itself, or with attention dropout the dropped probabilities (P stays undropped for the Jacobian)."""
    ws = m._ws
    d = ws.drop
    if d.pa > 0.0:
        m._call("eav_softmax_dropout_fwd", Pm, _lib.ptr(ws.Pd), rows, N, ldn, *d.site("attn", i), m._st)
        return _lib.ptr(ws.Pd)
    m._call("eav_softmax_fwd", Pm, rows, N, ldn, m._st)
    return Pm


def attention_backward_scores(m, g, i, qkv, dao, dqkv, scale):
    """Materialised-score path, backward of the attention core of layer i with the batched product `g`: dV = Pd^T dO,
    dP = dO V^T, dS = softmax backward (in place over dP), dQ = s dS K, dK = s dS^T Q.  With attention dropout the
    softmax backward gates dP and regenerates the dropped probabilities Pd, so it runs before the dV product."""
    c, ws = m._geo, m._ws
    D, N, H = c.hidden, c.ntok, c.heads
    hd, ldn, B = D // H, ws.ldn, ws.B
    P, d = _lib.ptr, ws.drop
    Pm, dP = P(ws.P[i]), P(ws.dP)
    sP, sQ, sO = (H * N * ldn, N * ldn), (N * 3 * D, hd), (N * D, hd)
    if d.pa > 0.0:
        g(dao, qkv + 8 * D, dP, N, N, hd, D, 3 * D, ldn, batch=B * H, heads=H, sA=sO, sB=sQ, sC=sP)
        m._call("eav_softmax_dropout_bwd", Pm, dP, P(ws.Pd), B * H * N, N, ldn, *d.site("attn", i), m._st)
        g(P(ws.Pd), dao, dqkv + 8 * D, N, hd, N, ldn, D, 3 * D, tA=1, tB=1, batch=B * H, heads=H, sA=sP, sB=sO, sC=sQ)
    else:
        g(Pm, dao, dqkv + 8 * D, N, hd, N, ldn, D, 3 * D, tA=1, tB=1, batch=B * H, heads=H, sA=sP, sB=sO, sC=sQ)
        g(dao, qkv + 8 * D, dP, N, N, hd, D, 3 * D, ldn, batch=B * H, heads=H, sA=sO, sB=sQ, sC=sP)
        m._call("eav_softmax_bwd", Pm, dP, B * H * N, N, ldn, m._st)
    g(dP, qkv + 4 * D, dqkv, N, hd, N, ldn, 3 * D, 3 * D, tB=1, batch=B * H, heads=H, sA=sP, sB=sQ, sC=sQ, alpha=scale)
    g(dP, qkv, dqkv + 4 * D, N, hd, N, ldn, 3 * D, 3 * D, tA=1, tB=1, batch=B * H, heads=H, sA=sP, sB=sQ, sC=sQ,
      alpha=scale)


# ----------------------------------------------------------------------------- exact fp32
class Fp32Layers:
    """The schedule on the exact-fp32 GEMM and attention kernels: fp32 copies of what the backward reads, one stream."""
    split, SPLITK_PLAN = False, "eav_gemm_f32_splitk_plan"

    def __init__(self, m):
        self.m = m

    @staticmethod
    def fp32_copies(nsave):
        """How many fp32 copies of a layer's GEMM inputs the workspace keeps: one per saved layer."""
        return nsave

    def gemm_name(self):
        m = self.m
        p = m.precision
        if p not in ("fp32", "split", "bf16", "bf16_bwd"):
            raise ValueError(f"unknown precision {p!r}")
        low = p == "bf16" or (p == "bf16_bwd" and m._phase == "bwd")
        return "eav_gemm_bf16" if low else "eav_gemm_f32"

    def gemm(self, A, B, C, M, N, K, lda, ldb, ldc, tA=0, tB=0, batch=1, heads=1, sA=(0, 0), sB=(0, 0), sC=(0, 0),
             alpha=1.0, bias=None, gelu=0, pre=None, resid=None, ldr=0, acc=0):
        self.m._call(self.gemm_name(), A, B, C, M, N, K, lda, ldb, ldc, tA, tB, batch, heads, sA[0], sA[1], sB[0],
                     sB[1], sC[0], sC[1], float(alpha), bias, gelu, pre, resid, ldr, acc, self.m._st)

    def wgrad(self, A, B, C, M, N, K, lda, ldb):
        """C[M,N] = A^T.B for A stored [K,M], B stored [K,N] (weight gradient: contraction over tokens)."""
        m = self.m
        m._call(self.gemm_name() + "_splitk", A, B, C, _lib.ptr(m._ws.splitk), M, N, K, lda, ldb, 1, 1, m._st)

    def bias_grad(self, dy_ptr, M, N, ld, out):
        m, ws = self.m, self.m._ws
        m._call("eav_colsum", dy_ptr, _lib.ptr(ws.part_cs), M, N, ld, m._st)
        m._call("eav_reduce_partials", _lib.ptr(ws.part_cs), ws.np_cs, N, N, 1.0, out, m._st)

    def alloc(self, ws, dev, nsave):
        pass

    def begin_forward(self, ws, dev, full):
        pass

    def begin_backward(self, ws):
        pass

    def patch_embed(self, ws, h0, bias):
        m, c, P = self.m, self.m._geo, _lib.ptr
        self.gemm(P(ws.col), m._w(f"{c.prefix}.embeddings.patch_embeddings.projection.weight"),
                  P(h0) + 4 * c.nextra * c.hidden, c.npatch, c.hidden, c.kp, c.kp, c.kp, c.hidden, batch=ws.B,
                  sA=(c.npatch * c.kp, 0), sC=(c.ntok * c.hidden, 0), bias=bias)

    def patch_wgrad(self, ws, gw, MP):
        c, P = self.m._geo, _lib.ptr
        self.wgrad(P(ws.demb), P(ws.col), gw, c.hidden, c.kp, MP, c.hidden, c.kp)

    def layer_forward(self, i, j, hin, hout, Lk, stp, scale):
        """One encoder layer on the exact-fp32 GEMM and attention kernels (precision "fp32"; gemm_name: also bf16)."""
        m = self.m
        c, ws = m._geo, m._ws
        P, L, st, w, gemm = _lib.ptr, m._call, m._st, m._w, self.gemm
        D, FF, N, H, M, B, ldn = c.hidden, c.ff, c.ntok, c.heads, ws.M, ws.B, ws.ldn
        hd = D // H
        drop = ws.drop
        L("eav_layernorm_fwd", P(hin), w(f"{Lk}.layernorm_before.weight"), w(f"{Lk}.layernorm_before.bias"),
          P(ws.y1[j]), stp, stp + 4 * M, M, D, c.eps, st)
        qkv = P(ws.qkv[j])
        gemm(P(ws.y1[j]), w(f"{Lk}.attention.q_proj.weight"), qkv, M, 3 * D, D, D, D, 3 * D,
             bias=w(f"{Lk}.attention.q_proj.bias"))
        if ws.fused and drop.pa > 0.0:
            L("eav_attn_fwd_dropout", qkv, P(ws.ao[j]), P(ws.lse[j]), B, H, N, hd, scale, *drop.site("attn", i), st)
        elif ws.fused:
            L("eav_attn_fwd", qkv, P(ws.ao[j]), P(ws.lse[j]), B, H, N, hd, scale, st)
        else:
            Pm = P(ws.P[j])
            gemm(qkv, qkv + 4 * D, Pm, N, N, hd, 3 * D, 3 * D, ldn, batch=B * H, heads=H,
                 sA=(N * 3 * D, hd), sB=(N * 3 * D, hd), sC=(H * N * ldn, N * ldn), alpha=scale)
            Pv = softmax_forward(m, i, Pm, B * H * N, N, ldn)
            gemm(Pv, qkv + 8 * D, P(ws.ao[j]), N, hd, N, ldn, 3 * D, D, tB=1, batch=B * H, heads=H,
                 sA=(H * N * ldn, N * ldn), sB=(N * 3 * D, hd), sC=(N * D, hd))
        m._outputs.attention(i, j, scale, qkv=qkv)
        # (hidden dropout sits between the bias and the residual add: the product leaves without the residual and one
        # element-wise pass forms resid + Dropout(product); drop path - a layer with p_i > 0 - takes the same road with its
        # per-sample scales)
        hd_on = drop.ph > 0.0
        dp_on = path_on(ws, i)
        bare = hd_on or dp_on
        gemm(P(ws.ao[j]), w(f"{Lk}.attention.o_proj.weight"), P(ws.hmid[j]), M, D, D, D, D, D,
             bias=w(f"{Lk}.attention.o_proj.bias"), resid=None if bare else P(hin), ldr=0 if bare else D)
        if hd_on:
            m._drop_add(P(ws.hmid[j]), P(hin), P(ws.hmid[j]), M * D, "attn_out", i)
        elif dp_on:
            m._path_add(P(ws.hmid[j]), P(hin), P(ws.hmid[j]), i, 0)
        L("eav_layernorm_fwd", P(ws.hmid[j]), w(f"{Lk}.layernorm_after.weight"), w(f"{Lk}.layernorm_after.bias"),
          P(ws.y2[j]), stp + 8 * M, stp + 12 * M, M, D, c.eps, st)
        gemm(P(ws.y2[j]), w(f"{Lk}.mlp.fc1.weight"), P(ws.act[j]), M, FF, D, D, D, FF,
             bias=w(f"{Lk}.mlp.fc1.bias"), gelu=1, pre=P(ws.pre[j]))
        gemm(P(ws.act[j]), w(f"{Lk}.mlp.fc2.weight"), P(hout), M, D, FF, FF, FF, D,
             bias=w(f"{Lk}.mlp.fc2.bias"), resid=None if bare else P(ws.hmid[j]), ldr=0 if bare else D)
        if hd_on:
            m._drop_add(P(hout), P(ws.hmid[j]), P(hout), M * D, "mlp_out", i)
        elif dp_on:
            m._path_add(P(hout), P(ws.hmid[j]), P(hout), i, 1)

    def layer_backward(self, i, Lk, stp, scale):
        """Backward of one layer on the exact-fp32 kernels: ws.dh holds the gradient w.r.t. the layer output on entry, the
        gradient w.r.t. the layer input on exit."""
        m = self.m
        c, ws = m._geo, m._ws
        P, L, st, w, gp = _lib.ptr, m._call, m._st, m._w, m._gp
        gemm, wgrad, bias_grad = self.gemm, self.wgrad, self.bias_grad
        D, FF, N, H, M, B = c.hidden, c.ff, c.ntok, c.heads, ws.M, ws.B
        hd = D // H
        drop = ws.drop
        dh, dy, dao, dact, dqkv = P(ws.dh), P(ws.dy), P(ws.dao), P(ws.dact), P(ws.dqkv)
        # fc2: h_out = h_mid + Dropout(act.W2^T + b2): the products see dh o M / (1 - p), the residual branch dh (drop path:
        # dh[b] s[b])
        g_dh = dh
        dp_on = path_on(ws, i)
        if drop.ph > 0.0:
            g_dh = P(ws.dhd)
            m._drop_add(dh, None, g_dh, M * D, "mlp_out", i)
        elif dp_on:
            g_dh = P(ws.dhd)
            m._path_add(dh, None, g_dh, i, 1)
        wgrad(g_dh, P(ws.act[i]), gp(f"{Lk}.mlp.fc2.weight"), D, FF, M, D, FF)
        bias_grad(g_dh, M, D, D, gp(f"{Lk}.mlp.fc2.bias"))
        gemm(g_dh, w(f"{Lk}.mlp.fc2.weight"), dact, M, FF, D, D, FF, FF, tB=1)
        L("eav_gelu_bwd", dact, P(ws.pre[i]), M * FF, st)
        # fc1
        wgrad(dact, P(ws.y2[i]), gp(f"{Lk}.mlp.fc1.weight"), FF, D, M, FF, D)
        bias_grad(dact, M, FF, FF, gp(f"{Lk}.mlp.fc1.bias"))
        gemm(dact, w(f"{Lk}.mlp.fc1.weight"), dy, M, D, FF, FF, D, D, tB=1)
        # layernorm_after: dh (now gradient w.r.t. h_mid) += LN backward
        L("eav_layernorm_bwd", dy, P(ws.hmid[i]), w(f"{Lk}.layernorm_after.weight"), stp + 8 * M,
          stp + 12 * M, dh, 1, P(ws.part_ln), M, D, st)
        m._reduce_ln(ws.part_ln, ws.np_ln, gp(f"{Lk}.layernorm_after.weight"), gp(f"{Lk}.layernorm_after.bias"))
        # o_proj
        if drop.ph > 0.0:
            m._drop_add(dh, None, g_dh, M * D, "attn_out", i)
        elif dp_on:
            m._path_add(dh, None, g_dh, i, 0)
        wgrad(g_dh, P(ws.ao[i]), gp(f"{Lk}.attention.o_proj.weight"), D, D, M, D, D)
        bias_grad(g_dh, M, D, D, gp(f"{Lk}.attention.o_proj.bias"))
        gemm(g_dh, w(f"{Lk}.attention.o_proj.weight"), dao, M, D, D, D, D, D, tB=1)
        # attention core
        qkv = P(ws.qkv[i])
        if ws.fused and drop.pa > 0.0:
            L("eav_attn_bwd_dropout", qkv, P(ws.ao[i]), dao, P(ws.lse[i]), P(ws.delta), dqkv, B, H, N, hd, scale,
              *drop.site("attn", i), st)
        elif ws.fused:
            L("eav_attn_bwd", qkv, P(ws.ao[i]), dao, P(ws.lse[i]), P(ws.delta), dqkv, B, H, N, hd, scale, st)
        else:     # materialised scores, batched over (image, head)
            attention_backward_scores(m, gemm, i, qkv, dao, dqkv, scale)
        # fused q/k/v projection
        wgrad(dqkv, P(ws.y1[i]), gp(f"{Lk}.attention.q_proj.weight"), 3 * D, D, M, 3 * D, D)
        bias_grad(dqkv, M, 3 * D, 3 * D, gp(f"{Lk}.attention.q_proj.bias"))
        gemm(dqkv, w(f"{Lk}.attention.q_proj.weight"), dy, M, D, 3 * D, 3 * D, D, D, tB=1)
        L("eav_layernorm_bwd", dy, P(ws.hs[i]), w(f"{Lk}.layernorm_before.weight"), stp, stp + 4 * M, dh, 1,
          P(ws.part_ln), M, D, st)
        m._reduce_ln(ws.part_ln, ws.np_ln, gp(f"{Lk}.layernorm_before.weight"), gp(f"{Lk}.layernorm_before.bias"))


# ----------------------------------------------------------------------------- side streams
class SideStreams:
    """The streams beside the main one of a split-precision step and who waits for whom.  Weight-gradient GEMMs go to `side`:
    nothing downstream reads them before the optimiser, and their MFMA work fills the matrix pipe while the main stream is in
    its HBM- / VALU-bound stretches.  The final reductions of bias / LayerNorm gradients go to `aux`, a stream of their OWN: a
    24-block kernel queued in order between persistent GEMMs waits for a CU whose LDS is not taken by two GEMM workgroups, and
    held the weight gradients behind it back by ~130 us per launch at ViT B=128 (9.6 ms of side-stream time per step).
    wgrad_done: operand planes -> event of the weight gradient that still reads them; part_busy: partial-sum buffer ->
    event of its reduction; ring_pos: position in each ring of partial-sum buffers."""

    def __init__(self, m):
        self.m = m
        self.side = self.aux = None
        self.wgrad_done, self.part_busy, self.ring_pos = {}, {}, {}

    @staticmethod
    def beside(stream, name, *args):
        """Launch `name` on `stream` once the current stream has come this far; returns the event of its completion."""
        ready = torch.cuda.Event()
        ready.record()
        stream.wait_event(ready)
        _lib.call(name, *args, stream.cuda_stream)
        done = torch.cuda.Event()
        done.record(stream)
        return done

    def side_stream(self, dev):
        if self.side is None or self.side.device != dev:
            self.side = torch.cuda.Stream(device=dev)
        return self.side

    def part_buf(self, pool):
        """Next buffer of a small ring of partial-sum buffers: the main stream waits for the reduction that last read a
        buffer only when the ring comes round to it (a layer later)."""
        ring = getattr(self.m._ws, pool)
        i = self.ring_pos.get(pool, -1) + 1
        self.ring_pos[pool] = i = i % len(ring)
        ev = self.part_busy.pop(ring[i].data_ptr(), None)
        if ev is not None:
            self.m._main.wait_event(ev)
        return ring[i]

    def reduce(self, buf, off_bytes, nparts, stride, n, out):
        """Final fixed-order reduction of a partial-sum buffer into a gradient nothing downstream reads: off the main stream
        when the step runs on several."""
        m = self.m
        if not (m._two_streams() and m.kernel_events is None):
            m._call("eav_reduce_partials", _lib.ptr(buf) + off_bytes, nparts, stride, n, 1.0, out, m._st)
            return
        if self.aux is None or self.aux.device != buf.device:
            self.aux = torch.cuda.Stream(device=buf.device)
        self.part_busy[buf.data_ptr()] = self.beside(self.aux, "eav_reduce_partials", _lib.ptr(buf) + off_bytes, nparts,
                                                     stride, n, 1.0, out)

    def before_overwrite(self, buf):
        """Main stream: the weight gradient that still reads `buf` (launched a layer ago on the side stream) must be
        finished before the next conversion overwrites it."""
        ev = self.wgrad_done.pop(buf.data_ptr(), None) if buf is not None else None
        if ev is not None:
            self.m._main.wait_event(ev)

    def join(self):
        main = self.m._main
        if self.side is not None and self.wgrad_done:
            main.wait_stream(self.side)
            self.wgrad_done.clear()
        if self.aux is not None and self.part_busy:
            main.wait_stream(self.aux)
            self.part_busy.clear()


# ----------------------------------------------------------------------------- split operands (fp16 hi / lo planes)
class SplitLayers:
    """The schedule on the split-operand GEMM and attention kernels: only operand planes are kept per layer, the weights'
    planes live in m._wplanes, scales in slots (FWD_SLOTS / BWD_SLOTS)."""
    split, SPLITK_PLAN = True, "eav_gemm_sp_splitk_plan"
    _SCALE_PARAMS = ("layernorm_before.weight", "layernorm_before.bias", "layernorm_after.weight", "layernorm_after.bias",
                     "mlp.fc1.bias", "attention.q_proj.bias")

    def __init__(self, m):
        self.m = m
        self.streams = SideStreams(m)
        self.scales_all = False

    # ------------------------------------------------------------------ allocation, per-step preparation
    @staticmethod
    def fp32_copies(nsave):
        """One transient fp32 buffer: what the backward reads is kept as planes."""
        return 1

    def alloc(self, ws, dev, nsave):
        c = self.m._geo
        D, FF, Lr, M = c.hidden, c.ff, c.layers, ws.M
        MP = ws.B * c.npatch
        kp = lambda k: _lib.plain("eav_sp_kpad", k)  # noqa: E731
        # Row planes only: the weight-gradient products contract over the ROWS (tokens) of the same planes the forward /
        # data-gradient products read (transposing LDS reads in gemm_sp.hip), so no transposed copy of any activation or
        # gradient exists.  Rows are padded to a multiple of 32 with zeros (contracted like real tokens; the conversion
        # never writes them).
        h = lambda r, k: torch.zeros((r + 31) // 32 * 32, 2 * kp(k), dtype=torch.float16, device=dev)  # noqa: E731
        ws.colp = h(MP, c.kp)
        ws.y1p = [h(M, D) for _ in range(nsave)]
        ws.aop = [h(M, D) for _ in range(nsave)]
        ws.y2p = [h(M, D) for _ in range(nsave)]
        ws.actp = [h(M, FF) for _ in range(nsave)]
        ws.fslots, ws.fslot = self.slots(1 + FS * Lr, dev)
        if ws.fused:   # attention operands: row planes of qkv and per-head transposed planes (csrc/attention_sp.hip)
            ws.qkvrow = [torch.empty(M, 6 * D, dtype=torch.float16, device=dev) for _ in range(nsave)]
        if ws.full:
            # backward operands: one set, reused by every layer.  dh is converted twice per layer (fc2 and o_proj stage)
            # and its weight gradients run on the side stream, so the two uses must not share one buffer
            ws.dhp, ws.dhp2 = h(M, D), h(M, D)
            ws.dactp, ws.dqkvp = h(M, FF), h(M, 3 * D)
            ws.dembp = h(MP, D)
            ws.np_cs2 = _lib.plain("eav_sp_convert_colsum_nparts", M)
            ws.part_cs2 = torch.empty(ws.np_cs2, max(FF, 3 * D), dtype=torch.float32, device=dev)
            ws.part_cs2_pool = [ws.part_cs2] + [torch.empty_like(ws.part_cs2) for _ in range(3)]
            ws.np_attn = ws.B * ((c.ntok + 31) // 32)          # bias-gradient partials of the attention backward: one row per 32-token tile
            ws.part_attn_pool = [torch.zeros(ws.np_attn, 3 * D, dtype=torch.float32, device=dev) for _ in range(4)]
            ws.bslots, ws.bslot = self.slots(2 + BS * Lr, dev)
            if c.hidden_dropout > 0.0:        # measured scales of the two gated gradients of every layer
                ws.dslots, ws.dslot = self.slots(2 * Lr, dev)
            if ws.fused:
                ws.dorow = torch.empty(M, 2 * D, dtype=torch.float16, device=dev)

    @staticmethod
    def slots(n, dev):
        """n zeroed scale slots ([n, SLOT] floats) and the device address of each."""
        table = torch.zeros(n, SLOT, dtype=torch.float32, device=dev)
        return table, [table.data_ptr() + 4 * SLOT * k for k in range(n)]

    def begin_forward(self, ws, dev, full):
        self.refresh_weight_planes(dev, full)
        ws.fslots.zero_()
        if full and ws.dpath is not None and getattr(ws, "dslots", None) is None:      # drop path: as under hidden dropout
            ws.dslots, ws.dslot = self.slots(2 * self.m._geo.layers, dev)

    def begin_backward(self, ws):
        m, c = self.m, self.m._geo
        if ws.drop.ph > 0.0 or ws.dpath is not None:
            ws.dslots.zero_()
        ws.bslots.zero_()
        # dh of the top layer comes from the head (token-row scatter): one pass for its maximum; every other dh
        # gets its maximum from the LayerNorm backward that produces it
        m._call("eav_sp_absmax", _lib.ptr(ws.dh), ws.M, c.hidden, c.hidden, ws.bslot[1 + BS * (c.layers - 1) + B_DH2], m._st)

    def refresh_weight_planes(self, dev, need_T):
        """(Re)build the fp16 hi/lo planes of the GEMM weights (and of their transposes, for the data-gradient
        products) that changed: FusedAdam records the byte ranges it updated (`_eav_dirty`), any torch in-place write
        to the flat buffer (load_state_dict, .copy_) bumps its version and invalidates everything."""
        m = self.m
        flat, offs = m._flat[0], m._flat[2]
        keys = m._weight_keys()
        wp = m._wplanes
        if wp is None or wp.dev != dev or (need_T and not wp.T):
            wp = m._wplanes = WeightPlanes([(k, 4 * offs[pn][0], out, inn) for k, pn, out, inn in keys],
                                           m.cfg.layers, dev, need_T)
            wp.main = m._main
        # Invalidation key: flatten_parameters rebinds p.data to views of the flat buffer, and a rebound .data has its
        # OWN version counter - load_state_dict, p.copy_/add_ under no_grad and torch.optim optimisers bump the
        # parameters' versions, never the flat buffer's.  So the key is the sum of the GEMM weights' versions (host-side,
        # ~50 attribute reads) plus the flat buffer's own version (flat.copy_ / flat.zero_ style writes);
        # load_state_dict / _apply also drop the cache outright.  FusedAdam writes through raw pointers (no version
        # moves): it reports the byte ranges it updated instead (`_eav_dirty`, recorded only because this model asked
        # for it through `_eav_track_dirty`).
        flat._eav_track_dirty = True
        versions = (flat._version, sum(m._pmap[pn]._version for _, pn, _, _ in keys))
        dirty, flat._eav_dirty = getattr(flat, "_eav_dirty", []), []
        stale = wp.stale(flat.data_ptr(), versions, dirty, need_T)
        # (the refresh goes to the side stream - idle during the forward - when this step runs on two streams)
        side = self.streams.side_stream(dev) if (stale and m._two_streams() and m.kernel_events is None) else None
        wp.refresh(stale, flat.data_ptr(), versions, side)

    def terms(self, kind):
        """MFMA terms of the backward products of `kind` ("dgrad" | "wgrad"): 3 = fp32-grade, 1 = hi.hi only; wgrad also 2 =
        hi.hi + lo_grad.hi_act (the activation operand rounded to fp16, the gradient operand at full split precision -
        the producers' a-priori gradient planes stay on)."""
        m = self.m
        t = m.wgrad_terms if kind == "wgrad" else m.dgrad_terms
        return m.grad_terms if t is None else int(t)

    def bwd_three_terms(self):
        """Every backward product on three terms: the producers may then write gradient planes under loose a-priori
        bounds (a hi.hi-only product needs the tight measured scale of its operands)."""
        return self.terms("dgrad") != 1 and self.terms("wgrad") != 1

    # ------------------------------------------------------------------ plane conversion and products
    def to_planes(self, src, R, C, ld, slot, dst, amax_done=False):
        """fp32 [R, C] -> row planes (one set serves the products that contract over columns AND those over rows)."""
        m = self.m
        if not amax_done:
            m._call("eav_sp_absmax", src, R, C, ld, slot, m._st)
        m._call("eav_sp_convert", src, R, C, ld, slot, _lib.ptr(dst), None, m._st)

    def to_planes_bias(self, src, R, C, slot, dst, bias_grad):
        """Conversion pass that also produces the bias gradient (column sums of src) - src's max|x| is already in slot."""
        m, s = self.m, self.streams
        s.before_overwrite(dst)
        part = s.part_buf("part_cs2_pool")
        m._call("eav_sp_convert_colsum", src, R, C, C, slot, _lib.ptr(dst), None, _lib.ptr(part), m._st)
        s.reduce(part, 0, m._ws.np_cs2, C, C, bias_grad)

    def gemm_sp(self, A, slotA, B, slotB, C, M, N, K, ldc, batch=1, sA=0, sC=0, alpha=1.0, bias=None, gelu=0,
                pre=None, resid=None, ldr=0, acc=0, amax=None, blockmax=True):
        """C[M,N] = epilogue(alpha A[M,K] . B[N,K]^T) on planes."""
        # flags: backward products with grad_terms = 1 run on the hi.hi term alone (see Encoder.grad_terms); the backward's
        # data gradients share the GPU with the side stream's weight gradients (EAV_GEMM_SHARED_GPU: see csrc/gemm_sp.hip)
        m = self.m
        bwd = m._phase == "bwd"
        flags = (GEMM_ONE_TERM if (self.terms("dgrad") if bwd else m.fwd_terms) == 1 else 0) \
            | (GEMM_SHARED_GPU if bwd and m._two_streams() else 0) | (0 if blockmax else GEMM_NO_BLOCKMAX)
        m._call("eav_gemm_sp_ex", A, B, C, slotA, slotB, M, N, K, ldc, batch, sA, sC, float(alpha), bias, gelu, pre,
                resid, ldr, acc, amax, None, None, None, flags, m._st)

    def wgrad_sp(self, AT, slotA, BT, slotB, C, M, N, K):
        """C[M,N] = sum over the K tokens of A[t,m] B[t,n]: ROW planes of A [K,M] and B [K,N] (the contraction runs over the
        rows: eav_gemm_sp_splitk reads the fragments with transposing LDS loads); split-K.  On the side stream when the step
        has one (SideStreams): it waits for the event recorded after the conversion that produced A; the main stream waits
        for a weight gradient only before it overwrites that gradient's A planes (one layer later) and at the end of the
        backward."""
        m, s = self.m, self.streams
        name = {1: "eav_gemm_sp_splitk_x1", 2: "eav_gemm_sp_splitk_x2"}.get(self.terms("wgrad"), "eav_gemm_sp_splitk")
        args = (_lib.ptr(AT), _lib.ptr(BT), C, _lib.ptr(m._ws.splitk), slotA, slotB, M, N, K, 0)
        if not m._two_streams() or (m.kernel_events is not None and name in m.kernel_events):
            m._call(name, *args, m._st)
        else:
            s.wgrad_done[AT.data_ptr()] = s.beside(s.side_stream(AT.device), name, *args)

    def patch_embed(self, ws, h0, bias):
        m, c, P = self.m, self.m._geo, _lib.ptr
        D = c.hidden
        self.to_planes(P(ws.col), ws.B * c.npatch, c.kp, c.kp, ws.fslot[0], ws.colp)
        wpl, wsl = m._wplanes.get("patch")
        self.gemm_sp(P(ws.colp), ws.fslot[0], wpl, wsl, P(h0) + 4 * c.nextra * D, c.npatch, D, c.kp, D, batch=ws.B,
                     sA=c.npatch * 4 * _lib.plain("eav_sp_kpad", c.kp), sC=c.ntok * D, bias=bias)    # (plane row stride in bytes)

    def patch_wgrad(self, ws, gw, MP):
        # demb (the patch rows of dh) gets its own maximum pass: the slot layer 0's LayerNorm backward filled is
        # indexed by the rows of dh (cls / distillation rows included), and the per-row-block maxima must be the
        # converted tensor's own
        c = self.m._geo
        s_demb = ws.bslot[1 + BS * c.layers]
        self.to_planes(_lib.ptr(ws.demb), MP, c.hidden, c.hidden, s_demb, ws.dembp)
        self.wgrad_sp(ws.dembp, s_demb, ws.colp, ws.fslot[0], gw, c.hidden, c.kp, MP)

    # ------------------------------------------------------------------ a-priori scales
    def scale_offsets(self, i):
        """(offset of layer i's first parameter in the flat buffer, the offsets relative to it of the parameters
        eav_tf_forward_scales_qkv reads, in its argument order)."""
        offs, Lk = self.m._flat[2], f"{self.m.cfg.prefix}.layers.{i}"
        first = offs[f"{Lk}.attention.q_proj.weight"][0]
        return first, tuple(offs[f"{Lk}.{n}"][0] - first for n in self._SCALE_PARAMS)

    def forward_scales(self):
        """A-priori operand scales (rigorous bounds: eav_tf_forward_scales_qkv) of y1, qkv, y2, act of EVERY layer in one
        launch - the flat parameter buffer lays the layers out identically.  Falls back to one launch per layer (inside
        layer_forward) if it does not."""
        m = self.m
        c, ws, wp = m.cfg, m._ws, m._wplanes
        self.scales_all = False
        if not (m.fused_planes and c.hidden % 8 == 0 and c.ff % 8 == 0):
            return
        first, rel = zip(*(self.scale_offsets(i) for i in range(c.layers)))
        stride = first[1] - first[0] if c.layers > 1 else 0
        if any(r != rel[0] for r in rel) or any(first[i] - first[0] != i * stride for i in range(c.layers)):
            return
        if wp.norm_ready is not None:              # the row norms come from the side-stream weight refresh
            m._main.wait_event(wp.norm_ready)
        m._call("eav_tf_forward_scales_qkv", _lib.ptr(m._flat[0]) + 4 * first[0], stride, c.layers, *rel[0],
                c.hidden, c.ff, wp.wnorm_fc1.data_ptr(), wp.wnorm_qkv.data_ptr(), ws.fslot[1], FS * SLOT, F_Y1, F_Y2, F_ACT,
                F_QKV if (m.fused_qkv and ws.fused) else -1, m._st)
        self.scales_all = True

    # ------------------------------------------------------------------ one layer
    def layer_forward(self, i, j, hin, hout, Lk, stp, scale):
        """One encoder layer with every projection on the split-operand GEMM; the attention core stays on the fp32
        kernels.  LayerNorm / attention / GELU outputs are converted to planes once (plus the transposed planes when
        a backward will follow); only the planes are kept per layer."""
        m = self.m
        if i == 0:
            self.forward_scales()
        c, ws, wp = m._geo, m._ws, m._wplanes
        P, L, st, w, gemm_sp = _lib.ptr, m._call, m._st, m._w, self.gemm_sp
        D, FF, N, H, M = c.hidden, c.ff, c.ntok, c.heads, ws.M
        hd = D // H
        f, o = ws.fslot, 1 + FS * i
        s_y1, s_qkv, s_ao, s_y2, s_act = f[o + F_Y1], f[o + F_QKV], f[o + F_AO], f[o + F_Y2], f[o + F_ACT]
        y, ao, act = ws.y1[0], ws.ao[j], ws.act[0]
        one_term = GEMM_ONE_TERM if m.fwd_terms == 1 else 0
        # Producers write the operand planes themselves where a rigorous bound of the tensor exists BEFORE it is computed
        # (LayerNorm outputs, the MLP's GELU output: eav_tf_forward_scales) - no fp32 copy, no measured maximum, no
        # conversion pass for y1, y2, act.  The attention output keeps the measured scale (its kernel emits max|O|).
        fusedp = m.fused_planes and D % 8 == 0 and FF % 8 == 0
        if fusedp:
            wp.get(f"fc1{i}")        # (waits for the side-stream refresh of this layer's fc1 planes / row norms)
            if not self.scales_all:
                first, rel = self.scale_offsets(i)
                L("eav_tf_forward_scales_qkv", P(m._flat[0]) + 4 * first, 0, 1, *rel, D, FF,
                  wp.wnorm_fc1.data_ptr() + 4 * i, wp.wnorm_qkv.data_ptr() + 4 * i, s_y1, 0, F_Y1, F_Y2, F_ACT,
                  F_QKV if (m.fused_qkv and ws.fused) else -1, st)
            L("eav_layernorm_fwd_planes", P(hin), w(f"{Lk}.layernorm_before.weight"), w(f"{Lk}.layernorm_before.bias"),
              None, P(ws.y1p[j]), s_y1, stp, stp + 4 * M, M, D, c.eps, st)
        else:
            L("eav_layernorm_fwd_amax", P(hin), w(f"{Lk}.layernorm_before.weight"), w(f"{Lk}.layernorm_before.bias"),
              P(y), stp, stp + 4 * M, M, D, c.eps, s_y1, st)
            self.to_planes(P(y), M, D, D, s_y1, ws.y1p[j], amax_done=True)
        qkv = P(ws.qkv[0 if ws.fused else j])
        wpl, wsl = wp.get(f"qkv{i}")
        qkvp = fusedp and m.fused_qkv and ws.fused
        if qkvp:
            # the projection writes the row planes of Q | K | V itself (lo without the 2^11 lift: the attention kernels' format,
            # scale = the bound eav_tf_forward_scales_qkv put into s_qkv); the per-head transposes (V^T for the forward; Q^T,
            # K^T for the backward) are a pure fp16 transposition of those planes
            L("eav_gemm_sp_ex", P(ws.y1p[j]), wpl, None, s_y1, wsl, M, 3 * D, D, 3 * D, 1, 0, 0, 1.0,
              w(f"{Lk}.attention.q_proj.bias"), 0, None, None, 0, 0, s_qkv, P(ws.qkvrow[j]), s_qkv, None,
              GEMM_PLANES_NOLIFT | GEMM_NO_BLOCKMAX | one_term, st)   # (+ the MEASURED max|qkv| into the slot's shards: the
            #                                                            backward's bound of |dqkv| uses it, eav_attn_dqkv_bound)
        else:
            gemm_sp(P(ws.y1p[j]), s_y1, wpl, wsl, qkv, M, 3 * D, D, 3 * D, bias=w(f"{Lk}.attention.q_proj.bias"),
                    amax=s_qkv if ws.fused else None)
        if ws.fused:
            if not qkvp:
                # row planes of Q | K | V and the per-head transposes (V^T for the forward; Q^T, K^T for the backward)
                L("eav_attn_sp_prep", qkv, s_qkv, P(ws.qkvrow[j]), None, ws.B, N, 3 * D, D, 0, st)
            if ws.drop.pa > 0.0:
                # attention dropout: the DROP instantiation, fp32 output and its measured maximum (the o-proj planes come
                # from the conversion pass below) - the plane-writing form's scale |O| <= max|V| assumes rows of P sum to 1
                ws.delta_from_planes = False
                L("eav_attn_fwd_sp_dropout", P(ws.qkvrow[j]), s_qkv, P(ao), P(ws.lse[j]), s_ao, ws.B, H, N, hd, scale,
                  *ws.drop.site("attn", i), st)
            elif fusedp and m.fused_ao:
                # the attention output leaves as the planes of the o-proj products (scale: qkv's own, |O| <= max|V|); its
                # fp32 copy is written only when a backward will read it
                # (... and only by the unfused gradient flow: the fused one forms delta = dO . O from these planes)
                # (recorded on the workspace: the backward forms delta from ws.aop ONLY if THIS kernel wrote them - its
                # planes carry one tensor-wide scale; eav_sp_convert's planes below have per-row-block boosts)
                ws.delta_from_planes = m.fused_dqkv and self.bwd_three_terms()
                need_ao = ws.full and not ws.delta_from_planes
                L("eav_attn_fwd_sp_planes", P(ws.qkvrow[j]), None, s_qkv, P(ao) if need_ao else None,
                  P(ws.lse[j]), None, P(ws.aop[j]), s_ao, ws.B, H, N, hd, scale, st)
            else:
                ws.delta_from_planes = False
                L("eav_attn_fwd_sp", P(ws.qkvrow[j]), None, s_qkv, P(ao), P(ws.lse[j]), s_ao, ws.B, H, N, hd,
                  scale, st)
        else:
            ldn = ws.ldn
            Pm = P(ws.P[j])
            gemm_f32(m, qkv, qkv + 4 * D, Pm, N, N, hd, 3 * D, 3 * D, ldn, batch=ws.B * H, heads=H,
                     sA=(N * 3 * D, hd), sB=(N * 3 * D, hd), sC=(H * N * ldn, N * ldn), alpha=scale)
            Pv = softmax_forward(m, i, Pm, ws.B * H * N, N, ldn)
            gemm_f32(m, Pv, qkv + 8 * D, P(ao), N, hd, N, ldn, 3 * D, D, tB=1, batch=ws.B * H, heads=H,
                     sA=(H * N * ldn, N * ldn), sB=(N * 3 * D, hd), sC=(N * D, hd))
        m._outputs.attention(i, j, scale, rowp=P(ws.qkvrow[j]) if ws.fused else None, slot=s_qkv)
        if not (ws.fused and fusedp and m.fused_ao) or (ws.fused and ws.drop.pa > 0.0):
            self.to_planes(P(ao), M, D, D, s_ao, ws.aop[j], amax_done=ws.fused)
        wpl, wsl = wp.get(f"o{i}")
        # (hidden dropout: the product leaves without the residual, one element-wise pass forms resid + Dropout(product) - the
        # split GEMM's epilogue stays as it is)
        # (drop path, a layer with p_i > 0: the same road with the per-sample scales of the forward's table)
        drop = ws.drop
        hd_on = drop.ph > 0.0
        dp_on = path_on(ws, i)
        bare = hd_on or dp_on
        gemm_sp(P(ws.aop[j]), s_ao, wpl, wsl, P(ws.hmid[j]), M, D, D, D, bias=w(f"{Lk}.attention.o_proj.bias"),
                resid=None if bare else P(hin), ldr=0 if bare else D)
        if hd_on:
            m._drop_add(P(ws.hmid[j]), P(hin), P(ws.hmid[j]), M * D, "attn_out", i)
        elif dp_on:
            m._path_add(P(ws.hmid[j]), P(hin), P(ws.hmid[j]), i, 0)
        if fusedp:
            L("eav_layernorm_fwd_planes", P(ws.hmid[j]), w(f"{Lk}.layernorm_after.weight"),
              w(f"{Lk}.layernorm_after.bias"), None, P(ws.y2p[j]), s_y2, stp + 8 * M, stp + 12 * M, M, D, c.eps, st)
            wpl, wsl = wp.get(f"fc1{i}")
            # fc1: bias + erf-GELU in the epilogue; the pre-activation is kept (fp32) for the backward only, the
            # activation leaves as planes - it never exists in fp32
            L("eav_gemm_sp_ex", P(ws.y2p[j]), wpl, None, s_y2, wsl, M, FF, D, FF, 1, 0, 0, 1.0,
              w(f"{Lk}.mlp.fc1.bias"), 1, P(ws.pre[j]) if ws.full else None, None, 0, 0, None, P(ws.actp[j]),
              s_act, None, one_term, st)
        else:
            L("eav_layernorm_fwd_amax", P(ws.hmid[j]), w(f"{Lk}.layernorm_after.weight"),
              w(f"{Lk}.layernorm_after.bias"), P(y), stp + 8 * M, stp + 12 * M, M, D, c.eps, s_y2, st)
            self.to_planes(P(y), M, D, D, s_y2, ws.y2p[j], amax_done=True)
            wpl, wsl = wp.get(f"fc1{i}")
            # fc1 stores the PRE-activation only (kept per layer for the backward; a scratch buffer in the frozen phase)
            # and max|GELU|; the conversion applies the GELU while it splits - the activation never exists in fp32
            pre = P(ws.pre[j]) if ws.full else P(act)
            gemm_sp(P(ws.y2p[j]), s_y2, wpl, wsl, pre, M, FF, D, FF, bias=w(f"{Lk}.mlp.fc1.bias"), gelu=3, amax=s_act)
            L("eav_sp_convert_gelu", pre, M, FF, FF, s_act, P(ws.actp[j]), None, st)
        wpl, wsl = wp.get(f"fc2{i}")
        gemm_sp(P(ws.actp[j]), s_act, wpl, wsl, P(hout), M, D, FF, D, bias=w(f"{Lk}.mlp.fc2.bias"),
                resid=None if bare else P(ws.hmid[j]), ldr=0 if bare else D)
        if hd_on:
            m._drop_add(P(hout), P(ws.hmid[j]), P(hout), M * D, "mlp_out", i)
        elif dp_on:
            m._path_add(P(hout), P(ws.hmid[j]), P(hout), i, 1)

    def layer_backward(self, i, Lk, stp, scale):
        """Backward of one layer: dh (gradient w.r.t. the layer output, fp32) in ws.dh on entry, gradient w.r.t. the
        layer input on exit.  Every weight gradient is a split-K GEMM over the transposed planes; data gradients use
        the planes of the transposed weights."""
        m, s = self.m, self.streams
        c, ws, wp = m._geo, m._ws, m._wplanes
        P, L, st, w, gp = _lib.ptr, m._call, m._st, m._w, m._gp
        gemm_sp, wgrad_sp, to_planes_bias = self.gemm_sp, self.wgrad_sp, self.to_planes_bias
        D, FF, N, H, M = c.hidden, c.ff, c.ntok, c.heads, ws.M
        hd = D // H
        dh, dy, dao, dact, dqkv = P(ws.dh), P(ws.dy), P(ws.dao), P(ws.dact), P(ws.dqkv)
        f, o = ws.fslot, 1 + FS * i
        s_y1, s_qkv, s_ao, s_y2, s_act = f[o + F_Y1], f[o + F_QKV], f[o + F_AO], f[o + F_Y2], f[o + F_ACT]
        b, o = ws.bslot, 1 + BS * i
        b_dh2, b_dact, b_dh1, b_dao = b[o + B_DH2], b[o + B_DACT], b[o + B_DH1], b[o + B_DAO]
        b_ds, b_dqkv, b_dy2, b_dy1 = b[o + B_DS], b[o + B_DQKV], b[o + B_DY2], b[o + B_DY1]
        b_below = b[o - BS + B_DH2] if i > 0 else b[0]     # max|dh| of the layer below (the embedding's)
        three = self.bwd_three_terms()
        fdh = m.fused_dh and three      # (hi.hi-only gradient products need the tight measured scales)
        # Hidden dropout: the gradient entering the fc2 / o_proj products is dh o M / (1 - p) (the residual branch keeps dh).
        # The gate is a pass of its own into ws.dhd; the gated tensor gets its own MEASURED scale slot (s_dh2 / s_dh1) - the
        # producers' slots hold max|dh| of the ungated tensor, up to 1 / (1 - p) too small.  fused_dh is off on such a step:
        # the LayerNorm backward's planes (and their a-priori bound) are those of the ungated dh.
        # Drop path gates per sample (dh[b] s[b], s up to 1 / (1 - p_i)) and per layer: the layers with p_i > 0 take this road,
        # the others keep the fused one - where the LayerNorm backward that would write a layer's planes belongs to a gated
        # neighbour, that hand-over alone falls back to the conversion pass (fdh_top / fdh_bot).
        drop = ws.drop
        hd_on = drop.ph > 0.0
        dp_on = path_on(ws, i)
        gated = lambda k: hd_on or path_on(ws, k)  # noqa: E731
        fdh = fdh and not gated(i)
        fdh_top = fdh and i < c.layers - 1 and not gated(i + 1)       # the layer above wrote the planes of this layer's dh
        fdh_bot = fdh and i > 0 and not gated(i - 1)                  # this layer writes those of the layer below
        s_dh2, s_dh1, g_dh = b_dh2, b_dh1, dh
        if hd_on or dp_on:
            s_dh2, s_dh1, g_dh = ws.dslot[2 * i], ws.dslot[2 * i + 1], P(ws.dhd)
            if hd_on:
                m._drop_add(dh, None, g_dh, M * D, "mlp_out", i)
            else:
                m._path_add(dh, None, g_dh, i, 1)
            L("eav_sp_absmax", g_dh, M, D, D, s_dh2, st)
        # fc2: h_out = h_mid + act.W2^T + b2.  max|dh| is already in b_dh2 (left there by the producer of dh); every
        # conversion pass also yields the bias gradient of its tensor.  (fused_dh: the layer above's LayerNorm backward
        # already wrote these planes and the bias-gradient partials - only the top layer's dh comes from the head)
        if not fdh_top:
            to_planes_bias(g_dh, M, D, s_dh2, ws.dhp, gp(f"{Lk}.mlp.fc2.bias"))
        wgrad_sp(ws.dhp, s_dh2, ws.actp[i], s_act, gp(f"{Lk}.mlp.fc2.weight"), D, FF, M)
        wpl, wsl = wp.get(f"fc2{i}", transposed=True)
        if m.fused_dact and FF % 8 == 0:
            # data gradient through fc2 and the GELU in one pass, result straight into the planes of dact: its scale comes
            # from |dact| = |(dh W2) gelu'(pre)| <= 1.13 sqrt(D) max|dh| max_j ||W2[:, j]||_2 (max|dh| is in b_dh2, the column
            # norms are refreshed with the weight planes); the epilogue also leaves fc1's bias-gradient partials
            L("eav_sp_bound_scale", b_dact, s_dh2, wp.wcolnorm_fc2.data_ptr() + 4 * i, 1.13 * float(np.sqrt(D)), st)
            s.before_overwrite(ws.dactp)
            part = s.part_buf("part_cs2_pool")
            flags = (GEMM_ONE_TERM if self.terms("dgrad") == 1 else 0) | (GEMM_SHARED_GPU if m._two_streams() else 0)
            L("eav_gemm_sp_ex", P(ws.dhp), wpl, None, s_dh2, wsl, M, FF, D, FF, 1, 0, 0, 1.0, None, 2, P(ws.pre[i]), None, 0,
              0, None, P(ws.dactp), b_dact, P(part), flags, st)
            s.reduce(part, 0, ws.np_cs2, FF, FF, gp(f"{Lk}.mlp.fc1.bias"))
        else:
            # ... the epilogue multiplies by gelu'(pre) and emits max|dact|; one conversion pass (planes + bias gradient)
            gemm_sp(P(ws.dhp), s_dh2, wpl, wsl, dact, M, FF, D, FF, gelu=2, pre=P(ws.pre[i]), amax=b_dact)
            to_planes_bias(dact, M, FF, b_dact, ws.dactp, gp(f"{Lk}.mlp.fc1.bias"))
        # fc1
        wgrad_sp(ws.dactp, b_dact, ws.y2p[i], s_y2, gp(f"{Lk}.mlp.fc1.weight"), FF, D, M)
        wpl, wsl = wp.get(f"fc1{i}", transposed=True)
        if fdh:
            gemm_sp(P(ws.dactp), b_dact, wpl, wsl, dy, M, D, FF, D, amax=b_dy2, blockmax=False)
            self.ln_bwd_planes(dy, P(ws.hmid[i]), w(f"{Lk}.layernorm_after.weight"), stp + 8 * M, stp + 12 * M, dh, b_dh1,
                               b_dh2, b_dy2, ws.dhp2, gp(f"{Lk}.layernorm_after.weight"), gp(f"{Lk}.layernorm_after.bias"),
                               gp(f"{Lk}.attention.o_proj.bias"), s_y2)
        else:
            gemm_sp(P(ws.dactp), b_dact, wpl, wsl, dy, M, D, FF, D)
            part = s.part_buf("part_ln_pool")
            L("eav_layernorm_bwd_amax", dy, P(ws.hmid[i]), w(f"{Lk}.layernorm_after.weight"), stp + 8 * M, stp + 12 * M, dh,
              1, P(part), M, D, b_dh1, st)
            m._reduce_ln(part, ws.np_ln, gp(f"{Lk}.layernorm_after.weight"), gp(f"{Lk}.layernorm_after.bias"), s.reduce)
            # o_proj
            if hd_on or dp_on:
                if hd_on:
                    m._drop_add(dh, None, g_dh, M * D, "attn_out", i)
                else:
                    m._path_add(dh, None, g_dh, i, 0)
                L("eav_sp_absmax", g_dh, M, D, D, s_dh1, st)
            to_planes_bias(g_dh, M, D, s_dh1, ws.dhp2, gp(f"{Lk}.attention.o_proj.bias"))
        wgrad_sp(ws.dhp2, s_dh1, ws.aop[i], s_ao, gp(f"{Lk}.attention.o_proj.weight"), D, D, M)
        wpl, wsl = wp.get(f"o{i}", transposed=True)
        # (dao goes to the attention operand preparation: one scale per tensor, no row-block maxima needed)
        gemm_sp(P(ws.dhp2), s_dh1, wpl, wsl, dao, M, D, D, D, amax=b_dao if ws.fused else None, blockmax=False)
        # attention core
        if ws.fused:
            L("eav_attn_sp_prep", dao, b_dao, P(ws.dorow), None, ws.B, N, D, D, 0, st)
            # dqkv as planes straight from the attention backward, delta = dO . O from the planes of O - only when the
            # forward of THIS step wrote those planes with eav_attn_fwd_sp_planes (EAV_FUSED_AO=0 / EAV_FUSED_PLANES=0 runs
            # convert a fp32 O with per-row-block boosts the planes-delta kernel does not read); hi.hi-only gradient
            # products need the tight measured scale
            fused_bwd = bool(getattr(ws, "delta_from_planes", False)) and m.fused_dqkv and three
            if fused_bwd:
                s.before_overwrite(ws.dqkvp)
                part = s.part_buf("part_attn_pool")
                # (delta = dO . O from the planes of dO and of the attention output: no fp32 attention output in the step)
                L("eav_attn_bwd_sp_planes", P(ws.qkvrow[i]), None, P(ws.dorow), None, s_qkv, b_dao, b_ds,
                  None, None, P(ws.lse[i]), P(ws.delta), None, None, P(ws.dqkvp), b_dqkv, P(part), P(ws.aop[i]), s_ao,
                  ws.B, H, N, hd, scale, st)
                s.reduce(part, 0, ws.np_attn, 3 * D, 3 * D, gp(f"{Lk}.attention.q_proj.bias"))
            elif drop.pa > 0.0:
                # (fused_dqkv is off on such a step - delta_from_planes is false: fp32 dqkv, the conversion pass measures it)
                L("eav_attn_bwd_sp_dropout", P(ws.qkvrow[i]), P(ws.dorow), s_qkv, b_dao, b_ds, P(ws.ao[i]), dao,
                  P(ws.lse[i]), P(ws.delta), dqkv, b_dqkv, ws.B, H, N, hd, scale, *drop.site("attn", i), st)
            else:
                L("eav_attn_bwd_sp", P(ws.qkvrow[i]), None, P(ws.dorow), None, s_qkv, b_dao, b_ds,
                  P(ws.ao[i]), dao, P(ws.lse[i]), P(ws.delta), dqkv, b_dqkv, ws.B, H, N, hd, scale, st)
        else:
            attention_backward_scores(m, partial(gemm_f32, m), i, P(ws.qkv[i]), dao, dqkv, scale)
        # fused q/k/v projection
        if not ws.fused:
            L("eav_sp_absmax", dqkv, M, 3 * D, 3 * D, b_dqkv, st)
        if not (ws.fused and fused_bwd):
            to_planes_bias(dqkv, M, 3 * D, b_dqkv, ws.dqkvp, gp(f"{Lk}.attention.q_proj.bias"))
        wgrad_sp(ws.dqkvp, b_dqkv, ws.y1p[i], s_y1, gp(f"{Lk}.attention.q_proj.weight"), 3 * D, D, M)
        wpl, wsl = wp.get(f"qkv{i}", transposed=True)
        # the gradient w.r.t. this layer's input is the next (lower) layer's dh: leave its max in that layer's slot
        if fdh_bot:
            gemm_sp(P(ws.dqkvp), b_dqkv, wpl, wsl, dy, M, D, 3 * D, D, amax=b_dy1, blockmax=False)
            below = Lk.rsplit(".", 1)[0] + f".{i - 1}"
            self.ln_bwd_planes(dy, P(ws.hs[i]), w(f"{Lk}.layernorm_before.weight"), stp, stp + 4 * M, dh,
                               b_below, b_dh1, b_dy1, ws.dhp, gp(f"{Lk}.layernorm_before.weight"),
                               gp(f"{Lk}.layernorm_before.bias"), gp(f"{below}.mlp.fc2.bias"), s_y1)
        else:
            gemm_sp(P(ws.dqkvp), b_dqkv, wpl, wsl, dy, M, D, 3 * D, D)
            part = s.part_buf("part_ln_pool")
            L("eav_layernorm_bwd_amax", dy, P(ws.hs[i]), w(f"{Lk}.layernorm_before.weight"), stp, stp + 4 * M, dh, 1,
              P(part), M, D, b_below, st)
            m._reduce_ln(part, ws.np_ln, gp(f"{Lk}.layernorm_before.weight"), gp(f"{Lk}.layernorm_before.bias"), s.reduce)

    def ln_bwd_planes(self, dy, x, gamma, mean, rstd, dh, slot_out, slot_old, slot_dy, planes, g_gamma, g_beta, g_bias,
                      slot_fwd):
        """LayerNorm backward, accumulated into dh, whose result ALSO leaves as the operand planes of the next gradient
        products (scale: the bound of eav_layernorm_bwd_bound - measured max|dh| before, max|dy|, max|gamma|, the forward's max
        rstd - formed inside the launch), with the bias-gradient partials of the linear layer that consumes dh: no conversion pass."""
        m, s = self.m, self.streams
        ws, D = m._ws, m.cfg.hidden
        s.before_overwrite(planes)
        part = s.part_buf("part_ln3_pool")
        m._call("eav_layernorm_bwd_planes", dy, x, gamma, mean, rstd, dh, 1, _lib.ptr(part), ws.M, D, slot_out,
                _lib.ptr(planes), slot_old, slot_dy, slot_fwd, m._st)
        if g_beta == g_gamma + 4 * D:
            s.reduce(part, 0, ws.np_ln, 3 * D, 2 * D, g_gamma)
        else:
            s.reduce(part, 0, ws.np_ln, 3 * D, D, g_gamma)
            s.reduce(part, 4 * D, ws.np_ln, 3 * D, D, g_beta)
        s.reduce(part, 8 * D, ws.np_ln, 3 * D, D, g_bias)
