"""The video CNN baseline of CNN_torch/CNN_Vision.py on MI355X, over libeav_hip.so (csrc/video_cnn.hip).

    IMAGE_TRANSFORM: Resize((224,224)) -> ToTensor -> Normalize(0.5, 0.5)             (:17-24)
        = preprocess.frames_to_pixel_values (Pillow-exact resize, float64 rescale, (x - 0.5) / 0.5)
    VideoModel(num_labels=5, ratio=1, backbone_weights=None)                          (:26-66)
        feature_extractor = the children of torchvision's resnet50() up to layer4      (:33-34)
        channel_attention, forward                                                     (:50-66)
    ImageClassifierTrainer(data, num_labels=5, lr=5e-5, batch_size=128)               (:69-107)
        accuracy(outputs, labels), train(epochs=3, lr=None, freeze=True), clear_loaders()   (:109-168)

The backbone is a restatement of torchvision's ResNet-50 v1.5 (stride on the 3x3 conv) with its module names and its
construction / initialisation order, so ``state_dict()`` keys match the reference's (``feature_extractor.4.0.conv1.weight``
...) and ``torch.manual_seed(s); VideoModel()`` draws the same numbers.  All training and inference arithmetic is in
hand-written gfx950 kernels: every conv, BatchNorm, ReLU, MaxPool and the attention head in csrc/video_cnn.hip, the 1x1
stride-1 convs and the Linear layers on eav_gemm_f32, the loss on eav_ce_fwd_bwd, AdamW on eav_adam_step.  There is no
CPU path.  Reference quirks and how they are treated: INTEGRATION.md.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .criteria import CrossEntropyLoss
from .optim import FusedAdam
from .runtime import (BN_M1, BN_M2, BN_SCALE, BN_SHIFT, DeviceLoader, KernelFn, KernelModule, bn_field,
                      eager_step)

NCMAX = 16                  # classes the head kernels take (eav_dense_softmax_*)
FEAT = 2048


# ---------------------------------------------------------------------------------------------- torchvision restatement
class Bottleneck(nn.Module):
    """torchvision.models.resnet.Bottleneck (expansion 4, groups 1, base width 64): the same attribute names and
    construction order."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        width = planes
        self.conv1 = nn.Conv2d(inplanes, width, kernel_size=1, stride=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, groups=1, bias=False, dilation=1)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * self.expansion, kernel_size=1, stride=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _resnet50_children():
    """The children of torchvision's resnet50() before avgpool / fc, built (and initialised) in torchvision's order: every
    conv draws its default kaiming_uniform_ at construction (a downsample conv before its block), the dropped fc its
    default init, then kaiming_normal_(fan_out, relu) over the convs in modules() order and BN weight 1 / bias 0."""
    inplanes = 64
    conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
    bn1 = nn.BatchNorm2d(64)
    relu = nn.ReLU(inplace=True)
    maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    layers = []
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        downsample = None
        if stride != 1 or inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * 4))
        seq = [Bottleneck(inplanes, planes, stride, downsample)]
        inplanes = planes * 4
        for _ in range(1, blocks):
            seq.append(Bottleneck(inplanes, planes))
        layers.append(nn.Sequential(*seq))
    fc = nn.Linear(512 * Bottleneck.expansion, 1000)
    children = [conv1, bn1, relu, maxpool, *layers]
    holder = nn.Sequential(*children, nn.AdaptiveAvgPool2d((1, 1)), fc)
    for m in holder.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    return children


def _torchvision_key(k):
    """feature_extractor.<i>.rest -> torchvision's resnet50 state_dict key."""
    names = {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3", "7": "layer4"}
    head, _, rest = k[len("feature_extractor."):].partition(".")
    return names[head] + "." + rest


# ---------------------------------------------------------------------------------------------- execution plan
class _Unit:
    """One conv + its BatchNorm: geometry for an input map H x W."""

    def __init__(self, conv, bn, H, W):
        self.conv, self.bn = conv, bn
        self.Co, self.Ci, kh, kw = conv.weight.shape
        self.k, self.s, self.p = kh, conv.stride[0], conv.padding[0]
        self.H, self.W = H, W
        self.OH, self.OW = (H + 2 * self.p - kh) // self.s + 1, (W + 2 * self.p - kw) // self.s + 1
        self.gemm = self.k == 1 and self.s == 1


def _plan(model, H, W):
    fe = model.feature_extractor
    stem = _Unit(fe[0], fe[1], H, W)
    PH, PW = (stem.OH + 2 - 3) // 2 + 1, (stem.OW + 2 - 3) // 2 + 1
    blocks = []
    h, w = PH, PW
    for li in range(4, 8):
        for blk in fe[li]:
            u1 = _Unit(blk.conv1, blk.bn1, h, w)
            u2 = _Unit(blk.conv2, blk.bn2, h, w)
            u3 = _Unit(blk.conv3, blk.bn3, u2.OH, u2.OW)
            ud = _Unit(blk.downsample[0], blk.downsample[1], h, w) if blk.downsample is not None else None
            blocks.append((u1, u2, u3, ud))
            h, w = u2.OH, u2.OW
    return stem, (PH, PW), blocks, (h, w)


class _Workspace:
    """Device buffers for one (B, H, W) problem size (fp32 unless noted)."""

    def __init__(self, model, B, H, W, dev):
        f = lambda n: torch.empty(max(int(n), 4), dtype=torch.float32, device=dev)  # noqa: E731
        self.stem, (PH, PW), self.blocks, (FH, FW) = _plan(model, H, W)
        self.B, self.PH, self.PW, self.HW = B, PH, PW, FH * FW
        units = [self.stem] + [u for blk in self.blocks for u in blk if u is not None]
        self.c, self.a, self.bn = {}, {}, {}
        for u in units:
            M = B * u.OH * u.OW
            self.c[id(u)] = f(M * u.Co)
            self.bn[id(u)] = f(6 * u.Co)
            u.M = M
        for u1, u2, u3, ud in self.blocks:
            self.a[id(u1)], self.a[id(u2)], self.a[id(u3)] = f(u1.M * u1.Co), f(u2.M * u2.Co), f(u3.M * u3.Co)
        self.a[id(self.stem)] = f(self.stem.M * 64)
        self.pool = f(B * PH * PW * 64)
        self.pidx = torch.empty(B * PH * PW * 64, dtype=torch.uint8, device=dev)
        # gradient scratch: the largest conv output or conv input map (a strided conv's data gradient is input-sized)
        big = max(max(u.M * u.Co, B * u.H * u.W * u.Ci) for u in units)
        self.D = [f(big), f(big)]
        self.Sg3, self.Sg, self.Sdc, self.Sda = f(big), f(big), f(big), f(big)
        self.stat = f(max(_lib.plain("eav_video_bn_nparts", u.M) * 2 * u.Co for u in units))
        wparts = []
        for u in units:
            if u.gemm:
                wparts.append(_lib.plain("eav_gemm_f32_splitk_plan", u.Co, u.Ci, u.M) * u.Co * u.Ci)
            else:
                wparts.append(_lib.plain("eav_video_wgrad_nparts", u.Co, u.Ci, u.k * u.k, u.M) * u.Co * u.Ci * u.k * u.k)
        B2 = 2 * B
        wparts += [_lib.plain("eav_gemm_f32_splitk_plan", FEAT, FEAT, B2) * FEAT * FEAT,
                   _lib.plain("eav_gemm_f32_splitk_plan", 1024, FEAT, B) * 1024 * FEAT,
                   _lib.plain("eav_colsum_nparts", B2) * FEAT]
        self.wpart = f(max(wparts))
        self.wrel = f(max(u.Co * u.Ci * u.k * u.k for u in units))      # re-laid weight (one conv at a time)
        self.P, self.H1, self.A = f(B2 * FEAT), f(B2 * FEAT), f(B2 * FEAT)
        self.hidx = torch.empty(B * FEAT, dtype=torch.uint8, device=dev)
        self.attn, self.z, self.h = f(B * FEAT), f(B * FEAT), f(B * 1024)
        self.logits = torch.empty(B, model.num_labels, dtype=torch.float32, device=dev)
        self.dh, self.dz = f(B * 1024), f(B * FEAT)
        self.dA, self.dH1, self.dP = f(B2 * FEAT), f(B2 * FEAT), f(B2 * FEAT)


class VideoModel(KernelModule):
    def __init__(self, num_labels: int = 5, ratio: int = 1, backbone_weights=None):
        super().__init__()
        if ratio != 1:
            # :40 builds attn_fc1 with 2048 // ratio inputs but :53 feeds it the 2048 pooled channels
            raise ValueError(f"VideoModel: ratio = {ratio} - the reference's attn_fc1 takes 2048 // ratio inputs but is "
                             "fed 2048 pooled channels, so only ratio = 1 runs")
        if not 1 <= num_labels <= NCMAX:
            raise ValueError(f"VideoModel: num_labels = {num_labels}; the gfx950 head kernels cover 1..{NCMAX}")
        self.num_labels = num_labels
        self.ratio = ratio

        self.feature_extractor = nn.Sequential(*_resnet50_children())
        if backbone_weights is None:
            print("VideoModel: backbone is not pretrained (seeded torchvision init; pass backbone_weights= for "
                  "ImageNet weights)")
        else:
            self.load_backbone(backbone_weights)

        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)

        self.attn_fc1 = nn.Linear(2048 // ratio, 2048)
        self.attn_fc2 = nn.Linear(2048, 2048)

        self.global_pool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(
            nn.Flatten(),
            nn.Linear(2048, 1024),
            nn.ReLU(),
            nn.Linear(1024, num_labels),
        )
        self._nbt = None

    def load_backbone(self, weights):
        """A torchvision-format ResNet-50 state_dict (``conv1.weight``, ``bn1.*``, ``layer1.0...``; ``fc.*`` ignored) or a
        path to one saved with torch.save."""
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        if not isinstance(weights, dict):
            raise TypeError("backbone_weights: a torchvision ResNet-50 state_dict or a path to one")
        own = self.feature_extractor.state_dict()
        mapped = {}
        for k in own:
            tk = _torchvision_key("feature_extractor." + k)
            if tk not in weights:
                raise KeyError(f"backbone_weights: missing {tk}")
            v = torch.as_tensor(weights[tk])
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError(f"backbone_weights: {tk} has shape {tuple(v.shape)}, expected {tuple(own[k].shape)}")
            mapped[k] = v
        extra = [k for k in weights if not k.startswith("fc.") and k not in {_torchvision_key("feature_extractor." + o)
                                                                             for o in own}]
        if extra:
            raise KeyError(f"backbone_weights: unexpected keys {extra[:4]}")
        self.feature_extractor.load_state_dict(mapped)

    # ------------------------------------------------------------------ plumbing
    def _bns(self):
        return [m for m in self.feature_extractor.modules() if isinstance(m, nn.BatchNorm2d)]

    def _check_bns(self):
        """Each nn.BatchNorm2d's own eps and momentum are used; the forms the kernels do not have are refused."""
        for name, b in self.feature_extractor.named_modules():
            if isinstance(b, nn.BatchNorm2d) and (b.momentum is None or not b.affine or not b.track_running_stats):
                raise ValueError(f"feature_extractor.{name}: BatchNorm2d with momentum=None, affine=False or "
                                 "track_running_stats=False is not supported (torchvision's ResNet-50 uses none of them)")

    def _ensure_flat(self):
        super()._ensure_flat()
        p0 = next(self.parameters())
        # every num_batches_tracked as a view of one device array: one launch counts them all
        bns = self._bns()
        if self._nbt is None or self._nbt.device != p0.device or any(
                b.num_batches_tracked.data_ptr() != self._nbt.data_ptr() + 8 * i for i, b in enumerate(bns)):
            nbt = torch.stack([b.num_batches_tracked.detach().to(p0.device) for b in bns]).contiguous()
            for i, b in enumerate(bns):
                b.num_batches_tracked = nbt[i]
            self._nbt = nbt

    def _grad_of(self, p):
        flat, gflat, off = p._eav_flat
        return gflat[off:off + p.numel()]

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected images [B,3,H,W], got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        self._check_bns()
        self._require_gpu(x)
        self._require_same_device(x)
        H, W = x.shape[2], x.shape[3]
        _, _, _, (FH, FW) = _plan(self, H, W)
        if FH < 1 or FW < 1 or FH * FW > 256:
            raise ValueError(f"VideoModel: a {H}x{W} image gives a {FH}x{FW} trunk output (1..256 positions supported)")
        self._ensure_flat()
        return KernelFn.apply(x.float().contiguous(), self, *self.parameters())

    # ------------------------------------------------------------------ kernels
    def _conv_fwd(self, u, src, dst, nchw=0):
        L, P, st, ws = _lib.call, _lib.ptr, _lib.stream_ptr(), self._ws
        B = ws.B
        if u.gemm:
            L("eav_gemm_f32", P(src), P(u.conv.weight), P(dst), u.M, u.Co, u.Ci, u.Ci, u.Ci, u.Co, 0, 0, 1, 1, 0, 0, 0, 0,
              0, 0, 1.0, None, 0, None, None, 0, 0, st)
        else:
            L("eav_video_conv_relayout", P(u.conv.weight), P(ws.wrel), None, u.Co, u.Ci, u.k * u.k, st)
            L("eav_video_conv_fwd", P(src), P(ws.wrel), P(dst), B, u.Ci, u.H, u.W, u.Co, u.k, u.k, u.s, u.p, u.OH, u.OW,
              nchw, st)

    def _bn_fwd(self, u, training):
        L, P, st, ws = _lib.call, _lib.ptr, _lib.stream_ptr(), self._ws
        c, bn, C = ws.c[id(u)], ws.bn[id(u)], u.Co
        npart = _lib.plain("eav_video_bn_nparts", u.M)
        if training:
            L("eav_video_bn_stats", P(c), P(ws.stat), u.M, C, st)
        self._bn_finalize(u.bn, ws.stat if training else None, npart if training else 0, u.M, bn, training)

    def _bn_apply(self, u, dst, relu=1, res=None, ures=None):
        L, P, st, ws = _lib.call, _lib.ptr, _lib.stream_ptr(), self._ws
        C, bn = u.Co, ws.bn[id(u)]
        rsc = rsh = None
        if ures is not None:
            rbn = ws.bn[id(ures)]
            rsc, rsh = bn_field(rbn, C, BN_SCALE), bn_field(rbn, C, BN_SHIFT)
        L("eav_video_bn_apply", P(ws.c[id(u)]), bn_field(bn, C, BN_SCALE), bn_field(bn, C, BN_SHIFT), P(res), rsc, rsh,
          P(dst), u.M, C, relu, st)

    def _launch_forward(self, x):
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        B, _, H, W = x.shape
        ws = self._workspace((B, H, W, str(x.device)), lambda: _Workspace(self, B, H, W, x.device), keep_unpinned=3)
        tr = self.training
        if tr:
            L("eav_video_counters_inc", P(self._nbt), self._nbt.numel(), st)
        stem = ws.stem
        self._conv_fwd(stem, x, ws.c[id(stem)], nchw=1)
        self._bn_fwd(stem, tr)
        self._bn_apply(stem, ws.a[id(stem)])
        L("eav_video_maxpool_fwd", P(ws.a[id(stem)]), P(ws.pool), P(ws.pidx), B, stem.OH, stem.OW, 64, ws.PH, ws.PW,
          3, 2, 1, st)
        cur = ws.pool
        for u1, u2, u3, ud in ws.blocks:
            for u, src in ((u1, cur), (u2, ws.a[id(u1)])):
                self._conv_fwd(u, src, ws.c[id(u)])
                self._bn_fwd(u, tr)
                self._bn_apply(u, ws.a[id(u)])
            self._conv_fwd(u3, ws.a[id(u2)], ws.c[id(u3)])
            self._bn_fwd(u3, tr)
            if ud is not None:
                self._conv_fwd(ud, cur, ws.c[id(ud)])
                self._bn_fwd(ud, tr)
                self._bn_apply(u3, ws.a[id(u3)], res=ws.c[id(ud)], ures=ud)
            else:
                self._bn_apply(u3, ws.a[id(u3)], res=cur)
            cur = ws.a[id(u3)]
        self._y = cur
        # head (:50-66): avg / max pools -> fc1 -> fc2 on both rows at once, x * attn, global average, classifier
        B2, HW = 2 * B, ws.HW
        L("eav_video_head_pool", P(cur), P(ws.P), P(ws.hidx), B, HW, FEAT, st)
        gemm = self._gemm
        gemm(ws.P, self.attn_fc1.weight, ws.H1, B2, FEAT, FEAT, bias=self.attn_fc1.bias)
        gemm(ws.H1, self.attn_fc2.weight, ws.A, B2, FEAT, FEAT, bias=self.attn_fc2.bias)
        L("eav_video_head_scale_pool", P(cur), P(ws.A), P(ws.attn), P(ws.z), B, HW, FEAT, st)
        c1, c3 = self.classifier[1], self.classifier[3]
        gemm(ws.z, c1.weight, ws.h, B, 1024, FEAT, bias=c1.bias)
        L("eav_relu_dropout", P(ws.h), B * 1024, 0.0, 0, None, None, st)
        L("eav_dense_softmax_fwd", P(ws.h), P(c3.weight), P(c3.bias), P(ws.logits), None, B, 1024, self.num_labels, st)
        self._token += 1
        self._saved = (self._token, x, tr, ws)
        return self._token

    @staticmethod
    def _gemm(a, w, c, M, N, K, bias=None, transB=0, resid=None, accumulate=0):
        """c[M,N] = a[M,K] . w^T (+ bias) with w [N,K] (transB=0) or a . w with w [K,N] (transB=1)."""
        _lib.call("eav_gemm_f32", _lib.ptr(a), _lib.ptr(w), _lib.ptr(c), M, N, K, K, N if transB else K, N, 0, transB,
                  1, 1, 0, 0, 0, 0, 0, 0, 1.0, _lib.ptr(bias), 0, None, _lib.ptr(resid), N if resid is not None else 0,
                  accumulate, _lib.stream_ptr())

    def _wgrad_gemm(self, dout, act, gout, M, N, K):
        """gout [M,N] = dout[K,M]^T . act[K,N] (split-K, fixed order)."""
        _lib.call("eav_gemm_f32_splitk", _lib.ptr(dout), _lib.ptr(act), _lib.ptr(gout), _lib.ptr(self._ws.wpart), M, N,
                  K, M, N, 1, 1, _lib.stream_ptr())

    def _bias_grad(self, dout, gout, M, N):
        L, P, st, ws = _lib.call, _lib.ptr, _lib.stream_ptr(), self._ws
        L("eav_colsum", P(dout), P(ws.wpart), M, N, N, st)
        L("eav_reduce_partials", P(ws.wpart), _lib.plain("eav_colsum_nparts", M), N, N, 1.0, P(gout), st)

    def _bn_bwd(self, u, dy, gate, gbuf, dx, training):
        """dy -> (gate) -> BN backward: writes g (when gated) to gbuf, dgamma / dbeta, and dx = d conv output."""
        L, P, st, ws = _lib.call, _lib.ptr, _lib.stream_ptr(), self._ws
        C, bn = u.Co, ws.bn[id(u)]
        base = bn.data_ptr()
        L("eav_video_bn_bwd", P(dy), P(gate), P(ws.c[id(u)]), base, P(gbuf) if gate is not None else None, P(ws.stat),
          u.M, C, st)
        L("eav_bn_bwd_finalize", P(ws.stat), _lib.plain("eav_video_bn_nparts", u.M), C, float(u.M), int(training),
          P(self._grad_of(u.bn.weight)), P(self._grad_of(u.bn.bias)), bn_field(bn, C, BN_M1), bn_field(bn, C, BN_M2), st)
        L("eav_bn_rows_bwd", P(gbuf if gate is not None else dy), P(ws.c[id(u)]), base, P(dx), u.M, C, st)

    def _conv_bwd(self, u, dc, act, din, add=None, accumulate=0, nchw=0):
        """weight gradient of u from dc [M,Co] and its input act; din (optional) = data gradient (+ add)."""
        L, P, st, ws = _lib.call, _lib.ptr, _lib.stream_ptr(), self._ws
        gw = self._grad_of(u.conv.weight)
        if u.gemm:
            self._wgrad_gemm(dc, act, gw, u.Co, u.Ci, u.M)
            if din is not None:
                self._gemm(dc, u.conv.weight, din, u.M, u.Ci, u.Co, transB=1, resid=add, accumulate=accumulate)
            return
        KK = u.k * u.k
        n = _lib.plain("eav_video_wgrad_nparts", u.Co, u.Ci, KK, u.M)
        L("eav_video_conv_wgrad", P(dc), P(act), P(ws.wpart), ws.B, u.Ci, u.H, u.W, u.Co, u.k, u.k, u.s, u.p, u.OH, u.OW,
          nchw, n, st)
        L("eav_reduce_partials", P(ws.wpart), n, u.Co * u.Ci * KK, u.Co * u.Ci * KK, 1.0, P(gw), st)
        if din is not None:
            L("eav_video_conv_relayout", P(u.conv.weight), None, P(ws.wrel), u.Co, u.Ci, KK, st)
            L("eav_video_conv_dgrad", P(dc), P(ws.wrel), P(add), P(din), ws.B, u.Ci, u.H, u.W, u.Co, u.k, u.k, u.s, u.p,
              u.OH, u.OW, st)

    def _launch_backward(self, dlogits, token):
        self._check_token(token)
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        _, x, tr, ws = self._saved
        B, B2, HW = ws.B, 2 * ws.B, ws.HW
        G = self._grad_of
        c1, c3 = self.classifier[1], self.classifier[3]
        # classifier
        L("eav_dense_softmax_bwd", P(dlogits), None, P(ws.h), P(c3.weight), P(G(c3.weight)), P(G(c3.bias)), P(ws.dh), B,
          1024, self.num_labels, st)
        L("eav_relu_dropout_bwd", P(ws.dh), P(ws.h), B * 1024, 0.0, st)
        self._wgrad_gemm(ws.dh, ws.z, G(c1.weight), 1024, FEAT, B)
        self._bias_grad(ws.dh, G(c1.bias), B, 1024)
        self._gemm(ws.dh, c1.weight, ws.dz, B, FEAT, 1024, transB=1)
        # attention: d attn (both rows of the fc chain), fc2, fc1
        y = self._y
        L("eav_video_head_attn_bwd", P(y), P(ws.dz), P(ws.dA), B, HW, FEAT, st)
        self._wgrad_gemm(ws.dA, ws.H1, G(self.attn_fc2.weight), FEAT, FEAT, B2)
        self._bias_grad(ws.dA, G(self.attn_fc2.bias), B2, FEAT)
        self._gemm(ws.dA, self.attn_fc2.weight, ws.dH1, B2, FEAT, FEAT, transB=1)
        self._wgrad_gemm(ws.dH1, ws.P, G(self.attn_fc1.weight), FEAT, FEAT, B2)
        self._bias_grad(ws.dH1, G(self.attn_fc1.bias), B2, FEAT)
        backbone = any(p.requires_grad for p in self.feature_extractor.parameters())
        if backbone:
            self._gemm(ws.dH1, self.attn_fc1.weight, ws.dP, B2, FEAT, FEAT, transB=1)
            cur, nxt = ws.D
            L("eav_video_head_feat_bwd", P(ws.dz), P(ws.attn), P(ws.dP), P(ws.hidx), P(cur), B, HW, FEAT, st)
            for bi in range(len(ws.blocks) - 1, -1, -1):
                u1, u2, u3, ud = ws.blocks[bi]
                xin = ws.blocks[bi - 1][2] if bi > 0 else None
                xin_t = ws.a[id(xin)] if xin is not None else ws.pool
                self._bn_bwd(u3, cur, ws.a[id(u3)], ws.Sg3, ws.Sdc, tr)             # g3 = ReLU'(y) dy, dc3
                self._conv_bwd(u3, ws.Sdc, ws.a[id(u2)], ws.Sda)                     # da2
                self._bn_bwd(u2, ws.Sda, ws.a[id(u2)], ws.Sg, ws.Sdc, tr)           # dc2
                self._conv_bwd(u2, ws.Sdc, ws.a[id(u1)], ws.Sda)                     # da1
                self._bn_bwd(u1, ws.Sda, ws.a[id(u1)], ws.Sg, ws.Sdc, tr)           # dc1
                if ud is None:      # identity shortcut: d block input = conv1's data gradient + g3
                    self._conv_bwd(u1, ws.Sdc, xin_t, nxt, add=ws.Sg3)
                else:               # downsample branch: its BN backward from g3 (no ReLU between), then its conv
                    self._conv_bwd(u1, ws.Sdc, xin_t, nxt)
                    self._bn_bwd(ud, ws.Sg3, None, None, ws.Sda, tr)
                    if ud.gemm:
                        self._conv_bwd(ud, ws.Sda, xin_t, nxt, accumulate=1)
                    else:
                        self._conv_bwd(ud, ws.Sda, xin_t, nxt, add=nxt)
                cur, nxt = nxt, cur
            stem = ws.stem
            L("eav_video_maxpool_bwd", P(cur), P(ws.pidx), P(ws.Sda), B, stem.OH, stem.OW, 64, ws.PH, ws.PW, 3, 2, 1, st)
            self._bn_bwd(stem, ws.Sda, ws.a[id(stem)], ws.Sg, ws.Sdc, tr)
            self._conv_bwd(stem, ws.Sdc, x, None, nchw=1)
        return self._grads_out(self._grad_views())


# ---------------------------------------------------------------------------------------------- trainer
class ImageClassifierTrainer:
    """:69-168 with the reference's surface and printed lines (INTEGRATION.md lists the quirks).

    data = [tr_x, tr_y, te_x, te_y], tr_x uint8 [N, F, H, W, 3]; every frame is one sample with its trial's label
    (np.repeat(y, F)).  Frames are pre-processed once on the device; batches are gathered there in the order
    DataLoader(shuffle=True / False) would visit them.  Per-batch accuracies stay on the device and are read once per
    epoch."""

    def __init__(self, data, num_labels=5, lr=5e-5, batch_size=128, backbone_weights=None):
        if not torch.cuda.is_available():
            raise _lib.EavError("ImageClassifierTrainer needs an MI355X (torch device 'cuda' on ROCm); no CPU fallback")
        self.tr_x, self.tr_y, self.te_x, self.te_y = data
        self.batch_size = batch_size
        self.num_labels = num_labels
        self.initial_lr = lr

        self.frames_per_sample = self.tr_x.shape[1]
        self.device = torch.device("cuda")

        self.model = VideoModel(num_labels, backbone_weights=backbone_weights).to(self.device)

        self.criterion = CrossEntropyLoss()
        self.optimizer = FusedAdam(self.model.parameters(), lr=lr, weight_decay=0.01, decoupled=True)

        print("Preprocessing images...")
        self.train_loader = self._build_loader(self.tr_x, self.tr_y, shuffle=True)
        self.test_loader = self._build_loader(self.te_x, self.te_y, shuffle=False)
        print("Done.")

    def _build_loader(self, x, y, shuffle=True):
        from .preprocess import frames_to_pixel_values
        x = np.asarray(x)
        frames = x.reshape(-1, *x.shape[2:])
        pix = frames_to_pixel_values(frames, size=(224, 224), device=self.device)
        y_expanded = torch.from_numpy(np.repeat(y, self.frames_per_sample)).long()
        return DeviceLoader(pix, y_expanded, self.batch_size, shuffle, self.device)

    @staticmethod
    def accuracy(outputs, labels):
        """The per-batch mean of (argmax == label) (:109-111; the reference's method lacks `self`) as a device scalar."""
        return (outputs.argmax(dim=1) == labels).float().mean()

    def train(self, epochs=3, lr=None, freeze=True):
        lr = lr if lr is not None else self.initial_lr
        for g in self.optimizer.param_groups:
            g["lr"] = lr

        for p in self.model.feature_extractor.parameters():
            p.requires_grad = not freeze

        print(f"Training ({'frozen' if freeze else 'unfrozen'}) | lr={lr}")

        for epoch in range(epochs):
            self.model.train()
            accs = []

            for x, y in self.train_loader:
                out, _ = eager_step(self.model, self.optimizer, self.criterion, x, y)
                accs.append(self.accuracy(out, y))

            self.criterion.check()
            train_acc = 0.0
            for v in torch.stack(accs).cpu().tolist() if accs else []:
                train_acc += v
            train_acc /= len(self.train_loader)

            self.model.eval()
            accs, outputs_all = [], []
            with torch.no_grad():
                for x, y in self.test_loader:
                    out = self.model(x)
                    accs.append(self.accuracy(out, y))
                    outputs_all.append(out)

            test_acc = 0.0
            for v in torch.stack(accs).cpu().tolist() if accs else []:
                test_acc += v
            test_acc /= len(self.test_loader)

            if epoch == epochs - 1 and not freeze:
                self.outputs_test = torch.cat(outputs_all).cpu().numpy()

            print(
                f"Epoch {epoch + 1} | "
                f"Train Acc: {train_acc * 100:.2f}% | "
                f"Test Acc: {test_acc * 100:.2f}%"
            )

    def clear_loaders(self):
        del self.train_loader
        del self.test_loader
        torch.cuda.empty_cache()


__all__ = ["VideoModel", "ImageClassifierTrainer", "Bottleneck"]
