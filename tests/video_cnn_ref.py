"""Plain-torch restatement of the video CNN step (CNN_torch/CNN_Vision.py VideoModel on torchvision's ResNet-50) on named
tensors, for any dtype: run in float64 it is the reference the GPU kernels are held to; run in float32 on the CPU it
measures torch's own fp32 error against that reference.  Gradients come from torch autograd."""
import torch
import torch.nn as nn
import torch.nn.functional as F

STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))


def block_names():
    """(prefix, stride, has_downsample) of every Bottleneck in order."""
    out = []
    for li, (_, n, s) in enumerate(STAGES):
        for j in range(n):
            out.append((f"feature_extractor.{li + 4}.{j}", s if j == 0 else 1, j == 0))
    return out


def _bn(x, sd, pre, training, eps=1e-5, momentum=0.1):
    return F.batch_norm(x, sd[pre + ".running_mean"], sd[pre + ".running_var"], sd[pre + ".weight"], sd[pre + ".bias"],
                        training, momentum, eps)


def _routed_pool(y, idx):
    """max pooling with a given argmax: idx [B,C,...] = flat indices into y's spatial map (torch's return_indices form)."""
    B, C = y.shape[:2]
    return y.flatten(2).gather(2, idx.reshape(B, C, -1)).view(idx.shape)


def _relu(v, routes, key, record=None):
    """ReLU, or (routes given) the GPU's gate: v where the GPU's stored output is > 0.  A pre-activation within rounding
    of zero may be gated differently by two implementations, and the gate routes a whole gradient element.  record: dict
    that receives the pre-activation under `key`."""
    if record is not None:
        record[key] = v.detach()
    if routes is None:
        return F.relu(v)
    return v * routes[2][key].to(v.dtype)


def trunk(x, sd, training, routes=None, record=None):
    """x [B,3,H,W] -> [B,2048,h,w]; updates the running statistics in sd when training (as nn.BatchNorm2d does).
    routes: optional (stem max-pool argmax, head max-pool argmax, ReLU gates) to route with - exact ties and near-ties
    within rounding may be decided differently by two implementations, and an argmax or a gate routes a whole gradient."""
    y = F.conv2d(x, sd["feature_extractor.0.weight"], stride=2, padding=3)
    y = _relu(_bn(y, sd, "feature_extractor.1", training), routes, "stem", record)
    y = F.max_pool2d(y, 3, 2, 1) if routes is None else _routed_pool(y, routes[0])
    for i, (pre, s, ds) in enumerate(block_names()):
        o = _relu(_bn(F.conv2d(y, sd[pre + ".conv1.weight"]), sd, pre + ".bn1", training), routes, (i, 1), record)
        o = _relu(_bn(F.conv2d(o, sd[pre + ".conv2.weight"], stride=s, padding=1), sd, pre + ".bn2", training), routes,
                  (i, 2), record)
        o = _bn(F.conv2d(o, sd[pre + ".conv3.weight"]), sd, pre + ".bn3", training)
        idn = _bn(F.conv2d(y, sd[pre + ".downsample.0.weight"], stride=s), sd, pre + ".downsample.1", training) if ds else y
        y = _relu(o + idn, routes, (i, 3), record)
    if record is not None:
        record["trunk"] = y.detach()
    return y


def head(y, sd, routes=None, record=None):
    B = y.shape[0]
    avg = F.adaptive_avg_pool2d(y, 1).view(B, -1)
    mx = F.adaptive_max_pool2d(y, 1).view(B, -1) if routes is None else _routed_pool(y, routes[1])
    fc = lambda v: F.linear(F.linear(v, sd["attn_fc1.weight"], sd["attn_fc1.bias"]),  # noqa: E731
                            sd["attn_fc2.weight"], sd["attn_fc2.bias"])
    attn = fc(avg) + fc(mx)
    z = F.adaptive_avg_pool2d(y * attn.unsqueeze(-1).unsqueeze(-1), 1).flatten(1)
    h = _relu(F.linear(z, sd["classifier.1.weight"], sd["classifier.1.bias"]), routes, "h", record)
    return F.linear(h, sd["classifier.3.weight"], sd["classifier.3.bias"])


def step(sd, x, y, training=True, freeze=False, dtype=torch.float64, routes=None, channels_last=False, record=None):
    """One forward + backward.  sd: state_dict tensors (copied, cast to dtype; running stats updated in the copy).
    channels_last: the same network with NHWC tensors (other CPU kernels, another summation order).
    Returns logits, loss, {param name: grad or None}, the updated copy of sd."""
    s = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
    if channels_last:
        s = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in s.items()}
        x = x.contiguous(memory_format=torch.channels_last)
    params = {k: v for k, v in s.items() if not any(k.endswith(t) for t in ("running_mean", "running_var",
                                                                             "num_batches_tracked"))}
    for k, v in params.items():
        v.requires_grad_(not (freeze and k.startswith("feature_extractor.")))
    if training:
        for k in s:
            if k.endswith("num_batches_tracked"):
                s[k] += 1
    logits = head(trunk(x.to(dtype), s, training, routes, record), s, routes, record)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = {k: (v.grad.detach() if v.grad is not None else None) for k, v in params.items()}
    out = {k: v.detach() for k, v in s.items()}
    return logits.detach(), loss.detach(), grads, out


# ---------------------------------------------------------------------------------------------- torch.nn form
class TvBottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        o = self.relu(self.bn1(self.conv1(x)))
        o = self.relu(self.bn2(self.conv2(o)))
        o = self.bn3(self.conv3(o))
        return self.relu(o + (self.downsample(x) if self.downsample is not None else x))


class TvResNet50(nn.Module):
    """torchvision.models.resnet.ResNet(Bottleneck, [3, 4, 6, 3]) restated in plain torch: its module names, its
    construction order and its init pass (torchvision is not a dependency).  The golden generator hands it to the
    reference as torchvision.models.resnet50; `pretrained` is ignored."""

    def __init__(self, pretrained=False, **kwargs):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, 3)
        self.layer2 = self._make_layer(128, 4, stride=2)
        self.layer3 = self._make_layer(256, 6, stride=2)
        self.layer4 = self._make_layer(512, 3, stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, 1000)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride, bias=False),
                                       nn.BatchNorm2d(planes * 4))
        layers = [TvBottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(TvBottleneck(self.inplanes, planes))
        return nn.Sequential(*layers)


class TvVideoModel(nn.Module):
    """CNN_Vision.py's VideoModel construction over TvResNet50: the same network as torch.nn modules (the CPU tests'
    seeded-init yardstick and tools/video_cnn_step_bench.py's torch.nn comparison)."""

    def __init__(self, num_labels=5):
        super().__init__()
        backbone = TvResNet50()
        self.feature_extractor = nn.Sequential(*list(backbone.children())[:-2])
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.attn_fc1 = nn.Linear(2048, 2048)
        self.attn_fc2 = nn.Linear(2048, 2048)
        self.global_pool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(2048, 1024), nn.ReLU(), nn.Linear(1024, num_labels))

    def forward(self, x):
        x = self.feature_extractor(x)
        B = x.size(0)
        fc = lambda v: self.attn_fc2(self.attn_fc1(v))  # noqa: E731
        attn = fc(self.avg_pool(x).view(B, -1)) + fc(self.max_pool(x).view(B, -1))
        return self.classifier(self.global_pool(x * attn.unsqueeze(-1).unsqueeze(-1)))


# ---------------------------------------------------------------------------------------------- golden fixtures
def load_golden(path):
    """A tests/golden/video_cnn_*.npz: (the npz, {pin name: (strided sample, [sum |.|, max |.|])})."""
    import numpy as np
    g = np.load(path)
    off, vals, ab = g["pin_offsets"], g["pin_values"], g["pin_abs"]
    pins = {str(n): (vals[off[i]:off[i + 1]], ab[i]) for i, n in enumerate(g["pin_names"])}
    return g, pins


def sample_of(t, n=48):
    """The generator's strided sample (flat[::ceil(numel / n)]) of a tensor, as a float32 numpy array."""
    a = t.detach().float().reshape(-1).numpy()
    return a[::max(1, -(-a.size // n))]


def golden_inputs(g, s):
    """Batch s of a step fixture: synth images [B,3,H,H] and labels, as the generator drew them."""
    import numpy as np
    from eav_amd import synth
    B, H, xs = int(g["B"]), int(g["H"]), int(g["xseed"])
    return (torch.from_numpy(synth.normal(xs + s, (B, 3, H, H), 0.0, 1.0)),
            torch.from_numpy(synth.labels(xs + 100 + s, B, 5).astype(np.int64)))
