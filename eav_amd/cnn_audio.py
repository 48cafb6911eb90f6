"""The audio CNN baseline of CNN_torch/CNN_audio.py on MI355X, over libeav_hip.so (csrc/audio_cnn.hip).

    AudioModel(num_classes=5)                                                         (:10-35)
        __call__(x[B,1,T] or the permuted view [B,T,1]) -> logits [B,num_classes], 176 <= T <= 183
    create_dataloader(x[N,T,1], y, batch_size=64, shuffle=True) -> DeviceLoader       (:38-43)
    ActivationSaver(model, val_loader, save_dir).save()                               (:46-70)
    train_model(model, train_loader, val_loader, epochs=100, lr=1e-3, save_dir="activations", subject_id=None,
                device=None)                                                          (:73-139)

The module owns the same ``features`` / ``classifier`` sub-modules at the reference's indices, so ``state_dict()`` keys
match and a seeded construction draws the reference's default initialisation bit for bit.  All training and inference
arithmetic is in hand-written gfx950 kernels (every Conv1d, ReLU, Dropout and MaxPool1d and their gradients in
csrc/audio_cnn.hip; the classifier, the loss and Adam in csrc/head_optim.hip); there is no CPU path.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib
from .criteria import CrossEntropyLoss
from .optim import FusedAdam
from .runtime import DeviceLoader, KernelFn, KernelModule, train_step

_PARAM_ORDER = ["features.0.weight", "features.0.bias", "features.2.weight", "features.2.bias", "features.6.weight",
                "features.6.bias", "features.8.weight", "features.8.bias", "classifier.weight", "classifier.bias"]
POOLED = 22                 # the classifier's fixed width 128 * 22 (:33): floor(T / 8) must be 22
T_MIN, T_MAX = 8 * POOLED, 8 * POOLED + 7
NCMAX = 16                  # classes the head kernels take

# train_model saves the final state_dict here when subject_id is given - the reference's literal directory string (:133)
MODEL_DIR = r"D:\.spyder-py3\finetuned_cnn_7030"


class _Workspace:
    """Device buffers for one (B, T) problem size (fp32 unless noted)."""

    def __init__(self, m, B, T, dev):
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        P = POOLED
        self.a1, self.da1 = f(B, 256, T), f(B, 256, T)
        self.p2, self.idx2 = f(B, 128, P), torch.empty(B, 128, P, dtype=torch.uint8, device=dev)
        self.a3, self.a4 = f(B, 128, P), f(B, 128, P)
        self.logits = f(B, m.num_classes)
        self.da4, self.dz3, self.dz2 = f(B, 128 * P), f(B, 128, P), f(B, 128, 8 * P)
        # weight-gradient partials of the four convs (one buffer, used in turn)
        self.np = {k: _lib.plain("eav_audio_wgrad_nparts", B, c, mo, lo)
                   for k, (c, mo, lo) in {1: (1, 256, T), 2: (256, 128, 8 * P), 3: (128, 128, P),
                                           4: (128, 128, P)}.items()}
        size = {1: 256 * 5 + 256, 2: 128 * 1280 + 128, 3: 128 * 640 + 128, 4: 128 * 640 + 128}
        self.size = size
        self.part = f(max(self.np[k] * size[k] for k in size))


class AudioModel(KernelModule):
    _PARAM_ORDER = _PARAM_ORDER

    def __init__(self, num_classes: int = 5):
        super().__init__()
        if not 1 <= num_classes <= NCMAX:
            raise NotImplementedError(f"eav_amd.AudioModel: the gfx950 head kernels cover 1..{NCMAX} classes")
        # the reference's modules at the reference's indices (:14-33): identical state_dict keys and default init
        self.features = nn.Sequential(
            nn.Conv1d(1, 256, kernel_size=5, padding=2),
            nn.ReLU(),

            nn.Conv1d(256, 128, kernel_size=5, padding=2),
            nn.ReLU(),
            nn.Dropout(0.1),

            nn.MaxPool1d(8),

            nn.Conv1d(128, 128, kernel_size=5, padding=2),
            nn.ReLU(),

            nn.Conv1d(128, 128, kernel_size=5, padding=2),
            nn.ReLU(),
            nn.Dropout(0.5),
        )
        self.classifier = nn.Linear(128 * 22, num_classes)
        self.num_classes = num_classes
        # (set_dropout_masks, tests: uint8 keep-masks [B,128,T] after conv2, [B,128,22] after conv4)
        self.dropout_seed = 0xA0D10C

    # ------------------------------------------------------------------ plumbing
    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or (x.shape[1] != 1 and x.shape[2] != 1):
            raise ValueError(f"expected input [B,1,T] (or the permuted loader view [B,T,1]), got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        B, T = x.shape[0], (x.shape[2] if x.shape[1] == 1 else x.shape[1])
        if not T_MIN <= T <= T_MAX:
            raise NotImplementedError(f"eav_amd.AudioModel: T = {T}; the classifier's fixed 128*22 inputs need "
                                      f"{T_MIN} <= T <= {T_MAX} (floor(T/8) = 22), as in the reference")
        self._require_gpu(x)
        self._require_same_device(x)
        self._ensure_flat()
        return KernelFn.apply(x.reshape(B, T).float().contiguous(), self, *self._params())

    def _drop(self):
        return (float(self.features[4].p), float(self.features[10].p)) if self.training else (0.0, 0.0)

    # ------------------------------------------------------------------ kernels
    def _launch_forward(self, x):
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        B, T = x.shape
        # one workspace per batch size, never freed while a captured hipGraph holds its raw pointers (cached_workspace);
        # three replaceable slots: train_model meets a full batch, a ragged last training batch and a ragged validation
        # batch in every epoch
        ws = self._workspace((B, T, str(x.device)), lambda: _Workspace(self, B, T, x.device), keep_unpinned=3)
        w1, b1, w2, b2, w3, b3, w4, b4, wc, bc = [P(p) for p in self._params()]
        d1, d2 = self._drop()

        def check(masks):
            if tuple(masks[0].shape) != (B, 128, T) or tuple(masks[1].shape) != (B, 128, POOLED) \
                    or masks[0].dtype != torch.uint8 or masks[1].dtype != torch.uint8 \
                    or masks[0].device != x.device or masks[1].device != x.device:
                raise _lib.EavError(f"set_dropout_masks: expected uint8 device masks [{B},128,{T}] and "
                                    f"[{B},128,{POOLED}]")
            return masks[0].contiguous(), masks[1].contiguous()

        cnt, mk = self._dropout(x.device, d1 > 0.0 or d2 > 0.0, check)
        self._token += 1
        seed1, seed2 = self.dropout_seed, self.dropout_seed + 1
        if cnt is not None:                 # device-resident dropout counter: graph replays draw fresh masks
            L("eav_counter_inc", cnt, st)
        m1, m2 = mk(0), mk(1)
        L("eav_audio_conv5_fwd", P(x), w1, b1, P(ws.a1), None, B, 1, 256, T, T, 0, 0.0, 0, None, None, st)
        L("eav_audio_conv5_fwd", P(ws.a1), w2, b2, P(ws.p2), P(ws.idx2), B, 256, 128, T, 8 * POOLED, 1, d1, seed1,
          m1, cnt, st)
        L("eav_audio_conv5_fwd", P(ws.p2), w3, b3, P(ws.a3), None, B, 128, 128, POOLED, POOLED, 0, 0.0, 0, None, None,
          st)
        L("eav_audio_conv5_fwd", P(ws.a3), w4, b4, P(ws.a4), None, B, 128, 128, POOLED, POOLED, 0, d2, seed2, m2, cnt,
          st)
        L("eav_dense_softmax_fwd", P(ws.a4), wc, bc, P(ws.logits), None, B, 128 * POOLED, self.num_classes, st)
        self._saved = (self._token, x, d1, d2, mk, ws)      # (mk keeps explicit masks alive)
        return self._token

    def _launch_backward(self, dlogits, token):
        self._check_token(token)
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        _, x, d1, d2, _, ws = self._saved
        B, T = x.shape
        g = self._grad_views()
        _, _, w2, _, w3, _, w4, _, wc, _ = [P(p) for p in self._params()]
        s1, s2 = 1.0 / (1.0 - d1), 1.0 / (1.0 - d2)
        Pn = POOLED

        def wgrad(layer, dout, gate, gscale, act, cact, mo, lact, lout, wkey):
            n = ws.np[layer]
            L("eav_audio_conv5_wgrad", P(dout), P(gate), gscale, P(act), P(ws.part), B, cact, mo, lact, lout, n, st)
            # weight and bias are adjacent in the flat gradient buffer (every weight is a multiple of 4 floats)
            L("eav_reduce_partials", P(ws.part), n, ws.size[layer], ws.size[layer], 1.0, P(g[wkey]), st)

        # classifier; then Dropout(0.5) <- ReLU <- conv4, folded into the operand loads of conv4's two gradients
        L("eav_dense_softmax_bwd", P(dlogits), None, P(ws.a4), wc, P(g["classifier.weight"]), P(g["classifier.bias"]),
          P(ws.da4), B, 128 * Pn, self.num_classes, st)
        L("eav_audio_conv5_dgrad", P(ws.da4), P(ws.a4), s2, w4, P(ws.dz3), P(ws.a3), None, 1.0, B, 128, 128, Pn, Pn, 0,
          st)
        wgrad(4, ws.da4, ws.a4, s2, ws.a3, 128, 128, Pn, Pn, "features.8.weight")
        # conv3: its data gradient lands, through MaxPool / Dropout(0.1) / ReLU, on the dense gradient of conv2's output
        L("eav_audio_conv5_dgrad", P(ws.dz3), None, 1.0, w3, P(ws.dz2), P(ws.p2), P(ws.idx2), s1, B, 128, 128, Pn, Pn,
          1, st)
        wgrad(3, ws.dz3, None, 1.0, ws.p2, 128, 128, Pn, Pn, "features.6.weight")
        # conv2 (data gradient gated by ReLU'(a1)), then conv1
        L("eav_audio_conv5_dgrad", P(ws.dz2), None, 1.0, w2, P(ws.da1), P(ws.a1), None, 1.0, B, 128, 256, 8 * Pn, T, 0,
          st)
        wgrad(2, ws.dz2, None, 1.0, ws.a1, 256, 128, T, 8 * Pn, "features.2.weight")
        wgrad(1, ws.da1, None, 1.0, x, 1, 256, T, T, "features.0.weight")
        return self._grads_out(g)


def create_dataloader(x, y, batch_size=64, shuffle=True):
    """:38-43.  x [N, T, 1], y [N].  The split is moved to HBM once; batches are gathered there in the order
    DataLoader(TensorDataset(x, y), batch_size, shuffle) would visit them (same samplers, same torch RNG draws)."""
    if not torch.cuda.is_available():
        raise _lib.EavError("eav_amd.cnn_audio.create_dataloader needs an MI355X (torch device 'cuda' on ROCm)")
    x_tensor = torch.tensor(x, dtype=torch.float32)
    y_tensor = torch.tensor(y, dtype=torch.long)
    return DeviceLoader(x_tensor, y_tensor, batch_size, shuffle, torch.device("cuda"))


class ActivationSaver:
    """:46-70: after every epoch, the eval-mode logits of the whole validation loader (in its visiting order) are saved
    as one numpy array with torch.save to save_dir/activations_epoch_{n}.pth."""

    def __init__(self, model, val_loader, save_dir):
        self.model = model
        self.val_loader = val_loader
        self.save_dir = save_dir
        self.epoch = 0

        os.makedirs(save_dir, exist_ok=True)

    def save(self):
        self.model.eval()
        activations = []

        with torch.no_grad():
            for x, _ in self.val_loader:
                x = x.permute(0, 2, 1)  # (B, 1, T)
                activations.append(self.model(x))
        activations = torch.cat(activations).cpu().numpy()       # one read-back per epoch
        path = os.path.join(self.save_dir, f"activations_epoch_{self.epoch + 1}.pth")
        torch.save(activations, path)

        self.epoch += 1
        self.model.train()


def train_model(model, train_loader, val_loader, epochs=100, lr=1e-3, save_dir="activations", subject_id=None,
                device=None):
    """:73-139 - CrossEntropyLoss + Adam(lr), one printed line per epoch, ActivationSaver after every epoch.

    The loaders are ``create_dataloader`` results.  Full batches run as one replayed hipGraph step (GraphStep:
    gather, forward, loss, backward, FusedAdam(capturable=True)); the last partial batch runs eagerly.  Per-batch losses
    and the hit count stay on the device and are read once per epoch; the printed loss is the reference's sum of the
    per-batch losses (in batch order) over len(train_loader).

    Quirk kept from the reference (:131-137): with ``subject_id`` set, the final state_dict is saved to
    ``os.path.join(MODEL_DIR, f"audio_finetuned_{subject_id}.pth")``, MODEL_DIR being the module-level
    ``r"D:\\.spyder-py3\\finetuned_cnn_7030"`` - on Linux a relative path with backslashes in its name; set
    ``eav_amd.cnn_audio.MODEL_DIR`` to save elsewhere."""
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.EavError("eav_amd.cnn_audio.train_model needs an MI355X (torch device 'cuda' on ROCm); no CPU "
                            "fallback")
    model.to(device)

    criterion = CrossEntropyLoss()
    optimizer = FusedAdam(model.parameters(), lr=lr, capturable=True)
    activation_saver = ActivationSaver(model, val_loader, save_dir)
    grad_sync = None
    graphs = {}

    for epoch in range(epochs):
        model.train()
        batches = train_loader.index_batches()
        losses = torch.zeros(max(len(batches), 1), dtype=torch.float32, device=device)
        correct = torch.zeros((), dtype=torch.int64, device=device)
        total = 0

        for k, idx in enumerate(batches):
            out, loss, y = train_step(graphs, model, optimizer, criterion, train_loader, idx, True, grad_sync,
                                      eager_input=lambda x: x.permute(0, 2, 1))
            if y is None:       # a replayed step: its labels were gathered inside the graph
                y = train_loader.gather_labels(idx)
            losses[k].copy_(loss)
            correct += (out.argmax(dim=1) == y).sum()
            total += len(idx)
        criterion.check()
        train_loss = 0.0
        for v in losses[:len(batches)].cpu().tolist():      # the epoch's read-back; summed in the reference's order
            train_loss += v
        train_acc = 100 * int(correct.item()) / total

        model.eval()
        correct = torch.zeros((), dtype=torch.int64, device=device)
        total = 0

        with torch.no_grad():
            for x, y in val_loader:
                x = x.permute(0, 2, 1)
                out = model(x)
                correct += (out.argmax(dim=1) == y).sum()
                total += y.size(0)

        val_acc = 100 * int(correct.item()) / total

        activation_saver.save()

        print(
            f"Epoch [{epoch + 1}/{epochs}] | "
            f"Loss: {train_loss / len(train_loader):.4f} | "
            f"Train Acc: {train_acc:.2f}% | "
            f"Val Acc: {val_acc:.2f}%"
        )

        if epoch == epochs - 1 and subject_id is not None:
            model_path = os.path.join(MODEL_DIR, f"audio_finetuned_{subject_id}.pth")
            torch.save(model.state_dict(), model_path)
            print(f"Model saved to {model_path}")


__all__ = ["AudioModel", "create_dataloader", "ActivationSaver", "train_model", "MODEL_DIR"]
