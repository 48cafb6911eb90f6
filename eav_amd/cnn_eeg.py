"""Canonical EEGNet + EEGNetTrainer on MI355X: the class API of CNN_torch/CNN_EEG.py over libeav_hip.so.

    EEGNet(nb_classes, Chans=64, Samples=128, dropoutRate=0.5, kernLength=64, F1=8, D=2, F2=16, norm_rate=0.25) (:12-13)
        __call__(x[B,Chans,Samples] or [B,1,Chans,Samples]) -> logits [B,nb_classes]                  (:58-67)
    EEGNetTrainer(model, train_dataset, val_dataset, batch_size=32, epochs=100, lr=0.001)             (:75)
        .train_epoch() / .validate_epoch() / .train() / .predict(dataset=None)                         (:91-162)

The module owns the same ``block1`` / ``block2`` / ``classifier`` sub-modules, so ``state_dict()`` keys match the
reference's, and the constructor repeats the reference's shape probe (a train-mode dummy forward on the host,
:48-54), which leaves ``running_var = 0.9`` / ``num_batches_tracked = 1`` in every BatchNorm and advances the torch
RNG by the two dropout draws - a freshly constructed model is therefore in the reference's state.  All training and
inference arithmetic is in hand-written gfx950 kernels (csrc/eegnet_canon.hip, eegnet_block.hip, head_optim.hip);
there is no CPU path: calling the model with a host tensor raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, eegnet_canon
from .criteria import CrossEntropyLoss
from .optim import FusedAdam
from .runtime import DeviceLoader, KernelFn, KernelModule, train_step

_PARAM_ORDER = [
    "block1.0.weight", "block1.1.weight", "block1.1.bias", "block1.2.weight", "block1.3.weight", "block1.3.bias",
    "block2.0.weight", "block2.1.weight", "block2.2.weight", "block2.2.bias", "classifier.weight", "classifier.bias",
]


class _Workspace(eegnet_canon.Workspace):
    """eegnet_canon.Workspace + block 2 (depthwise temporal conv d3, pointwise conv z3, pooled a3) and the logits."""

    def __init__(self, m, B, dev):
        super().__init__(m, B, dev)
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        C2, F2, T2 = m.F1 * m.D, m.F2, self.T2
        self.d3, self.dd3 = f(B, C2, T2), f(B, C2, T2)
        self.z3, self.dz3 = f(B, F2, T2), f(B, F2, T2)
        self.a3, self.da3 = f(B, self.NF), f(B, self.NF)
        self.logits = f(B, m.nb_classes)
        self.np_c = _lib.plain("eav_sepconv_fwd_nparts", B, T2)
        self.part_c = f(self.np_c, 2 * F2)
        self.np_pw = _lib.plain("eav_pointwise_bwd_nparts", B, T2)
        self.part_pw = f(self.np_pw, F2 * C2)
        self.part_dw = f(B, C2 * m.K2)


class EEGNet(KernelModule):
    _PARAM_ORDER = _PARAM_ORDER
    K2 = 16   # taps of the depthwise temporal conv of block2 (CNN_EEG.py:35)

    def __init__(self, nb_classes, Chans=64, Samples=128, dropoutRate=0.5, kernLength=64, F1=8, D=2, F2=16,
                 norm_rate=0.25):
        super().__init__()
        if not (1 <= F1 <= 16 and 1 <= D <= 8 and D * F1 <= 64 and 1 <= F2 <= 64 and 1 <= kernLength <= 1024
                and 1 <= Chans <= 256 and 1 <= nb_classes <= 16 and Samples >= 32):
            raise NotImplementedError("eav_amd.EEGNet: the gfx950 kernels cover F1<=16, D<=8, D*F1<=64, F2<=64, "
                                      "kernLength<=1024, Chans<=256, nb_classes<=16, Samples>=32")
        self.Chans, self.Samples = Chans, Samples
        # the reference's modules at the reference's indices (:20-42): identical state_dict keys and default init
        self.block1 = nn.Sequential(
            nn.Conv2d(1, F1, (1, kernLength), padding='same', bias=False),
            nn.BatchNorm2d(F1),
            nn.Conv2d(F1, D * F1, (Chans, 1), groups=F1, bias=False),
            nn.BatchNorm2d(D * F1),
            nn.ELU(),
            nn.AvgPool2d((1, 4)),
            nn.Dropout(dropoutRate),
        )
        self.block2 = nn.Sequential(
            nn.Conv2d(D * F1, D * F1, (1, self.K2), padding='same', groups=D * F1, bias=False),
            nn.Conv2d(D * F1, F2, (1, 1), bias=False),
            nn.BatchNorm2d(F2),
            nn.ELU(),
            nn.AvgPool2d((1, 8)),
            nn.Dropout(dropoutRate),
        )
        self.flatten = nn.Flatten()
        # the reference sizes the classifier with a train-mode dummy forward (:48-54); repeated on the host so that the
        # BatchNorm buffers and the torch RNG end up exactly where the reference's constructor leaves them
        with torch.no_grad():
            n_flatten = self.flatten(self.block2(self.block1(torch.zeros(1, 1, Chans, Samples)))).shape[1]
        assert n_flatten == F2 * (Samples // 4 // 8)
        self.classifier = nn.Linear(n_flatten, nb_classes)

        self.nb_classes, self.kernLength, self.F1, self.D, self.F2 = nb_classes, kernLength, F1, D, F2
        self.dropoutRate, self.norm_rate = float(dropoutRate), norm_rate      # norm_rate: accepted, unused (:13)
        self.dropout_seed = 0x0CA2EED          # (set_dropout_masks, tests: uint8 keep-masks [B,C2,S/4], [B,F2,S/32])

    # ------------------------------------------------------------------ plumbing
    def forward(self, x):
        self._require_gpu(x)
        if x.dim() == 3:
            x = x.unsqueeze(1)                                                           # :61-62
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.Chans or x.shape[3] != self.Samples:
            raise ValueError(f"expected input [B,{self.Chans},{self.Samples}], got {tuple(x.shape)}")
        self._require_same_device(x)
        self._ensure_flat()
        return KernelFn.apply(x.contiguous().float(), self, *self._params())

    # ------------------------------------------------------------------ kernels
    def _bn_finalize(self, bn, part, nparts, count, buf, training):
        """... and nn.BatchNorm2d's step count, bumped on the host right behind each launch."""
        super()._bn_finalize(bn, part, nparts, count, buf, training)
        if training:
            bn.num_batches_tracked += 1

    def _launch_forward(self, x):
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        B, C2, F2 = x.shape[0], self.F1 * self.D, self.F2
        # one workspace per batch size, never freed while a captured hipGraph holds its raw pointers (cached_workspace)
        ws = self._workspace((B, self.Chans, self.Samples, str(x.device)), lambda: _Workspace(self, B, x.device))
        training = bool(self.training)
        w1, _, _, wd, _, _, wdw, wp, _, _, wc, bc = self._params()
        drop = self.dropoutRate if training else 0.0
        self._token += 1
        cnt, mk = self._dropout(x.device, drop > 0.0)
        if cnt is not None:                 # device-resident dropout counter: graph replays draw fresh masks
            L("eav_counter_inc", cnt, st)
        drop1, drop2 = (drop, self.dropout_seed, mk(0), cnt), (drop, self.dropout_seed + 1, mk(1), cnt)
        eegnet_canon.block1_forward(self, ws, x, w1, self.block1[1], wd, self.block1[3], 0, training, drop1)
        L("eav_sepconv_fwd", P(ws.a2), P(wdw), P(wp), P(ws.d3), P(ws.z3), P(ws.part_c), B, C2, F2, ws.T2, self.K2, st)
        self._bn_finalize(self.block2[2], ws.part_c, ws.np_c, B * ws.T2, ws.bn3, training)
        L("eav_bn_elu_pool_fwd", P(ws.z3), P(ws.bn3), P(ws.a3), B, F2, ws.T2, 8, *drop2, st)
        L("eav_dense_softmax_fwd", P(ws.a3), P(wc), P(bc), P(ws.logits), None, B, ws.NF, self.nb_classes, st)
        self._saved = eegnet_canon.Saved(self._token, x, training, drop1, drop2, mk, ws)
        return self._token

    def _launch_backward(self, dlogits, token):
        self._check_token(token)
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        s = self._saved
        x, training, drop1, drop2, ws = s.x, s.training, s.drop1, s.drop2, s.ws
        B, K2, F2, C2, T2 = x.shape[0], self.K2, self.F2, self.F1 * self.D, ws.T2
        g = self._grad_views()
        _, _, _, wd, _, _, wdw, wp, _, _, wc, _ = self._params()
        L("eav_dense_softmax_bwd", P(dlogits), None, P(ws.a3), P(wc), P(g["classifier.weight"]),
          P(g["classifier.bias"]), P(ws.da3), B, ws.NF, self.nb_classes, st)
        # block2 tail: Dropout <- AvgPool8 <- ELU <- BatchNorm
        self._bn_elu_pool_bwd(ws.da3, ws.z3, ws.dz3, ws.bn3, ws.part_pb, g["block2.2.weight"], g["block2.2.bias"], B, F2,
                              T2, 8, drop2, training)
        # pointwise and depthwise temporal convs
        L("eav_pointwise_bwd", P(ws.dz3), P(ws.d3), P(wp), P(ws.dd3), P(ws.part_pw), B, C2, F2, T2, st)
        L("eav_reduce_partials", P(ws.part_pw), ws.np_pw, F2 * C2, F2 * C2, 1.0, P(g["block2.1.weight"]), st)
        L("eav_dwt_bwd", P(ws.dd3), P(ws.a2), P(wdw), P(ws.da2), P(ws.part_dw), B, C2, T2, K2, st)
        L("eav_reduce_partials", P(ws.part_dw), B, C2 * K2, C2 * K2, 1.0, P(g["block2.0.weight"]), st)
        eegnet_canon.block1_backward(self, ws, x, wd, [g[k] for k in _PARAM_ORDER[:6]], 0, training, drop1)
        return self._grads_out(g)


class EEGNetTrainer:
    """CNN_EEG.py:70-162.  The datasets are ``TensorDataset(x, y)``; both splits are moved to HBM once and batches
    are assembled there (eav_amd.runtime.DeviceLoader: same samplers and torch RNG consumption as DataLoader)."""

    def __init__(self, model, train_dataset, val_dataset, batch_size=32, epochs=100, lr=0.001):
        if not torch.cuda.is_available():
            raise _lib.EavError("eav_amd.EEGNetTrainer needs an MI355X (torch device 'cuda' on ROCm); no CPU fallback")
        self.device = torch.device("cuda")
        print(f"Using device: {self.device}")
        self.model = model.to(self.device)
        self.epochs = epochs
        self.batch_size = batch_size
        self.train_loader = DeviceLoader(*train_dataset.tensors, batch_size, True, self.device)
        self.test_loader = DeviceLoader(*val_dataset.tensors, batch_size, False, self.device)
        self.criterion = CrossEntropyLoss()                                          # :88
        self.optimizer = FusedAdam(model.parameters(), lr=lr, capturable=True)       # :89
        self.grad_sync = None     # set by eav_amd.dist.attach(trainer) under torchrun
        self.use_graph = True
        self._graphs = {}

    def train_epoch(self):
        self.model.train()
        running_loss = torch.zeros((), dtype=torch.float32, device=self.device)
        dl = self.train_loader
        batches = dl.index_batches()
        for idx in batches:
            _, loss, _ = train_step(self._graphs, self.model, self.optimizer, self.criterion, dl, idx, self.use_graph,
                                    self.grad_sync)
            running_loss += loss          # accumulated on the device: one host read per epoch, not per step (:106)
        self.criterion.check()            # labels outside [0, classes) seen by any step of this epoch raise here
        return running_loss.item() / len(batches)

    def validate_epoch(self):
        self.model.eval()
        val_loss, correct, total = 0.0, 0, 0
        with torch.no_grad():
            for inputs, labels in self.test_loader:
                outputs = self.model(inputs)
                val_loss += self.criterion(outputs, labels).item()
                correct += (outputs.argmax(1) == labels).sum().item()
                total += labels.size(0)
        return val_loss / len(self.test_loader), 100 * correct / total

    def train(self):
        print(f"Starting training for {self.epochs} epochs...")
        for epoch in range(self.epochs):
            train_loss = self.train_epoch()
            val_loss, accuracy = self.validate_epoch()
            print(f'Epoch {epoch + 1}/{self.epochs} | Train Loss: {train_loss:.4f} | Val Loss: {val_loss:.4f} | '
                  f'Val Acc: {accuracy:.2f}%')

    def predict(self, dataset=None):
        loader = self.test_loader
        if dataset is not None:
            loader = DeviceLoader(*dataset.tensors, 32, False, self.device)
        predictions = []
        self.model.eval()
        with torch.no_grad():
            for inputs, _ in loader:
                predictions.extend(self.model(inputs).argmax(1).cpu().tolist())
        return predictions
