"""What the kernel-backed models and their trainers share on the host.

    KernelModule     base class of EEGNet_tor, cnn_eeg.EEGNet, ShallowConvNet, AudioModel, VideoModel and
                     transformer.Encoder: flat parameter storage and the gradient views a backward returns, the workspace
                     cache, the device checks, the one-outstanding-forward guard, the dropout set-up of a forward, the
                     BatchNorm launches the convolutional models share, and what GraphStep asks of a model
    KernelFn         the autograd bridge of all of them
    cached_workspace / gather_batch / DeviceLoader / GraphStep / eager_step   the device-resident training loop
    train_step       the graph-or-eager step of every trainer

Imports _lib and optim only, never a model module.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .optim import flatten_parameters, unit_gradient

# A BatchNorm parameter block of n channels: six fields of n floats each, in the order the kernels take them
# (include/eav_hip.h: "mean, invstd, scale, shift, m1, m2"; m1 / m2 are the two means of the backward).
BN_MEAN, BN_INVSTD, BN_SCALE, BN_SHIFT, BN_M1, BN_M2 = range(6)


def bn_field(buf, n, k):
    """Device address of field k (BN_*) of the n-channel BatchNorm parameter block `buf`."""
    return buf.data_ptr() + 4 * n * k


def cached_workspace(cache, key, make, keep_unpinned=2):
    """Workspace cache of a KernelModule.  A captured hipGraph (GraphStep) has the raw device pointers of the
    workspace it was captured with baked in, so THOSE workspaces (marked `pinned` by GraphStep after capture) live as long
    as the model; eager sizes - ragged last batches, validation, user-chosen inference batches - share `keep_unpinned`
    replaceable slots (most recently used first), so varying batch sizes do not accumulate multi-GB workspaces."""
    ws = cache.get(key)
    if ws is None:
        if not torch.cuda.is_current_stream_capturing():
            loose = [k for k, w in cache.items() if not getattr(w, "pinned", False)]
            for k in loose[:max(0, len(loose) - (keep_unpinned - 1))]:     # dict order = insertion / last-use order
                del cache[k]
        ws = make()
    else:
        del cache[key]          # re-insert: most recently used last
    cache[key] = ws
    return ws


def gather_batch(xs, ys, idx_dev):
    """(xs[idx], ys[idx]) assembled in HBM by the library's gather kernels (eav_gather_rows / eav_gather_i64)."""
    n = idx_dev.numel()
    if not xs.is_cuda:   # host tensors (CPU-side unit tests of the loader only)
        return xs.index_select(0, idx_dev), ys.index_select(0, idx_dev)
    data = torch.empty((n,) + tuple(xs.shape[1:]), dtype=torch.float32, device=xs.device)
    _lib.call("eav_gather_rows", xs.data_ptr(), idx_dev.data_ptr(), data.data_ptr(), n, xs[0].numel(), _lib.stream_ptr())
    return data, gather_labels(ys, idx_dev)


def gather_labels(ys, idx_dev):
    """ys[idx] in HBM: int64 class indices [N] through eav_gather_i64, fp32 label rows [N] / [N, NC] (regression and
    multi-label targets, DeviceLoader(label_dtype=torch.float32)) through eav_gather_rows."""
    n = idx_dev.numel()
    out = torch.empty((n,) + tuple(ys.shape[1:]), dtype=ys.dtype, device=ys.device)
    if ys.dtype == torch.float32:
        _lib.call("eav_gather_rows", ys.data_ptr(), idx_dev.data_ptr(), out.data_ptr(), n, ys[0].numel(), _lib.stream_ptr())
    else:
        _lib.call("eav_gather_i64", ys.data_ptr(), idx_dev.data_ptr(), out.data_ptr(), n, _lib.stream_ptr())
    return out


class KernelFn(torch.autograd.Function):
    """forward(x) / backward(d) of a model whose arithmetic is kernel launches: `model._launch_forward(x)` returns a token,
    `model._forward_output()` the tensor handed to autograd, `model._launch_backward(d, token)` the parameter gradients."""

    @staticmethod
    def forward(ctx, x, model, *params):
        ctx.model = model
        ctx.token = model._launch_forward(x)
        return model._forward_output()

    @staticmethod
    def backward(ctx, dout):
        return (None, None, *ctx.model._launch_backward(dout.contiguous(), ctx.token))


class KernelModule(nn.Module):
    """An nn.Module that drives libeav_hip.so: its parameters are views of one flat buffer (`_flat`), its activations live
    in per-problem-size workspaces (`_wss`, the current one in `_ws`), and one forward at a time may await its backward
    (`_token` / `_saved`).  A subclass provides `_launch_forward(x) -> token` and `_launch_backward(dout, token)`."""

    _PARAM_ORDER = None        # the named_parameters() order the kernels' argument lists assume (asserted when flattening)
    _OUTPUT = "logits"         # the workspace tensor a forward returns a clone of

    def __init__(self):
        super().__init__()
        self._ws = None
        self._wss = {}                 # workspaces by problem size and device: see _workspace()
        self._flat = None              # (flat parameters, flat gradients, {name: (offset, numel)})
        self._token = 0
        self._saved = None
        self._fwd_counter = None       # device int64: number of training forwards (dropout stream)
        self._dropout_masks = None     # tests: explicit uint8 keep-masks

    # ------------------------------------------------------------------ parameters
    def _pad_after(self):
        """{parameter name: zero floats to leave after it in the flat buffers} (flatten_parameters)."""
        return None

    def _ensure_flat(self):
        p0 = next(self.parameters())
        if self._flat is None or self._flat[0].device != p0.device or getattr(p0, "_eav_flat", None) is None \
                or p0.data_ptr() != self._flat[0].data_ptr():
            self._names = [n for n, _ in self.named_parameters()]
            assert self._PARAM_ORDER is None or self._names == self._PARAM_ORDER, self._names
            self._flat = flatten_parameters(self, pad_after=self._pad_after())

    def _params(self):
        """The parameters in the order of the autograd bridge's gradients: named_parameters() order (= _PARAM_ORDER)."""
        return list(self.parameters())

    def _grad_views(self):
        """{parameter name: its 1-D view of the flat gradient buffer}."""
        gflat, offs = self._flat[1], self._flat[2]
        return {k: gflat[offs[k][0]:offs[k][0] + offs[k][1]] for k in self._names}

    def _grads_out(self, views):
        """What a backward hands to autograd: the views in the parameters' shapes, None where requires_grad is off."""
        named = dict(self.named_parameters())
        return [views[k].view(named[k].shape) if named[k].requires_grad else None for k in self._names]

    def set_dropout_masks(self, masks):
        """Testing hook: explicit uint8 keep-masks instead of the counter-based generator; None restores the generator."""
        self._dropout_masks = masks

    def _counter(self, dev):
        """The device-resident count of training forwards on `dev` (the dropout stream: no host argument changes from
        step to step, so a captured step draws fresh masks on every replay).  The caller launches the increment."""
        if self._fwd_counter is None or self._fwd_counter.device != dev:
            self._fwd_counter = torch.zeros((), dtype=torch.int64, device=dev)
        return self._fwd_counter

    def _dropout(self, dev, active, check=None):
        """(counter pointer, mk) of a forward: mk(i) is the pointer of the i-th explicit keep-mask, which a training-mode
        forward uses when set (`check(masks)` validates them first), else None; the counter pointer is that of _counter()
        when a rate is `active` and the generator draws the masks, else None."""
        masks = self._dropout_masks if self.training else None
        if masks is not None:
            masks = list(masks if check is None else check(masks))
        cnt = _lib.ptr(self._counter(dev)) if active and masks is None else None
        return cnt, (lambda i: None if masks is None else masks[i].data_ptr())

    # ------------------------------------------------------------------ BatchNorm launches
    def _bn_finalize(self, bn, part, nparts, count, buf, training):
        """Partial sums of `count` values per channel -> mean, invstd, scale, shift in buf[0:4n] and bn's running statistics
        (eval mode: scale / shift from the running statistics).  num_batches_tracked is the caller's."""
        n = bn.num_features
        _lib.call("eav_bn_finalize", _lib.ptr(part), nparts, n, float(count), _lib.ptr(bn.weight), _lib.ptr(bn.bias),
                  _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), int(training), float(bn.momentum), float(bn.eps),
                  *(bn_field(buf, n, k) for k in (BN_MEAN, BN_INVSTD, BN_SCALE, BN_SHIFT)), _lib.stream_ptr())

    def _bn_elu_pool_bwd(self, dy, z, dz, buf, part, gw, gb, B, nch, T, pool, dropout, training):
        """Backward of z [B,nch,T] -> BatchNorm (buf) -> ELU -> AvgPool(pool) -> Dropout from dy: BatchNorm's gradients to
        gw / gb, its two backward means to buf[4n:6n], d z to dz.  dropout = (rate, seed, mask pointer, counter pointer) of
        the forward; dz = None stops after the means (the next kernel forms d z itself)."""
        L, P, st, b = _lib.call, _lib.ptr, _lib.stream_ptr(), _lib.ptr(buf)
        m1, m2 = bn_field(buf, nch, BN_M1), bn_field(buf, nch, BN_M2)
        L("eav_bn_elu_pool_bwd_reduce", P(dy), P(z), b, P(part), B, nch, T, pool, *dropout, st)
        L("eav_bn_bwd_finalize", P(part), B, nch, float(B * T), int(training), P(gw), P(gb), m1, m2, st)
        if dz is not None:
            L("eav_bn_elu_pool_bwd_apply", P(dy), P(z), b, m1, P(dz), B, nch, T, pool, *dropout, st)

    # ------------------------------------------------------------------ checks
    def _require_gpu(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.EavError(f"eav_amd.{type(self).__name__} runs on an MI355X only: move the model and the input to "
                                "the ROCm device (there is no CPU fallback)")

    def _require_same_device(self, x):
        if next(self.parameters()).device != x.device:
            raise _lib.EavError("model and input are on different devices")

    def _check_token(self, token):
        if self._saved is None or self._saved[0] != token:
            raise _lib.EavError(f"{type(self).__name__}.backward: the activations of this forward were overwritten by a "
                                "later forward (one outstanding forward per backward)")

    # ------------------------------------------------------------------ workspaces
    def _workspace(self, key, make, keep_unpinned=2):
        """One workspace per problem size; the ones a hipGraph was captured with are pinned for the life of the model,
        the others share a small replaceable set (cached_workspace)."""
        self._ws = cached_workspace(self._wss, key, make, keep_unpinned)
        return self._ws

    def _forward_output(self):
        return getattr(self._ws, self._OUTPUT).clone()

    # ------------------------------------------------------------------ what GraphStep asks of a model
    def forward_batch(self, xs, ys, idx, optimizer):
        """(scores, targets) of the samples `idx` (device int64) of the device-resident data set (xs, ys)."""
        data, targets = gather_batch(xs, ys, idx)
        return self(data), targets

    def refresh_batch_tables(self, xs):
        """GraphStep.run saw the data set `xs` change (xs._version): a model that keeps anything derived from it rebuilds
        that IN PLACE - a captured step holds the pointers.  (EEGNet_tor: the InputTables of its FFT weight gradient.)"""

    def _pin_workspace(self):
        """A hipGraph was just captured over the current workspace and holds its raw pointers (cached_workspace)."""
        if self._ws is not None:
            self._ws.pinned = True


def eager_step(model, optimizer, criterion, data, targets, grad_sync=None, post_step=None):
    """One training step outside a hipGraph (the ragged last batch of an epoch, or a trainer with use_graph off):
    forward, loss, backward, [grad sync], optimiser step, [post_step].  Returns detached (scores, loss)."""
    scores = model(data)
    loss = criterion(scores, targets)
    optimizer.zero_grad()
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    optimizer.step()
    if post_step is not None:
        post_step()
    # drop the eager step's autograd graph now: its AccumulateGrad nodes, kept alive into the next
    # GraphStep capture, would tie that capture to this stream
    return scores.detach(), loss.detach()


def train_step(graphs, model, optimizer, criterion, loader, idx, use_graph, grad_sync=None, post_step=None,
               eager_input=None):
    """One training step on the samples `idx` of a DeviceLoader.  A full-size batch with `use_graph` on runs the GraphStep
    of its (batch size, BN mode), built in `graphs` (the caller's dict) on first use; any other batch is gathered and runs
    eager_step, the model being fed `eager_input(data)` where given.  Returns detached (scores, loss, targets): targets are
    the gathered labels of an eager step, None after a GraphStep (which gathers its own inside the graph)."""
    if use_graph and len(idx) == loader.batch_size:
        key = (len(idx), bool(model.training))
        if key not in graphs:
            graphs[key] = GraphStep(model, optimizer, criterion, loader.x, loader.y, len(idx), grad_sync, post_step)
        return (*graphs[key].run(idx), None)
    data, targets = loader.gather(idx)
    if eager_input is not None:
        data = eager_input(data)
    return (*eager_step(model, optimizer, criterion, data, targets, grad_sync, post_step), targets)


class GraphStep:
    """One training step of a KernelModule (batch gather, forward, CE, backward, [grad sync], fused Adam) captured in a
    hipGraph and replayed: at the reference's own shape ([32,1,30,500]) the step is ~35 tiny kernels and is
    bound by launch overhead, not by the GPU.  Everything that varies between steps lives in device memory
    (batch indices, dropout counter, Adam step count), so a replay needs no host-side argument updates."""

    def __init__(self, model, optimizer, criterion, xs, ys, batch, grad_sync=None, post_step=None):
        if not getattr(optimizer, "capturable", False):
            raise _lib.EavError("GraphStep needs FusedAdam(capturable=True)")
        if not isinstance(model, KernelModule):
            raise _lib.EavError("GraphStep needs a KernelModule")
        self.model, self.batch, self.grad_sync = model, batch, grad_sync
        self.idx = torch.zeros(batch, dtype=torch.long, device=xs.device)
        # The data set is assumed to stay put; what a model derives from it once (KernelModule.refresh_batch_tables) follows
        # in-place torch writes through the version counter.  Writes torch does not see (a raw kernel, a DLPack alias) need
        # the model's own refresh (EEGNet_tor.refresh_input_tables).
        self.xs, self._xs_version = xs, xs._version

        def compute():       # batch gather + forward + loss + backward
            scores, targets = model.forward_batch(xs, ys, self.idx, optimizer)
            loss = criterion(scores, targets)
            optimizer.zero_grad(set_to_none=True)
            loss.backward(gradient=unit_gradient(loss.device))      # no ones_like fill, no scaling launch
            return scores, loss

        def update():        # fused Adam (+ e.g. the max-norm projection of Transformer_EEG.py:195-199)
            optimizer.step()
            if post_step is not None:
                post_step()

        self.warm_steps = 0
        self.graph = None          # compute (and, without a grad_sync, update) graph
        self.graph_update = None   # data parallel: the update is its own graph, the all-reduce runs between the two
        self._compute, self._update = compute, update

    def _eager(self):
        scores, loss = self._compute()
        if self.grad_sync is not None:
            self.grad_sync()
        self._update()
        return scores, loss

    def run(self, idx):
        """idx: sequence of `batch` dataset indices.  The first two calls run eagerly (they are real training
        steps), the third is captured, later ones are replays.  Under data parallelism (grad_sync) the collective is
        not captured: replay(compute) -> all-reduce on the live stream -> replay(update)."""
        self.idx.copy_(torch.as_tensor(idx, dtype=torch.long))     # pageable source: staged, no host race
        if self.xs._version != self._xs_version:
            self._xs_version = self.xs._version
            self.model.refresh_batch_tables(self.xs)
        if self.graph is None:
            if self.warm_steps < 2:
                self.warm_steps += 1
                scores, loss = self._eager()
                return scores.detach(), loss.detach()     # keep no reference to the autograd graph
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                scores, loss = self._compute()
                self.scores, self.loss = scores.detach(), loss.detach()
                if self.grad_sync is None:
                    self._update()
            del scores, loss
            self.model._pin_workspace()
            if self.grad_sync is not None:
                # the gradients the update graph reads live in the model's flat buffer (static address); capture the
                # update on its own (its launches are recorded, not executed)
                self.graph_update = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_update, pool=self.graph.pool()):
                    self._update()
            # capture does not execute: fall through to a replay so that this call is a real step too
        self.graph.replay()
        if self.grad_sync is not None:
            self.grad_sync()
            self.graph_update.replay()
        return self.scores, self.loss


# ----------------------------------------------------------------------------- data plumbing
class DeviceLoader:
    """DataLoader-shaped iterator over a device-resident TensorDataset.

    The reference builds ``DataLoader(TensorDataset(x, y), batch_size, shuffle)`` on
    the host and copies every batch to the device inside the loop
    (EEGNet_tor.py:91-94,100-101).  Here the whole split lives in HBM once and a
    batch is assembled by one gather; the *index order* is produced by the same
    torch samplers (RandomSampler / SequentialSampler + BatchSampler), consuming
    the torch RNG exactly as ``iter(DataLoader)`` does, so a seeded run visits
    the same batches as the reference.

    label_dtype: torch.long (default) keeps class indices [N]; torch.float32 keeps regression / multi-label targets as
    fp32 [N] or [N, NC], gathered by rows.
    """

    def __init__(self, x, y, batch_size, shuffle, device, label_dtype=torch.long):
        from torch.utils.data import TensorDataset
        if label_dtype not in (torch.long, torch.float32):
            raise ValueError(f"DeviceLoader: label_dtype must be torch.long or torch.float32, not {label_dtype}")
        self.x = torch.as_tensor(x, dtype=torch.float32).to(device).contiguous()
        self.y = torch.as_tensor(y, dtype=label_dtype).to(device).contiguous()
        if label_dtype == torch.float32 and self.y.dim() not in (1, 2):
            raise ValueError(f"DeviceLoader: labels of shape {tuple(self.y.shape)}")
        self.dataset = TensorDataset(self.x, self.y)
        self.batch_size, self.shuffle, self.device = batch_size, shuffle, device
        self.order_override = None  # tests: list of index arrays, one per epoch

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def index_batches(self):
        """The index lists iter(DataLoader) would visit (same samplers, same torch RNG consumption)."""
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        n = len(self.dataset)
        # iter(DataLoader) draws its base seed first (torch/utils/data/dataloader.py, _BaseDataLoaderIter)
        torch.empty((), dtype=torch.int64).random_()
        if self.order_override:
            order = [int(i) for i in self.order_override.pop(0)]
            return [order[i:i + self.batch_size] for i in range(0, n, self.batch_size)]
        sampler = RandomSampler(range(n)) if self.shuffle else SequentialSampler(range(n))
        return list(BatchSampler(sampler, self.batch_size, drop_last=False))

    def gather(self, idx):
        if idx[-1] - idx[0] == len(idx) - 1 and all(b - a == 1 for a, b in zip(idx, idx[1:])):
            return self.x[idx[0]:idx[-1] + 1], self.y[idx[0]:idx[-1] + 1]
        return gather_batch(self.x, self.y, torch.as_tensor(idx, dtype=torch.long, device=self.device))

    def gather_labels(self, idx):
        """The labels of a batch only (a step that already holds the batch's features needs no copy of x)."""
        if idx[-1] - idx[0] == len(idx) - 1 and all(b - a == 1 for a, b in zip(idx, idx[1:])):
            return self.y[idx[0]:idx[-1] + 1]
        i = torch.as_tensor(idx, dtype=torch.long, device=self.device)
        if not self.y.is_cuda:   # host tensors (CPU-side unit tests of the loader only)
            return self.y.index_select(0, i)
        return gather_labels(self.y, i)

    def __iter__(self):
        for idx in self.index_batches():
            yield self.gather(idx)
