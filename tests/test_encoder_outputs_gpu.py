"""An Encoder called with output_hidden_states= / output_attentions= and Encoder.attention_rollout on the MI355X: reduced two-layer
ViT / AST encoders, both precisions, head_dim 64 (fused attention: the probabilities come from csrc/attn_probs.hip) and
head_dim 16 (materialised scores: copied out of the softmax buffer), at the native geometry and at another image size /
clip length.  References: the float64 restatements of tests/attn_probs_ref.py (its hidden states are pinned to the CPU oracle
in tests/test_attn_probs_cpu.py; here the last one goes through the final LayerNorm against oracle.vit_oracle.forward's
return_hidden sequence as well)."""
import functools

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import attn_probs_ref as R
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "split"]
HEADS = {"hd64": dict(hidden=128, heads=2, ff=256), "hd16": dict(hidden=64, heads=4, ff=128)}
LAYERS, BATCH = 2, 3
NATIVE = {"vit": 32, "ast": 96}          # image side (5 tokens) / frames (12 x 9 + 2 = 110 tokens)
OTHER = {"vit": 48, "ast": 66}           # 3 x 3 + 1 = 10 tokens through interpolate_pos_encoding / 12 x 6 + 2 = 74 through variable_length
NEW_SYMBOLS = ("eav_attn_probs", "eav_attn_probs_sp", "eav_rollout_step")
CASES = [(k, h, p) for k in ("vit", "ast") for h in HEADS for p in PRECISIONS]


def _ocfg(kind, heads):
    from oracle import vit_oracle as vo
    kw = dict(HEADS[heads], layers=LAYERS)
    return vo.cfg_vit(**kw, image=NATIVE["vit"]) if kind == "vit" else vo.cfg_ast(**kw, frames=NATIVE["ast"])


@functools.lru_cache(maxsize=None)
def _weights(kind, heads):
    from oracle import vit_oracle as vo
    W = tf_weights(77, vo.param_shapes(_ocfg(kind, heads)), std=0.08)
    for v in W.values():
        v.setflags(write=False)
    return W


def _input(kind, size, seed=9):
    return (synth.frame_batch(seed, BATCH, size) if kind == "vit" else synth.mel_batch(seed, BATCH, size))[0]


def _model(kind, heads, precision, **cfg_kw):
    from eav_amd import transformer as T
    size = dict(image=NATIVE["vit"]) if kind == "vit" else dict(frames=NATIVE["ast"])
    model = T.Encoder(T.make_config(kind, **HEADS[heads], layers=LAYERS, **size, **cfg_kw),
                      {k: v.copy() for k, v in _weights(kind, heads).items()}).cuda().eval()
    model.precision = precision
    return model


@functools.lru_cache(maxsize=None)
def _reference(kind, heads):
    """(float64 hidden states, final sequence) of the native geometry - computed once, shared, never written."""
    hs, last = R.hidden_states(_weights(kind, heads), _input(kind, NATIVE[kind]), _ocfg(kind, heads))
    for a in hs + [last]:
        a.setflags(write=False)
    return hs, last


def _forward(model, kind, size, **kw):
    x = torch.from_numpy(_input(kind, size)).cuda()
    if size != NATIVE[kind]:
        if kind == "vit":
            kw["interpolate_pos_encoding"] = True
        else:
            model.variable_length = True
    with torch.no_grad():
        out = model(x, **kw)
    torch.cuda.synchronize()
    return out


def _ntok(kind, size):
    return (size // 16) ** 2 + 1 if kind == "vit" else 12 * ((size - 16) // 10 + 1) + 2


def hidden_figures(kind, heads, precision):
    """max |hidden_states[i] - float64| / max|float64| per entry, at the native geometry."""
    out = _forward(_model(kind, heads, precision), kind, NATIVE[kind], output_hidden_states=True)
    ref, _ = _reference(kind, heads)
    return [float(np.abs(h.cpu().double().numpy() - r).max() / np.abs(r).max()) for h, r in zip(out.hidden_states, ref)]


def attention_figures(kind, heads, precision, size):
    """Per layer (max |err| where the reference is below 1e-6, max |err| / P elsewhere, max |rowsum - 1|) of attentions[i]
    against the float64 restatement from the model's own hidden_states[i]."""
    out = _forward(_model(kind, heads, precision), kind, size, output_hidden_states=True, output_attentions=True)
    figs = []
    for i, a in enumerate(out.attentions):
        ref = R.layer_probs(_weights(kind, heads), _ocfg(kind, heads), i, out.hidden_states[i].cpu().double().numpy())
        got = a.cpu().double().numpy()
        figs.append((*R.split_errors(got, ref), float(np.abs(got.sum(-1) - 1.0).max())))
    return figs


@pytest.mark.parametrize("kind,heads,precision", CASES)
def test_hidden_states_match_the_reference(kind, heads, precision):
    from oracle import vit_oracle as vo
    c = _ocfg(kind, heads)
    out = _forward(_model(kind, heads, precision), kind, NATIVE[kind], output_hidden_states=True)
    assert out.attentions is None and len(out.hidden_states) == LAYERS + 1
    ref, last = _reference(kind, heads)
    for i, (h, r) in enumerate(zip(out.hidden_states, ref)):
        assert tuple(h.shape) == (BATCH, c["ntok"], c["hidden"]) and h.dtype == torch.float32 and not h.requires_grad
        err = np.abs(h.cpu().double().numpy() - r).max() / np.abs(r).max()
        print(kind, heads, precision, "hidden", i, err)
        assert err <= R.HIDDEN_BOUND[precision], (i, err)
    # the last one is BEFORE the final LayerNorm: through it, it is the oracle's return_hidden sequence
    W = _weights(kind, heads)
    with torch.no_grad():
        _, seq = vo.forward({k: torch.from_numpy(v.copy()) for k, v in W.items()},
                            torch.from_numpy(_input(kind, NATIVE[kind])), c, return_hidden=True)
    p = c["prefix"]
    normed = R._ln(out.hidden_states[-1].cpu().double().numpy(), W[f"{p}.layernorm.weight"].astype(np.float64),
                   W[f"{p}.layernorm.bias"].astype(np.float64), c["eps"])
    # (the oracle is fp32: 1e-5 of max|ref| is its own distance from float64, test_attn_probs_cpu)
    assert np.abs(normed - seq.double().numpy()).max() <= (R.HIDDEN_BOUND[precision] + 1e-5) * np.abs(last).max()
    # elsewhere the oracle has no resampling: shapes only
    other = _forward(_model(kind, heads, precision), kind, OTHER[kind], output_hidden_states=True)
    assert [tuple(h.shape) for h in other.hidden_states] == [(BATCH, _ntok(kind, OTHER[kind]), c["hidden"])] * (LAYERS + 1)
    assert all(bool(torch.isfinite(h).all()) for h in other.hidden_states)


@pytest.mark.parametrize("size", ["native", "other"])
@pytest.mark.parametrize("kind,heads,precision", CASES)
def test_attentions_match_the_restatement_layer_by_layer(kind, heads, precision, size):
    c = _ocfg(kind, heads)
    sz = NATIVE[kind] if size == "native" else OTHER[kind]
    N = _ntok(kind, sz)
    out = _forward(_model(kind, heads, precision), kind, sz, output_hidden_states=True, output_attentions=True)
    assert len(out.attentions) == LAYERS
    for i, a in enumerate(out.attentions):
        assert tuple(a.shape) == (BATCH, c["heads"], N, N) and a.dtype == torch.float32 and not a.requires_grad
        ref = R.layer_probs(_weights(kind, heads), c, i, out.hidden_states[i].cpu().double().numpy())
        got = a.cpu().double().numpy()
        err = np.abs(got - ref)
        print(kind, heads, precision, sz, "layer", i, R.split_errors(got, ref), np.abs(got.sum(-1) - 1.0).max())
        assert np.isfinite(got).all() and (got >= 0).all()
        assert (err <= R.error_bounds(ref, precision, R.ENCODER_BOUNDS)).all(), (i, err.max())
        assert np.abs(got.sum(-1) - 1.0).max() <= R.BOUNDS[precision][2]


def _trace(model):
    """Record the names that pass through Encoder._call."""
    names, inner = [], model._call

    def call(name, *args):
        names.append(name)
        inner(name, *args)
    model._call = call
    return names


@pytest.mark.parametrize("kind,heads,precision", CASES)
def test_nothing_changes_with_the_flags_off(kind, heads, precision):
    model = _model(kind, heads, precision)
    _forward(model, kind, NATIVE[kind])                                   # (first forward: builds the weight planes)
    names = _trace(model)
    off = _forward(model, kind, NATIVE[kind])
    seq_off = list(names)
    del names[:]
    on = _forward(model, kind, NATIVE[kind], output_hidden_states=True, output_attentions=True)
    seq_on = list(names)
    assert off.hidden_states is None and off.attentions is None
    assert torch.equal(on.logits, off.logits)
    assert not set(seq_off) & set(NEW_SYMBOLS)
    assert [n for n in seq_on if n not in NEW_SYMBOLS] == seq_off
    new = [n for n in seq_on if n in NEW_SYMBOLS]
    want = {"hd16": [], "hd64": ["eav_attn_probs_sp" if precision == "split" else "eav_attn_probs"] * LAYERS}[heads]
    assert new == want
    # the attributes are the defaults of the arguments
    model.output_attentions = model.output_hidden_states = True
    dflt = _forward(model, kind, NATIVE[kind])
    assert all(torch.equal(a, b) for a, b in zip(dflt.attentions, on.attentions))
    assert all(torch.equal(a, b) for a, b in zip(dflt.hidden_states, on.hidden_states))
    assert _forward(model, kind, NATIVE[kind], output_attentions=False).attentions is None
    # fresh allocations: a later forward leaves the earlier results alone
    kept = [h.clone() for h in on.hidden_states]
    x2 = torch.from_numpy(_input(kind, NATIVE[kind], seed=10)).cuda()
    with torch.no_grad():
        other = model(x2)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kept, on.hidden_states))
    assert not torch.equal(other.hidden_states[0], on.hidden_states[0])
    assert other.hidden_states[0].data_ptr() != on.hidden_states[0].data_ptr()


@pytest.mark.parametrize("kind,heads,precision", CASES)
def test_training_step_is_bit_equal_with_the_flags_on(kind, heads, precision):
    from eav_amd.optim import CrossEntropyLoss
    model = _model(kind, heads, precision).train()
    x = torch.from_numpy(_input(kind, NATIVE[kind])).cuda()
    y = torch.from_numpy(synth.labels(4, BATCH)).cuda()

    def step(**kw):
        for p in model.parameters():
            p.grad = None
        out = model(x, **kw)
        CrossEntropyLoss()(out.logits, y).backward()
        torch.cuda.synchronize()
        return out, {k: p.grad.clone() for k, p in model.named_parameters()}

    step()
    off, g_off = step()
    on, g_on = step(output_hidden_states=True, output_attentions=True)
    assert torch.equal(on.logits, off.logits)
    assert sorted(g_on) == sorted(g_off) and all(torch.equal(g_on[k], g_off[k]) for k in g_off)
    assert all(not t.requires_grad and t.grad_fn is None for t in on.hidden_states + on.attentions)
    assert len(on.hidden_states) == LAYERS + 1 and len(on.attentions) == LAYERS
    # ... and they are what the eval forward returns (no dropout in this configuration)
    ev = _forward(model.eval(), kind, NATIVE[kind], output_hidden_states=True, output_attentions=True)
    assert all(torch.equal(a, b) for a, b in zip(ev.attentions, on.attentions))
    assert all(torch.equal(a, b) for a, b in zip(ev.hidden_states, on.hidden_states))


@pytest.mark.parametrize("size", ["native", "other"])
@pytest.mark.parametrize("kind,heads,precision", CASES)
def test_rollout_is_the_recursion_over_the_returned_attentions(kind, heads, precision, size):
    sz = NATIVE[kind] if size == "native" else OTHER[kind]
    model = _model(kind, heads, precision).train()                       # (rollout runs in eval mode and restores the mode)
    out = _forward(model, kind, sz, output_attentions=True)
    x = torch.from_numpy(_input(kind, sz)).cuda()
    names = _trace(model)
    roll = model.attention_rollout(x, interpolate_pos_encoding=True if (kind == "vit" and sz != NATIVE[kind]) else None)
    grid = model.attention_rollout(x, as_grid=True,
                                   interpolate_pos_encoding=True if (kind == "vit" and sz != NATIVE[kind]) else None)
    torch.cuda.synchronize()
    assert model.training and not roll.requires_grad
    N, nextra = _ntok(kind, sz), 1 if kind == "vit" else 2
    assert tuple(roll.shape) == (BATCH, N)
    ref = R.rollout([a.cpu().double().numpy() for a in out.attentions], nextra)
    # LAYERS steps, each within rollout_step_bound (<= (N + 2) 2^-24 of a value <= 1) and fed a head mean within the kernels'
    # bound atol + rtol P <= atol + rtol of the float64 one (twice: the returned probabilities and the means come from
    # different launches; r sums to 1, so the mean's error enters once), the pair mean one rounding
    tol = LAYERS * ((N + 2) * 2.0 ** -24 + 2 * (R.BOUNDS[precision][0] + R.BOUNDS[precision][1])) + 2.0 ** -24
    got = roll.cpu().double().numpy()
    print(kind, heads, precision, sz, "rollout err", np.abs(got - ref).max(), "rowsum", np.abs(got.sum(-1) - 1.0).max())
    assert np.abs(got - ref).max() <= tol
    assert np.abs(got.sum(-1) - 1.0).max() <= LAYERS * R.BOUNDS[precision][2] + N * tol
    gy, gx = (sz // 16, sz // 16) if kind == "vit" else (12, (sz - 16) // 10 + 1)
    assert tuple(grid.shape) == (BATCH, gy, gx) and torch.equal(grid.reshape(BATCH, -1), roll[:, nextra:])
    assert names.count("eav_rollout_step") == 2 * LAYERS
    if heads == "hd64":       # the head mean comes straight from the kernel: no [B, H, N, N] buffer
        assert names.count("eav_attn_probs_sp" if precision == "split" else "eav_attn_probs") == 2 * LAYERS


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(precision):
    model = _model("vit", "hd64", precision, attention_dropout=0.1)
    x = torch.from_numpy(_input("vit", NATIVE["vit"])).cuda()
    with pytest.raises(NotImplementedError, match="attention_probs_dropout_prob"):
        model.train()(x, output_attentions=True)
    model.train()(x, output_hidden_states=True)                      # hidden states alone are served
    with torch.no_grad():
        assert model.eval()(x, output_attentions=True).attentions is not None     # and eval mode drops nothing
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = x + 0.0                                             # (so that the capture is not empty)
        with pytest.raises(NotImplementedError, match="capturing"):
            model(x, output_attentions=True)
        with pytest.raises(NotImplementedError, match="capturing"):
            model(x, output_hidden_states=True)
        with pytest.raises(NotImplementedError, match="capturing"):
            model.attention_rollout(x)
    del static
