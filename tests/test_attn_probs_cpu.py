"""The float64 restatement behind the output_attentions / attention_rollout tests (tests/attn_probs_ref.py), pinned without a
GPU: against torch.softmax in float64, the rollout on cases that can be checked by hand, the hidden-state restatement against
the CPU oracle, the new keywords and fields, and a negative control of the element-wise bound."""
import inspect

import numpy as np
import pytest
import torch

from tests import attn_probs_ref as R

SCALE = R.HD ** -0.5


@pytest.mark.parametrize("N", [1, 33, 197])
def test_restatement_is_torch_softmax_in_float64(N):
    qkv = R.inputs(R.SEEDS[0], N)
    x = torch.from_numpy(qkv).double().view(R.B, N, 3, R.H, R.HD)
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)                    # [B, H, N, hd]
    ref = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * SCALE, dim=-1).numpy()
    got = R.probs(qkv, R.B, R.H, N, SCALE)
    assert got.shape == (R.B, R.H, N, N)
    assert np.abs(got - ref).max() <= 1e-14 and np.abs(got.sum(-1) - 1.0).max() <= 1e-14
    assert np.abs(R.head_mean(got) - ref.mean(1)).max() <= 1e-15
    if N > 1:       # the hostile rows: near one-hot, and a row most of whose other probabilities underflow in fp32
        assert got[:, :, 0, N - 1].min() > 0.5
        others = np.delete(got[:, :, N // 2], 0, axis=-1)
        assert np.median(others, -1).max() < 2.0 ** -126 and got[:, :, N // 2, 0].min() > 1.0 - 1e-12


def test_rollout_of_identity_attention_is_the_readout_token():
    N, L = 7, 3
    eye = np.broadcast_to(np.eye(N), (2, 4, N, N))
    for nextra in (1, 2):
        r = R.rollout([eye] * L, nextra)
        want = np.zeros((2, N))
        want[:, :nextra] = 1.0 / nextra                    # (0.5 I + 0.5 I)^L = I; the mean of e_0 .. e_{nextra-1}
        assert np.array_equal(r, want)


def test_rollout_of_uniform_attention_has_a_closed_form():
    """A = U = 1 1^T / N in every layer.  U U = U, so with M = (I + U) / 2:  M^L = 2^-L sum_j C(L, j) U^j = 2^-L (I + (2^L - 1) U)
    (binomial theorem, U^j = U for j >= 1).  Row e_0 of it: 2^-L e_0 + (1 - 2^-L) / N everywhere."""
    N, L = 9, 4
    U = np.full((3, 2, N, N), 1.0 / N)
    r = R.rollout([U] * L, 1)
    want = np.full((3, N), (1.0 - 2.0 ** -L) / N)
    want[:, 0] += 2.0 ** -L
    assert np.abs(r - want).max() <= 1e-15 and np.abs(r.sum(-1) - 1.0).max() <= 1e-15
    # one step, by hand: e_0 -> 0.5 / N + 0.5 e_0
    one = R.rollout_step(np.eye(N)[None, :1], U[:1, 0])
    assert np.abs(one[0, 0] - (0.5 / N + 0.5 * np.eye(N)[0])).max() <= 1e-16


@pytest.mark.parametrize("kind", ["vit", "ast"])
def test_hidden_state_restatement_matches_the_oracle(kind):
    """hidden_states()'s last entry through the final LayerNorm is the sequence oracle.vit_oracle.forward returns with
    return_hidden=True (fp32 against float64: 1e-5 of max|ref|)."""
    from eav_amd import synth
    from oracle import vit_oracle as vo
    from tests.golden_util import tf_weights
    kw = dict(hidden=64, layers=2, heads=4, ff=128)
    if kind == "vit":
        ocfg = vo.cfg_vit(**kw, image=32)
        x = synth.frame_batch(5, 2, 32)[0]
    else:
        ocfg = vo.cfg_ast(**kw, frames=96)
        x = synth.mel_batch(5, 2, 96)[0]
    W = tf_weights(31, vo.param_shapes(ocfg), std=0.08)
    with torch.no_grad():
        _, seq = vo.forward({k: torch.from_numpy(v.copy()) for k, v in W.items()}, torch.from_numpy(x), ocfg,
                            return_hidden=True)
    hs, last = R.hidden_states(W, x, ocfg)
    assert len(hs) == ocfg["layers"] + 1 and all(h.shape == (2, ocfg["ntok"], 64) for h in hs)
    assert np.abs(last - seq.double().numpy()).max() <= 1e-5 * np.abs(last).max()
    a = R.layer_probs(W, ocfg, 1, hs[1])
    assert a.shape == (2, 4, ocfg["ntok"], ocfg["ntok"]) and np.abs(a.sum(-1) - 1.0).max() <= 1e-14


def test_forward_takes_the_keywords_and_out_has_the_fields():
    from eav_amd import transformer as T
    # the two keywords belong to the call, model(x, output_attentions=...); forward()'s own parameter list is pinned elsewhere
    sig = inspect.signature(T.Encoder.__call__).parameters
    for name in ("output_attentions", "output_hidden_states"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    out = T._Out(torch.zeros(1))
    assert out.hidden_states is None and out.attentions is None and out.loss is None
    model = T.Encoder(T.make_config("vit", hidden=64, layers=1, heads=4, ff=128, image=32))
    assert model.output_attentions is False and model.output_hidden_states is False
    assert inspect.signature(T.Encoder.attention_rollout).parameters["as_grid"].default is False


def test_config_json_sets_the_defaults(tmp_path):
    import json
    from eav_amd import transformer as T
    model = T.Encoder(T.make_config("vit", hidden=64, layers=1, heads=4, ff=128, image=32))
    model.save_pretrained(tmp_path)
    assert T.Encoder.from_pretrained(tmp_path).output_attentions is False
    cfg = json.load(open(tmp_path / "config.json"))
    cfg.update(output_attentions=True, output_hidden_states=True)
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    again = T.Encoder.from_pretrained(tmp_path)
    assert again.output_attentions is True and again.output_hidden_states is True


@pytest.mark.parametrize("precision", ["fp32", "split"])
@pytest.mark.parametrize("N", [33, 197])
def test_the_bound_rejects_wrong_probabilities(precision, N):
    """Negative control: float64 probabilities from K rolled by one token, and from scale = 1, violate the bound on the test
    inputs; the reference itself, rounded to fp32, passes it."""
    qkv = R.inputs(R.SEEDS[0], N)
    ref = R.probs(qkv, R.B, R.H, N, SCALE)
    bound = R.error_bounds(ref, precision)
    assert (np.abs(ref.astype(np.float32).astype(np.float64) - ref) <= bound).all()
    x = qkv.reshape(R.B, N, 3, R.H, R.HD).copy()
    x[:, :, 1] = np.roll(x[:, :, 1], 1, axis=1)
    rolled = R.probs(x.reshape(qkv.shape), R.B, R.H, N, SCALE)
    unscaled = R.probs(qkv, R.B, R.H, N, 1.0)
    for wrong in (rolled, unscaled):
        assert (np.abs(wrong - ref) > bound).any()
        assert (np.abs(R.head_mean(wrong) - R.head_mean(ref)) > R.error_bounds(R.head_mean(ref), precision)).any()
