"""Dropout of the AST / ViT encoders on the MI355X (hidden_dropout_prob / attention_probs_dropout_prob of the HF config):
parity with the Hugging Face classes under explicit masks on both attention paths and in both precisions, the agreement of
the forward and backward kernels on the regenerated mask, the generator's statistics, eval / p = 0 invariance, the two
trainers and two data-parallel ranks."""
import io
import json
import os
import subprocess
import sys
import textwrap
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import encoder_dropout_ref as R
from tests.golden_util import tf_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ["fp32", "split"]


def close(got, ref, rtol, atol, what):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    print(f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}, bound {atol:.3e} + {rtol:.0e} |ref|")
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(ref).max():.3e}"


def _model(kind, precision, ph, pa, fused=True, model=None, wseed=None, std=R.STD):
    from eav_amd import transformer as T
    from oracle import vit_oracle as vo
    model = model or R.MODEL
    extra = {"frames": R.AST_FRAMES} if kind == "ast" else {}
    cfg = T.make_config(kind, hidden_dropout=ph, attention_dropout=pa, **model, **extra)
    ocfg = vo.cfg_ast(frames=R.AST_FRAMES, **model) if kind == "ast" else vo.cfg_vit(**model)
    W = tf_weights(R.WSEED[kind] if wseed is None else wseed, vo.param_shapes(ocfg), std=std)
    m = T.Encoder(cfg, W).cuda().train()
    m.precision = precision
    m.use_fused_attention = fused
    return m, cfg, ocfg, W


def _batch(kind, cfg, seed, B):
    x, y = synth.mel_batch(seed, B, cfg.W, cfg.H) if kind == "ast" else synth.frame_batch(seed, B, cfg.H)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def _cuda_masks(masks):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in masks.items()}


def _train_step(model, x, y):
    from eav_amd.optim import CrossEntropyLoss
    for p in model.parameters():
        p.grad = None
    out = model(x)
    loss = CrossEntropyLoss()(out.logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return out.logits.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


# ============================================================================================ golden parity
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "materialised"])
@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_training_steps_match_hf_under_explicit_masks(golden_dir, kind, precision, case, fused):
    """Cases a-c (hidden / attention 0.1 / 0.1, 0.0 / 0.3, 0.25 / 0.0) and the p = 0 control d of
    tests/golden/encoder_dropout_{kind}.npz: one unfrozen AdamW step, then one frozen step, masks through set_dropout_masks.
    Bounds: exactly those of test_reduced_model_training_steps_match_hf - logits and loss close(1e-4, 1e-4) (5e-4 on the frozen
    step), gradients rtol 1e-3 with atol 1e-3 (5e-3) of the tensor's maximum, that test's post-step rule - on the stored
    strided samples; max |.| under the same bound and sum |.| under what the element bound implies for a sum.  The control
    runs under the same bounds.  `fused`: the head_dim-64 fused attention kernels of the precision (attention.hip /
    attention_sp.hip, their DROP instantiations where the case has attention dropout); `materialised` forces the GEMM +
    softmax path."""
    from eav_amd.optim import FusedAdam
    g = np.load(os.path.join(golden_dir, f"encoder_dropout_{kind}.npz"))
    ph, pa = R.CASES[case]
    model, cfg, _, _ = _model(kind, precision, ph, pa, fused)
    lr = float(g["lr"])
    opt = FusedAdam(model.parameters(), lr=lr, weight_decay=0.01, decoupled=True)
    from eav_amd.optim import CrossEntropyLoss
    crit = CrossEntropyLoss()
    for s, freeze in enumerate((False, True)):
        x, y = _batch(kind, cfg, int(g["xseed"]) + s, int(g["B"]))
        model.set_dropout_masks(_cuda_masks(R.site_masks(int(g["mseed"]), s, int(g["B"]), cfg.ntok, cfg.hidden, cfg.heads,
                                                         cfg.layers, ph, pa)))
        for k, p in model.named_parameters():
            p.requires_grad = (not freeze) or k.startswith("classifier.")
        opt.zero_grad()
        out = model(x)
        loss = crit(out.logits, y)
        loss.backward()
        if s == 0:
            assert model._ws.fused == fused
        close(out.logits, g[f"{case}.logits{s}"], 1e-4, 1e-4 if s == 0 else 5e-4, f"{case}.logits{s}")
        close(loss, g[f"{case}.loss{s}"], 1e-4, 1e-4, f"{case}.loss{s}")
        named = dict(model.named_parameters())
        pre = f"{case}.grad{s}."
        gkeys = sorted(k[len(pre):] for k in g.files if k.startswith(pre) and "#" not in k)
        assert sorted(k for k, p in named.items() if p.grad is not None) == gkeys
        worst = 0.0
        for k in gkeys:
            ref, rmax, rsum = g[pre + k], float(g[pre + k + "#maxabs"]), float(g[pre + k + "#sumabs"])
            atol = max((1e-3 if s == 0 else 5e-3) * rmax, 1e-6)
            smp, sa, mx = R.summarise(named[k].grad)
            err = np.abs(smp.astype(np.float64) - ref)
            worst = max(worst, float(err.max()) / max(rmax, 1e-12))
            assert (err <= atol + 1e-3 * np.abs(ref)).all(), f"grad{s}.{k}: max err {err.max():.3e}, ref max {rmax:.3e}"
            assert abs(mx - rmax) <= atol + 1e-3 * rmax, f"grad{s}.{k}: max {mx:.6e} vs {rmax:.6e}"
            assert abs(sa - rsum) <= atol * named[k].numel() + 1e-3 * rsum, f"grad{s}.{k}: sum {sa:.6e} vs {rsum:.6e}"
        print(f"{case}.grad{s}: worst sampled error {worst:.2e} of the tensor maximum")
        opt.step()
        torch.cuda.synchronize()
        for k in gkeys:
            err = np.abs(R.summarise(named[k])[0].astype(np.float64) - g[f"{case}.post{s}.{k}"])
            assert err.max() <= 2.1 * lr, f"post{s}.{k}: {err.max():.3e}"
            if not k.endswith("k_proj.bias"):
                assert (err <= 0.05 * lr).mean() >= 0.97, f"post{s}.{k}: tight fraction {(err <= 0.05 * lr).mean():.4f}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_head_dim_16_matches_float64_restatement(kind, precision):
    """hidden 64, 4 heads (head_dim 16: the materialised-score path is the only one), both probabilities 0.2, against the
    float64 restatement of the four sites (tests/encoder_dropout_ref.forward).  Bounds of the golden test's unfrozen step."""
    ph = pa = 0.2
    small = dict(hidden=64, layers=2, heads=4, ff=128)
    model, cfg, ocfg, W = _model(kind, precision, ph, pa, model=small, wseed=33)
    B = 2
    x, y = _batch(kind, cfg, 160, B)
    masks = R.site_masks(7200, 0, B, cfg.ntok, cfg.hidden, cfg.heads, cfg.layers, ph, pa)
    model.set_dropout_masks(_cuda_masks(masks))
    logits, grads = _train_step(model, x, y)
    assert not model._ws.fused
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in W.items()}
    ref = R.forward(P, x.cpu().double(), ocfg, masks, ph, pa)
    torch.nn.functional.cross_entropy(ref, y.cpu()).backward()
    close(logits, ref.detach().numpy(), 1e-4, 1e-4, "logits")
    assert sorted(grads) == sorted(P)
    for k, p in P.items():
        r = p.grad.numpy()
        close(grads[k], r, 1e-3, max(1e-3 * np.abs(r).max(), 1e-6), f"grad.{k}")


# ============================================================================================ mask regeneration
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "materialised"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_forward_and_backward_kernels_regenerate_the_same_mask(kind, precision, fused):
    """A generator-mode training step, then the same step with every site's mask dumped through eav_tf_dropout_mask for that
    seed and counter and fed back through set_dropout_masks: logits and every gradient bit-equal.  The explicit-mask run
    reads ONE mask in forward and backward, so equality shows that the generator-mode forward and both backward kernels of
    every site drew that same mask."""
    model, cfg, _, _ = _model(kind, precision, 0.1, 0.1, fused)
    x, y = _batch(kind, cfg, 170, 2)
    _train_step(model, x, y)                                     # (counter 1: the checked step is not the first)
    logits, grads = _train_step(model, x, y)
    cnt = model.forward_counter()
    assert cnt == 2
    masks = model.generated_dropout_masks(2, cnt)
    assert list(masks) == R.site_names(cfg.layers, 0.1, 0.1)
    model.set_dropout_masks(masks)
    logits2, grads2 = _train_step(model, x, y)
    assert model.forward_counter() == cnt                        # explicit masks do not advance the generator
    assert torch.equal(logits, logits2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    model.set_dropout_masks(None)                                # the generator is back: next counter, another mask
    logits3, _ = _train_step(model, x, y)
    assert model.forward_counter() == cnt + 1 and not torch.equal(logits, logits3)


# ============================================================================================ generator statistics
def _frac_bound(p, n):
    return 5.0 * np.sqrt(p * (1.0 - p) / n)


def test_generator_statistics_per_site_step_and_rank():
    """Per site the kept fraction k/n satisfies |k/n - (1 - p)| <= 5 sqrt(p (1 - p) / n); the masks of two consecutive forwards,
    of two sites of one shape and of two ranks' seeds differ in a fraction within the same bound of 2 p (1 - p)."""
    from eav_amd import transformer as T
    ph, pa = 0.1, 0.3
    model, cfg, _, _ = _model("vit", "fp32", ph, pa)
    B = 2
    m1 = model.generated_dropout_masks(B, 1)
    m2 = model.generated_dropout_masks(B, 2)
    mr = model.generated_dropout_masks(B, 1, seed=T.rank_dropout_seed(model.dropout_seed, 1))
    for name, (_, shape, p) in model.dropout_sites(B).items():
        n = int(np.prod(shape))
        kept = float(m1[name].float().mean())
        print(f"{name}: kept {kept:.5f} (1 - p = {1 - p:.2f}, n = {n}, bound {_frac_bound(p, n):.2e})")
        assert tuple(m1[name].shape) == shape and m1[name].dtype == torch.uint8
        assert abs(kept - (1.0 - p)) <= _frac_bound(p, n), name
        for what, other in (("next forward", m2[name]), ("rank 1", mr[name])):
            d = float((m1[name] != other).float().mean())
            assert abs(d - 2 * p * (1 - p)) <= _frac_bound(p, n), (name, what, d)
    pairs = [(m1[a], m1[b], p, (a, b)) for a, b, p in (("attn_out.0", "mlp_out.0", ph), ("emb", "mlp_out.1", ph),
                                                         ("attn.0", "attn.1", pa))]
    for x, y, p, what in pairs:
        d = float((x != y).float().mean())
        assert abs(d - 2 * p * (1 - p)) <= _frac_bound(p, x.numel()), (what, d)
    # no stream is another one shifted by a few elements (seeds that differ by a multiple of the hash's index stride would be)
    for name, (_, _, p) in model.dropout_sites(B).items():
        pairs += [(m1[name], m2[name], p, (name, "next forward")), (m1[name], mr[name], p, (name, "rank 1"))]
    for x, y, p, what in pairs:
        x, y = x.flatten(), y.flatten()
        for k in range(1, 9):
            for u, v in ((x[k:], y[:-k]), (x[:-k], y[k:])):
                d = float((u != v).float().mean())
                assert abs(d - 2 * p * (1 - p)) <= _frac_bound(p, u.numel()), (what, "shift", k, d)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_replayed_captured_step_draws_a_fresh_mask_every_replay(precision):
    """Forward + backward captured in one hipGraph: the counter is advanced by a captured launch, so each of three replays
    draws another mask with no host argument changing - the replays' logits differ pairwise, and each equals, bit for bit,
    an eager forward under the masks dumped for that replay's counter value."""
    from eav_amd.optim import CrossEntropyLoss, unit_gradient
    model, cfg, _, _ = _model("vit", precision, 0.1, 0.1)
    model.overlap_wgrad = False
    twin, _, _, _ = _model("vit", precision, 0.1, 0.1)
    twin.overlap_wgrad = False
    twin.dropout_seed = model.dropout_seed
    x, y = _batch("vit", cfg, 180, 2)
    crit = CrossEntropyLoss()
    dev = x.device

    def step():
        for p in model.parameters():
            p.grad = None
        logits = model(x).logits
        crit(logits, y).backward(gradient=unit_gradient(dev))
        return logits

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    c0 = model.forward_counter()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_logits = step()
    model._pin_workspace()
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        seen.append(static_logits.detach().clone())
        assert model.forward_counter() == c0 + k + 1
        twin.set_dropout_masks(twin.generated_dropout_masks(2, c0 + k + 1))
        with torch.no_grad():
            want = twin(x).logits
        assert torch.equal(seen[-1], want), k
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])


# ============================================================================================ eval and p = 0
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_eval_never_drops_and_p0_ignores_masks(kind, precision):
    drop, cfg, _, _ = _model(kind, precision, 0.2, 0.3)
    plain, _, _, _ = _model(kind, precision, 0.0, 0.0)
    x, y = _batch(kind, cfg, 190, 2)
    with torch.no_grad():
        a = drop.eval()(x).logits
        b = plain.eval()(x).logits
    assert torch.equal(a, b)                                     # eval: bit-identical to the same weights without dropout
    assert drop.forward_counter() == 0
    # a p = 0 model's training step: bit-identical whether or not masks were ever set
    plain.train()
    l0, g0 = _train_step(plain, x, y)
    plain.set_dropout_masks({"emb": torch.zeros(2, cfg.ntok, cfg.hidden, dtype=torch.uint8, device="cuda")})
    l1, g1 = _train_step(plain, x, y)
    plain.set_dropout_masks(None)
    l2, g2 = _train_step(plain, x, y)
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    assert all(torch.equal(g0[k], g1[k]) and torch.equal(g0[k], g2[k]) for k in g0)
    assert plain.forward_counter() == 0
    # ... and in training mode the dropout model does drop
    assert not torch.equal(_train_step(drop.train(), x, y)[0], l0)
    # a mask of the wrong shape is refused, not read out of bounds
    drop.set_dropout_masks({k: v[..., :-1].contiguous() for k, v in drop.generated_dropout_masks(2, 1).items()})
    from eav_amd import _lib
    with pytest.raises(_lib.EavError, match="set_dropout_masks"):
        drop(x)


# ============================================================================================ trainers
def _save_model_dir(tmp_path, kind, ph, pa):
    from safetensors.numpy import save_file
    from oracle import vit_oracle as vo
    ocfg = R.oracle_cfg(kind)
    W = tf_weights(R.WSEED[kind], vo.param_shapes(ocfg), std=R.STD)
    save_file({k: np.ascontiguousarray(v) for k, v in W.items()}, str(tmp_path / "model.safetensors"))
    common = {"hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 2, "intermediate_size": 256,
              "patch_size": 16, "layer_norm_eps": 1e-12, "hidden_act": "gelu", "hidden_dropout_prob": ph,
              "attention_probs_dropout_prob": pa, "id2label": {str(i): f"LABEL_{i}" for i in range(5)}}
    if kind == "ast":
        cfg = dict(common, model_type="audio-spectrogram-transformer", num_mel_bins=128, max_length=R.AST_FRAMES,
                   frequency_stride=10, time_stride=10)
    else:
        cfg = dict(common, model_type="vit", image_size=224, num_channels=3)
        json.dump({"do_normalize": True, "do_rescale": True, "do_resize": True, "image_mean": [0.5, 0.5, 0.5],
                   "image_std": [0.5, 0.5, 0.5], "image_processor_type": "ViTImageProcessor", "resample": 2,
                   "rescale_factor": 1 / 255, "size": {"height": 224, "width": 224}},
                  open(tmp_path / "preprocessor_config.json", "w"))
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    return str(tmp_path)


@pytest.mark.parametrize("precision", ["split", "fp32"])
@pytest.mark.parametrize("kind", ["ast", "vit"])
def test_trainers_honour_the_dropout_of_the_hf_directory(tmp_path, monkeypatch, kind, precision):
    """AudioModelTrainer / ImageClassifierTrainer on a reduced config with hidden / attention dropout 0.1 / 0.1, six train and
    four test items: the frozen epoch bypasses the feature cache (and says so once per phase), outputs_test is deterministic
    for a fixed torch.manual_seed, and two seeds differ."""
    from eav_amd.audio import AudioModelTrainer
    from eav_amd.vision import ImageClassifierTrainer
    monkeypatch.setenv("EAV_ENCODER_PRECISION", precision)
    path = _save_model_dir(tmp_path, kind, 0.1, 0.1)
    monkeypatch.chdir(tmp_path)
    if kind == "ast":       # (log-mel features of the reduced config's 256 frames, handed to the trainer as they are)
        x, y = torch.from_numpy(synth.mel_batch(95, 10, R.AST_FRAMES, 128)[0]), synth.labels(96, 10)
    else:
        x, y = (synth.uniform(97, (10, 2, 56, 56, 3)) * 255).astype(np.uint8), synth.labels(98, 10)
    data = [x[:6], y[:6], x[6:], y[6:]]

    def run(seed):
        torch.manual_seed(seed)
        buf = io.StringIO()
        with redirect_stdout(buf):
            tr = (AudioModelTrainer(data, path, sub="s", num_classes=5, batch_size=4) if kind == "ast" else
                  ImageClassifierTrainer(data, path, sub="s", num_labels=5, batch_size=4))
            assert tr.model.cfg.hidden_dropout == pytest.approx(0.1) and tr.model.cfg.attention_dropout == pytest.approx(0.1)
            assert tr.model.dropout_seed == seed
            tr.train(epochs=2, lr=5e-4, freeze=True)
            assert tr._feat_cache is None                        # bypassed: the backbone ran every step, in training mode
            frozen_forwards = tr.model.forward_counter()
            tr.train(epochs=1, lr=5e-6, freeze=False)
        said = buf.getvalue()
        assert said.count("feature cache bypassed") == 1, said   # once, for the frozen phase
        nb = len(tr.train_dataloader)
        assert frozen_forwards == 2 * nb and tr.model.forward_counter() == 3 * nb      # evaluation never draws
        return tr.outputs_test.copy()

    a, b, c = run(3), run(3), run(4)
    assert a.shape == (8 if kind == "vit" else 4, 5) and np.isfinite(a).all()
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)


# ============================================================================================ two ranks, one GPU
WORKER = r"""
import os, sys
sys.path.insert(0, ROOT)
from types import SimpleNamespace
import numpy as np, torch, torch.distributed as dist
from eav_amd import dist as ed, synth, transformer as T
from eav_amd.optim import CrossEntropyLoss, FusedAdam
from tests.golden_util import tf_weights

rank, world, _ = ed.init_from_env("gloo")
assert world == 2
torch.cuda.set_device(0)
p = 0.1
cfg = T.make_config("vit", hidden=128, layers=2, heads=2, ff=256, hidden_dropout=p, attention_dropout=p)
W = tf_weights(31, T.param_shapes(cfg), std=0.08)
torch.manual_seed(5)                                  # the same seed on both ranks: only the rank mix separates them
model = T.Encoder(cfg, W).cuda().train()
assert model.dropout_seed == 5
tr = ed.attach(SimpleNamespace(model=model))
assert tr.grad_sync is not None and model.dropout_seed == T.rank_dropout_seed(5, rank)
opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=0.01, decoupled=True)
B = 4
x, y = synth.frame_batch(40, B, cfg.H)
lo, hi = ed.shard_batch(B, rank, world)
xd, yd = torch.from_numpy(x[lo:hi]).cuda(), torch.from_numpy(y[lo:hi]).cuda()
opt.zero_grad()
CrossEntropyLoss()(model(xd).logits, yd).backward()
tr.grad_sync()
opt.step()
torch.cuda.synchronize()
assert model.forward_counter() == 1
masks = model.generated_dropout_masks(hi - lo, 1)
for name, m in masks.items():
    both = [torch.empty_like(m) for _ in range(2)]
    dist.all_gather(both, m)
    d = float((both[0] != both[1]).float().mean())
    n = m.numel()
    assert abs(d - 2 * p * (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, (name, d)       # the ranks' masks differ
    a, b = both[0].flatten(), both[1].flatten()
    for k in range(1, 5):                                  # ... and neither is the other shifted by a few elements
        for u, v in ((a[k:], b[:-k]), (a[:-k], b[k:])):
            d = float((u != v).float().mean())
            assert abs(d - 2 * p * (1 - p)) <= 5 * (p * (1 - p) / u.numel()) ** 0.5, (name, "shift", k, d)
flat = model._flat[0]
both = [torch.empty_like(flat) for _ in range(2)]
dist.all_gather(both, flat)
assert torch.equal(both[0], both[1]), "replicas diverged"
assert not torch.equal(flat.cpu(), torch.cat([torch.from_numpy(np.ascontiguousarray(W[k])).reshape(-1) for k in model._names]))
dist.barrier()
dist.destroy_process_group()
open(os.path.join(OUT, f"ok_{rank}"), "w").write("ok")
"""


def test_two_ranks_on_one_gpu_draw_different_masks(tmp_path):
    """Two gloo ranks (fresh child processes) share the one MI355X: dist.attach mixes the rank into dropout_seed, so the
    replicas' masks differ like independent draws (also against each other shifted by a few elements), and after one synchronised AdamW step both hold equal parameters."""
    import socket
    script = tmp_path / "worker.py"
    body = textwrap.indent(textwrap.dedent(WORKER), "    ")
    script.write_text(f"ROOT = {ROOT!r}\nOUT = {str(tmp_path)!r}\nimport os, traceback\ntry:\n{body}\nexcept BaseException:\n"
                      "    open(os.path.join(OUT, 'err_' + os.environ.get('RANK', '0')), 'w').write(traceback.format_exc())\n"
                      "    raise\n")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                       capture_output=True, text=True, env=env, timeout=400, cwd=str(tmp_path))
    errs = "".join(open(tmp_path / f).read() for f in sorted(os.listdir(tmp_path)) if f.startswith("err_"))
    assert r.returncode == 0, (errs or (r.stdout[-3000:] + r.stderr[-6000:]))
    assert all((tmp_path / f"ok_{k}").exists() for k in range(2)), r.stdout[-3000:] + r.stderr[-3000:]
