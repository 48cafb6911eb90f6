"""The fine-tuning regularisers in AudioModelTrainer / ImageClassifierTrainer (finetune.FineTuneBase: label_smoothing,
class_weights, mixup_alpha, augment_seed; time_mask / freq_mask; hflip) on the 2-layer, 64-wide AST / ViT directories of
test_transformer_trainers_gpu: 6 training items in batches of 4 - the ragged last batch of 2 included - in fp32 precision.

The trainer's augmented epoch is held to a hand-driven loop over the same plan_epoch table (bit-equal parameters), and
the first step's loss to the Hugging Face class on the CPU, fed the NumPy restatement's augmented batch and soft targets:
within 2e-3 - the 1e-3 logit bound the trainer tests hold against HF, times the 2-Lipschitz constant of cross-entropy in
the logits' maximum norm for targets that sum to 1."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import augment_ref as ar
from tests.test_transformer_trainers_gpu import _save_model_dir

pytestmark = pytest.mark.gpu

ORDER = [3, 0, 5, 1, 4, 2]                 # -> micro-batches [3, 0, 5, 1] and [4, 2]
KINDS = ["ast", "vit"]


def _data(kind):
    if kind == "ast":
        x = synth.normal(95, (10, 80000), 0.0, 0.1)
        y = synth.labels(96, 10)
    else:
        x = (synth.uniform(97, (10, 2, 56, 56, 3)) * 255).astype(np.uint8)
        y = synth.labels(98, 10)
        return [x[:3], y[:3], x[3:5], y[3:5]]       # 3 trials x 2 frames = 6 training frames
    return [x[:6], y[:6], x[6:], y[6:]]


def _trainer(kind, path, **options):
    from eav_amd.audio import AudioModelTrainer
    from eav_amd.vision import ImageClassifierTrainer
    torch.manual_seed(3)                            # same head, same shuffles
    with redirect_stdout(io.StringIO()):
        tr = (AudioModelTrainer(_data(kind), path, sub="s", num_classes=5, batch_size=4) if kind == "ast" else
              ImageClassifierTrainer(_data(kind), path, sub="s", num_labels=5, batch_size=4))
    for k, v in options.items():
        setattr(tr, k, v)
    assert len(tr.train_dataloader.dataset) == 6
    return tr


def _options(kind):
    extra = dict(time_mask=8, freq_mask=8) if kind == "ast" else dict(hflip=True)
    return dict(mixup_alpha=0.4, label_smoothing=0.1, augment_seed=11, **extra)


def _train(tr, epochs, lr, freeze):
    with redirect_stdout(io.StringIO()):
        tr.train(epochs=epochs, lr=lr, freeze=freeze)


@pytest.fixture
def setup(kind, tmp_path, monkeypatch):
    """The model directory, fp32 precision, the cwd the trainers log to, and a record of BatchAugment.apply's calls."""
    from eav_amd.augment import BatchAugment
    monkeypatch.setenv("EAV_ENCODER_PRECISION", "fp32")
    path = _save_model_dir(tmp_path, kind, 5)
    monkeypatch.chdir(tmp_path)
    applied = []
    real = BatchAugment.apply

    def spy(self, loader, table_slice, need_soft_targets, num_classes=None):
        applied.append((table_slice.cpu().numpy().copy(), bool(need_soft_targets)))
        return real(self, loader, table_slice, need_soft_targets, num_classes)

    monkeypatch.setattr(BatchAugment, "apply", spy)
    return path, applied


def _params(tr):
    return {k: v.detach().clone() for k, v in tr.model.state_dict().items()}


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_never_enter_the_augmenting_path(kind, setup):
    from eav_amd.optim import CrossEntropyLoss
    path, applied = setup
    runs = []
    for _ in range(2):
        tr = _trainer(kind, path)
        first = tr.loss_fn
        _train(tr, 1, 5e-4, True)
        _train(tr, 1, 5e-6, False)
        assert tr.loss_fn is first and type(first) is CrossEntropyLoss and first.weight is None \
            and first.label_smoothing == 0.0                                  # the criterion was never rebuilt
        runs.append((_params(tr), tr.outputs_test))
    assert applied == []
    assert np.array_equal(runs[0][1], runs[1][1])
    assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])


@pytest.mark.parametrize("kind", KINDS)
def test_augmented_epoch_equals_the_hand_driven_loop_and_hugging_face(kind, setup):
    from transformers import ASTForAudioClassification, ViTForImageClassification
    from eav_amd.augment import BatchAugment, sample_matrix_shape
    from eav_amd.optim import CrossEntropyLoss, FusedAdam
    path, applied = setup
    opts = _options(kind)

    # through the trainer
    tr = _trainer(kind, path, **opts)
    start = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    tr.train_dataloader.order_override = [ORDER]
    seen = {}
    real_epoch = tr._train_one_epoch
    tr._train_one_epoch = lambda *a, **k: seen.setdefault("epoch", real_epoch(*a, **k))
    _train(tr, 1, 5e-6, False)
    assert tr.loss_fn.label_smoothing == 0.1 and len(applied) == 2 and all(soft for _, soft in applied)
    through_trainer = _params(tr)
    correct, count = seen["epoch"]

    # by hand: the same Encoder and data, a new criterion and optimiser, the table replayed
    hand = _trainer(kind, path)
    dl, model = hand.train_dataloader, hand.model
    assert all(torch.equal(v.cpu(), start[k]) for k, v in model.state_dict().items())
    R, C = sample_matrix_shape(dl.x)
    aug = BatchAugment(opts["mixup_alpha"], opts.get("time_mask", 0), opts.get("freq_mask", 0), opts.get("hflip", False),
                       opts["augment_seed"])
    batches = [ORDER[:4], ORDER[4:]]
    table = aug.plan_epoch(batches, 0, (R, C))
    assert np.array_equal(np.concatenate([t for t, _ in applied]), table)
    assert (ar.lam_of(table) < 1.0).any()
    dev_table = torch.from_numpy(table).cuda()
    crit = CrossEntropyLoss(label_smoothing=0.1)
    opt = FusedAdam(model.parameters(), lr=5e-6, weight_decay=0.01, decoupled=True)
    model.train()
    hits, pos, first_loss = 0, 0, None
    for idx in batches:
        xb, tb = aug.apply(dl, dev_table[pos:pos + len(idx)], True, 5)
        pos += len(idx)
        opt.zero_grad()
        logits = model(xb).logits
        loss = crit(logits, tb)
        loss.backward()
        opt.step()
        hits += int((logits.argmax(-1) == dl.y[torch.as_tensor(idx, device="cuda")]).sum())      # the primary labels
        first_loss = float(loss.detach()) if first_loss is None else first_loss
    by_hand = _params(hand)
    for k in by_hand:
        assert torch.equal(by_hand[k], through_trainer[k]), k
    assert count == 6 and int(correct) == hits
    assert any(not torch.equal(by_hand[k].cpu(), start[k]) for k in by_hand)

    # the first step against Hugging Face on the NumPy restatement's batch
    x, y = dl.x.cpu().numpy(), dl.y.cpu().numpy()
    part = table[:4]
    xb_ref, _, _ = ar.gather(x.reshape(len(x), R, C), part, 0.0)
    tb_ref = ar.soft_targets(y, part, 5)
    hf = (ASTForAudioClassification if kind == "ast" else ViTForImageClassification).from_pretrained(path)
    hf.load_state_dict(start)
    hf.eval()
    with torch.no_grad():
        inputs = torch.from_numpy(xb_ref.astype(np.float32)).reshape((4,) + x.shape[1:])
        logits = hf(inputs).logits
        ref_loss = float(torch.nn.functional.cross_entropy(logits, torch.from_numpy(tb_ref).float(), label_smoothing=0.1))
    print(f"{kind}: first-step loss {first_loss:.6f}, Hugging Face on the reference batch {ref_loss:.6f}")
    assert abs(first_loss - ref_loss) <= 2e-3, (first_loss, ref_loss)


@pytest.mark.parametrize("kind", KINDS)
def test_accumulation_keeps_partners_inside_micro_batches(kind, setup):
    path, applied = setup
    tr = _trainer(kind, path, gradient_accumulation_steps=2, class_weights="balanced", **_options(kind))
    tr.train_dataloader.order_override = [ORDER]
    before = _params(tr)
    _train(tr, 1, 5e-6, False)
    assert tr.loss_fn.weight is not None and tr.loss_fn.weight.numel() == 5
    assert [t.shape[0] for t, _ in applied] == [4, 2]
    for (t, _), idx in zip(applied, (ORDER[:4], ORDER[4:])):
        assert t[:, 0].tolist() == idx and sorted(t[:, 1].tolist()) == sorted(idx)
    after = _params(tr)
    assert any(not torch.equal(after[k], before[k]) for k in after) and all(torch.isfinite(v).all() for v in after.values())
    assert tr.outputs_test.shape == (len(tr.test_dataloader.dataset), 5) and np.isfinite(tr.outputs_test).all()


@pytest.mark.parametrize("kind", KINDS)
def test_frozen_epochs_keep_their_feature_cache(kind, setup):
    path, applied = setup
    tr = _trainer(kind, path, **_options(kind))
    calls = []
    real_forward = tr.model.forward
    tr.model.forward = lambda *a, **k: (calls.append(1), real_forward(*a, **k))[1]
    _train(tr, 2, 5e-4, True)
    assert applied == []                                                      # the inputs are not augmented
    assert tr.loss_fn.label_smoothing == 0.1                                  # the criterion options hold in every phase
    fc = tr._feat_cache
    assert fc is not None and fc["have_train"] and fc["have_test"]
    assert len(calls) == 2 + 1                                                # backbone: first epoch's batches only
    _train(tr, 1, 5e-6, False)                                                # and the unfrozen phase then augments
    assert len(applied) == 2
