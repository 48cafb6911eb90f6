"""The reference's per-subject AUDIO and VISION drivers (Dataload_audio.py:80-115, Transformer_torch/Transformer_Vision.py:
132-188) on MI355X, subject-sharded, through the public trainers.

    python tools/run_finetune_subjects.py audio  [--subjects 42] [--frozen-epochs 10] [--unfrozen-epochs 15]
    python tools/run_finetune_subjects.py vision [--subjects 42] [--frozen-epochs 10] [--unfrozen-epochs 5]
    python tools/run_finetune_subjects.py vision --image-size 112     (frames resized to 112 x 112, not the processor's 224:
                                                                       the ViT resamples its position table, 50 tokens)
    python tools/run_finetune_subjects.py audio --max-length auto     (clips at their own length, not padded to 1024 frames:
                                                                       5 s -> 506 frames, 602 tokens instead of 1214)
    python tools/run_finetune_subjects.py audio --audio-root Datasets/EAV      (the dataset folder, Dataload_audio.py:87-93)
    python tools/run_finetune_subjects.py audio --label-smoothing 0.1 --mixup-alpha 0.4 --time-mask 48 --freq-mask 24
                                                     (the regularisers of finetune.FineTuneBase; vision: --hflip)
    python tools/run_finetune_subjects.py audio --patch-dropout 0.5   (the unfrozen epochs train on half of every clip's patches:
                                                                       608 tokens instead of 1214)
    python tools/run_finetune_subjects.py vision --drop-path 0.1      (stochastic depth in the unfrozen epochs, timm's DropPath)
    python -m torch.distributed.run --nproc-per-node 8 tools/run_finetune_subjects.py audio ...

Every subject is one `AudioModelTrainer` / `ImageClassifierTrainer` run with the reference's hyper-parameters
(audio: batch 8, train(10, 5e-4, freeze=True) + train(15, 5e-6, freeze=False); vision: batch 128, 10 + 5 epochs) on a
synthetic subject of the reference's sizes (280 + 120 clips of 5 s at 16 kHz; 200 + 200 trials x 25 frames of 56 x 56).
eav_amd.dist.SubjectSchedule places them: whole rounds one subject per rank with no collective, the remainder on groups of
ranks - every member holds a replica, every n-th training item and 1 / n of the batch size, gradients all-reduced inside the
group (the reference's nn.DataParallel wrap, Transformer_Audio.py:59-60 / Transformer_Vision.py:82-83).  At the end ONE
all_gather of `outputs_test` (SURVEY 8e level 1); vision adds the trial vote + weighted F1 of Transformer_Vision.py:174-185.
`--audio-root DIR` (audio only) loads every subject from DIR/subjectNN/Audio instead: eav_amd.audio_data.DataLoadAudio
(WAV files, resampled to 16 kHz on the GPU, 5 s clips) and EAVDataSplit(...).get_split(h_idx=56), as the reference driver
does.  `--save-dir DIR` keeps every subject's fine-tuned model as DIR/subjectNN/ (FineTuneBase.save_pretrained).  For vision, replace `synthetic_subject` by the pickles the reference driver reads.  The model directory is an HF-format
directory (`--model-path`); without one a random-init full-size model is written to a temporary directory.
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eav_amd import dist as eav_dist, synth  # noqa: E402


def synthetic_subject(kind, sub, small):
    if kind == "audio":
        ntr, nte = (16, 8) if small else (280, 120)
        wav = synth.normal(100 + sub, (ntr + nte, 80000), 0.0, 0.1)
        y = synth.labels(200 + sub, ntr + nte)
        return [wav[:ntr], y[:ntr], wav[ntr:], y[ntr:]]
    ntri = 8 if small else 200
    fr = synth.uniform(300 + sub, (2 * ntri, 25, 56, 56, 3), 0, 256).astype(np.uint8)
    y = synth.labels(400 + sub, 2 * ntri)
    return [fr[:ntri], y[:ntri], fr[ntri:], y[ntri:]]


def audio_subject(root, sub):
    """Dataload_audio.py:87-93: one subject's WAV folder -> [tr_x, tr_y, te_x, te_y]."""
    from eav_amd.audio_data import DataLoadAudio
    from eav_amd.datasplit import EAVDataSplit
    x, y = DataLoadAudio(subject=sub, parent_directory=root).process()
    return list(EAVDataSplit(x, y).get_split(h_idx=56))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=("audio", "vision"))
    ap.add_argument("--subjects", type=int, default=42)
    ap.add_argument("--frozen-epochs", type=int, default=10)
    ap.add_argument("--unfrozen-epochs", type=int, default=None)
    ap.add_argument("--model-path", default=None)
    ap.add_argument("--small", action="store_true", help="tiny synthetic subjects (logic check)")
    ap.add_argument("--audio-root", default=None, help="audio only: dataset folder holding subjectNN/Audio/*.wav")
    ap.add_argument("--no-hybrid", action="store_true", help="plain round-robin: the remainder one subject per rank")
    ap.add_argument("--backend", default=os.environ.get("EAV_DIST_BACKEND"))
    ap.add_argument("--save-dir", default=None, help="write every fine-tuned subject model to DIR/subjectNN/ (HF directory: "
                    "config.json, model.safetensors, preprocessor_config.json when the source had one); off by default")
    ap.add_argument("--image-size", type=int, default=None, help="vision only: train on N x N frames with "
                    "interpolate_pos_encoding (ImageClassifierTrainer(image_size=N)); default: the processor's size")
    ap.add_argument("--max-length", default=None, help="audio only: N frames or 'auto' (the longest clip's own length) instead "
                    "of the checkpoint's 1024 (AudioModelTrainer(max_length=...)); default: the checkpoint's")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="F", help="clip the gradients' global L2 norm to F "
                    "inside every optimiser step (trainer.max_grad_norm); default: no clipping, like the reference")
    ap.add_argument("--grad-accum", type=int, default=1, metavar="K", help="one optimiser step per K micro-batches "
                    "(trainer.gradient_accumulation_steps): effective batch K x the launch batch")
    ap.add_argument("--lr-scheduler", default="constant", choices=("constant", "constant_with_warmup", "linear", "cosine"),
                    help="learning-rate schedule of every train() call (trainer.lr_scheduler_type, the lambdas of "
                    "transformers.get_scheduler); default: the reference's constant rate")
    ap.add_argument("--warmup-ratio", type=float, default=0.0, metavar="R", help="share of a train() call's optimiser steps "
                    "spent warming up from 0 (trainer.warmup_ratio)")
    ap.add_argument("--layer-decay", type=float, default=1.0, metavar="D", help="layer-wise learning-rate decay in (0, 1]: the "
                    "head at lr, layer i at lr * D ** (layers + 1 - i) (trainer.layer_decay)")
    ap.add_argument("--no-decay-bias-norm", action="store_true", help="no weight decay on biases, LayerNorm weights, tokens "
                    "and the position table, HF Trainer's rule (trainer.decay_bias_and_norm = False)")
    ap.add_argument("--label-smoothing", type=float, default=0.0, metavar="E", help="cross-entropy label smoothing in [0, 1] "
                    "(trainer.label_smoothing, HF's label_smoothing_factor)")
    ap.add_argument("--class-weights", choices=("balanced",), default=None, help="weight the classes by n / (classes x "
                    "count) over the training labels (trainer.class_weights)")
    ap.add_argument("--mixup-alpha", type=float, default=0.0, metavar="A", help="mixup with lambda ~ Beta(A, A) in the unfrozen "
                    "epochs (trainer.mixup_alpha)")
    ap.add_argument("--time-mask", type=int, default=0, metavar="T", help="audio only: two bands of < T frames masked per clip "
                    "in the unfrozen epochs (trainer.time_mask)")
    ap.add_argument("--freq-mask", type=int, default=0, metavar="F", help="audio only: two bands of < F mel bins masked per "
                    "clip in the unfrozen epochs (trainer.freq_mask)")
    ap.add_argument("--hflip", action="store_true", help="vision only: mirror every frame left-right with probability 0.5 in "
                    "the unfrozen epochs (trainer.hflip)")
    ap.add_argument("--augment-seed", type=int, default=0, help="seed of the augmentation draws (trainer.augment_seed)")
    ap.add_argument("--patch-dropout", type=float, default=0.0, metavar="P", help="every sample of an unfrozen epoch keeps a "
                    "random max(1, int(patches x (1 - P))) of its patch tokens, timm's PatchDropout (trainer.patch_dropout); "
                    "0 <= P < 1")
    ap.add_argument("--drop-path", type=float, default=0.0, metavar="R", help="stochastic depth: every sample of an unfrozen "
                    "epoch drops the residual branches of layer i with probability R i / (layers - 1), timm's DropPath "
                    "(trainer.drop_path); 0 <= R < 1")
    ap.add_argument("--weight-averaging", choices=("ema", "swa"), default=None, help="evaluate, report and save an average of "
                    "the weights kept inside the optimiser step (trainer.weight_averaging): exponential (timm's ModelEma) or "
                    "equal-weight (SWA); default: the last iterate, like the reference")
    ap.add_argument("--ema-decay", type=float, default=0.999, metavar="D", help="decay of --weight-averaging ema, in [0, 1] "
                    "(trainer.ema_decay)")
    ap.add_argument("--ema-warmup", action="store_true", help="use min(D, (1 + n) / (10 + n)) while few steps have been "
                    "averaged (trainer.ema_warmup)")
    ap.add_argument("--averaging-start-epoch", type=int, default=0, metavar="E", help="epochs, counted over both phases, "
                    "trained before the first averaging step (trainer.averaging_start_epoch)")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args()
    if args.grad_accum < 1 or (args.max_grad_norm is not None and not args.max_grad_norm > 0):
        ap.error("--grad-accum takes K >= 1 and --max-grad-norm F > 0")
    if not 0.0 <= args.label_smoothing <= 1.0 or not args.mixup_alpha >= 0.0 or args.time_mask < 0 or args.freq_mask < 0:
        ap.error("--label-smoothing takes E in [0, 1], --mixup-alpha A >= 0, --time-mask / --freq-mask integers >= 0")
    if not 0.0 <= args.warmup_ratio <= 1.0 or not 0.0 < args.layer_decay <= 1.0:
        ap.error("--warmup-ratio takes R in [0, 1] and --layer-decay D in (0, 1]")
    if not 0.0 <= args.patch_dropout < 1.0:
        ap.error("--patch-dropout takes P with 0 <= P < 1")
    if not 0.0 <= args.drop_path < 1.0:
        ap.error("--drop-path takes R with 0 <= R < 1")
    if not 0.0 <= args.ema_decay <= 1.0 or args.averaging_start_epoch < 0:
        ap.error("--ema-decay takes D in [0, 1] and --averaging-start-epoch E >= 0")
    audio = args.kind == "audio"
    if audio and args.hflip:
        ap.error("--hflip is a vision option")
    if not audio and (args.time_mask or args.freq_mask):
        ap.error("--time-mask and --freq-mask are audio options")
    if audio and args.image_size is not None:
        ap.error("--image-size is a vision option")
    if not audio and args.max_length is not None:
        ap.error("--max-length is an audio option")
    max_length = args.max_length if args.max_length in (None, "auto") else int(args.max_length)
    unfrozen = args.unfrozen_epochs if args.unfrozen_epochs is not None else (15 if audio else 5)
    if "EAV_FORCE_DEVICE" in os.environ:                      # several ranks on one GPU (logic runs on a 1-GPU box)
        os.environ["LOCAL_RANK"] = os.environ["EAV_FORCE_DEVICE"]
    rank, world, local = eav_dist.init_from_env(args.backend)
    torch.cuda.set_device(local)
    from eav_amd.audio import AudioModelTrainer
    from eav_amd.vision import ImageClassifierTrainer, trial_vote
    sched = eav_dist.subject_schedule(world, args.subjects, hybrid=not args.no_hybrid)
    groups = sched.make_groups() if world > 1 else {}
    tmp = tempfile.mkdtemp(prefix="eav_subjects_")
    cwd = os.getcwd()
    os.chdir(tmp)                                             # the trainers append their log files to the cwd (Q17)
    try:
        path = args.model_path
        if path is None:
            import bench
            path = bench._save_full_model_dir("ast" if audio else "vit", os.path.join(tmp, "model"))
        bs = 8 if audio else 128
        out, t0 = {}, time.perf_counter()
        mine = sched.group_of(rank)
        plan = [(s, None) for s in sched.solo[rank]] + ([mine] if mine else [])
        for sub, ranks in plan:
            if audio and args.audio_root:
                data = audio_subject(os.path.join(cwd, args.audio_root), sub)
            else:
                data = synthetic_subject(args.kind, sub, args.small)
            n = len(ranks) if ranks else 1
            # this rank's replica sees every n-th training item: equal shard lengths and batch sizes on every member,
            # hence equal step counts (eav_amd.dist.replica_shard)
            sl, bsz = eav_dist.replica_shard(len(data[0]), bs, ranks.index(rank) if n > 1 else 0, n)
            data = [data[0][sl], data[1][sl], data[2], data[3]]
            torch.manual_seed(sub)                            # the fresh head: identical on every member of a group
            with contextlib.redirect_stdout(sys.stdout if args.verbose else io.StringIO()):
                if audio:
                    tr = AudioModelTrainer(data, model_path=path, sub=f"subject_{sub:02d}", num_classes=5,
                                           weight_decay=1e-5, lr=0.005, batch_size=bsz, max_length=max_length)
                else:
                    tr = ImageClassifierTrainer(data, model_path=path, sub=f"subject_{sub:02d}", num_labels=5, lr=5e-5,
                                                batch_size=bsz, image_size=args.image_size)
                tr.max_grad_norm, tr.gradient_accumulation_steps = args.max_grad_norm, args.grad_accum
                tr.lr_scheduler_type, tr.warmup_ratio = args.lr_scheduler, args.warmup_ratio
                tr.layer_decay, tr.decay_bias_and_norm = args.layer_decay, not args.no_decay_bias_norm
                tr.label_smoothing, tr.class_weights = args.label_smoothing, args.class_weights
                tr.mixup_alpha, tr.augment_seed = args.mixup_alpha, args.augment_seed
                tr.patch_dropout = args.patch_dropout
                tr.drop_path = args.drop_path
                tr.weight_averaging, tr.ema_decay, tr.ema_warmup = args.weight_averaging, args.ema_decay, args.ema_warmup
                tr.averaging_start_epoch = args.averaging_start_epoch
                if audio:
                    tr.time_mask, tr.freq_mask = args.time_mask, args.freq_mask
                else:
                    tr.hflip = args.hflip
                if n > 1:
                    eav_dist.attach(tr, group=groups[sub])
                tr.train(epochs=args.frozen_epochs, lr=5e-4, freeze=True)
                tr.train(epochs=unfrozen, lr=5e-6, freeze=False)
            if n == 1 or ranks[0] == rank:                    # one report per subject
                if args.save_dir:                             # after the subject's last phase
                    tr.save_pretrained(os.path.join(cwd, args.save_dir, f"subject{sub:02d}"))
                out[sub] = (np.asarray(tr.outputs_test, dtype=np.float32), np.asarray(data[3]))
            del tr
            torch.cuda.empty_cache()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        gathered = [None] * world
        if world > 1:
            torch.distributed.all_gather_object(gathered, out)          # the job's only whole-world collective
        else:
            gathered = [out]
        if rank == 0:
            allr = {k: v for d in gathered for k, v in d.items()}
            accs, f1s = [], []
            for sub in sorted(allr):
                logits, te_y = allr[sub]
                if audio:
                    accs.append(float((logits.argmax(1) == te_y).mean()))
                else:
                    pred, acc, f1 = trial_vote(logits, te_y, frames_per_trial=25)
                    accs.append(float(acc))
                    f1s.append(float(f1))
            rep = {"modality": args.kind, "subjects": len(allr), "world": world, "seconds": round(dt, 2),
                   "schedule": {"rounds": sched.rounds, "groups": sched.groups},
                   "outputs_test_shape": list(next(iter(allr.values()))[0].shape),
                   "mean_test_acc": round(float(np.mean(accs)), 4)}
            if f1s:
                rep["mean_weighted_f1"] = round(float(np.mean(f1s)), 4)
            print(json.dumps(rep))
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
