"""AudioModelTrainer on MI355X - the reference's class, same constructor and train() signature.

API of Transformer_torch/Transformer_Audio.py:9-103:
    AudioModelTrainer(DATA, model_path, sub='', num_classes=5, weight_decay=1e-5, lr=0.001, batch_size=128)
        .train(epochs=20, lr=None, freeze=True)      attribute: outputs_test  (float32 [N_test, num_classes])
The model is eav_amd.transformer.Encoder (HIP kernels) instead of the Hugging Face ASTForAudioClassification;
`model_path` may be the stock download (ast-finetuned-audioset: a 527-label head, loaded and then replaced, as
Transformer_Audio.py:22-24 does) and `num_classes` anything up to transformer.HEAD_MAX_CLASSES;
equal-length clips go through the HIP log-mel front-end, ragged ones through the reference's own host call of
ASTFeatureExtractor.  Kept quirks: `weight_decay` is accepted and ignored (Q10); one optimiser spans both phases
(Q11); outputs_test only after the last unfrozen epoch (Q15); one line per epoch appended to
training_performance_audio.txt in the cwd (Q17).  Beyond the reference: the keyword-only `problem_type`
("multi_label_classification" / "regression": fp32 label rows, BCE-with-logits / MSE, the epoch lines of
finetune.FineTuneBase's docstring), `save_pretrained(dir)`, and the keyword-only `max_length`: None is the reference's
behaviour (every clip padded to the checkpoint's 1024 frames, 1214 tokens); an int is the number of log-mel frames the clips
are padded or truncated to; "auto" is the longest clip's own length (auto_max_length: 506 frames, 602 tokens for EAV's 5 s
clips).  The front-end extracts that many frames and the AST runs with variable_length on - the checkpoint's position table
fitted along time (transformer.Encoder, pos_time); `save_pretrained` then writes a stock HF AST of that length.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .finetune import FineTuneBase, require_gpu


def auto_max_length(n_samples, patch=16, tstride=10):
    """The shortest admissible length for clips of up to n_samples samples at 16 kHz: the front-end's frame count
    n = 1 + (n_samples - 400) // 160 (25 ms windows, 10 ms hop), rounded up to the next T' with (T' - patch) % tstride == 0,
    so that the patch grid covers every frame and no padding beyond the last patch is carried."""
    n = max(1 + (int(n_samples) - 400) // 160, patch)
    return n + (-(n - patch)) % tstride


def _longest_clip(x):
    arr = np.asarray(x) if not isinstance(x, (list, tuple)) else None
    if arr is not None and arr.dtype != object and arr.ndim == 2:
        return arr.shape[1]
    return max(len(w) for w in x)


class AudioModelTrainer(FineTuneBase):
    # SpecAugment-style masking of the log-mel features in unfrozen epochs, set between construction and train() like
    # FineTuneBase's regularisers: up to two bands of < time_mask frames and two of < freq_mask mel bins per clip are set
    # to mask_fill - 0.0, the mean of the normalised features (torchaudio's TimeMasking / FrequencyMasking, AST's recipe)
    time_mask = 0
    freq_mask = 0
    mask_fill = 0.0

    def __init__(self, DATA, model_path, sub='', num_classes=5, weight_decay=1e-5, lr=0.001, batch_size=128, *,
                 problem_type=None, max_length=None):
        device = require_gpu("AudioModelTrainer")
        self.device = device
        self.tr, self.tr_y, self.te, self.te_y = DATA
        self.max_length = self._resolve_max_length(max_length, model_path)      # refuses a bad length before any extraction
        self.tr_x, self.te_x = self._feature_extract(self.tr), self._feature_extract(self.te)
        self.sub, self.batch_size, self.problem_type = sub, batch_size, problem_type
        self.train_dataloader = self._prepare_dataloader(self.tr_x, self.tr_y, shuffle=True)
        self.test_dataloader = self._prepare_dataloader(self.te_x, self.te_y, shuffle=False)
        self._build(model_path, num_classes, lr, device, problem_type)          # :22-31
        self.model.variable_length = self.max_length is not None

    def _prepare_dataloader(self, x, y, shuffle=False):
        return self._loader(x, y, shuffle)

    def _resolve_max_length(self, max_length, model_path):
        """None, or the frame count the clips are extracted at: an int as given, "auto" from the longest clip of train +
        test; checked against the checkpoint's configuration (transformer.ast_length_geometry)."""
        if max_length is None:
            return None
        from .transformer import ast_length_geometry, config_from_hf
        cfg = config_from_hf(json.load(open(os.path.join(model_path, "config.json"))))
        if isinstance(max_length, str):
            if max_length != "auto":
                raise ValueError(f'max_length must be None, an int or "auto", got {max_length!r}')
            feats = [x for x in (self.tr, self.te) if isinstance(x, torch.Tensor) and x.dim() == 3]
            if feats:                            # features extracted by the caller: their own length
                max_length = max(int(x.shape[1]) for x in feats)
            else:
                max_length = auto_max_length(max(_longest_clip(self.tr), _longest_clip(self.te)), cfg.patch, cfg.sx)
        elif not isinstance(max_length, (int, np.integer)) or isinstance(max_length, bool):
            raise ValueError(f'max_length must be None, an int or "auto", got {max_length!r}')
        return ast_length_geometry(cfg, int(max_length)).W

    def _feature_extract(self, x):
        """:38-42 - log-mel features [N, 1024, 128] ([N, max_length, 128] with the keyword)."""
        if isinstance(x, torch.Tensor) and x.dim() == 3:
            return x
        T = {} if self.max_length is None else {"max_length": self.max_length}
        arr = np.asarray(x)
        if arr.ndim == 2 and arr.dtype != object and arr.shape[1] >= 400:
            from .preprocess import waveforms_to_input_values
            return waveforms_to_input_values(arr, device=self.device, **T).cpu()
        from transformers import ASTFeatureExtractor
        return ASTFeatureExtractor(**T)(x, sampling_rate=16000, padding='max_length', return_tensors='pt')['input_values']

    def train(self, epochs=20, lr=None, freeze=True):
        self._enter_phase(lr, freeze, epochs)
        for epoch in range(epochs):
            correct, seen = self._train_one_epoch()
            if not self._classifies():
                train_metric = float(correct.item()) / seen
                lr_text = self._lr_text()
                rows = self._evaluate()
                test_metric = self._metric_text(sum(r[1] for r in rows) / sum(r[2] for r in rows))
                self._keep_outputs(rows, epoch == epochs - 1, freeze)
                print(f"Epoch {epoch + 1}/{epochs}, Training {self._metric_text(train_metric)}, Test {test_metric}{lr_text}")
                with open('training_performance_audio.txt', 'a') as f:
                    f.write(f"{self.sub}, Epoch {epoch + 1}, Test {test_metric}\n")
                continue
            train_accuracy = int(correct.item()) / seen
            lr_text = self._lr_text()
            rows = self._evaluate()
            test_accuracy = sum(r[1] for r in rows) / sum(r[2] for r in rows)      # sample-weighted (:92-97)
            self._keep_outputs(rows, epoch == epochs - 1, freeze)
            print(f"Epoch {epoch + 1}/{epochs}, Training Accuracy: {train_accuracy * 100:.2f}%, Test Accuracy: {test_accuracy * 100:.2f}%{lr_text}")
            with open('training_performance_audio.txt', 'a') as f:
                f.write(f"{self.sub}, Epoch {epoch + 1}, Test Accuracy: {test_accuracy * 100:.2f}%\n")
