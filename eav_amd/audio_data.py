"""DataLoadAudio on MI355X - the reference's audio loading class (Dataload_audio.py:10-78), same constructor, methods,
attributes and outputs, with the resampling on the GPU:

    feature_extraction()   torchaudio.load + torchaudio.transforms.Resample(sr, 16000)  -> eav_resample_sinc_f32

One launch resamples all of a subject's files (zero-padded to the longest; each row is cut back to its own
ceil(new * L / orig) outputs, which is exact because torchaudio pads with zeros too).  Reading the WAV files stays on the
host (scipy.io.wavfile, the reference's own dependency) with torchaudio.load's normalisation to float32.  process() returns
what the reference returns, (feature float32 [N, 5 * target], label_indexes int64 [N]); the clips also stay on the device
as `feature_dev` for preprocess.waveforms_to_input_values.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .preprocess import resample_waveforms

EMOTION_TO_INDEX = {'Neutral': 0, 'Happiness': 3, 'Sadness': 1, 'Anger': 2, 'Calmness': 4}


def read_wav_mono(path):
    """(float32 waveform [n], sampling rate) of a mono WAV file, scaled as torchaudio.load(normalize=True) scales it."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if data.ndim != 1:
        if data.shape[1] != 1:
            raise ValueError(f"{path}: {data.shape[1]} channels - DataLoadAudio takes mono recordings")
        data = data[:, 0]
    if data.dtype == np.int16:
        wav = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        wav = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif data.dtype == np.uint8:
        wav = (data.astype(np.float32) - 128.0) / 128.0
    elif data.dtype.kind == 'f':
        wav = data.astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported sample type {data.dtype}")
    return wav, int(rate)


class DataLoadAudio:
    def __init__(self, subject='all', parent_directory='./Datasets/EAV', target_sampling_rate=16000):
        self.parent_directory = parent_directory
        self.original_sampling_rate = int()
        self.target_sampling_rate = target_sampling_rate
        self.subject = subject
        self.file_path = list()
        self.file_emotion = list()

        self.seg_length = 5  # 5s
        self.feature = None
        self.feature_dev = None
        self.label = None
        self.label_indexes = None
        self.test_prediction = list()
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

    def data_files(self):
        # Dataload_audio.py:25-33
        subject = f'subject{self.subject:02d}'
        path = os.path.join(self.parent_directory, subject, 'Audio')
        for i in os.listdir(path):
            emotion = i.split('_')[4]
            self.file_emotion.append(emotion)
            self.file_path.append(os.path.join(path, i))

    def feature_extraction(self):
        # Dataload_audio.py:35-68
        if self.device.type != "cuda":
            raise _lib.EavError("eav_amd.DataLoadAudio resamples on an MI355X (no CPU fallback)")
        waves, rates = [], []
        for path in self.file_path:
            wav, rate = read_wav_mono(path)
            waves.append(wav)
            rates.append(rate)
            self.original_sampling_rate = rate
        segment_length = self.target_sampling_rate * self.seg_length
        clips = [None] * len(waves)
        for rate in sorted(set(rates)):                       # one launch per sampling rate met (one, in the dataset)
            rows = [i for i, r in enumerate(rates) if r == rate and len(waves[i])]
            if not rows:
                continue
            lengths = [len(waves[i]) for i in rows]
            batch = np.zeros((len(rows), max(lengths)), dtype=np.float32)
            for k, i in enumerate(rows):
                batch[k, :lengths[k]] = waves[i]
            y, out_lengths = resample_waveforms(batch, rate, self.target_sampling_rate, lengths=lengths,
                                                device=self.device)
            for k, i in enumerate(rows):
                num_sections = int(out_lengths[k]) // segment_length
                clips[i] = y[k, :num_sections * segment_length].reshape(num_sections, segment_length)
        kept = [c for c in clips if c is not None and c.shape[0]]
        y_names = [self.file_emotion[i] for i, c in enumerate(clips) if c is not None for _ in range(c.shape[0])]
        print(f"Original sf: {self.original_sampling_rate}, resampled into {self.target_sampling_rate}")

        y_idx = [EMOTION_TO_INDEX[emotion] for emotion in y_names]
        self.feature_dev = (torch.cat(kept) if kept else
                            torch.empty(0, segment_length, dtype=torch.float32, device=self.device))
        self.feature = np.squeeze(self.feature_dev.cpu().numpy())
        self.label_indexes = np.array(y_idx, dtype=np.int64)
        self.label = np.array(y_names)

    def process(self):
        self.data_files()
        self.feature_extraction()
        return self.feature, self.label_indexes

    def label_emotion(self):
        self.data_files()
        self.feature_extraction()
        return self.label
