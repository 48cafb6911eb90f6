"""Seeded WAV files for the DataLoadAudio tests and their golden (tests/golden/make_goldens_audio_load.py), and the host
side of the loader restated for the tests: a WAV reader with torchaudio.load's normalisation.  Reduced rates keep the
dataset's 44100 -> 16000 ratio (441 / 160): 882 Hz files, 320 Hz target, so a 5 s clip is 1600 samples."""
import os

import numpy as np

from eav_amd import synth

RATE, TARGET, SUBJECT = 882, 320, 3
CLIP_IN = 5 * RATE          # 4410 input samples give one 5 s clip
# (file name - field 4 is the emotion -, sample type, samples, seed)
SPECS = [
    ("003_Trial_01_Listening_Neutral_aud.wav", "int16", 2 * CLIP_IN + 100, 11),
    ("003_Trial_02_Speaking_Happiness_aud.wav", "float32", CLIP_IN + 7, 12),
    ("003_Trial_03_Listening_Anger_aud.wav", "int16", 3000, 13),               # shorter than a clip: no output
    ("003_Trial_04_Speaking_Anger_aud.wav", "float32", 3 * CLIP_IN - 1, 14),     # ceil() makes the third clip whole
    ("003_Trial_05_Listening_Calmness_aud.wav", "int16", CLIP_IN, 15),
    ("003_Trial_06_Speaking_Sadness_aud.wav", "float32", 9000, 16),
]


def samples(kind, n, seed):
    u = synth.uniform(seed, (n,), -0.8, 0.8)
    return np.round(u.astype(np.float64) * 32767.0).astype(np.int16) if kind == "int16" else u


def write_subject(root):
    """Writes SPECS under root/subject03/Audio and returns that folder."""
    from scipy.io import wavfile
    folder = os.path.join(root, f"subject{SUBJECT:02d}", "Audio")
    os.makedirs(folder, exist_ok=True)
    for name, kind, n, seed in SPECS:
        wavfile.write(os.path.join(folder, name), RATE, samples(kind, n, seed))
    return folder


def read_wav(path):
    """(float32 [n], rate) as torchaudio.load(path) normalises a mono file."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    assert data.ndim == 1, path
    if data.dtype == np.int16:
        return data.astype(np.float32) / np.float32(32768.0), rate
    if data.dtype == np.int32:
        return (data.astype(np.float64) / 2.0 ** 31).astype(np.float32), rate
    if data.dtype == np.uint8:
        return (data.astype(np.float32) - np.float32(128.0)) / np.float32(128.0), rate
    return data.astype(np.float32), rate


def expected_in_order(golden, names):
    """(features [N, clip], label_indexes [N], labels [N]) of the golden for files listed in the order `names`."""
    gnames = [str(n) for n in golden["names"]]
    off = np.concatenate([[0], np.cumsum(golden["clip_counts"])])
    feats, idx, lab = [], [], []
    for n in names:
        i = gnames.index(n)
        feats.append(golden["features"][off[i]:off[i + 1]])
        idx += [int(golden["file_label_index"][i])] * int(golden["clip_counts"][i])
        lab += [str(golden["file_emotion"][i])] * int(golden["clip_counts"][i])
    return np.concatenate(feats), np.array(idx, dtype=np.int64), np.array(lab)
