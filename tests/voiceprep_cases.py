"""Shared by tests/test_voiceprep_host.py and tests/test_gpu_voiceprep.py: the ratios and lengths the resampler is held to,
waveforms whose trim decisions are far from the threshold, and a tiny corpus of synthetic voices at two rates.

Every waveform is built from seeded generators, so both files see the same bytes, and the statements are evaluated once
per session (``functools.lru_cache``)."""
import functools
import os

import numpy as np

from acousticswarms_speech_amd import voiceprep as vp

# the ratios and lengths scipy.signal.resample_poly was compared on when the formula was written down
HOST_RATIOS = ((3, 1), (1, 3), (160, 147), (147, 160), (160, 441), (2, 3), (320, 147), (6, 1))
HOST_LENGTHS = (1, 2, 7, 50, 333, 1501)
# on the device: the identity, small ratios, the 44.1 kHz family and the LDS limit (max(up, down) = 640)
DEVICE_RATIOS = ((1, 1), (3, 1), (1, 3), (2, 3), (160, 147), (147, 160), (160, 441), (640, 147))
RAGGED_LENGTHS = (1, 2, 63, 1025, 3000)
MARGIN_DB = 1e-6


def signal(n, seed):
    """n float32 samples: seeded noise under a slow envelope, peak below 1."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)
    return (0.4 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * t / 977.0 + seed))).clip(-0.99, 0.99).astype(np.float32)


def packed(lengths, seed=0):
    """(x float32 packed, row_offset, rows): rows of the given lengths one after the other."""
    rows = [signal(n, seed + 17 * k) for k, n in enumerate(lengths)]
    offs = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    return np.concatenate(rows + [np.zeros(1, dtype=np.float32)]), [int(o) for o in offs], rows


@functools.lru_cache(maxsize=None)
def resampled(lengths, up, down, seed=0):
    """The statement on every row of ``packed(lengths, seed)``: a tuple of float64 arrays."""
    return tuple(vp.resample_poly_f64(r, up, down) for r in packed(lengths, seed)[2])


def trim_margin_db(x32, top_db=18.0):
    """Smallest distance in dB (float64) of any frame's level from the decision threshold of ``voiceprep.trim_f64``: how
    far a waveform is from a decision that another rounding of the same levels could take differently."""
    ms, level = vp.trim_levels(x32, top_db)
    with np.errstate(divide="ignore"):
        return float(np.min(np.abs(10.0 * np.log10(np.maximum(vp.TRIM_A2, ms) / level))))


def _speech(n, seed, level=0.3):
    rng = np.random.RandomState(seed)
    t = np.arange(n)
    return (level * np.sin(2 * np.pi * t * (180.0 + 13 * seed) / 48000.0) * (0.6 + 0.4 * np.sin(2 * np.pi * t / 4111.0))
            + 0.01 * rng.standard_normal(n))


def _floor(n, seed):
    return 1e-4 * np.random.RandomState(1000 + seed).standard_normal(n)


@functools.lru_cache(maxsize=None)
def trim_cases():
    """name -> float32 waveform.  Silence is noise 70 dB below the voice, so the frames away from an edge are tens of dB
    from the 18 dB threshold, and the frames that straddle an edge were looked at on the CPU: none lies within 1e-6 dB."""
    c = {}
    c["below_one_block"] = _speech(300, 1)                                   # T < 512: one block, one frame
    c["empty"] = np.zeros(0)
    c["zeros"] = np.zeros(3000)                                              # non-silent everywhere, as in librosa
    c["silence_first"] = np.concatenate([_floor(7000, 2), _speech(9000, 2)])
    c["silence_last"] = np.concatenate([_speech(9000, 3), _floor(7000, 3)])
    x = _floor(12000, 4)
    x[5300:6000] += _speech(700, 4)                                          # a burst shorter than a frame
    c["burst"] = x
    x = _floor(512 * 9 + 100, 5)
    x[-60:] += 0.5                                                           # the peak in the last, partial block
    c["peak_in_the_partial_block"] = x
    c["both_ends"] = np.concatenate([_floor(5000, 6), _speech(20000, 6), _floor(3100, 6)])
    c["one_sample"] = np.array([0.25])
    c["exact_blocks"] = np.concatenate([_floor(1024, 7), _speech(2048, 7), _floor(1024, 7)])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def long_row():
    """One row of 100 000 samples: 196 blocks, a variance over 390 passes of the workgroup."""
    return np.ascontiguousarray(np.concatenate([_floor(21000, 8), _speech(60000, 8), _floor(19000, 8)]), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def trim_statement(name):
    return vp.trim_f64(long_row() if name == "long_row" else trim_cases()[name])


def make_corpus(root):
    """Six speaker directories of three short wav files each, at 16 kHz and 44.1 kHz in turn: a voiced stretch between
    two silences; one file is silence only (rejected) and one is int16.  -> root."""
    from scipy.io import wavfile
    for s in range(6):
        d = os.path.join(root, f"p{s:03d}")
        os.makedirs(d, exist_ok=True)
        sr = 16000 if s % 2 == 0 else 44100
        for k in range(3):
            n = int(sr * (0.9 + 0.6 * k))
            a, b = int(0.1 * n), int(0.8 * n)
            x = _floor(n, 10 * s + k)
            t = np.arange(b - a) / sr
            x[a:b] += 0.3 * np.sin(2 * np.pi * (150 + 40 * s) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
            if s == 1 and k == 0:
                x = 0.1 * _floor(n, 99)
            x = x.astype(np.float32)
            wavfile.write(os.path.join(d, f"u{k}.wav"), sr, (x * 32767).astype(np.int16) if (s == 2 and k == 1) else x)
    return root


GENERATE_ARGS = ["--n_outputs", "2", "--sr", "48000", "--duration", "0.5", "--n_voices_min", "2", "--n_voices_max", "3",
                 "--max_order", "2", "--n_mics", "4", "--batch", "3"]


def tree(path):
    """{relative file name: bytes} of everything below ``path``."""
    out = {}
    for base, _dirs, files in os.walk(path):
        for f in files:
            full = os.path.join(base, f)
            with open(full, "rb") as fh:
                out[os.path.relpath(full, path)] = fh.read()
    return out
