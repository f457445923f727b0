"""Small host-side DSP helpers of the search path (numpy only).

Rows a-J / a-R of SURVEY.md §8: windowed-RMS energy, SI-SDR, voiced-segment
splitting.  The reference obtains its STFT framing from pyroomacoustics 0.5.0 and
its RMS/split from librosa (both absent offline and un-pinned by any reference
test): ``stft_frames``, ``frame_rms`` and ``nonsilent_intervals`` restate the
published behaviour of those third-party calls -- "parity unpinned" for the
framing itself; everything built on top of them is pinned by
fixtures g7-g10.
"""
import math

import numpy as np

MIN_ERR = 1e-8            # sep/helpers/eval_utils.py:9


# ---- third-party call sites, restated ------------------------------------
def stft_frames(x: np.ndarray, nfft: int, hop: int) -> np.ndarray:
    """pyroomacoustics.transform.stft.analysis(x, nfft, hop) as called at
    sep/Traditional_SP/SRP_Prunning.py:404-409: rectangular window, no padding,
    frames at multiples of ``hop``, one-sided FFT, single precision for a
    float32 input.  Returns [n_frames, nfft//2+1]."""
    n = (x.shape[0] - nfft) // hop + 1
    idx = np.arange(nfft)[None, :] + hop * np.arange(n)[:, None]
    X = np.fft.rfft(x[idx], axis=1)
    return X.astype(np.complex64 if x.dtype == np.float32 else np.complex128)


def frame_rms(y: np.ndarray, frame_length: int = 1024, hop_length: int = 256) -> np.ndarray:
    """librosa.feature.rms(y=, frame_length=, hop_length=) (centered, zero padded):
    returns [1, 1 + len(y)//hop].  The samples are squared once and the frames are a strided
    view of that array (no gather, no per-frame re-squaring)."""
    pad = frame_length // 2
    yp = np.pad(y, (pad, pad), mode="constant")
    sq = yp * yp
    frames = np.lib.stride_tricks.sliding_window_view(sq, frame_length)[::hop_length]
    return np.sqrt(np.mean(frames, axis=1))[None, :]


def nonsilent_intervals(y, top_db=60, ref=np.max, frame_length=2048, hop_length=512, rms=None):
    """librosa.effects.split: frames whose RMS is within ``top_db`` of ``ref``.  ``rms`` may
    carry frame_rms(y, frame_length, hop_length) when the caller already has it."""
    rms = frame_rms(y, frame_length, hop_length)[0] if rms is None else rms[0]
    amin = 1e-5
    ref_value = np.abs(ref(rms)) if callable(ref) else np.abs(ref)
    db = 10.0 * np.log10(np.maximum(amin ** 2, rms ** 2)) - 10.0 * np.log10(max(amin ** 2, ref_value ** 2))
    ns = db > -top_db
    edges = [np.flatnonzero(np.diff(ns.astype(int))) + 1]
    if ns[0]:
        edges.insert(0, np.array([0]))
    if ns[-1]:
        edges.append(np.array([len(ns)]))
    e = np.concatenate(edges) * hop_length
    e = np.minimum(e, y.shape[-1])
    return e.reshape((-1, 2))


# ---- reference helpers ----------------------------------------------------
def si_sdr(est: np.ndarray, ref: np.ndarray) -> float:
    """Scale-invariant SDR, sep/helpers/eval_utils.py:11-39."""
    rss = np.dot(ref, ref)
    a = np.dot(ref, est) / rss
    target = a * ref
    resid = est - target
    return 10 * math.log10((target ** 2).sum() / ((resid ** 2).sum() + MIN_ERR))


def split_wav(wav: np.ndarray, top_db: float = 18):
    """Voiced segments of 1000..4000 samples, sep/helpers/eval_utils.py:43-70."""
    lo, hi = 1000, 4000
    rms = frame_rms(wav, 1024, 256)
    peak = np.amax(rms)
    if peak < 0.04:
        iv = nonsilent_intervals(wav, top_db=top_db, ref=0.04, frame_length=1024, hop_length=256, rms=rms)
    else:
        iv = nonsilent_intervals(wav, top_db=top_db, frame_length=1024, hop_length=256, rms=rms)
    segs = []
    for a, b in iv:
        n = b - a
        if n < lo:
            continue
        if n > hi:
            k = n // hi
            for i in range(k):
                segs.append([a + i * hi, b if i >= k - 1 else a + (i + 1) * hi])
        else:
            segs.append([a, b])
    return segs


# ---- voiced segments, stated for a kernel (csrc/misc_kernels.hip: asw_voiced_segments) --------
VOICED_A2 = 1e-10                       # amin**2 of nonsilent_intervals
VOICED_Q = 0.04 * 0.04                  # split_wav's quiet bound on the peak RMS, squared


def _frame_ms_f64(wav: np.ndarray) -> np.ndarray:
    """Mean square of librosa's centred, zero-padded 1024 / 256 frames, [1 + T//256] float64, in one fixed order of
    additions: the 256-sample block sums come from 64 partial sums of 4 consecutive samples each and a six-step
    butterfly over them (what a 64-lane wavefront does), and a frame is the sum of its four blocks, left to right."""
    y = np.ascontiguousarray(wav, dtype=np.float32).astype(np.float64)
    T = y.shape[0]
    nblk = -(-T // 256)
    q = np.zeros(nblk * 256, dtype=np.float64)
    q[:T] = y * y                                   # exact: a float32 squared fits a double
    q = q.reshape(nblk, 64, 4)
    p = ((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3]
    for s in (32, 16, 8, 4, 2, 1):
        p = p[:, :s] + p[:, s:2 * s]
    nfr = 1 + T // 256
    b = np.zeros(nfr + 3, dtype=np.float64)         # b[k] = block k - 2; blocks outside [0, nblk) are 0
    b[2:2 + nblk] = p[:, 0]
    return (((b[0:nfr] + b[1:nfr + 1]) + b[2:nfr + 2]) + b[3:nfr + 3]) / 1024.0


def _voiced_reference(ms: np.ndarray, top_db: float):
    """(thr, ref2) of the decision ``max(A2, ms[f]) > thr * ref2``."""
    thr = 10.0 ** (-float(top_db) / 10.0)
    peak2 = float(np.max(ms))
    ref2 = max(VOICED_A2, VOICED_Q) if peak2 < VOICED_Q else max(VOICED_A2, peak2)
    return thr, ref2


def voiced_segments_f64(wav: np.ndarray, top_db: float = 18.0):
    """``split_wav`` restated in float64 without logarithms, so that a kernel reproduces it bit for bit: returns
    (segments as a list of [start, end], ms [1 + T//256] float64).  Frame f is voiced iff
    ``max(A2, ms[f]) > thr * ref2`` with ``thr = 10 ** (-top_db / 10)`` and ``ref2`` the peak mean square (``Q`` when the
    peak lies below it); maximal voiced runs [f0, f1) become the intervals [min(256 f0, T), min(256 f1, T)), and
    the intervals are cut as in ``split_wav``: shorter than 1000 samples dropped, longer than 4000 cut into
    ``n // 4000`` pieces of which the last takes the remainder.  The segments are ascending, disjoint and at least
    1000 samples long, so there are at most ``T // 1000`` of them."""
    T = int(np.shape(wav)[0])
    ms = _frame_ms_f64(wav)
    thr, ref2 = _voiced_reference(ms, top_db)
    voiced = np.maximum(VOICED_A2, ms) > thr * ref2
    edges = np.flatnonzero(np.diff(np.concatenate([[False], voiced, [False]]).astype(np.int8)))
    segs = []
    for f0, f1 in edges.reshape(-1, 2):
        a, b = min(256 * int(f0), T), min(256 * int(f1), T)
        n = b - a
        if n < 1000:
            continue
        if n > 4000:
            k = n // 4000
            for i in range(k):
                segs.append([a + 4000 * i, b if i == k - 1 else a + 4000 * (i + 1)])
        else:
            segs.append([a, b])
    return segs, ms


def voiced_margin_db(wav: np.ndarray, top_db: float = 18.0) -> float:
    """Smallest distance in dB (float64) of any frame's level from the decision threshold of
    ``voiced_segments_f64`` and of the peak from the quiet bound ``Q``: how far a waveform is from a decision that
    another rounding of the same levels could take differently.  For the tests."""
    ms = _frame_ms_f64(wav)
    thr, ref2 = _voiced_reference(ms, top_db)
    with np.errstate(divide="ignore"):
        frames = np.abs(10.0 * np.log10(np.maximum(VOICED_A2, ms) / (thr * ref2)))
        peak = abs(10.0 * np.log10(np.float64(np.max(ms)) / VOICED_Q))
    return float(min(np.min(frames), peak))


def split_wise_sisdr(est, ref, segments):
    """sep/helpers/eval_utils.py:73-82."""
    assert len(segments) > 0
    return [si_sdr(est[a:b], ref[a:b]) for a, b in segments]


def max_avg_power(x: np.ndarray, window_size: int = 12000) -> float:
    """max over start index of sqrt(mean(x^2 over a forward window, zero padded));
    sep/helpers/local_utils_3d.py:13-17 (value only)."""
    sq = (x ** 2).astype(np.float64)
    c = np.concatenate([[0.0], np.cumsum(sq)])
    n = sq.shape[0]
    hi = np.minimum(np.arange(n) + window_size, n)
    return float(np.sqrt(np.abs((c[hi] - c[:n]) / window_size)).max())


def mean_removed_energies(sep: np.ndarray, in_place: bool = False):
    """The reference's host energy loop over the candidate outputs ``sep`` [N,T] (local_utils_3d.py:349-354 /
    Mic_Array.py:290-295): per row the mean is removed, then power = ``np.sum(x ** 2)`` in the array's own dtype and
    power2 = ``max_avg_power(x)``.  -> (powers, powers2), two lists of N scalars.  ``in_place``: the mean-removed row
    is written back into ``sep`` (Mic_Array.py:291 -- the fine stage hands these rows on as the heads' audio);
    otherwise ``sep`` is left as it is."""
    powers, powers2 = [], []
    for i in range(sep.shape[0]):
        x = sep[i, :] - np.mean(sep[i, :])
        if in_place:
            sep[i, :] = x
            x = sep[i, :]
        powers.append(np.sum(x ** 2))
        powers2.append(max_avg_power(x))
    return powers, powers2
