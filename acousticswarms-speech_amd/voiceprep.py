"""Corpus voices as the reference's ``get_voices`` prepares them (datasets/generate_dataset.py:71-127), stated in numpy
float64 so that ``torch.ops.asw.voice_resample`` / ``voice_trim`` (csrc/voice_kernels.hip) reproduce them bit for bit, and
the two array recipes the generator still lacked.

* ``resample_poly_f64``: a polyphase resampler pinned to ``scipy.signal.resample_poly`` (its default Kaiser-5 filter),
  every product and every sum rounded on its own, the taps in ascending order.
* ``trim_f64``: ``librosa.effects.trim`` over centred, zero-padded 2048 / 512 frames, without logarithms and in one fixed
  order of additions (as ``hostdsp.voiced_segments_f64`` restates ``split_wav``), and the variance of the kept span.
* ``clip_voice`` / ``get_voices``: the draws of ``get_voices`` over a ``VoiceIndex`` that holds, per file, what the draws
  depend on (resampled length, trim bounds, acceptance).  The index is filled one speaker directory at a time, so the
  sequential draws need no device round trip of their own.
* ``colocated_array`` and ``draw_three_desks``: the arrays of ``--generate_colocated`` and ``--generate_size``.

Unpinned, as everywhere else here: ``librosa.load`` resamples with ``soxr_hq``, not with this filter; librosa's ``trim``
forms its levels in float32; ``pyroomacoustics.circular_2D_array`` is restated from its documentation.
"""
import json
import math
import os

import numpy as np

TRIM_A2 = 1e-10                 # amin**2 of librosa's power_to_db
MAX_RATIO = 640                 # max(up, down) after reduction: the filter then fits the LDS of one workgroup
ACTIVITY_PAD = 0.2              # seconds kept before and after the trimmed span
MIN_ACTIVITY = 0.5              # seconds of activity a voice must have
MIN_VAR = 2e-4 * 2e-4           # voice_trimmed.std() > 2e-4, squared


# ---- resampling ---------------------------------------------------------------------------------------------------------
def reduced(up, down):
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"up = {up} and down = {down} must be positive")
    g = math.gcd(up, down)
    return up // g, down // g


def resample_filter(up, down):
    """The table ``h`` of ``resample_poly_f64`` (float64 [2 * half + 1], ``half = 10 * max(up, down)`` of the reduced
    ratio): scipy's default design, already scaled by ``up``.  [1.0] for the ratio 1/1."""
    from scipy.signal import firwin
    up, down = reduced(up, down)
    if up == down == 1:
        return np.ones(1, dtype=np.float64)
    big = max(up, down)
    half = 10 * big
    return np.ascontiguousarray(firwin(2 * half + 1, 1.0 / big, window=("kaiser", 5.0)) * up, dtype=np.float64)


def resampled_length(n, up, down):
    up, down = reduced(up, down)
    return -(-int(n) * up // down)


def resample_poly_f64(x, up, down, h=None):
    """``scipy.signal.resample_poly(x, up, down)`` of a 1-D signal as one formula, float64 [ceil(N * up / down)]:

        m = n * down + half;   y[n] = sum_j h[m % up + j * up] * x[m // up - j]

    with j ascending from 0 while the tap index stays <= 2 * half; terms whose sample index lies outside [0, N) are left
    out.  Every product and every sum is rounded on its own, starting from +0.0.  The ratio 1/1 is the identity."""
    up, down = reduced(up, down)
    x = np.ascontiguousarray(x).astype(np.float64)
    N = x.shape[0]
    if up == down == 1:
        return x.copy()
    h = resample_filter(up, down) if h is None else np.asarray(h, dtype=np.float64)
    half = (h.shape[0] - 1) // 2
    n_out = -(-N * up // down)
    m = np.arange(n_out, dtype=np.int64) * down + half
    phase, q = m % up, m // up
    y = np.zeros(n_out, dtype=np.float64)
    for j in range(2 * half // up + 1):
        k, i = phase + j * up, q - j
        ok = (k <= 2 * half) & (i >= 0) & (i < N)
        term = np.zeros(n_out, dtype=np.float64)
        term[ok] = h[k[ok]] * x[i[ok]]
        y = y + term                                    # y + 0.0 is y: y is never -0.0
    return y


def window_f64(y, win_begin, win_len, T_out):
    """What one row of ``voice_resample`` holds: y[win_begin + t] for t < win_len while that index is below len(y), else 0."""
    out = np.zeros(int(T_out), dtype=np.asarray(y).dtype)
    n = max(0, min(int(win_len), int(T_out), len(y) - int(win_begin)))
    out[:n] = y[int(win_begin):int(win_begin) + n]
    return out


# ---- trimming -----------------------------------------------------------------------------------------------------------
def _frame_ms_2048(x32):
    """Mean square of the centred, zero-padded 2048 / 512 frames, [1 + T // 512] float64: a 512-sample block sum comes from
    64 partial sums of 8 consecutive squares, left to right, and a six-step butterfly over them; a frame is its four
    blocks added left to right, divided by 2048."""
    y = np.ascontiguousarray(x32, dtype=np.float32).astype(np.float64)
    T = y.shape[0]
    nblk = -(-T // 512)
    q = np.zeros(nblk * 512, dtype=np.float64)
    q[:T] = y * y                                       # exact: a float32 squared fits a double
    q = q.reshape(nblk, 64, 8)
    p = q[:, :, 0]
    for i in range(1, 8):
        p = p + q[:, :, i]
    for s in (32, 16, 8, 4, 2, 1):
        p = p[:, :s] + p[:, s:2 * s]
    nfr = 1 + T // 512
    b = np.zeros(nfr + 3, dtype=np.float64)             # b[k] = block k - 2; blocks outside [0, nblk) are 0
    b[2:2 + nblk] = p[:, 0]
    return (((b[0:nfr] + b[1:nfr + 1]) + b[2:nfr + 2]) + b[3:nfr + 3]) / 2048.0


def _span_sum(v):
    """Sum of a float64 vector in the order of a 256-thread workgroup: thread t adds v[t], v[t + 256], ... in ascending
    order, then the 256 partial sums go through the butterfly p[:s] + p[s:2s], s = 128 .. 1."""
    n = v.shape[0]
    rows = -(-n // 256)
    a = np.zeros(max(rows, 1) * 256, dtype=np.float64)
    a[:n] = v
    p = np.cumsum(a.reshape(-1, 256), axis=0)[-1]       # a cumulative sum adds strictly in order
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        p = p[:s] + p[s:2 * s]
    return float(p[0])


def span_var_f64(x32, begin, end):
    """Two-pass population variance of x[begin:end] in float64: the mean is ``_span_sum(x) / n``, the variance
    ``_span_sum((x - mean) ** 2) / n``, each difference, square and sum rounded on its own; 0.0 for an empty span."""
    v = np.ascontiguousarray(x32, dtype=np.float32)[begin:end].astype(np.float64)
    n = v.shape[0]
    if n == 0:
        return 0.0
    mean = _span_sum(v) / n
    d = v - mean
    return _span_sum(d * d) / n


def trim_levels(x32, top_db=18.0):
    """(ms, level): frame f is non-silent iff ``max(A2, ms[f]) > level``."""
    ms = _frame_ms_2048(x32)
    thr = 10.0 ** (-float(top_db) / 10.0)
    return ms, thr * max(TRIM_A2, float(np.max(ms)))


def trim_f64(x32, top_db=18.0):
    """``librosa.effects.trim(x, top_db)`` -> (begin, end, peak_ms, var): ``begin = 512 * first`` and
    ``end = min(T, 512 * (last + 1))`` over the non-silent frames, the largest frame mean square, and
    ``span_var_f64(x, begin, end)``.  An all-zero row is non-silent everywhere; T = 0 gives (0, 0)."""
    T = int(np.shape(x32)[0])
    ms, level = trim_levels(x32, top_db)
    on = np.flatnonzero(np.maximum(TRIM_A2, ms) > level)
    if on.size == 0:                                    # only with top_db < 0: the peak frame is non-silent otherwise
        return 0, 0, float(np.max(ms)), 0.0
    begin, end = 512 * int(on[0]), min(T, 512 * (int(on[-1]) + 1))
    return begin, end, float(np.max(ms)), span_var_f64(x32, begin, end)


def accept(begin, end, var, fs):
    """Condition (1) of ``get_voices``: ``voice_trimmed.std() > 2e-4 and end - begin > round(0.5 * fs)``."""
    return bool(var > MIN_VAR and end - begin > int(round(MIN_ACTIVITY * fs)))


# ---- the draws of get_voices --------------------------------------------------------------------------------------------
def clip_voice(rng, n, begin, end, T, fs):
    """The tail of ``get_voices`` -> (win_begin, win_len): the trimmed span [begin, end) of a voice of ``n`` samples, widened
    by 0.2 s and clamped to [0, n]; shorter than T it is kept whole (the caller pads zeros at the end), longer it is cut
    to T samples from one ``rng.choice(L - T)``, equal it costs no draw."""
    pad = int(round(fs * ACTIVITY_PAD))
    b, e = max(begin - pad, 0), min(end + pad, n)
    L = e - b
    if L > T:
        return b + int(rng.choice(L - T)), T
    return b, L


def get_voices(rng, speaker_dirs, n_voices, T, fs, index):
    """``get_voices`` draw for draw -> ([(file, win_begin, win_len)], speaker ids), no audio: ``n_voices`` distinct
    speaker directories, per speaker one ``choice`` over the directory's sorted wav files, repeated until the file's
    index entry is accepted, then ``clip_voice``.  ``index``: ``files(directory)`` and ``entry(path)`` with ``n``,
    ``begin``, ``end``, ``ok`` (a ``VoiceIndex``)."""
    if len(speaker_dirs) < n_voices:
        raise ValueError(f"{n_voices} talkers need as many speaker directories, {len(speaker_dirs)} found")
    picks, ids = [], []
    for d in rng.choice(len(speaker_dirs), n_voices, replace=False):
        directory = speaker_dirs[int(d)]
        files = index.files(directory)
        if not any(index.entry(f)["ok"] for f in files):
            raise ValueError(f"no voice file of {directory} has {MIN_ACTIVITY} s of activity")
        while True:
            path = files[int(rng.choice(len(files)))]
            e = index.entry(path)
            if e["ok"]:
                break
        picks.append((path,) + clip_voice(rng, e["n"], e["begin"], e["end"], T, fs))
        ids.append(os.path.basename(directory.rstrip("/")))
    return picks, ids


def list_speaker_dirs(voices_dir):
    """The directories below ``voices_dir`` that hold wav files themselves, sorted."""
    found = [base for base, _dirs, files in sorted(os.walk(voices_dir)) if any(f.lower().endswith(".wav") for f in files)]
    if not found:
        raise ValueError(f"no wav files below {voices_dir}")
    return found


class VoiceIndex:
    """Per voice file: the source rate ``sr``, the length ``n`` at ``fs``, the trim bounds ``begin`` / ``end`` and ``ok``
    (``accept``).  A speaker directory is filled on the first draw from it: all of its files go through one resample and
    one trim call per source rate (``backend="device"``) or through the statements (``"host"``).  ``path``: a JSON file
    the entries are read from and ``save`` writes to, keyed by file path and valid while size and mtime are unchanged."""

    def __init__(self, fs, backend="device", device="cuda:0", path=None, top_db=18.0):
        if backend not in ("device", "host"):
            raise ValueError(f"backend {backend!r} is neither 'device' nor 'host'")
        self.fs, self.backend, self.device, self.path, self.top_db = int(fs), backend, device, path, float(top_db)
        self._entries, self._files, self._dirty = {}, {}, False
        if path and os.path.exists(path):
            with open(path) as f:
                stored = json.load(f)
            if stored.get("fs") == self.fs and stored.get("top_db") == self.top_db:
                self._entries = stored["files"]

    def files(self, directory):
        if directory not in self._files:
            names = sorted(f for f in os.listdir(directory) if f.lower().endswith(".wav"))
            self._files[directory] = [os.path.join(directory, f) for f in names]
            self._fill(self._files[directory])
        return self._files[directory]

    def entry(self, path):
        if not self._fresh(path):
            self._fill([path])
        return self._entries[path]

    def _fresh(self, path):
        e, st = self._entries.get(path), os.stat(path)
        return e is not None and e["size"] == st.st_size and e["mtime"] == st.st_mtime

    def _fill(self, paths):
        from .room_scenes import read_voice
        todo = [p for p in paths if not self._fresh(p)]
        if not todo:
            return
        audio = [read_voice(p, self.fs, resample=True) for p in todo]
        for (p, (x, sr), (n, begin, end, var)) in zip(todo, audio, prepare([a for a, _ in audio], [s for _, s in audio], self.fs,
                                                                           self.top_db, self.backend, self.device)):
            st = os.stat(p)
            self._entries[p] = {"size": st.st_size, "mtime": st.st_mtime, "sr": int(sr), "n": int(n), "begin": int(begin),
                                "end": int(end), "var": float(var), "ok": accept(begin, end, var, self.fs)}
        self._dirty = True

    def save(self):
        if self.path and self._dirty:
            with open(self.path, "w") as f:
                json.dump({"fs": self.fs, "top_db": self.top_db, "files": self._entries}, f, indent=1)
            self._dirty = False


def prepare(signals, rates, fs, top_db=18.0, backend="device", device="cuda:0"):
    """The index pass: float32 signals at ``rates`` -> [(n, begin, end, var)] of each at ``fs``.  On the device the
    signals of one rate are one ``voice_resample`` call (the whole rows, float32) and one ``voice_trim`` call on its
    result, and only the bounds and the statistics come back."""
    out = [None] * len(signals)
    groups = {}
    for i, sr in enumerate(rates):
        groups.setdefault(int(sr), []).append(i)
    for sr, idx in groups.items():
        if backend == "host":
            for i in idx:
                y = resample_poly_f64(signals[i], fs, sr).astype(np.float32)
                begin, end, _peak, var = trim_f64(y, top_db)
                out[i] = (y.shape[0], begin, end, var)
            continue
        import torch
        from . import native, ops
        lens = [int(signals[i].shape[0]) for i in idx]
        n_out = [resampled_length(n, fs, sr) for n in lens]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        with torch.cuda.device(device):
            x = native.to_device(np.concatenate([signals[i] for i in idx] + [np.zeros(1, dtype=np.float32)]), torch.device(device))
            y = ops.voice_resample(x, offs[:-1], lens, fs, sr, [0] * len(idx), n_out, max(n_out + [1]))
            bounds, stats = ops.voice_trim(y.reshape(-1), [r * y.shape[1] for r in range(len(idx))], n_out, top_db)
            bounds, stats = native.read_back(bounds, stats)
        for r, i in enumerate(idx):
            out[i] = (n_out[r], int(bounds[r, 0]), int(bounds[r, 1]), float(stats[r, 1]))
    return out


def fetch(picks, T, fs, backend="device", device="cuda:0"):
    """The fetch pass: [(file, win_begin, win_len)] -> dry [len(picks), T] float32, row r the ``win_len`` samples of the
    file at ``fs`` from ``win_begin`` on and zeros after them.  On the device (a tensor that stays there) it is one
    ``voice_resample`` call per distinct source rate; on the host a numpy array from the statements."""
    from .room_scenes import read_voice
    audio = [read_voice(p, fs, resample=True) for p, _b, _n in picks]
    if backend == "host":
        dry = np.zeros((len(picks), T), dtype=np.float32)
        for r, ((x, sr), (_p, b, n)) in enumerate(zip(audio, picks)):
            dry[r] = window_f64(resample_poly_f64(x, fs, sr).astype(np.float32), b, n, T)
        return dry
    import torch
    from . import native, ops
    groups = {}
    for r, (_x, sr) in enumerate(audio):
        groups.setdefault(int(sr), []).append(r)
    with torch.cuda.device(device):
        dry = torch.empty((len(picks), T), dtype=torch.float32, device=device)
        for sr, rows in groups.items():
            lens = [int(audio[r][0].shape[0]) for r in rows]
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            x = native.to_device(np.concatenate([audio[r][0] for r in rows] + [np.zeros(1, dtype=np.float32)]), torch.device(device))
            y = ops.voice_resample(x, offs[:-1], lens, fs, sr, [picks[r][1] for r in rows], [picks[r][2] for r in rows], T)
            if len(groups) == 1:
                return y
            dry[torch.tensor(rows, device=device)] = y
    return dry


# ---- the arrays of --generate_colocated and --generate_size -------------------------------------------------------------
ECHO_DOT_DIAMETER = 0.1
THREE_DESKS = (((1.9, 2), (1.1, 1.2)), ((1.4, 1.5), (0.8, 0.9)), ((1, 1.1), (0.5, 0.6)))       # large, middle, small


def colocated_array(rng, center, n_mics, diameter=ECHO_DOT_DIAMETER):
    """[n_mics, 3]: a circle of that diameter around ``center[:2]`` at the robots' height 0.02, microphone k at
    ``center + r * (cos(phi0 + 2 pi k / M), sin(phi0 + 2 pi k / M))`` with one draw ``phi0 = uniform(0, 2 pi)``
    (``colocated_array`` over ``pyroomacoustics.circular_2D_array``, whose parity is unpinned)."""
    from .room_scenes import MIC_HEIGHT
    r = diameter / 2
    phi = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(n_mics) / n_mics
    c = np.asarray(center, dtype=np.float64)
    return np.stack([c[0] + r * np.cos(phi), c[1] + r * np.sin(phi), MIC_HEIGHT * np.ones(n_mics)], axis=1)


def draw_three_desks(rng, n_mics, room):
    """``get_random_mic_positions_three_desks`` draw for draw -> ([large, middle, small] microphones [n_mics, 3] each,
    [[length, width]] * 3, wall): the six desk sides first, then the robot fans of the three desks, then one placement
    (by the large desk's length) shared by all three; all of it is drawn again while any array has a microphone within
    6 cm of a wall."""
    from . import room_scenes as rs
    while True:
        desks = [[rng.uniform(low=lo, high=hi) for lo, hi in sides] for sides in THREE_DESKS]
        fans = [rs._fan_mics(rng, n_mics, length, width) for length, width in desks]
        wall, rot, centre = rs._place_desk(rng, room, desks[0][0])
        placed = [xy.dot(rot) + centre for xy in fans]
        if all(rs._off_the_walls(xy, room) for xy in placed):
            height = rs.MIC_HEIGHT * np.ones((n_mics, 1))
            return [np.concatenate([xy, height], axis=1) for xy in placed], desks, wall
