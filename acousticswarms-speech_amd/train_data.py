"""Training batches: the float64 statements of the perturbation, the roll and the losses.

Host code only (numpy).  These are the definitions the device ops ``ops.colored_noise``, ``ops.train_batch`` and
``ops.train_losses`` (csrc/augment_kernels.hip) are tested against:

* ``pink_from_normals`` restates the reference's ``powerlaw_psd_gaussian`` from its two arrays of unit normals onward;
* ``philox_normals`` is the counter-based generator that stands in for ``numpy.random`` where the device draws the
  noise: the same key, row and index give the same normal on the host and on the device;
* ``perturb_f64`` is ``perturb_audio`` with the two levels and the two keys drawn by the caller;
* ``roll_rows`` is ``shift_mixture_given_samples``;
* ``row_losses_f64`` and ``loss_from_rows`` are ``CompositeLoss``, ``SISDRLoss`` and ``nn.L1Loss`` per row and combined.

``asteroid`` is not a dependency, so ``SingleSrcNegSDR`` is restated here from its published source (zero-mean of both
signals, EPS = 1e-8 in the denominator and inside the logarithm, ``-10 log10``): parity with an installed asteroid is
unpinned.  ``opuslib`` is not a dependency either: ``check_compression_prob`` refuses every ``compression_prob`` that
would ever apply the Opus codec.
"""
import numpy as np

# sep/helpers/constants.py
MAX_SHIFTS = [2, 4]
ROOM_DIM = 6
MAX_SPEAKER_RELATIVE_HEIGHT = 0.8
NEG_SAMPLE_INTIAL_CANDIDATES = 30
CHANNELS_PER_MIC = 1

# ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) --------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
STREAM_PINK, STREAM_WHITE = 0, 1
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or scalars) of 32-bit words, key: two 32-bit words -> four uint64 arrays holding the 32-bit
    output words.  The products are taken in uint64, the high and low words split off."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _MASK32 for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK32]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c


def words_to_uniform(hi, lo):
    """THE word-to-uniform rule (the kernel follows it): the top 52 bits m of the 64-bit word hi:lo give
    u = (2 m + 1) / 2^53 -- an odd numerator below 2^53, so every value is an exactly representable double and lies
    strictly inside (0, 1): 2^-53 for the all-zero words, 1 - 2^-53 for the all-one words."""
    hi = np.asarray(hi, dtype=np.uint64) & _MASK32
    lo = np.asarray(lo, dtype=np.uint64) & _MASK32
    m = (hi << np.uint64(20)) | (lo >> np.uint64(12))
    return (2.0 * m.astype(np.float64) + 1.0) * 2.0 ** -53


def philox_normals(key, row, count, stream=STREAM_PINK):
    """-> (z0, z1), two float64 arrays of ``count`` unit normals.  Index i of row ``row`` is the Philox4x32-10 block of
    counter (i, row, stream, 0) under the 64-bit ``key`` (low word first); its words 0:1 and 2:3 make the uniforms u1, u2
    (``words_to_uniform``) and Box-Muller in float64 makes z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = ... sin(2 pi u2)."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32((np.arange(count, dtype=np.uint64), int(row), int(stream), 0), (key & 0xFFFFFFFF, key >> 32))
    u1, u2 = words_to_uniform(w[0], w[1]), words_to_uniform(w[2], w[3])
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


# ---- the noise --------------------------------------------------------------------------------------------------------
def pink_scale(T, exponent=1.0, fmin=0):
    """-> (s_scale [T//2 + 1], sigma) of ``powerlaw_psd_gaussian``: f^(-exponent/2) with the low-frequency cutoff, and the
    theoretical standard deviation of the output."""
    f = np.fft.rfftfreq(T)
    if not 0 <= fmin <= 0.5:
        raise ValueError("fmin must be chosen between 0 and 0.5.")
    fmin = max(fmin, 1.0 / T)
    ix = int(np.sum(f < fmin))
    if ix and ix < len(f):
        f[:ix] = f[ix]
    s_scale = f ** (-exponent / 2.0)
    w = s_scale[1:].copy()
    w[-1] *= (1 + (T % 2)) / 2.0
    sigma = 2 * np.sqrt(np.sum(w ** 2)) / T
    return s_scale, sigma


def pink_from_normals(sr, si, T, exponent=1.0, fmin=0):
    """``powerlaw_psd_gaussian`` from its two draws onward: sr, si [..., T//2 + 1] unit normals (the reference draws them
    already scaled, ``normal(scale=s_scale)``, which is the unit normal times s_scale) -> [..., T] float64."""
    s_scale, sigma = pink_scale(T, exponent, fmin)
    sr = np.array(sr, dtype=np.float64) * s_scale
    si = np.array(si, dtype=np.float64) * s_scale
    if not T % 2:
        si[..., -1] = 0
        sr[..., -1] *= np.sqrt(2)
    si[..., 0] = 0
    sr[..., 0] *= np.sqrt(2)
    return np.fft.irfft(sr + 1j * si, n=T, axis=-1) / sigma


def colored_noise_f64(key, rows, T, exponent=1.0):
    """The statement of ``ops.colored_noise``: row r is ``pink_from_normals`` of ``philox_normals(key[r], row[r], T//2+1)``.
    ``key``: one integer for all rows, or one per row; ``rows``: a count (rows 0..rows-1) or the row indices."""
    rows = list(range(rows)) if np.isscalar(rows) else [int(r) for r in rows]
    keys = [int(key)] * len(rows) if np.isscalar(key) else [int(k) for k in key]
    assert len(keys) == len(rows)
    out = np.empty((len(rows), T), dtype=np.float64)
    for i, (k, r) in enumerate(zip(keys, rows)):
        z0, z1 = philox_normals(k, r, T // 2 + 1, STREAM_PINK)
        out[i] = pink_from_normals(z0, z1, T, exponent)
    return out


def perturb_f64(x, pink_level, white_level, pink_key, white_key, rounded=True):
    """``perturb_audio`` with its draws named: x [C][T] float32 -> x + white_level w + pink_level p in float64, rounded to
    float32 once (the reference's ``.float()``).  Row c takes w from ``philox_normals(white_key, c, T, STREAM_WHITE)[0]``
    (one normal per sample) and p from ``colored_noise_f64(pink_key, ...)`` row c.  A level of zero leaves its term out.
    ``rounded=False`` returns the float64 sum (tests)."""
    x = np.asarray(x)
    C, T = x.shape
    out = x.astype(np.float64)
    if white_level != 0:
        w = np.stack([philox_normals(white_key, c, T, STREAM_WHITE)[0] for c in range(C)])
        out = out + white_level * w
    if pink_level != 0:
        out = out + pink_level * colored_noise_f64(pink_key, C, T)
    return out.astype(np.float32) if rounded else out


def roll_rows(mix, shifts):
    """``shift_mixture_given_samples``: out[c][t] = mix[c][(t - shifts[c]) mod T]; a row is all zeros when
    |shifts[c]| > T."""
    mix = np.asarray(mix)
    out = np.zeros_like(mix)
    T = mix.shape[-1]
    for c, s in enumerate(shifts):
        if abs(int(s)) <= T:
            out[c] = np.roll(mix[c], int(s))
    return out


def train_batch_f64(mix, item_mix, shifts, counts, pink_level, white_level, pink_key, white_key, rounded=True):
    """The statement of ``ops.train_batch``: mix [K][M][T] float32, shifts [I][S_max][M] -> [I][S_max * M][T].  Block s of
    item i is mixture item_mix[i] rolled by shifts[i][s] for s < counts[i] and zero beyond; the whole item is then
    perturbed (``perturb_f64``), zero blocks included."""
    mix = np.asarray(mix, dtype=np.float32)
    shifts = np.asarray(shifts)
    n_items, S, M = shifts.shape
    T = mix.shape[-1]
    out = np.empty((n_items, S * M, T), dtype=np.float32 if rounded else np.float64)
    for i in range(n_items):
        x = np.zeros((S * M, T), dtype=np.float32)
        for s in range(int(counts[i])):
            x[s * M:(s + 1) * M] = roll_rows(mix[int(item_mix[i])], shifts[i, s])
        out[i] = perturb_f64(x, float(pink_level[i]), float(white_level[i]), int(pink_key[i]), int(white_key[i]), rounded)
    return out


# ---- the losses -------------------------------------------------------------------------------------------------------
EPS = 1e-8
LOSS_PARAMS = {"l1": None, "snr": (0.0, 1.0), "snr_w_scaled_neg": (0.0, 500.0), "fused": (0.05, 1.0), "sisdr": None}   # (r, n)


def snr_loss_f64(est, gt):
    """``SingleSrcNegSDR('snr')`` per row in float64: both signals zero-meaned, -10 log10(sum g^2 / (sum (e - g)^2 + EPS)
    + EPS)."""
    e = np.asarray(est, dtype=np.float64)
    g = np.asarray(gt, dtype=np.float64)
    e = e - e.mean(axis=-1, keepdims=True)
    g = g - g.mean(axis=-1, keepdims=True)
    return -10.0 * np.log10(np.sum(g * g, axis=-1) / (np.sum((e - g) ** 2, axis=-1) + EPS) + EPS)


def sisdr_loss_f64(est, gt):
    """``SingleSrcNegSDR('sisdr')`` per row in float64: the target is scaled by dot / (sum g^2 + EPS) first."""
    e = np.asarray(est, dtype=np.float64)
    g = np.asarray(gt, dtype=np.float64)
    e = e - e.mean(axis=-1, keepdims=True)
    g = g - g.mean(axis=-1, keepdims=True)
    a = np.sum(e * g, axis=-1, keepdims=True) / (np.sum(g * g, axis=-1, keepdims=True) + EPS)
    s = a * g
    return -10.0 * np.log10(np.sum(s * s, axis=-1) / (np.sum((e - s) ** 2, axis=-1) + EPS) + EPS)


def row_losses_f64(est, gt):
    """est, gt [N][T] -> float64 [N][4]: mean |e - g|, the negative SNR, the negative SI-SDR, max |g| -- the statement of
    ``ops.train_losses``."""
    e = np.asarray(est, dtype=np.float64)
    g = np.asarray(gt, dtype=np.float64)
    return np.stack([np.mean(np.abs(e - g), axis=-1), snr_loss_f64(e, g), sisdr_loss_f64(e, g), np.max(np.abs(g), axis=-1)],
                    axis=-1)


def _composite(rows, r, n):
    """``CompositeLoss(r, n)`` from the per-row terms: n times the L1 of the negative rows (max |gt| == 0) plus, over the
    positive rows, r times the L1 and 1 - r times the negative SNR."""
    neg = rows[:, 3] == 0
    loss = 0.0
    if neg.any():
        loss += np.mean(rows[neg, 0]) * n
    if (~neg).any():
        loss += np.mean(rows[~neg, 0]) * r + np.mean(rows[~neg, 1]) * (1 - r)
    return float(loss)


def loss_from_rows(rows, name):
    """The scalar loss the reference's ``set_loss(name)`` would give, from the [N][4] per-row terms.  The row mask is
    max |gt| == 0, as in the reference.  ``sisdr`` over no positive row is nan (the mean of nothing), as there."""
    rows = np.asarray(rows, dtype=np.float64)
    if name not in LOSS_PARAMS:
        raise ValueError(f"loss {name!r}: one of {sorted(LOSS_PARAMS)}")
    if name == "l1":
        return float(np.mean(rows[:, 0]))               # every row has T samples: the mean of the row means
    if name == "sisdr":
        pos = rows[:, 3] != 0
        return float(np.mean(rows[pos, 2])) if pos.any() else float("nan")
    return _composite(rows, *LOSS_PARAMS[name])


def _loss_rows(est, gt):
    """[N][1][t] (localization) or [N][S][t] (separation, reshaped to [N * S][1][t] as the network does) -> [N'][t]."""
    est, gt = np.asarray(est), np.asarray(gt)
    assert est.shape == gt.shape and est.ndim == 3
    return est.reshape(-1, est.shape[-1]), gt.reshape(-1, gt.shape[-1])


def composite_loss(est, gt, r=0.0, n=1.0):
    """``CompositeLoss(r, n)`` in float64."""
    return _composite(row_losses_f64(*_loss_rows(est, gt)), r, n)


def sisdr_loss(est, gt):
    """``SISDRLoss`` in float64."""
    return loss_from_rows(row_losses_f64(*_loss_rows(est, gt)), "sisdr")


def l1_loss(est, gt):
    """``nn.L1Loss()`` in float64."""
    return loss_from_rows(row_losses_f64(*_loss_rows(est, gt)), "l1")


def loss_f64(est, gt, name):
    """The loss of ``set_loss(name)`` for est, gt [N][S][t], in float64."""
    return loss_from_rows(row_losses_f64(*_loss_rows(est, gt)), name)


# ---- codec ------------------------------------------------------------------------------------------------------------
def check_compression_prob(compression_prob, dataset_type):
    """The reference applies the Opus codec with probability ``compression_prob`` on the train set and always on the
    other sets when ``abs(compression_prob) > 1e-6``.  The codec is not available here: any value that would ever apply it
    raises."""
    applies = compression_prob > 0 if dataset_type == "train" else abs(compression_prob) > 1e-6
    if applies:
        raise NotImplementedError(f"compression_prob = {compression_prob} on the {dataset_type!r} set would apply the Opus codec, "
                                  "which this project does not carry; use compression_prob = 0")


# ---- region decisions and the two datasets ------------------------------------------------------------------------------
# Every draw below is made in the reference's order from ``numpy.random`` and ``random``, so that under the same seeds the
# host backend is the reference draw for draw (tests/golden/g18_training_batches.npz records the reference's outputs).
SPEED_OF_SOUND = 343.0


def shift_vector(position, mic_positions, sr):
    """``utils.get_shift_vector`` with reference channel 0: the rounded shifts that align the channels on ``position``."""
    position = np.asarray(position)
    c = [-(np.linalg.norm(position - mic_positions[m], axis=0) * sr / SPEED_OF_SOUND) for m in range(mic_positions.shape[0])]
    return np.round(np.array([v - c[0] for v in c])).astype(np.int32)


def _is_real(metadata):
    return "real" in metadata and metadata["real"] == True          # noqa: E712 -- the reference's own test


def _metadata_shift(entry):
    s = np.array(entry["shifts"])
    s -= s[0]
    return -s


def voice_offsets(metadata, sr):
    """[voices][M] shifts of every talker: from the metadata's ``shifts`` for a real sample, from the positions otherwise."""
    voices = [k for k in metadata if "voice" in k]
    mic_positions = np.array([metadata[k]["position"] for k in metadata if "mic" in k])
    out = np.zeros((len(voices), mic_positions.shape[0]))
    for i, v in enumerate(voices):
        out[i] = _metadata_shift(metadata[v]) if _is_real(metadata) else shift_vector(np.array(metadata[v]["position"]), mic_positions, sr)
    return out, mic_positions


def negative_region(metadata, window_condition, sr):
    """``get_negative_region``: 30 candidates in the box of +/-ROOM_DIM around the array (z in 0..0.8 for 3-D arrays), kept
    when the L-inf distance to every talker exceeds MAX_SHIFTS[w] + 1, one drawn with inverse-L1 weights.
    -> (shifts [M] int32, point)."""
    offsets, mic_positions = voice_offsets(metadata, sr)
    lx, ux = np.min(mic_positions[:, 0]) - ROOM_DIM, np.max(mic_positions[:, 0]) + ROOM_DIM
    ly, uy = np.min(mic_positions[:, 1]) - ROOM_DIM, np.max(mic_positions[:, 1]) + ROOM_DIM
    shifts = []
    while len(shifts) == 0:
        n = NEG_SAMPLE_INTIAL_CANDIDATES
        pts = [np.random.uniform(lx, ux, size=n), np.random.uniform(ly, uy, size=n)]
        if len(mic_positions[0]) == 3:
            pts.append(np.random.uniform(0, MAX_SPEAKER_RELATIVE_HEIGHT, size=n))
        pts = np.array(pts).T
        shifts, distances, points = [], [], []
        for p in pts:
            s = shift_vector(p, mic_positions, sr)
            diff = np.absolute(offsets - s)
            if np.min(np.max(diff, axis=1)) > MAX_SHIFTS[window_condition] + 1:
                shifts.append(s)
                points.append(p)
                distances.append(np.min(np.linalg.norm(diff, ord=1, axis=1)))
    w = np.zeros(len(shifts))
    for i in range(len(shifts)):
        w[i] = np.min(1 / distances[i])
    w /= np.sum(w)
    idx = np.random.choice(len(shifts), p=w)
    return shifts[idx], points[idx]


def negative_region_srp(metadata, window_condition, negative_list, sr):
    """``get_negative_region_SRP``: a mined SRP-PHAT false positive, jittered by +/-2 on its six channels, redrawn until it
    lies outside every talker's patch.  -> shifts [M]."""
    offsets, _ = voice_offsets(metadata, sr)
    width = MAX_SHIFTS[window_condition]
    while True:
        pick = negative_list[np.random.choice([i for i in range(len(negative_list))])]
        s = -1 * np.array([0] + list(pick))
        s[1:] += np.random.choice([-2, -1, 0, 1, 2], 6)
        if all(np.amax(np.abs(offsets[i] - s)) > width + 1 for i in range(offsets.shape[0])):
            return s


def positive_region(metadata, window_condition, training):
    """``get_positive_region``: a random talker's shifts, perturbed by +/-MAX_SHIFTS[w] on a synthetic training sample."""
    import random
    key = random.choice([k for k in metadata if "voice" in k])
    s = _metadata_shift(metadata[key])
    if not _is_real(metadata) and training:
        s += np.random.randint(low=-MAX_SHIFTS[window_condition], high=MAX_SHIFTS[window_condition] + 1, size=s.shape[-1])
        s[0] = 0
    return s


def neg_prob(n_false_positives, n_speakers, negatives, scale_neg_prob):
    """The probability of a negative region: ``negatives``, or with ``scale_neg_prob`` the reference's line through
    (6, 0.3) and (14, 0.5) false positives per talker, clipped to 0.2..0.5."""
    if not scale_neg_prob:
        return negatives
    p = (0.5 - 0.3) / (14 - 6) * (n_false_positives / n_speakers) + 0.15
    return 0.5 if p > 0.5 else 0.2 if p < 0.2 else p


def _wav(path):
    from .evalkit import _read_wav
    return _read_wav(path)


def item_seed(seed, position):
    """What ``batches`` seeds ``random`` and ``numpy.random`` with before the item at ``position`` of an epoch."""
    return (int(seed) * 1000003 + int(position)) % 2 ** 32


class _Decision:
    """What one item is made of before any sample is touched: the sample directory, the shifts of every talker block
    [S][M] (int32; a channel shifted by more than T is a row of zeros), the number of blocks in use, the ground truth
    [S_out][T] float32, the third member of the tuple, and the noise (None on a set that is not perturbed)."""
    __slots__ = ("dir", "mix", "shifts", "count", "gt", "extra", "noise")


class _BaseDataset:
    def __init__(self, input_dir, dataset_type, sr, compression_prob, max_white_noise_variance=1e-3, max_pink_noise_variance=5e-3):
        from pathlib import Path
        self.dirs = sorted(list(Path(input_dir).glob("[0-9]*")))
        self.dataset_type = dataset_type
        self.training = dataset_type == "train"
        check_compression_prob(compression_prob, dataset_type)
        self.compression_prob = compression_prob if self.training else abs(compression_prob) > 1e-6
        self.sr = sr
        self.max_white_noise_variance = max_white_noise_variance
        self.max_pink_noise_variance = max_pink_noise_variance

    def __len__(self):
        return len(self.dirs)

    def _metadata(self, idx):
        import json
        import os
        d = self.dirs[idx % len(self.dirs)]
        with open(os.path.join(d, "metadata.json"), "rb") as f:
            return d, json.load(f)

    def _mixture(self, d, metadata):
        import os
        return np.stack([_wav(os.path.join(d, m) + "_mixed.wav") for m in metadata if "mic" in m])

    def _noise_draws(self, shape, backend):
        """``perturb_audio``'s draws in its order.  host: the reference's own arrays (``default_rng(seed)`` for the pink
        noise, ``numpy.random.normal`` for the white).  device: the seed becomes the pink key, and one more key draw
        stands in place of the white-noise array."""
        pink_level = self.max_pink_noise_variance * np.random.rand()
        seed = np.random.randint(2 ** 31)
        if backend == "host":
            rng = np.random.default_rng(seed)
            size = list(shape[:-1]) + [shape[-1] // 2 + 1]
            sr_, si_ = rng.normal(size=size), rng.normal(size=size)
            pink = pink_from_normals(sr_, si_, shape[-1])
            white_level = self.max_white_noise_variance * np.random.rand()
            return pink_level, pink, white_level, np.random.normal(0, 1, size=shape)
        white_level = self.max_white_noise_variance * np.random.rand()
        return pink_level, int(seed), white_level, int(np.random.randint(2 ** 31))

    def _finish(self, dec, metadata, rows, backend):
        T = dec.mix.shape[-1]
        dec.noise = self._noise_draws((rows, T), backend) if self.training else None
        if not _is_real(metadata):
            np.random.random()                                  # the codec's draw; it never applies here (checked at construction)
        return dec

    def _host_item(self, dec):
        S, M = dec.shifts.shape
        T = dec.mix.shape[-1]
        x = np.zeros((S * M, T), dtype=np.float32)
        for s in range(dec.count):
            x[s * M:(s + 1) * M] = roll_rows(dec.mix, dec.shifts[s])
        if dec.noise is not None:
            pink_level, pink, white_level, white = dec.noise
            x = ((x.astype(np.float64) + white_level * white) + pink_level * pink).astype(np.float32)
        return x

    def __getitem__(self, idx):
        import torch
        dec = self.decide(idx, "host")
        return torch.from_numpy(self._host_item(dec)), torch.from_numpy(dec.gt), self._extra_tensor(dec.extra)

    def batches(self, batch_size, shuffle=False, seed=None, backend="device", device=None):
        """Yield the batch tuples of an epoch.  ``seed``: ``random`` and ``numpy.random`` are seeded from (seed, position in
        the epoch) before every item, so that the decisions of an item do not depend on the backend or the batch size, and
        the order (``shuffle``) comes from a generator of its own.  ``backend="device"``: the decisions are drawn on the
        host, the wavs of a batch are uploaded once, and the tensors come from one ``ops.colored_noise`` call and one
        ``ops.train_batch`` call and stay on ``device``; ``"host"``: ``__getitem__`` stacked."""
        import random
        import torch
        if backend not in ("device", "host"):
            raise ValueError(f"backend must be 'device' or 'host', got {backend!r}")
        order = np.arange(len(self))
        if shuffle:
            np.random.RandomState(seed).shuffle(order)
        for b0 in range(0, len(order), batch_size):
            decs = []
            for pos in range(b0, min(b0 + batch_size, len(order))):
                if seed is not None:
                    random.seed(item_seed(seed, pos))
                    np.random.seed(item_seed(seed, pos))
                decs.append(self.decide(int(order[pos]), backend))
            gt = torch.from_numpy(np.stack([d.gt for d in decs]))
            extra = torch.stack([self._extra_tensor(d.extra) for d in decs])
            if backend == "host":
                yield torch.from_numpy(np.stack([self._host_item(d) for d in decs])), gt, extra
            else:
                dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
                yield self._device_batch(decs, dev), gt.to(dev), extra.to(dev)

    def _device_batch(self, decs, dev):
        import torch
        from . import ops
        dirs = []
        for d in decs:
            if d.dir not in dirs:
                dirs.append(d.dir)
        mix = torch.from_numpy(np.stack([next(d.mix for d in decs if d.dir == p) for p in dirs])).to(dev)
        S, M = decs[0].shifts.shape
        T = mix.shape[-1]
        n = len(decs)
        levels = [(d.noise[0], d.noise[2]) if d.noise is not None else (0.0, 0.0) for d in decs]
        pink = None
        if any(p != 0.0 for p, _ in levels):
            keys = [d.noise[1] if d.noise is not None else 0 for d in decs for _ in range(S * M)]
            pink = ops.colored_noise(keys, list(range(S * M)) * n, T, device=dev).reshape(n, S * M, T)
        return ops.train_batch(mix, [dirs.index(d.dir) for d in decs], np.stack([d.shifts for d in decs]), [d.count for d in decs],
                               [p for p, _ in levels], [w for _, w in levels], [d.noise[3] if d.noise is not None else 0 for d in decs],
                               pink=pink)


class LocalizationDataset(_BaseDataset):
    """The reference's ``SpeakerLocalization.dataset.Dataset``: ``(data [M][T], gt [1][T], width [2])`` per item -- a
    positive region (a talker's shifts) or a negative one (a random point, or a mined SRP-PHAT false positive from
    ``challeng_sample.json``), the mixture rolled by the region's shifts, and on the train set white and pink noise."""

    def __init__(self, input_dir, dataset_type, n_mics=7, sr=48000, negatives=0.3, max_white_noise_variance=1e-3,
                 max_pink_noise_variance=5e-3, compression_prob=0.7, fixed_window_condition=-1, challenge_ratio=0.8,
                 use_dereverb=False, use_denoised=False, scale_neg_prob=False):
        super().__init__(input_dir, dataset_type, sr, compression_prob, max_white_noise_variance, max_pink_noise_variance)
        self.n_mics = n_mics
        self.window_condition = fixed_window_condition
        self.negatives = negatives
        self.challenge_ratio = challenge_ratio
        self.scale_neg_prob = scale_neg_prob
        self.dereverb = use_dereverb
        self.use_denoised = use_denoised

    def _extra_tensor(self, extra):
        import torch
        onehot = np.zeros(2)
        onehot[extra] = 1
        return torch.from_numpy(onehot).float()

    def decide(self, idx, backend="host"):
        import json
        import os
        d, metadata = self._metadata(idx)
        real = _is_real(metadata)
        if not real:
            for key in metadata:
                if key.startswith("voice"):
                    metadata[key]["shifts"] = [0] + metadata[key]["shifts"]
        w = np.random.randint(2) if self.window_condition < 0 else self.window_condition
        with open(os.path.join(d, "challeng_sample.json")) as f:
            false_positives = json.load(f)["negative_sample"]
        voices = [k for k in metadata if "voice" in k]
        p_neg = neg_prob(len(false_positives), len(voices), self.negatives, self.scale_neg_prob)
        if np.random.uniform() < p_neg:
            target = None
            if np.random.uniform() < self.challenge_ratio and len(false_positives) > 0:
                target = negative_region_srp(metadata, w, false_positives, self.sr)
            if target is None:
                target, _ = negative_region(metadata, w, self.sr)
            pos = False
        else:
            target = positive_region(metadata, w, self.training)
            pos = True
        dec = _Decision()
        dec.dir, dec.mix, dec.extra, dec.count = d, self._mixture(d, metadata), int(w), 1
        T = dec.mix.shape[-1]
        target = np.round(target).astype(np.int32)
        assert target[0] == 0, f"Sample shift on reference microphone should be equal to 0. Found {target[0]}."
        dec.shifts = target[None, :].copy()
        target[np.abs(target) > T] = T        # shift_mixture_given_samples zeroes such a row and writes T back into the shift
        # the closest talker within MAX_SHIFTS[w] (L-inf) is the ground truth
        included = []
        for i, v in enumerate(voices):
            dist = np.linalg.norm(_metadata_shift(metadata[v]) - target, ord=np.inf)
            if dist <= MAX_SHIFTS[w]:
                included.append((dist, i))
        included = sorted(included, key=lambda x: x[0])
        dec.gt = np.zeros((1, T), dtype=np.float32)
        if included:
            mic0 = [k for k in metadata if "mic" in k][0]
            base = os.path.join(d, mic0 + "_" + str(voices[included[0][1]]))
            if self.use_denoised:
                path = base + "_denoised.wav" if os.path.exists(base + "_denoised.wav") else base + ".wav"
            else:
                path = base + ("_dereverb" if self.dereverb else "") + ".wav"
            dec.gt = _wav(path)[None, :]
        self._finish(dec, metadata, dec.mix.shape[0], backend)
        if pos:
            assert (dec.gt > 0).any()
        else:
            assert (dec.gt == 0).all()
        return dec


class SeparationDataset(_BaseDataset):
    """The reference's ``SpeakerSeparation.dataset.Dataset``: ``(data [S*M][T], gt [S][T], n_speakers)`` per item -- one
    block of M rolled channels per talker (shuffled; on the train set one may be dropped and a fake one added at a
    negative region, and every talker's shifts are perturbed by +/-MAX_SHIFTS[0]), zero blocks for the missing talkers,
    and on the train set noise over the whole tensor, zero blocks included."""

    def __init__(self, input_dir, dataset_type, n_mics=7, n_speakers=5, sr=48000, compression_prob=0.7,
                 max_white_noise_variance=1e-3, max_pink_noise_variance=5e-3, speaker_drop_prob=0.1, speaker_add_prob=0.1):
        super().__init__(input_dir, dataset_type, sr, compression_prob, max_white_noise_variance, max_pink_noise_variance)
        self.n_mics = n_mics
        self.n_speakers = n_speakers
        self.speaker_drop_prob = speaker_drop_prob
        self.speaker_add_prob = speaker_add_prob

    def _extra_tensor(self, extra):
        import torch
        return torch.tensor(extra)

    def __getitem__(self, idx):
        data, gt, n = super().__getitem__(idx)
        return data, gt, int(n)

    def decide(self, idx, backend="host"):
        import os
        import random
        d, metadata = self._metadata(idx)
        real = _is_real(metadata)
        voices = [k for k in metadata if "voice" in k]
        if self.training:
            random.shuffle(voices)
            if random.random() < self.speaker_drop_prob:
                voices.pop()
                random.shuffle(voices)
            if len(voices) < self.n_speakers:
                if random.random() < self.speaker_add_prob:
                    voices.append("fake_voice")
                    fake_shifts, fake_pos = negative_region(metadata, 1, self.sr)
                    metadata["fake_voice"] = dict(position=fake_pos, shifts=-fake_shifts)
                    random.shuffle(voices)
        mics = [k for k in metadata if "mic" in k]
        mic_positions = np.array([metadata[k]["position"] for k in mics])
        assert len(voices) <= self.n_speakers, f"Dataset has too many speakers\nExpected <= {self.n_speakers}. Found {len(voices)}"
        dec = _Decision()
        dec.dir, dec.mix, dec.extra, dec.count = d, self._mixture(d, metadata), len(voices), len(voices)
        T = dec.mix.shape[-1]
        dec.shifts = np.zeros((self.n_speakers, self.n_mics), dtype=np.int32)
        dec.gt = np.zeros((self.n_speakers, T), dtype=np.float32)
        for i, v in enumerate(voices):
            if v != "fake_voice":
                base = os.path.join(d, mics[0] + "_" + str(v))
                dec.gt[i] = _wav(base + "_denoised.wav" if os.path.exists(base + "_denoised.wav") else base + ".wav")
            shift = _metadata_shift(metadata[v]) if real else shift_vector(np.array(metadata[v]["position"]), mic_positions, self.sr)
            if self.training and not real:
                jitter = np.random.randint(low=-MAX_SHIFTS[0], high=MAX_SHIFTS[0] + 1, size=shift.shape[-1])
                jitter[0] = 0
                shift += jitter
            dec.shifts[i] = shift.astype(np.int32)
        return self._finish(dec, metadata, self.n_speakers * self.n_mics, backend)


# ---- hard negatives ---------------------------------------------------------------------------------------------------
def label_patches(sample_offsets, sample_offsets_gt):
    """``check_label`` of generate_SRP_sample.py: a patch offset [M-1] is positive when some talker's ground-truth offsets
    [M-1][S] lie within 4.9 samples of it on every channel.  -> (negatives, positives), lists of lists."""
    negatives, positives = [], []
    for sample in sample_offsets:
        sample = np.asarray(sample)
        inside = any(np.amax(np.abs(sample_offsets_gt[:, i] - sample)) < 4.9 for i in range(sample_offsets_gt.shape[1]))
        (positives if inside else negatives).append(sample.tolist())
    return negatives, positives


def mine_negatives(dataset_dir, sample_number=1, start=0, seconds=3.0, device=None, mic_array=None):
    """The counterpart of datasets/generate_SRP_sample.py: for samples ``start`` .. ``start + sample_number - 1`` of
    ``dataset_dir`` run ``MicArray(..., Prone_method="SRP", grid_size=0.065).Apply_SRP_PHAT`` on the first ``seconds`` of
    the mixture, label every patch's ``sample_offset`` against the ground-truth offsets and write
    ``challeng_sample.json`` ({"negative_sample", "positive_sample"}) into the sample directory.  A sample without
    ``metadata.json`` is skipped with a warning.  ``mic_array``: the pruner's constructor (tests pass a stub).
    -> {sample directory: (negatives, positives)}."""
    import json
    import os
    import warnings
    from . import evalkit
    from .patch import FS
    if mic_array is None:
        from .mic_array import MicArray as mic_array
    done = {}
    for idx in range(start, start + sample_number):
        d = os.path.join(dataset_dir, f"{idx:05d}")
        if not os.path.exists(os.path.join(d, "metadata.json")):
            warnings.warn(f"{d}: no metadata.json, sample skipped")
            continue
        metadata, mix, _gt = evalkit.get_items(d)
        _mics, mic_positions, _voices, _pos, offsets_gt, roi = evalkit.preprocess_metadata(metadata)
        if _is_real(metadata):
            for j, v in enumerate(_voices):
                s = np.array(metadata[v]["shifts"])
                offsets_gt[:, j] = (s - s[0])[1:]
        kw = {} if device is None else {"device": device}
        array = mic_array(mic_positions, Spk_Range=list(metadata["ROI"]), Prone_method="SRP", grid_size=0.065, **kw)
        patches, _ = array.Apply_SRP_PHAT(mix[:, :int(seconds * FS)])
        negatives, positives = label_patches([p.sample_offset for p in patches], offsets_gt)
        with open(os.path.join(d, "challeng_sample.json"), "w") as f:
            json.dump({"negative_sample": negatives, "positive_sample": positives}, f, indent=4)
        done[d] = (negatives, positives)
    return done


# ---- validation ---------------------------------------------------------------------------------------------------------
VAL_SEED = 0


def normalize_input(data):
    """``normalize_input`` of both networks, per item: 16-bit rounding, then the mean and standard deviation of the
    channel average.  data [B][C][T] tensor -> (normalised, means, stds)."""
    data = (data * 2 ** 15).round() / 2 ** 15
    ref = data.mean(1)
    means = ref.mean(1).unsqueeze(1).unsqueeze(2)
    stds = ref.std(1).unsqueeze(1).unsqueeze(2)
    return (data - means) / stds, means, stds


def forward_batch(model, data, extra):
    """One validation forward: normalise per item, ``model.forward`` (SpotModel takes the window one-hot, SepModel the
    talker counts), un-normalise.  -> [B][S_out][T] on the model's device."""
    import torch
    data = torch.as_tensor(data).to(model.device)
    normed, means, stds = normalize_input(data)
    third = extra if extra.dim() == 2 else extra.reshape(-1, 1)
    return model.forward(normed, third) * stds + means


def validate(model, dataset, loss="snr", batch_size=8, backend="device", losses=None):
    """``test_epoch`` of both trainers: seed with VAL_SEED, run the dataset in order through ``forward_batch``, take the
    loss ``loss`` (a ``set_loss`` name) of every batch from ``ops.train_losses`` (the separation network's [N][S][t] is
    reshaped to [N * S][1][t] as its ``loss`` does) and average over the batches; the SI-SDR of the input's first channel
    and of the output against every positive row go through ``hostdsp.si_sdr``.  ``losses``: the per-row op (tests pass the
    float64 statement).  -> {"loss", "batch_losses", "input_si_sdr", "output_si_sdr"}."""
    from . import hostdsp, native
    if loss not in LOSS_PARAMS:
        raise ValueError(f"loss {loss!r}: one of {sorted(LOSS_PARAMS)}")
    if losses is None:
        from .ops import train_losses as losses
    batch_losses, si_in, si_out = [], [], []
    for data, gt, extra in dataset.batches(batch_size, shuffle=False, seed=VAL_SEED, backend=backend, device=model.device):
        out = forward_batch(model, data, extra)
        gt = gt.to(out.device)
        t = gt.shape[-1]
        rows = losses(out.reshape(-1, t).contiguous(), gt.reshape(-1, t).contiguous())
        batch_losses.append(loss_from_rows(native.to_host(rows) if hasattr(rows, "is_cuda") else rows, loss))
        first = data.to(out.device)[:, :1, :].expand(-1, gt.shape[1], -1).reshape(-1, t)
        o, g, x = native.read_back(out.reshape(-1, t), gt.reshape(-1, t), first)
        for r in np.nonzero(np.abs(g).max(axis=1) > 0)[0]:
            si_in.append(hostdsp.si_sdr(x[r].astype(np.float64), g[r].astype(np.float64)))
            si_out.append(hostdsp.si_sdr(o[r].astype(np.float64), g[r].astype(np.float64)))
    return {"loss": float(np.mean(batch_losses)), "batch_losses": batch_losses, "input_si_sdr": si_in, "output_si_sdr": si_out}
