"""The oracle mask baselines of the reference's evaluation -- the ideal ratio mask (sep/helpers/irm.py: do_irm) and the
ideal binary mask (sep/helpers/ibm.py: do_ibm) -- and the STFT / inverse STFT they rest on, restated in numpy float64
with ``numpy.fft`` only.  Torch-free host code: the statements ``asw_stft``, ``asw_istft`` and ``asw_oracle_masks``
(csrc/stft_kernels.hip) are pinned to.

The reference calls ``scipy.signal.stft(x, nperseg=2048)`` and ``scipy.signal.istft(Y)`` with every other argument at
its default.  Spelled out:

forward   periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / 2048), hop 1024, one-sided (1025 bins); the signal is
          extended by 1024 zeros on each side and zero-padded at the end to a whole number of hops, which gives
          F = ceil(N / 1024) + 1 frames (``frame_count``); every spectrum is divided by sum(w).
inverse   one-sided inverse FFT (the imaginary parts of bins 0 and 1024 do not count), times w * sum(w), overlap-add,
          divided sample by sample by the overlap-added w^2 where that exceeds 1e-10, the first and last 1024 samples
          removed; the caller keeps the first N.  Inside the kept range every sample is covered by exactly two frames,
          so the divisor is the 1024-entry table w[r + 1024]^2 + w[r]^2 -- not a constant.

For N < 2048 scipy silently shrinks the window to the signal; the statements and the device refuse instead
(``ValueError``)."""
import numpy as np

NFFT, HOP, NBINS = 2048, 1024, 1025
EPS = float(np.finfo(np.float64).eps)
KINDS = ("irm", "ibm")


def window():
    """(w [2048], sum(w)): the periodic Hann window of the analysis and its sum."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)
    return w, float(np.sum(w))


def synthesis_tables():
    """(w * sum(w) [2048], divisor [1024]): what a frame of the inverse is multiplied by, and the overlap-added w^2 of
    the two frames that cover a sample at offset r in its hop -- the earlier frame first, as the overlap-add runs --
    replaced by 1 where it does not exceed 1e-10 (nowhere, for this window)."""
    w, wsum = window()
    norm = w[HOP:] ** 2 + w[:HOP] ** 2
    return w * wsum, np.where(norm > 1e-10, norm, 1.0)


def frame_count(N: int) -> int:
    """Frames of the STFT of N samples: (L - 2048) / 1024 + 1 with L = N + 2048 padded up to a whole hop."""
    N = int(N)
    if N < NFFT:
        raise ValueError(f"N = {N} samples are fewer than the window of {NFFT}")
    return -(-N // HOP) + 1


def _rows_f64(x, what):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)          # float32 values, widened exactly
    if x.ndim != 2:
        raise ValueError(f"{what} {x.shape} is not [rows, N]")
    return x


def stft_f64(x):
    """x [R, N] -> complex128 [R, 1025, F], as ``scipy.signal.stft(x, nperseg=2048)[2]``."""
    x = _rows_f64(x, "x")
    R, N = x.shape
    F = frame_count(N)
    w, wsum = window()
    padded = np.zeros((R, (F + 1) * HOP))
    padded[:, HOP:HOP + N] = x
    frames = np.stack([padded[:, f * HOP:f * HOP + NFFT] for f in range(F)], axis=1)        # [R, F, 2048]
    return np.ascontiguousarray(np.transpose(np.fft.rfft(frames * w, axis=-1) / wsum, (0, 2, 1)))


def istft_f64(Z, N: int):
    """Z complex [R, 1025, F] -> [R, N] float64, as ``scipy.signal.istft(Z)[1][..., :N]``; N <= (F - 1) * 1024."""
    Z = np.asarray(Z, dtype=np.complex128)
    if Z.ndim != 3 or Z.shape[1] != NBINS or Z.shape[2] < 2:
        raise ValueError(f"Z {Z.shape} is not [rows, {NBINS}, F >= 2]")
    R, _, F = Z.shape
    N = int(N)
    if not 0 <= N <= (F - 1) * HOP:
        raise ValueError(f"N = {N} outside 0..{(F - 1) * HOP}, what {F} frames cover")
    synth, _ = synthesis_tables()
    w, _wsum = window()
    y = np.fft.irfft(Z, n=NFFT, axis=1) * synth[None, :, None]                              # [R, 2048, F]
    x, norm = np.zeros((R, (F + 1) * HOP)), np.zeros((F + 1) * HOP)
    for f in range(F):
        x[:, f * HOP:f * HOP + NFFT] += y[:, :, f]
        norm[f * HOP:f * HOP + NFFT] += w ** 2
    x, norm = x[:, HOP:-HOP], norm[HOP:-HOP]
    return np.ascontiguousarray((x / np.where(norm > 1e-10, norm, 1.0))[:, :N])


def _mask_inputs(gt, mix):
    gt, mix = _rows_f64(gt, "gt"), np.asarray(mix, dtype=np.float32).astype(np.float64)
    if mix.ndim != 1 or gt.shape[1] != mix.shape[0]:
        raise ValueError(f"gt {gt.shape} and mix {mix.shape} are not [S, N] and [N]")
    if gt.shape[0] == 0:
        raise ValueError("no ground-truth rows (S = 0)")
    frame_count(mix.shape[0])
    return gt, mix


def irm_f64(gt, mix, alpha: float = 1.0):
    """The ideal ratio mask estimates [S, N] float64 (``do_irm``): mask_j = |S_j|^alpha / (eps + sum_k |S_k|^alpha) --
    the sum taken in source order, starting from eps -- and Y_j = X mask_j, with X the STFT of ``mix`` [N] and S_k those
    of the rows of ``gt`` [S, N]; eps = np.finfo(np.float64).eps."""
    gt, mix = _mask_inputs(gt, mix)
    X = stft_f64(mix[None])[0]
    P = np.abs(stft_f64(gt)) ** float(alpha)
    model = EPS
    for j in range(gt.shape[0]):
        model = model + P[j]
    return istft_f64(X[None] * (P / model), mix.shape[0])


def ibm_f64(gt, mix, alpha: float = 1.0, theta: float = 0.5):
    """The ideal binary mask estimates [S, N] float64 (``do_ibm``): r_j = |S_j|^alpha / (eps + |X|^alpha), mask_j = 1
    where r_j >= theta and 0 otherwise, Y_j = X mask_j.  The reference gives ``alpha`` and ``theta`` no defaults;
    alpha = 1.0 and theta = 0.5 are this project's."""
    gt, mix = _mask_inputs(gt, mix)
    X = stft_f64(mix[None])[0]
    r = np.abs(stft_f64(gt)) ** float(alpha) / (EPS + np.abs(X) ** float(alpha))
    mask = np.where(r >= float(theta), 1.0, r)              # the reference's two assignments, in its order: with
    mask = np.where(mask < float(theta), 0.0, mask)         # theta > 1 the ones of the first fall to the second
    return istft_f64(X[None] * mask, mix.shape[0])


def ibm_ratio_f64(gt, mix, alpha: float = 1.0):
    """r_j of ``ibm_f64`` [S, 1025, F]: what a test looks at to see how far its inputs are from the threshold."""
    gt, mix = _mask_inputs(gt, mix)
    return np.abs(stft_f64(gt)) ** float(alpha) / (EPS + np.abs(stft_f64(mix[None])[0]) ** float(alpha))


def check_kind(kind):
    if kind not in KINDS:
        raise ValueError(f"oracle mask must be one of {KINDS}, got {kind!r}")


def masks_f64(gt, mix, kind, alpha: float = 1.0, theta: float = 0.5):
    """``irm_f64`` or ``ibm_f64`` by name."""
    check_kind(kind)
    return irm_f64(gt, mix, alpha) if kind == "irm" else ibm_f64(gt, mix, alpha, theta)
