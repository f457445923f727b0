"""Inputs shared by the BSS-eval SDR tests (host and GPU) and by ``perf_bss_eval.py``: speech-like references and the
three kinds of estimate, all rounded to float32 once so that the device op and ``evalkit.bss_eval_sdr`` read the same
numbers."""
import numpy as np

KINDS = ("noisy", "mixture", "filtered")


def references(rng, S, T):
    """[S, T] float32: noise through a 2nd-order low-pass at a quarter of Nyquist, gated to silence (exact zeros) over
    about a third of its length in runs of T/16 samples, with talker-dependent level."""
    from scipy.signal import butter, lfilter
    b, a = butter(2, 0.25)
    x = lfilter(b, a, rng.standard_normal((S, T + 64)), axis=1)[:, 64:]
    run = max(1, T // 16)
    for s in range(S):
        gate = rng.random(-(-T // run)) < 0.35
        gate[rng.integers(0, gate.size)] = False                       # never silent throughout
        x[s] *= np.repeat(~gate, run)[:T]
        x[s] *= 0.05 * (1.0 + s)
    return np.ascontiguousarray(x, dtype=np.float32)


def estimates(rng, ref, kind):
    """[S, T] float32 estimates of ``ref``: the reference plus noise at -12 dB ("noisy"), the sum of all references
    ("mixture", the unprocessed microphone), or a short FIR of the reference plus a -15 dB leak of the next one
    ("filtered")."""
    S, T = ref.shape
    r64 = ref.astype(np.float64)
    if kind == "noisy":
        rms = np.sqrt(np.mean(r64 ** 2, axis=1, keepdims=True)) + 1e-12
        est = r64 + 0.25 * rms * rng.standard_normal((S, T))
    elif kind == "mixture":
        est = np.repeat(r64.sum(axis=0, keepdims=True), S, axis=0) + 1e-3 * rng.standard_normal((S, T))
    elif kind == "filtered":
        fir = np.array([0.8, 0.3, -0.15, 0.05])
        est = np.stack([np.convolve(r64[s], fir)[:T] + 0.18 * r64[(s + 1) % S] * (S > 1)
                        + 2e-3 * rng.standard_normal(T) for s in range(S)])
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(est, dtype=np.float32)


def make_batch(seed, counts, T, kinds=("mixture", "noisy")):
    """(refs, est_sets): per item ``ref`` [S, T] and ``est`` [R, S, T] with R = len(kinds)."""
    rng = np.random.default_rng([seed, T, len(counts)] + [int(c) for c in counts])
    refs, ests = [], []
    for S in counts:
        ref = references(rng, S, T) if S else np.zeros((0, T), dtype=np.float32)
        refs.append(ref)
        ests.append(np.stack([estimates(rng, ref, k) if S else np.zeros((0, T), dtype=np.float32) for k in kinds]))
    return refs, ests


def pack(refs, ests):
    """The op's layout: ref [N, T], est [R, N, T], counts."""
    counts = [int(r.shape[0]) for r in refs]
    return np.concatenate(refs, axis=0), np.concatenate(ests, axis=1), counts


def host_sdr(refs, ests, flen):
    """[R, N] float64 by ``evalkit.bss_eval_sdr``, item after item."""
    from acousticswarms_speech_amd import evalkit
    R = ests[0].shape[0]
    rows = [[evalkit.bss_eval_sdr(ref, est[r], flen) for ref, est in zip(refs, ests) if ref.shape[0]] for r in range(R)]
    return np.stack([np.concatenate(r) if r else np.zeros(0) for r in rows])
