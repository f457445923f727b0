"""Float64 numpy restatement of the reference's MUSIC and TOPS pruning maps
(sep/Traditional_SP/SRP_Prunning.py:436-497, MUSIC_block.py, TOPS_block.py:62-136).

Test-side only: the fixtures store the spread between the reference's own (complex64) map and
this restatement, and the GPU tests compare the HIP maps against both.  The geometry comes from
an ``SRPPhat`` node (``tau``, ``omega``, ``tops_delta``, ``tops_coef``, ``freq_bins``).
"""
import numpy as np

from acousticswarms_speech_amd.hostdsp import stft_frames

NUM_SRC = 3
TOPS_WINDOW = 72000


def whole_windows(T, window):
    return T // window


def window_stft(mix, start, window, nfft):
    """[M, nfft//2+1, frames] of one window (rectangular, hop nfft/4), float64 arithmetic."""
    seg = np.asarray(mix[:, start:start + window], dtype=np.float64)
    return np.stack([stft_frames(x, nfft, nfft // 4).T for x in seg])


def covariance(X, freq_bins):
    """C[k] = mean_frames X X^H per bin [nbins, M, M] and sum_m sum_f |X| per bin."""
    Xb = X[:, freq_bins, :]                                    # [M, K, F]
    C = np.einsum("mkf,nkf->kmn", Xb, np.conj(Xb)) / Xb.shape[2]
    return C, np.abs(Xb).sum(axis=(0, 2))


def music_window(X, freq_bins, tau, omega):
    C, _ = covariance(X, freq_bins)
    _, v = np.linalg.eigh(C)
    En = v[..., :-NUM_SRC]                                     # [K, M, M-3]
    P = np.zeros((len(freq_bins), tau.shape[0]))
    for k in range(len(freq_bins)):
        a = np.exp(1j * omega[k] * tau)                        # [G, M]
        P[k] = 1.0 / np.sum(np.abs(a @ np.conj(En[k])) ** 2, axis=1)
    P /= P.max(axis=1, keepdims=True)
    return P.mean(axis=0)


def music_map(mix, window, node):
    n = whole_windows(mix.shape[1], window)
    out = np.zeros(node.tau.shape[0])
    for j in range(n):
        out += music_window(window_stft(mix, j * window, window, node.n_fft), node.freq_bins, node.tau, node.omega)
    return out / n


def tops_window(X, freq_bins, delta, coef, chunk=512):
    """-> (values [G], max_bin)."""
    C, mag = covariance(X, freq_bins)
    max_bin = int(np.argmax(mag))
    f0 = int(freq_bins[max_bin])
    _, v = np.linalg.eigh(C)
    F0 = v[max_bin][:, -NUM_SRC:]                              # [M, 3]
    K = len(freq_bins) - 1
    W = v[:K, :, :-NUM_SRC]                                    # [K, M, M-3]
    Q = np.einsum("ms,kmn->ksnm", np.conj(F0), W)              # [K, 3, M-3, M]
    kk = np.arange(K) - f0
    G = delta.shape[0]
    vals = np.zeros(G)
    for g0 in range(0, G, chunk):
        d = delta[g0:g0 + chunk]
        phi = np.exp(1j * coef * kk[None, :, None] * d[:, None, :])   # [g, K, M]
        B = np.einsum("ksnm,gkm->gskn", Q, np.conj(phi))               # [g, 3, K, M-3]
        D = B.reshape(B.shape[0], NUM_SRC, -1)
        vals[g0:g0 + chunk] = 1.0 / np.linalg.svd(D, compute_uv=False)[:, -1]
    return vals, max_bin


def tops_map(mix, node):
    """-> (map [G], max_bin per window)."""
    n = whole_windows(mix.shape[1], TOPS_WINDOW)
    out, bins = np.zeros(node.tops_delta.shape[0]), []
    for j in range(n):
        X = window_stft(mix, j * TOPS_WINDOW, TOPS_WINDOW, node.n_fft)
        v, b = tops_window(X, node.freq_bins, node.tops_delta, node.tops_coef)
        out += v
        bins.append(b)
    return out / n, np.array(bins)
