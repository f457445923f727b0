"""Inputs shared by the oracle mask tests (host and GPU): seeded sources, mixtures, the special rows of the transform
tests and a small hand-made evaluation batch.  No GPU, no scipy, nothing of the reference."""
import numpy as np

LENGTHS = (2048, 3071, 3072, 3073, 5000)          # the minimum and the three sides of the padding boundary


def sources(seed, S, N):
    """(gt [S, N] float32 Gaussian sources, mix [N] float32: their sum plus 10 % noise)."""
    rng = np.random.default_rng(seed)
    gt = rng.standard_normal((S, N)).astype(np.float32)
    mix = (gt.astype(np.float64).sum(axis=0) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    return gt, mix


def transform_rows(seed, R, N):
    """[R, N] float32: Gaussian rows; from three rows on, row 0 is a unit impulse at sample 0, row 1 one at sample
    N - 1 and row 2 a full-scale sinusoid exactly on bin 1024 (+1, -1, ...)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, N)).astype(np.float32)
    if R >= 3:
        x[0], x[1] = 0.0, 0.0
        x[0, 0], x[1, N - 1] = 1.0, 1.0
        x[2] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    return x


def threshold_margin(gt, mix, alpha=1.0, theta=0.5):
    """The smallest |r / theta - 1| over the bins of the binary mask's ratio: how far the inputs are from a decision
    that could fall either way."""
    from acousticswarms_speech_amd.oracle_masks import ibm_ratio_f64
    return float(np.min(np.abs(ibm_ratio_f64(gt, mix, alpha) / theta - 1.0)))


def eval_batch(seed=5, T=4096, n_samples=2):
    """(samples, results) for ``records_from_results``: ``n_samples`` samples of 4 microphones and 3 talkers, of which the
    hand-made result finds talkers 0 and 2 (in that order reversed) and one false positive far away; talker 1 stays
    unmatched.  No network runs."""
    rng = np.random.default_rng(seed)
    mics = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [-0.1, 0.0, 0.0]])
    spk = np.array([[1.0, 1.0, 0.3], [-1.0, 1.5, 0.3], [0.5, 2.0, 0.3]])
    meta = {"ROI": [-2.0, 2.0, 0.0, 3.0, 0.0, 1.0]}
    for m in range(4):
        meta[f"mic{m:02d}"] = {"position": mics[m].tolist()}
    for s in range(3):
        meta[f"voice{s:02d}"] = {"position": spk[s].tolist()}
    samples, results = [], []
    for _ in range(n_samples):
        gt = rng.standard_normal((3, T)).astype(np.float32)
        mix = np.stack([gt.sum(axis=0) + 0.1 * rng.standard_normal(T) for _m in range(4)]).astype(np.float32)
        found = [2, 0]
        audio = np.stack([gt[s] + 0.3 * rng.standard_normal(T) for s in found]
                         + [0.2 * rng.standard_normal(T)]).astype(np.float32)
        centres = np.stack([spk[2] + [0.05, -0.05, 0.0], spk[0] + [-0.1, 0.05, 0.0], [1.9, 0.1, 0.3]])
        offsets = rng.integers(-5, 5, (3, 3))
        samples.append((meta, mix, gt))
        results.append({"centres": centres, "offsets": list(offsets), "audio_offsets": list(offsets), "audio_loc": audio,
                        "audio": None})
    return samples, results
