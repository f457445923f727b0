"""Shared by tests/test_lattice_nms_host.py and tests/test_gpu_lattice_nms.py: the planted score bumps, the coarse stage
of ``Prone_method="DENSE_NMS"`` written out by hand, and the nearness checks.  No test lives here."""
import numpy as np

from acousticswarms_speech_amd.dense_grid import lattice_local_maxima
from acousticswarms_speech_amd.search import MAX_BIG_PATCH, SPOT_POWER_THRESHOLD1, stage_energies


def chebyshev(cells, i, j):
    return np.max(np.abs(cells[i].astype(np.int64) - cells[j].astype(np.int64)), axis=-1)


def no_two_near(cells, idx, radius):
    idx = np.asarray(idx)
    d = np.max(np.abs(cells[idx, None, :].astype(np.int64) - cells[None, idx, :]), axis=2)
    return bool(np.all(d[~np.eye(len(idx), dtype=bool)] > radius))


def planted_scores(cells, seed, sigma, K=5, apart=6):
    """K cubes taken greedily from a seeded permutation, pairwise more than ``apart`` cells apart (Chebyshev), and
    the score max_k amp_k exp(-|cells - cells_k|^2 / 2 sigma^2) with amplitudes 1.0 ... 0.3."""
    picks = []
    for i in np.random.default_rng(seed).permutation(cells.shape[0]):
        if all(chebyshev(cells, i, j) > apart for j in picks):
            picks.append(int(i))
        if len(picks) == K:
            break
    assert len(picks) == K
    amp = np.linspace(1.0, 0.3, K)
    d2 = np.sum((cells[:, None, :].astype(np.float64) - cells[None, picks, :]) ** 2, axis=2)
    return picks, np.max(amp[None, :] * np.exp(-d2 / (2.0 * sigma * sigma)), axis=1)


def coarse_by_hand(ma, mix_t, p1, spot, cells, radius):
    """The coarse stage of DENSE_NMS written out: score, the statement, then the reference's loop with the skip."""
    _, powers_win = stage_energies(spot, mix_t, p1, 0)
    best, _degree = lattice_local_maxima(cells, powers_win, radius)
    kept = []
    for i in np.argsort(-1 * np.array(powers_win)):
        d = np.linalg.norm(p1[i].center_pos() - ma.mic_positions[0])
        if powers_win[i] * (d + 1) < SPOT_POWER_THRESHOLD1 or best[i] != i:
            continue
        if len(kept) >= MAX_BIG_PATCH:
            break
        kept.append(int(i))
    return kept
