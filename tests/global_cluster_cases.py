"""Inputs of the global clustering's decisions (``global_cluster.global_clusters_f64`` / ``asw_global_clusters``), shared
by tests/test_global_clusters_host.py and tests/test_gpu_global_clusters.py: generated cases and one counted by hand."""
import numpy as np

from acousticswarms_speech_amd.global_cluster import global_clusters_f64

NEAR_M = 0.45                             # the merge distance of Clustering_new


def statement(case, **kw):
    return global_clusters_f64(case["full"], case["seg"], case["counts"], case["near"], **kw)


def near_of(centres):
    """uint8 [n, n]: the pairs of centres closer than 0.45 m in the (x, y) plane."""
    d = centres[:, None, :2] - centres[None, :, :2]
    return (np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < NEAR_M).astype(np.uint8)


def make_case(seed, n, K, full_range=(-10.0, 3.0), seg_range=(-12.0, 2.0), area=6.0, garbage=None):
    """``full`` uniform in [-10, 3] dB, ``seg`` uniform in [-12, 2], ``counts`` in 0..K, and ``near`` = the pairs of
    ``centres`` (uniform in an ``area`` m square: a few per cent of the pairs) closer than 0.45 m.  ``full``'s diagonal is
    +inf as an SI-SDR of a waveform with itself is large; no decision reads it.  ``garbage``: what the slots from a
    row's count on hold -- None: NaN, as the torch adapter fills them; "finite": values that would flip decisions."""
    rng = np.random.default_rng(seed)
    full = rng.uniform(*full_range, size=(n, n))
    full[np.arange(n), np.arange(n)] = np.inf
    seg = rng.uniform(*seg_range, size=(n, n, K))
    counts = rng.integers(0, K + 1, size=n).astype(np.int32)
    unused = np.arange(K)[None, None, :] >= counts[:, None, None]
    centres = np.concatenate([rng.uniform(0.0, area, size=(n, 2)), rng.uniform(0.0, 1.0, size=(n, 1))], axis=1)
    fill = np.nan if garbage is None else rng.choice([-100.0, 0.0, 100.0], size=seg.shape)    # (drawn last)
    seg = np.where(np.broadcast_to(unused, seg.shape), fill, seg)
    return {"full": np.ascontiguousarray(full), "seg": np.ascontiguousarray(seg), "counts": counts,
            "near": near_of(centres), "centres": centres}


def unmerged_case(n, K, seed=0):
    """n rows of which none merges with or is shadowed by another: every row becomes a head (every best holds a value
    below best_lo).  The base of the cases that need a long head list."""
    rng = np.random.default_rng(seed)
    full = rng.uniform(-10.0, -3.0, size=(n, n))
    seg = rng.uniform(-12.0, -5.5, size=(n, n, K))          # nothing > win_hi: no window merge; everything < best_lo
    counts = rng.integers(1, K + 1, size=n).astype(np.int32)
    return {"full": full, "seg": seg, "counts": counts, "near": np.zeros((n, n), dtype=np.uint8)}


def hand_case():
    """-> (case, label, merge), n = 11, K = 3, at the default thresholds (full > -1; window > -2 and none < -7; best
    > -1 and none < -5).  Wherever nothing is said full = -10 and seg = -6: no merge, and a best of -6 < -5 makes a head.

    row 0   c = 2                                                          first head                      ->  0
    row 1   c = 0                                                          no segments                     -> -1
    row 2   c = 3                                                          nothing in common with 0        ->  2
    row 3   c = 2, seg[3][0] = [-0.5, -8]: a window with a slot < -7 is no merge; best = [-0.5, -6]: one value > -1
            but one < -5                                                   a head all the same             ->  3
    row 4   c = 2, seg[4][0] = [-0.5, -8], seg[4][2] = [-6, -3]: no merge; best over heads 0, 2, 3 = [-0.5, -3]:
            one > -1, none < -5                                            shadowed                        -> -2
    row 5   full[5][2] = 0 and near[5][3] = 1: the second and the third head; the second wins            ->  2
    row 6   near[6][3] = 1 only                                                                            ->  3
    row 7   c = 3, seg[7][0] = [-1.5, -6.9, -3]: window only                                               ->  0
    row 8   full[8][2] = -0.5 only                                                                         ->  2
    row 9   c = 3, seg[9][0] = [NaN, -6, -6], seg[9][2] = [-0.5, -6, -8], seg[9][3] = [-6, -3, -3]: no merge (NaN
            compares false; -8 < -7); best = [NaN, -3, -3]: the NaN stays, nothing > -1      a head        ->  9
            (a maximum that skipped the NaN would give best[0] = -0.5 and shadow the row)
    row 10  c = 2, full[10][0] = NaN, seg[10][9] = [-1, -1]: window with the fourth head only              ->  9

    The unused slots hold values that flip a decision if read: row 0's slot 2 = +100 (every merge[0][j] would be set),
    row 3's = 0.0 (a window with head 2), row 4's = -100 (a best < -5: a head instead of shadowed)."""
    n, K = 11, 3
    full = np.full((n, n), -10.0)
    seg = np.full((n, n, K), -6.0)
    near = np.zeros((n, n), dtype=np.uint8)
    counts = np.array([2, 0, 3, 2, 2, 3, 1, 3, 3, 3, 2], dtype=np.int32)
    seg[0, :, 2] = 100.0
    seg[3, 0, :2] = [-0.5, -8.0]
    seg[3, :, 2] = 0.0
    seg[4, 0, :2] = [-0.5, -8.0]
    seg[4, 2, :2] = [-6.0, -3.0]
    seg[4, :, 2] = -100.0
    full[5, 2] = 0.0
    near[5, 3] = 1
    near[6, 3] = 1
    seg[7, 0] = [-1.5, -6.9, -3.0]
    full[8, 2] = -0.5
    seg[9, 0] = [np.nan, -6.0, -6.0]
    seg[9, 2] = [-0.5, -6.0, -8.0]
    seg[9, 3] = [-6.0, -3.0, -3.0]
    full[10, 0] = np.nan
    seg[10, 9, :2] = [-1.0, -1.0]
    seg[10, :, 2] = 100.0
    label = np.array([0, -1, 2, 3, -2, 2, 3, 0, 2, 9, 9], dtype=np.int32)
    merge = np.zeros((n, n), dtype=np.uint8)
    for i, j in ((5, 2), (5, 3), (6, 3), (7, 0), (8, 2), (10, 9)):
        merge[i, j] = 1
    return {"full": full, "seg": seg, "counts": counts, "near": near}, label, merge
