"""A recording of any length as overlapping blocks of one network length: where the blocks start, the taper at their
seams, the normalised overlap-add that puts the separated blocks back together, and the linking of the talkers found in
one block to those of the next.

Host code in float64, torch-free: the statements ``asw_frame_blocks`` and ``asw_stitch_blocks``
(csrc/longform_kernels.hip) are pinned to, and the tables both are driven with.  No counterpart in the reference, whose
README only names the use ("reuse this setup for successive inferences over chunks")."""
import numpy as np

LINK_RADIUS = 0.25       # metres; the scenes keep talkers at least 0.51 m apart (MIN_SPEAKER_DIST, scenes.make_scene)


def block_starts(Ttot: int, T: int, hop: int) -> np.ndarray:
    """First samples of the blocks of length ``T`` that cover ``Ttot`` samples, int64 [K], strictly increasing: ``k*hop``
    while the block ends inside the recording, then one more block at ``Ttot - T`` when the grid does not end there (it
    is full of real audio and may overlap its neighbour by more than V = T - hop).  ``Ttot <= T``: the single block 0,
    zero-filled past ``Ttot``.  ``ValueError`` unless 1 <= V <= T // 2, so that at most the two ramps of neighbouring
    blocks meet on the regular grid."""
    Ttot, T, hop = int(Ttot), int(T), int(hop)
    V = T - hop
    if Ttot < 1 or T < 2:
        raise ValueError(f"a recording of {Ttot} samples in blocks of {T}")
    if not 1 <= V <= T // 2:
        raise ValueError(f"hop {hop} leaves an overlap of {V} samples; blocks of {T} need 1 <= T - hop <= {T // 2}")
    if Ttot <= T:
        return np.zeros(1, dtype=np.int64)
    starts = list(range(0, Ttot - T + 1, hop))
    if starts[-1] + T != Ttot:
        starts.append(Ttot - T)
    return np.asarray(starts, dtype=np.int64)


def taper(T: int, V: int) -> np.ndarray:
    """float64 [T]: sin^2(pi/2 (j + 1/2) / V) on the first V samples, mirrored at the end, 1 in between.  The half
    sample keeps every weight strictly positive, and w[j] + w[V-1-j] = 1: two ramps that meet on the grid sum to 1."""
    T, V = int(T), int(V)
    if not 1 <= V <= T // 2:
        raise ValueError(f"a taper of {V} samples on a block of {T}")
    w = np.ones(T, dtype=np.float64)
    ramp = np.sin(np.pi / 2 * (np.arange(V, dtype=np.float64) + 0.5) / V) ** 2
    w[:V] = ramp
    w[T - V:] = ramp[::-1]
    return w


def _spans(starts, Ttot, T):
    """(first sample, samples inside the recording) of every block."""
    return [(int(a), min(int(T), int(Ttot) - int(a))) for a in starts]


def frame_f64(mix, starts, T: int, dtype=np.float64) -> np.ndarray:
    """mix [M, Ttot] -> the blocks [K, M, T]; samples past ``Ttot`` are zero."""
    mix = np.asarray(mix)
    out = np.zeros((len(starts), mix.shape[0], int(T)), dtype=dtype)
    for k, (a, n) in enumerate(_spans(starts, mix.shape[1], T)):
        out[k, :, :n] = mix[:, a:a + n]
    return out


def stitch_f64(rows, starts, row_of, Ttot: int, T: int, V: int) -> np.ndarray:
    """The normalised overlap-add: out[s, t] = sum_k w[t - a_k] x_k[s][t - a_k] / sum_k w[t - a_k] over the blocks k that
    cover t, float64 [S, Ttot].  ``rows`` [N, T]; x_k[s] is row ``row_of[k][s]``, zeros when that is -1 (the talker is
    absent from block k; its weight still counts below the line, so the track fades instead of jumping).  One formula
    for every sample: a single cover returns the sample itself, two ramps on the grid sum to 1, three covers (the
    shifted last block) are weighted like two.  The sums run over k in ascending order."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, int(T))
    row_of = np.asarray(row_of, dtype=np.int64).reshape(len(starts), -1)
    w = taper(T, V)
    num = np.zeros((row_of.shape[1], int(Ttot)), dtype=np.float64)
    den = np.zeros(int(Ttot), dtype=np.float64)
    for k, (a, n) in enumerate(_spans(starts, Ttot, T)):
        den[a:a + n] += w[:n]
        for s, r in enumerate(row_of[k]):
            if r >= 0:
                num[s, a:a + n] += w[:n] * rows[r, :n]
    return num / den


def link_tracks(block_centres, radius: float = LINK_RADIUS):
    """Which detection of which block is which talker.  ``block_centres[k]`` is the [n_k, 3] array of the positions
    found in block k.  The blocks are walked in order; a block's detections are matched one to one to the tracks opened
    so far, each track standing where it was detected last: among the pairs no farther apart than ``radius`` the
    matching holds as many pairs as possible and, of those, the least total distance (``scipy``'s assignment routine, as
    in ``evalkit.find_best_permutation``; matchings of one size and exactly equal total are told apart by that routine
    alone, the same way on every run).  A detection left over opens a track; a track without a detection is absent from
    the block (an empty block: every track).  A track never closes: a talker comes back to it when found again within
    ``radius`` of where it was last.

    -> (det_of int64 [K, n_tracks]: the detection of block k that is track s, -1 when absent; positions float64
    [n_tracks, K, 3], NaN where absent).  With talkers at least 2 * radius apart two detections of different talkers
    cannot both lie within ``radius`` of one track's position."""
    from scipy.optimize import linear_sum_assignment
    K = len(block_centres)
    last, table = [], []                                     # per track: latest position; per block: {track: detection}
    for centres in block_centres:
        c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        found = {}
        if c.shape[0] and last:
            dist = np.linalg.norm(c[:, None, :] - np.asarray(last)[None, :, :], axis=2)
            near = dist <= radius
            if near.any():
                big = radius * (min(dist.shape) + 1) + 1.0   # one more pair always beats any change of distance
                di, tr = linear_sum_assignment(np.where(near, dist - big, 0.0))
                found = {int(t): int(d) for d, t in zip(di, tr) if near[d, t]}
        taken = set(found.values())
        for d in range(c.shape[0]):
            if d not in taken:
                found[len(last)] = d
                last.append(c[d])
        for t, d in found.items():
            last[t] = c[d]
        table.append((found, c))
    det_of = np.full((K, len(last)), -1, dtype=np.int64)
    positions = np.full((len(last), K, 3), np.nan)
    for k, (found, c) in enumerate(table):
        for t, d in found.items():
            det_of[k, t] = d
            positions[t, k] = c[d]
    return det_of, positions


def rows_of(det_of, counts) -> np.ndarray:
    """``det_of`` [K, S] (detection within its block, -1 absent) -> the ``row_of`` table of ``stitch_f64``, int32 [K, S],
    for rows that hold block after block, ``counts[k]`` rows for block k."""
    det_of = np.asarray(det_of, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))[:-1]]).reshape(-1, 1)
    return np.where(det_of >= 0, det_of + first, -1).astype(np.int32)
