"""Shared by tests/test_voiced_segments_host.py and tests/test_gpu_voiced_segments.py: waveforms whose voiced segments are
counted by hand, the scene waveforms of the comparison with ``split_wav``, and the statement's tables in the layout
``asw_voiced_segments`` writes.

The hand-counted waveforms are block-wise constant in magnitude (alternating sign): block j is samples
[256 j, 256 j + 256), frame f is the mean square of blocks f-2 .. f+1 and ``thr = 10 ** -1.8 = 0.01585``.

* A block of magnitude 1.0 alone gives its frame 0.25: with a peak of 1.0 a frame is voiced when ANY of its four
  blocks is loud, so L loud blocks from j0 on give the L + 3 frames j0-1 .. j0+L+1.
* A block of magnitude 0.2 gives 0.01 per block: beside a peak of 1.0 a frame needs TWO of them (0.02 > 0.01585 > 0.01),
  so L >= 2 such blocks from j0 on give the L + 1 frames j0 .. j0+L.
"""
import numpy as np

from acousticswarms_speech_amd.hostdsp import voiced_segments_f64


def _blocks(T, levels):
    """float32 [T]: magnitude levels[j] over block j, alternating sign."""
    y = np.zeros(T, dtype=np.float32)
    for j, a in levels.items():
        y[256 * j:min(256 * j + 256, T)] = a
    y[1::2] *= -1
    return y


def envelope_wave():
    """T = 24 676 = 96 blocks and 100 samples; frames 0 .. 96.

    blocks  4 ..  7 at 1.0: frames  3 ..  9, [  768,  2560), 1792 samples -> one segment (and the peak, exactly 1.0)
    blocks 16 .. 17 at 0.2: frames 16 .. 18, [ 4096,  4864),  768 samples -> dropped
    blocks 26 .. 40 at 0.2: frames 26 .. 41, [ 6656, 10752), 4096 samples -> one segment (4096 // 4000 = 1)
    blocks 50 .. 80 at 0.2: frames 50 .. 81, [12800, 20992), 8192 samples -> two, the last takes the remainder
    blocks 90 .. 96 at 0.2: frames 90 .. 96 (frame 96: two whole blocks and 100 samples, 0.0239), the run reaches the
                            last frame, [23040, min(24832, T)) -> one segment clipped to T"""
    T = 256 * 96 + 100
    levels = {j: 1.0 for j in range(4, 8)}
    for lo, hi in ((16, 17), (26, 40), (50, 80), (90, 96)):
        levels.update({j: 0.2 for j in range(lo, hi + 1)})
    want = [[768, 2560], [6656, 10752], [12800, 16800], [16800, 20992], [23040, T]]
    return _blocks(T, levels), want


def clipped_wave(length):
    """A wave whose only run is loud (1.0) from block 5 to the end, T = 1024 + length: frames 4 .. end are voiced and
    the interval is [1024, T), exactly ``length`` samples (1000 <= length: 1000 and 4000 give one segment each)."""
    T = 1024 + length
    levels = {j: 1.0 for j in range(5, -(-T // 256))}
    k = max(1, length // 4000)
    want = [[1024 + 4000 * i, T if i == k - 1 else 1024 + 4000 * (i + 1)] for i in range(k)] if length >= 1000 else []
    return _blocks(T, levels), want


def scene_waves(seeds, T=48000, gains=True):
    """The 7 mixture channels and 5 sources of make_scene(seed, 5, T=T, reverb=True) per seed, each at gain 1 and (with
    ``gains``) at one seeded gain in [0.01, 0.2] -- that reaches the quiet branch --, cast to float32, mean removed."""
    from acousticswarms_speech_amd.scenes import make_scene
    out = []
    for seed in seeds:
        sc = make_scene(seed, 5, T=T, reverb=True)
        rng = np.random.default_rng(seed)
        for w in list(sc.mix) + list(sc.sources):
            g = rng.uniform(0.01, 0.2)
            for gain in ((1.0, g) if gains else (1.0,)):
                x = (np.asarray(w, dtype=np.float64) * gain).astype(np.float32)
                out.append(x - np.mean(x))
    return out


def statement_tables(waves, top_db=18.0):
    """(segments int32 [n, kcap, 2] zero beyond the count, counts int32 [n], ms float64 [n, 1 + T//256], lists) of
    equally long waveforms by ``voiced_segments_f64``: what the kernel must write, byte for byte."""
    waves = np.asarray(waves, dtype=np.float32)
    n, T = waves.shape
    kcap = max(1, T // 1000)
    seg = np.zeros((n, kcap, 2), dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    ms = np.zeros((n, 1 + T // 256), dtype=np.float64)
    lists = []
    for i in range(n):
        s, ms[i] = voiced_segments_f64(waves[i], top_db)
        assert len(s) <= kcap
        cnt[i] = len(s)
        seg[i, :len(s)] = np.asarray(s, dtype=np.int32).reshape(-1, 2)
        lists.append(s)
    return seg, cnt, ms, lists


def check_structure(segs, T):
    """Ascending, disjoint, each at least 1000 samples, inside [0, T], at most T // 1000 of them."""
    end = 0
    for a, b in segs:
        assert end <= a and b - a >= 1000 and b <= T, (segs, T)
        end = b
    assert len(segs) <= T // 1000
