"""Shared by tests/test_fine_clusters_host.py and tests/test_gpu_fine_clusters.py: generated groups of candidate
outputs, whole calls of ``fine_clusters`` made of them, and a case counted by hand.

A generated group is ``n`` rows made of 1-3 random "sources" (white noise): each row is one source scaled by a gain in
[0.3, 1] plus white noise at an SNR uniform in [-8, 8] dB, mean removed.  Two rows of one source then compare at about
-8 .. +6 dB SI-SDR, on both sides of the -4 dB threshold, and rows of different sources far below it: both joins and
new heads occur.  (120 such groups of 2-39 rows at T = 12 000: 0-28 clusters per group, none within 1e-3 dB of the
threshold, float32 ``si_sdr`` and the float64 statement 3e-6 dB apart at most.)
"""
import numpy as np

from acousticswarms_speech_amd.hostdsp import max_avg_power


def make_group(rng, n, T):
    """float32 [n, T], mean removed."""
    n_src = int(rng.integers(1, 4))
    src = rng.standard_normal((n_src, T))
    rows = np.zeros((n, T), dtype=np.float32)
    for i in range(n):
        s = src[int(rng.integers(0, n_src))] * rng.uniform(0.3, 1.0)
        snr_db = rng.uniform(-8.0, 8.0)
        noise = rng.standard_normal(T)
        noise *= np.sqrt(np.sum(s * s) / (np.sum(noise * noise) * 10.0 ** (snr_db / 10.0)))
        x = (s + noise).astype(np.float32)
        rows[i] = x - np.mean(x)
    return rows


def energies_of(waves):
    """float64 [N, 2] = (power, power2) as the reference forms them on the host (Mic_Array.py:290-295)."""
    waves = np.asarray(waves, dtype=np.float32)
    out = np.zeros((waves.shape[0], 2), dtype=np.float64)
    for i, w in enumerate(waves):
        out[i] = (np.sum(w.astype(np.float64) ** 2), max_avg_power(w))
    return out


def make_call(seed, sizes, T, closed=(), groups=None):
    """One call's inputs from generated groups of the given sizes (0 allowed): dict with waves [N, T], bounds [G + 1]
    int32, energies [N, 2], gate [N], group_gate [G], min_trigger.  The thresholds are placed among the energies so
    that every rule acts: gate[k] is power2[k] times a factor in [0.6, 1.15] (about a third of the candidates fail it),
    min_trigger is the 10 % quantile of the powers, group_gate is half the group's best power2 -- twice it for the
    groups listed in ``closed``.  ``groups`` replaces the generated rows (a list of [n, T] arrays)."""
    rng = np.random.default_rng(seed)
    if groups is None:
        groups = [make_group(rng, n, T) for n in sizes]
    sizes = [len(g) for g in groups]
    bounds = np.zeros(len(sizes) + 1, dtype=np.int32)
    bounds[1:] = np.cumsum(sizes)
    N = int(bounds[-1])
    waves = np.concatenate([np.asarray(g, dtype=np.float32).reshape(-1, T) for g in groups] +
                           [np.zeros((0, T), dtype=np.float32)])
    en = energies_of(waves)
    gate = en[:, 1] * rng.uniform(0.6, 1.15, N)
    group_gate = np.zeros(len(sizes), dtype=np.float64)
    for g, n in enumerate(sizes):
        best = float(np.max(en[bounds[g]:bounds[g + 1], 1])) if n else 1.0
        group_gate[g] = best * (2.0 if g in closed else 0.5)
    min_trigger = float(np.quantile(en[:, 0], 0.1)) if N else 0.0
    return {"waves": waves, "bounds": bounds, "energies": en, "gate": gate, "group_gate": group_gate,
            "min_trigger": min_trigger}


def statement(call, sim_db=-4.0):
    from acousticswarms_speech_amd.fine_cluster import fine_clusters_f64
    return fine_clusters_f64(call["waves"], call["bounds"], call["energies"], call["gate"], call["group_gate"],
                             call["min_trigger"], sim_db)


def hand_case():
    """Five groups at T = 8 whose outcome is counted by hand; every value is a small integer or a half, so every sum
    is exact in any order.  ratio = 10 ** -0.4 = 0.398.

    group 0, rows 0-1, CLOSED: best power2 3 < group_gate 5                       -> labels -1, -1; order by power: 1, 0
    group 1, rows 2-3, open, nobody eligible: row 2 fails its gate (power2 1 < 2), row 3 the trigger (power 1 < 2)
    group 2, row 4 alone, eligible                                                -> a head: label 4
    group 3, rows 5-8:
        row 5 = 4 e0 and row 6 = 4 e1: power 16 both -> visited 5 then 6 (ascending index); e0 . e1 = 0: two heads
        row 8 = 3 e0 + e3, power 10: against head 5 es = 12, sss = 144 / 16 = 9, snn = 1 + 1e-8 -> joins 5
        row 7 = 3 e1 + 0.5 e2, power 9.25: against head 5 es = 0 -> no; against head 6 es = 12, sss = 9,
              snn = 0.25 + 1e-8 -> joins 6: a candidate that matches the SECOND head only
        visiting order 5, 6, 8, 7
    group 4: empty
    -> (call, order, label, gram)"""
    T = 8
    e = np.eye(T, dtype=np.float32)
    waves = np.stack([e[0], 2 * e[1],                       # group 0: powers 1, 4
                      3 * e[0], e[1],                       # group 1: powers 9, 1
                      2 * e[2],                             # group 2: power 4
                      4 * e[0], 4 * e[1], 3 * e[1] + 0.5 * e[2], 3 * e[0] + e[3]])
    bounds = np.array([0, 2, 4, 5, 9, 9], dtype=np.int32)
    power = np.array([1, 4, 9, 1, 4, 16, 16, 9.25, 10], dtype=np.float64)
    power2 = np.array([3, 2, 1, 6, 5, 7, 7, 7, 7], dtype=np.float64)
    call = {"waves": waves, "bounds": bounds, "energies": np.stack([power, power2], axis=1),
            "gate": np.array([1, 1, 2, 1, 1, 1, 1, 1, 1], dtype=np.float64),
            "group_gate": np.array([5, 5, 5, 5, 5], dtype=np.float64), "min_trigger": 2.0}
    order = np.array([1, 0, 2, 3, 4, 5, 6, 8, 7], dtype=np.int32)
    label = np.array([-1, -1, -1, -1, 4, 5, 6, 6, 5], dtype=np.int32)
    w = waves.astype(np.float64)
    gram = np.concatenate([(w[a:b] @ w[a:b].T).reshape(-1) for a, b in zip(bounds[:-1], bounds[1:])])
    return call, order, label, gram


def gram_entry(a, b):
    """One Gram entry in the stated order, written with scalar loops (independent of ``_gram_rows``)."""
    a, b = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    p = [0.0] * 256
    for t in range(a.shape[0]):
        p[t % 256] = p[t % 256] + float(a[t]) * float(b[t])
    w = []
    for q in range(4):
        v = p[64 * q:64 * q + 64]
        for s in (32, 16, 8, 4, 2, 1):
            v = [v[l] + v[l + s] for l in range(s)]
        w.append(v[0])
    return (w[0] + w[1]) + (w[2] + w[3])
