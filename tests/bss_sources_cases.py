"""Inputs shared by the full BSS-eval tests (host and GPU) and by ``perf_bss_sources.py``: the generators of
``bss_eval_cases.py``, the list of device-test cases, and the host statement of each case computed once per process and
handed out read-only.

SIR and SAR are differences of nearly equal projections, so the inputs are chosen to keep the statement's own values
moderate (``tests/test_bss_sources_host.py`` asserts -30 .. +50 dB on every finite SIR and SAR of the cases below).  The
"mixture" kind makes every estimate of a set identical, so its permutations tie: the permutation cases use "noisy" and
"filtered" estimates only, their rows shuffled by a known permutation."""
import functools

import numpy as np

from tests import bss_eval_cases as cases

KINDS = cases.KINDS

# (seed, counts, T, flen, kinds): matched mode, the shapes at which the grid logic can go wrong
RAGGED = [(11, c, 1000, 16, ("mixture", "noisy")) for c in [(1,), (2,), (3, 1, 2), (0, 2, 0), (5,)]]
ORDERS = [(12, (S,), 1000, flen, ("mixture", "noisy")) for S, flen in [(3, 21), (1, 64), (5, 13), (3, 43), (2, 64)]]
# one- and two-tap filters leave the noise of a "noisy" estimate next to no room in the other reference (SIR above 60 dB):
# the leak of the "filtered" kind keeps it moderate
ORDERS += [(12, (2,), 1000, flen, ("mixture", "filtered")) for flen in (1, 2)]
LENGTHS = [(13, (2, 1), T, 32, ("mixture", "noisy")) for T in (257, 1000, 4099)]
THREE_KINDS = [(14, (3, 2), 2000, 24, KINDS)]
WORKING = [(15, (3,), 16000, 512, ("mixture", "noisy"))]
MATCHED = RAGGED + ORDERS + LENGTHS + THREE_KINDS + WORKING
# all-pairs mode: the [S, S] matrices
PAIRS = [(11, (3, 1, 2), 1000, 16, ("mixture", "noisy")), (12, (5,), 1000, 13, ("mixture", "noisy"))]
# permutation inputs: (seed, counts, T, flen); the estimate sets are "noisy" and "filtered", rows shuffled
SHUFFLED = [(21, (3, 1, 2), 1000, 16), (22, (5,), 1000, 13), (23, (2,), 4099, 64), (24, (3,), 257, 21)]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def batch(seed, counts, T, kinds):
    refs, ests = cases.make_batch(seed, list(counts), T, kinds)
    _freeze(*refs, *ests)
    return refs, ests


@functools.lru_cache(maxsize=None)
def matched(seed, counts, T, flen, kinds):
    """(refs, ests, (sdr, sir, sar) each [R, N]) by ``evalkit.bss_eval_sources`` item after item."""
    from acousticswarms_speech_amd import evalkit
    refs, ests = batch(seed, counts, T, kinds)
    R = len(kinds)
    want = np.zeros((3, R, sum(counts)))
    n0 = 0
    for ref, est in zip(refs, ests):
        S = ref.shape[0]
        for r in range(R if S else 0):
            want[:, r, n0:n0 + S] = evalkit.bss_eval_sources(ref, est[r], flen)[:3]
        n0 += S
    _freeze(want)
    return refs, ests, want


@functools.lru_cache(maxsize=None)
def pairs(seed, counts, T, flen, kinds):
    """(refs, ests, (sdr, sir, sar) each [R, Q]) by ``evalkit.bss_eval_matrices``: item k a row-major [S_k, S_k] block."""
    from acousticswarms_speech_amd import evalkit
    refs, ests = batch(seed, counts, T, kinds)
    R = len(kinds)
    want = np.zeros((3, R, sum(S * S for S in counts)))
    q0 = 0
    for ref, est in zip(refs, ests):
        S = ref.shape[0]
        for r in range(R if S else 0):
            want[:, r, q0:q0 + S * S] = np.stack(evalkit.bss_eval_matrices(ref, est[r], flen)).reshape(3, S * S)
        q0 += S * S
    _freeze(want)
    return refs, ests, want


@functools.lru_cache(maxsize=None)
def shuffled(seed, counts, T, flen):
    """(refs, ests, perms, matrices): ``ests[k]`` [2, S, T] are the "noisy" and the "filtered" estimates of ``refs[k]`` with
    the estimate of reference j moved to row ``perms[k][r][j]`` (never the identity for S > 1); ``matrices[k]`` is
    [2, 3, S, S], the statement's (sdr, sir, sar) matrices of each set."""
    from acousticswarms_speech_amd import evalkit
    rng = np.random.default_rng([seed, T, flen] + list(counts))
    refs, ests, perms, mats = [], [], [], []
    for S in counts:
        ref = cases.references(rng, S, T) if S else np.zeros((0, T), dtype=np.float32)
        sets, ps = [], []
        for kind in ("noisy", "filtered"):
            est = cases.estimates(rng, ref, kind) if S else np.zeros((0, T), dtype=np.float32)
            perm = rng.permutation(S)
            while S > 1 and np.array_equal(perm, np.arange(S)):
                perm = rng.permutation(S)
            moved = np.zeros_like(est)
            moved[perm] = est
            sets.append(moved)
            ps.append(perm)
        refs.append(ref)
        ests.append(np.stack(sets))
        perms.append(np.stack(ps))
        mats.append(np.stack([np.stack(evalkit.bss_eval_matrices(ref, s, flen)) for s in sets]))
    _freeze(*refs, *ests, *perms, *mats)
    return refs, ests, perms, mats


def pack(refs, ests):
    return cases.pack(refs, ests)
