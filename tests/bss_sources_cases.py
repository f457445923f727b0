"""Inputs shared by the full BSS-eval tests (host and GPU) and by ``perf_bss_sources.py``: the generators of
``bss_eval_cases.py``, the list of device-test cases, and the host statement of each case computed once per process and
handed out read-only.

SIR and SAR are differences of nearly equal projections, so the inputs are chosen to keep the statement's own values
moderate (``tests/test_bss_sources_host.py`` asserts -30 .. +50 dB on every finite SIR and SAR of the cases below).  The
"mixture" kind makes every estimate of a set identical, so its permutations tie: the permutation cases use "noisy" and
"filtered" estimates only, their rows shuffled by a known permutation.

Also the helpers that the tests of both BSS ops share: the stand-in for the device op, the library's workspace query, a
call of either C entry point on host memory, and a model whose forward pass runs once."""
import ctypes
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


# ---- helpers shared by the tests of torch.ops.asw.bss_eval_sdr and torch.ops.asw.bss_eval_sources -----------------------
def stand_in(marked=(), seen=None):
    """Either device op on CPU tensors: ``op(ref, est, counts, flen)`` -> (sdr, status) as ``bss_eval_sdr`` and
    ``op(ref, est, counts, flen, all_pairs)`` -> (sdr, sir, sar, status) as ``bss_eval_sources``.  The host statement per
    item; status 1 and NaN for the items of ``marked`` (indices within the call); ``seen`` receives the shapes and
    arguments of every call."""
    import torch
    from acousticswarms_speech_amd import evalkit

    def op(ref, est, counts, flen, *mode):
        if seen is not None:
            seen.append((tuple(ref.shape), tuple(est.shape), list(counts), flen, *mode))
        all_pairs = bool(mode and mode[0])
        R, N, _T = est.shape
        ncol = sum(S * S for S in counts) if all_pairs else N
        vals, status, n0, c0 = np.zeros((3, R, ncol)), np.zeros(len(counts), dtype=np.int32), 0, 0
        for k, S in enumerate(counts):
            width = S * S if all_pairs else S
            for r in range(R if S else 0):
                r_k, e_k = ref[n0:n0 + S].numpy(), est[r, n0:n0 + S].numpy()
                if k in marked:
                    vals[:, r, c0:c0 + width] = np.nan
                elif all_pairs:
                    vals[:, r, c0:c0 + width] = np.stack(evalkit.bss_eval_matrices(r_k, e_k, flen)).reshape(3, width)
                else:
                    vals[:, r, c0:c0 + width] = evalkit.bss_eval_sources(r_k, e_k, flen)[:3]
            status[k] = int(k in marked)
            n0, c0 = n0 + S, c0 + width
        return tuple(torch.from_numpy(v) for v in (vals if mode else vals[:1])) + (torch.from_numpy(status),)
    return op


def c_bytes(counts, R, T, flen, all_pairs=None):
    """The library's workspace query: ``asw_bss_eval_sdr_workspace_bytes`` without ``all_pairs``, else
    ``asw_bss_eval_sources_workspace_bytes``."""
    from acousticswarms_speech_amd import native
    c = (ctypes.c_int32 * max(1, len(counts)))(*counts)
    if all_pairs is None:
        return native.lib().asw_bss_eval_sdr_workspace_bytes(c, len(counts), R, T, flen)
    return native.lib().asw_bss_eval_sources_workspace_bytes(c, len(counts), R, T, flen, int(all_pairs))


def c_call(entry, counts=(2, 1), R=2, T=100, flen=8, all_pairs=0, null=(), ws_delta=0, ws_shift=0, K=None, sdr_only_size=False):
    """One call of the C entry point ``entry`` ("asw_bss_eval_sdr" or "asw_bss_eval_sources"), host memory standing in for
    every pointer: what is refused is refused before the first launch.  ``null``: the name(s) of the pointers passed as
    null.  -> (status, last error, workspace bytes asked for)."""
    from acousticswarms_speech_amd import evalkit, native
    L, full = native.lib(), entry == "asw_bss_eval_sources"
    null = (null,) if isinstance(null, str) else tuple(null or ())
    K = len(counts) if K is None else K
    c = (ctypes.c_int32 * max(1, len(counts)))(*counts)
    n = max(1, sum(max(0, v) for v in counts))
    q = max(1, sum(v * v for v in counts)) if full else n
    ref = (ctypes.c_float * (n * max(T, 1)))()
    est = (ctypes.c_float * (max(R, 1) * n * max(T, 1)))()
    outs = {name: (ctypes.c_double * (max(R, 1) * q))() for name in (("sdr", "sir", "sar") if full else ("sdr",))}
    status = (ctypes.c_int32 * max(1, len(counts)))()
    need = getattr(L, entry + "_workspace_bytes")(c, K, R, T, flen, *((all_pairs,) if full else ()))
    if sdr_only_size:
        need = evalkit.bss_sources_workspace_bytes(counts, R, T, flen, bool(all_pairs), sdr_only=True)
    ws = (ctypes.c_double * (need // 8 + 2))()
    ptr = {"ref": ref, "est": est, "counts": c, "status": status, "ws": ws, **outs}
    arg = {k: (None if k in null else ctypes.cast(v, ctypes.c_void_p)) for k, v in ptr.items()}
    if arg["ws"] is not None:
        arg["ws"] = ctypes.c_void_p(arg["ws"].value + ws_shift)
    mode = (all_pairs,) if full else ()
    rc = getattr(L, entry)(arg["ref"], arg["est"], arg["counts"], K, R, T, flen, *mode, *(arg[name] for name in outs),
                           arg["status"], arg["ws"], need + ws_delta, None)
    return rc, L.asw_last_error().decode(), need


class Once:
    """A JointModel whose forward pass runs once: the records made from it differ in the metric only."""

    def __init__(self, jm):
        self.jm, self.out = jm, None

    def setup(self, **kw):
        if self.out is None:
            self.jm.setup(**kw)

    def __call__(self, mix):
        if self.out is None:
            self.out = self.jm(mix)
        return self.out
