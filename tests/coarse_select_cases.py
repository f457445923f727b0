"""Generated inputs of the coarse selection (``search.coarse_select_f64`` / ``torch.ops.asw.coarse_select``) and the
statement's outputs in the op's layout.  Shared by tests/test_coarse_select_host.py and tests/test_gpu_coarse_select.py;
not a test module."""
import numpy as np

SLICE = 1024                     # COARSE_SLICE of csrc/cluster_kernels.hip: cubes per workgroup of the slice pass
THR1 = 0.008

KINDS = ("random", "none", "exact", "cap_plus_1", "all", "first_slice", "last_slice", "ties", "two_valued", "zeros",
         "nan_inf", "best_removes_top")
SIZES = (0, 1, 29, 30, 31, 63, 64, 65, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE, 3364, 15970, 70001)
CAPS = (1, 30, 64)


def make_case(N, cap, kind, relative, seed=0):
    """-> dict(energies [N,2], dis1 [N], best int32 [N] or None, thr1, relative, rel, cap).  ``dis1`` lies in [1, 5) and
    the powers around ``THR1``, so a random case has cubes on both sides of the threshold."""
    rng = np.random.default_rng([seed, N, cap, KINDS.index(kind), int(relative)])
    dis1 = 1.0 + 4.0 * rng.random(N)
    pw = rng.random(N) * 0.01
    best = None
    thr1, rel = THR1, 0.4
    low = lambda n: rng.random(n) * 1e-4                       # wd < 5e-4: below THR1 and below 0.4 * any winner's wd
    high = lambda n: 0.01 + rng.random(n)                      # wd >= 0.01: above THR1
    pick = lambda n: rng.choice(N, size=min(n, N), replace=False)
    if kind == "none":
        pw = low(N)                                            # (with relative the cubes near the maximum still pass)
    elif kind == "exact":
        pw = low(N)
        w = pick(cap)
        pw[w] = high(w.size)
    elif kind == "cap_plus_1":
        pw = low(N)
        w = pick(cap + 1)
        pw[w] = high(w.size)
    elif kind == "all":
        pw = high(N)
    elif kind == "first_slice":
        pw = low(N)
        w = rng.choice(min(N, SLICE), size=min(N, SLICE, cap + 5), replace=False)
        pw[w] = high(w.size)
    elif kind == "last_slice":
        pw = low(N)
        lo = ((N - 1) // SLICE) * SLICE if N else 0
        w = lo + rng.choice(N - lo, size=min(N - lo, cap + 5), replace=False)
        pw[w] = high(w.size)
    elif kind == "ties":
        # runs of equal powers that straddle every slice boundary, and one value shared by the whole table's tail
        pw = np.repeat(high((N + 36) // 37 + 1), 37)[5:5 + N].copy()
        pw[N // 2:] = 0.5
    elif kind == "two_valued":
        pw = np.where(rng.random(N) < 0.5, 0.25, 0.125)
    elif kind == "zeros":
        pw = np.where(rng.random(N) < 0.5, 0.0, -0.0)
        if N > 2:
            pw[pick(1)] = 1e-300
        thr1 = 0.0                                             # not (wd < 0.0): every zero passes
    elif kind == "nan_inf":
        pw[pick(max(1, N // 7))] = np.nan
        pw[pick(max(1, N // 11))] = np.inf
        if N > 3:
            pw[pick(1)] = -np.inf
    elif kind == "best_removes_top":
        pw = high(N)
        best = np.arange(N, dtype=np.int32)
        top = np.argsort(-pw, kind="stable")[:cap]
        best[top] = (top + 1) % max(N, 1)                      # (N = 1: the cube stays its own best)
        far = pick(3)
        best[far] = np.array([-7, N, 2 ** 31 - 1], dtype=np.int64)[:far.size].astype(np.int32)
    energies = np.stack([rng.random(N), pw], axis=1) if N else np.zeros((0, 2))
    return {"energies": np.ascontiguousarray(energies, dtype=np.float64), "dis1": dis1, "best": best, "thr1": float(thr1),
            "relative": bool(relative), "rel": rel, "cap": int(cap)}


def expected(case, statement):
    """(kept int32 [cap] padded with -1, counts int32 [2], thr float64 [2]) of ``statement`` = coarse_select_f64."""
    N = case["dis1"].shape[0]
    alive = None if case["best"] is None else case["best"] == np.arange(N, dtype=np.int32)
    stats = {}
    kept, n_pass, thr = statement(case["energies"][:, 1], case["dis1"], alive, thr1=case["thr1"],
                                  relative=case["relative"], rel=case["rel"], cap=case["cap"], stats=stats)
    out = np.full(case["cap"], -1, dtype=np.int32)
    out[:kept.shape[0]] = kept
    return (out, np.array([n_pass, stats["non_finite"]], dtype=np.int32),
            np.array([thr, stats["max_wd"]], dtype=np.float64))
