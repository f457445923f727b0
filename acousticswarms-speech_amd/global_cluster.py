"""The global clustering's decisions, stated for a kernel (csrc/cluster_kernels.hip: asw_global_clusters).

``MicArray.Clustering_new`` walks the cluster heads of the fine stage by descending power: a head joins the first
earlier head it is "the same talker" as -- by the whole-length SI-SDR, by the segment-wise SI-SDR window test or by
distance --, is shadowed when the best segment-wise SI-SDR over all earlier heads passes a second window test, or becomes
a talker.  ``global_clusters_f64`` restates those decisions on the tensors the device ops already wrote.  They are
comparisons of float64 values, a first-hit scan and a running maximum: no arithmetic, so the kernels equal the statement
on every input.
"""
import numpy as np

MAX_ROWS = 8192                         # asw_global_clusters refuses more candidates


def global_clusters_f64(full, seg, counts, near, *, sim_db=-1.0, win_hi=-2.0, win_lo=-7.0, best_hi=-1.0, best_lo=-5.0):
    """-> (label [n] int32, merge [n, n] uint8).

    ``full`` float64 [n, n]: SI-SDR of est i against ref j (``pair_sisdr``); ``seg`` float64 [n, n, K], K >= 1: the
    segment-wise SI-SDR (``segment_sisdr``); ``counts`` int32 [n]: the segment counts, c_i = min(max(counts[i], 0), K),
    and only the slots k < c_i of row i are ever read (the slots beyond may hold anything); ``near`` uint8 [n, n]: the
    host's ``dis < 0.45``.  The rows are in visiting order (descending power).

    * win[i][j] = (any k < c_i: seg[i][j][k] > win_hi) and not (any k < c_i: seg[i][j][k] < win_lo);
    * merge[i][j] = full[i][j] > sim_db or win[i][j] or near[i][j] != 0; NaN compares false everywhere;
    * walking i = 0 .. n - 1 with the heads kept in creation order:
      1. c_i == 0: label[i] = -1 (discarded, "no valid split");
      2. some head h has merge[i][h]: label[i] = the FIRST such head in creation order;
      3. otherwise, with at least one head: best[k] = max over ALL heads h of seg[i][h][k], k < c_i, a maximum that
         propagates NaN (``np.amax``); if (any best[k] > best_hi) and not (any best[k] < best_lo): label[i] = -2
         (shadowed: neither a head nor a member);
      4. otherwise label[i] = i and i joins the heads."""
    full = np.asarray(full, dtype=np.float64)
    seg = np.asarray(seg, dtype=np.float64)
    counts = np.asarray(counts)
    near = np.asarray(near)
    if full.ndim != 2 or full.shape[0] != full.shape[1]:
        raise ValueError("full must be [n, n]")
    n = full.shape[0]
    if seg.ndim != 3 or seg.shape[:2] != (n, n) or seg.shape[2] < 1:
        raise ValueError("seg must be [n, n, K] with K >= 1")
    if counts.shape != (n,) or near.shape != (n, n):
        raise ValueError("counts must be [n] and near [n, n]")
    K = seg.shape[2]
    c = np.clip(counts.astype(np.int64), 0, K)
    used = (np.arange(K)[None, :] < c[:, None])[:, None, :]             # [n, 1, K]
    with np.errstate(invalid="ignore"):
        hi = np.any((seg > win_hi) & used, axis=2)
        lo = np.any((seg < win_lo) & used, axis=2)
        merge = (full > sim_db) | (hi & ~lo) | (near != 0)
    label = np.empty(n, dtype=np.int32)
    heads = []
    for i in range(n):
        ci = int(c[i])
        if ci == 0:
            label[i] = -1
            continue
        hit = np.flatnonzero(merge[i, heads]) if heads else ()
        if len(hit):
            label[i] = heads[int(hit[0])]
            continue
        if heads:
            with np.errstate(invalid="ignore"):
                best = np.amax(seg[i, heads, :ci], axis=0)
                if np.any(best > best_hi) and not np.any(best < best_lo):
                    label[i] = -2
                    continue
        label[i] = i
        heads.append(i)
    return label, merge.astype(np.uint8)


def clusters_of_labels(label):
    """{head: [head, members in ascending row]} with the heads in creation order -- the ``clusters`` dict
    ``MicArray.Clustering_new`` builds (a member always comes after its head)."""
    clusters = {}
    for i, h in enumerate(np.asarray(label).tolist()):
        if h == i:
            clusters[i] = [i]
        elif h >= 0:
            clusters[h].append(i)
    return clusters
