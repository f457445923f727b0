"""The fine stage's per-coarse-patch clustering, stated for a kernel (csrc/cluster_kernels.hip: asw_fine_clusters).

``MicArray._cluster_group`` sorts the candidates of one coarse patch by power, applies two thresholds and runs the
greedy "join the first head with SI-SDR > -4 dB" loop.  ``fine_clusters_f64`` restates those decisions for ALL coarse
patches of a call in float64, without a logarithm and with one fixed order of additions, so that the kernels reproduce
it bit for bit: the inner products of the SI-SDR come from a block-diagonal Gram matrix whose every entry is summed in
the order ``_gram_rows`` fixes, and "SI-SDR > sim_db" is the same comparison with the ``log10`` taken off both sides.
"""
import numpy as np

GRAM_LANES = 256                        # partial sums per inner product: one per thread of the kernel's workgroup
GRAM_MAX_ELEMS = 1 << 27                # cap of sum(n_g ** 2) over the groups of one call (asw_fine_clusters refuses more)
MIN_ERR = 1e-8                          # si_sdr's floor on the residual energy


def _gram_rows(y: np.ndarray) -> np.ndarray:
    """G[a][b] = sum_t y[a][t] * y[b][t] of the rows of one group, y [n, T] float64 holding float32 values (so every
    product is exact, and a fused multiply-add rounds the same value).  The order of the additions is fixed and does
    not depend on n: partial p[l], l < 256, is the sequential sum over t = l, l + 256, ... starting from 0.0; each
    64-wide quarter of p is reduced by p[:s] += p[s:2s] for s = 32 .. 1 (a wavefront's butterfly); the four quarter
    sums meet as (w0 + w1) + (w2 + w3).  G[a][b] and G[b][a] are the same bits."""
    n, T = y.shape
    steps = -(-T // GRAM_LANES)
    pad = np.zeros((n, steps * GRAM_LANES), dtype=np.float64)       # + 0.0 * 0.0 leaves a partial as it is
    pad[:, :T] = y
    pad = pad.reshape(n, steps, GRAM_LANES)
    p = np.zeros((n, n, GRAM_LANES), dtype=np.float64)
    for s in range(steps):
        p += pad[:, None, s, :] * pad[None, :, s, :]
    q = p.reshape(n, n, 4, 64)
    for s in (32, 16, 8, 4, 2, 1):
        q = q[..., :s] + q[..., s:2 * s]
    w = q[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _same_terms(ee, ss, es):
    """(sss, snn) of ``si_sdr``'s 10 log10(sss / snn) from the three inner products (estimate k, reference h)."""
    sss = es * es / ss
    snn = ee - sss
    snn = (snn if snn > 0 else 0.0) + MIN_ERR
    return sss, snn


def _walk(waves, bounds, energies, gate, group_gate, min_trigger, sim_db):
    waves = np.ascontiguousarray(waves, dtype=np.float32)
    bounds = np.asarray(bounds, dtype=np.int64)
    energies = np.asarray(energies, dtype=np.float64).reshape(-1, 2)
    gate = np.asarray(gate, dtype=np.float64)
    group_gate = np.asarray(group_gate, dtype=np.float64)
    N, G = waves.shape[0], bounds.shape[0] - 1
    if G < 0 or bounds[0] != 0 or bounds[-1] != N or np.any(np.diff(bounds) < 0):
        raise ValueError("bounds must start at 0, not decrease and end at the number of rows")
    if energies.shape[0] != N or gate.shape[0] != N or group_gate.shape[0] != G:
        raise ValueError("energies [N, 2], gate [N] and group_gate [G] must fit waves [N, T] and bounds [G + 1]")
    sizes = np.diff(bounds)
    if int(np.sum(sizes * sizes)) > GRAM_MAX_ELEMS:
        raise ValueError(f"sum of n_g ** 2 exceeds {GRAM_MAX_ELEMS}")
    ratio = 10.0 ** (float(sim_db) / 10.0)
    min_trigger = float(min_trigger)
    order = np.zeros(N, dtype=np.int32)
    label = np.full(N, -1, dtype=np.int32)
    grams, margin = [], np.inf
    with np.errstate(all="ignore"):
        for g in range(G):
            b0, n = int(bounds[g]), int(sizes[g])
            if n == 0:
                continue
            gram = _gram_rows(waves[b0:b0 + n].astype(np.float64))
            grams.append(gram.reshape(-1))
            power, power2 = energies[b0:b0 + n, 0], energies[b0:b0 + n, 1]
            visit = np.argsort(-power, kind="stable")
            order[b0:b0 + n] = b0 + visit
            if np.max(power2) < group_gate[g]:
                continue                                            # closed: every label stays -1
            heads = []
            for k in visit:
                if power2[k] < gate[b0 + k] or power[k] < min_trigger:
                    continue
                home = None
                for h in heads:
                    sss, snn = _same_terms(gram[k, k], gram[h, h], gram[k, h])
                    margin = min(margin, abs(10.0 * np.log10(sss / snn) - float(sim_db)))
                    if sss > ratio * snn:
                        home = h
                        break
                if home is None:
                    heads.append(k)
                    label[b0 + k] = b0 + k
                else:
                    label[b0 + k] = b0 + home
    packed = np.concatenate(grams) if grams else np.zeros(0, dtype=np.float64)
    return order, label, packed, float(margin)


def fine_clusters_f64(waves, bounds, energies, gate, group_gate, min_trigger, sim_db=-4.0):
    """-> (order [N] int32, label [N] int32, gram [sum n_g ** 2] float64).

    ``waves`` float32 [N, T]: the mean-removed candidate outputs; ``bounds`` int [G + 1]: CSR groups (one group = one
    coarse patch; bounds[0] = 0, non-decreasing, bounds[G] = N, empty groups allowed); ``energies`` float64 [N, 2] =
    (power, power2); ``gate`` float64 [N] = thr_new / (1 + d_k); ``group_gate`` float64 [G] = thr_new / (1 + d_big);
    ``min_trigger`` = MIN_TRIGGER_POWER / (3 * 48000) * T_len.

    * group g is OPEN unless it is empty or max(power2 over the group) < group_gate[g]; every candidate of a closed
      group gets label -1;
    * within a group the candidates are visited by descending power, equal powers by ascending index;
      order[bounds[g] + r] is the global row of the r-th visited candidate (written for closed groups too);
    * candidate k is skipped (label -1) iff power2[k] < gate[k] or power[k] < min_trigger;
    * any other k joins the first head h, in creation order, with same(k, h) -- label[k] = h, a global row -- or
      becomes a head, label[k] = k;
    * same(k, h): with ee = G[k][k], ss = G[h][h], es = G[k][h]: sss = es * es / ss, snn = max(ee - sss, 0) + 1e-8;
      the same talker iff sss > ratio * snn, ratio = 10.0 ** (sim_db / 10.0): ``si_sdr(k, h) > sim_db`` without log10;
    * gram: the block-diagonal Gram matrix packed group after group, group g row-major n_g x n_g at element offset
      sum_{h<g} n_h ** 2, every entry summed in the order of ``_gram_rows``.

    With NaN or Inf in ``waves`` or ``energies`` the result is unspecified."""
    return _walk(waves, bounds, energies, gate, group_gate, min_trigger, sim_db)[:3]


def fine_cluster_margin_db(waves, bounds, energies, gate, group_gate, min_trigger, sim_db=-4.0) -> float:
    """Smallest |10 log10(sss / snn) - sim_db| over the comparisons the greedy loop of ``fine_clusters_f64`` made
    (inf if it made none): how far the call is from a decision that another rounding of the same similarities
    could take differently.  For the tests."""
    return _walk(waves, bounds, energies, gate, group_gate, min_trigger, sim_db)[3]


def clusters_of_group(order, label, b0, n):
    """{head: [members]} of the group at rows b0 .. b0 + n with LOCAL indices, heads in creation order and members in
    visiting order -- the ``clusters`` dict ``MicArray._cluster_group`` builds."""
    clusters = {}
    for r in range(n):
        k = int(order[b0 + r])
        h = int(label[k])
        if h >= 0:
            clusters.setdefault(h - b0, []).append(k - b0)
    return clusters
