"""CPU only: non-maximum suppression over the coarse TDoA lattice stated in numpy
(``dense_grid.lattice_local_maxima``) and the search mode built on it, ``Prone_method="DENSE_NMS"``.

The statement is checked on a table counted by hand, by its invariants on the g7 lattice, and against an unchunked
brute force.  The capability -- several talkers found on a lattice whose cubes around each talker are all strong -- is
checked on planted bumps with a stand-in scorer.  The mode is checked against the stages driven by hand with the
surrogate scorer, its coarse stage on two gloo ranks against one rank, and the C entry points' refusals through
ctypes."""
import io
import os
import socket
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import search
from acousticswarms_speech_amd.dense_grid import coarse_lattice, lattice_local_maxima, lattice_patches
from acousticswarms_speech_amd.joint import JointModel
from acousticswarms_speech_amd.mic_array import MicArray
from acousticswarms_speech_amd.scenes import make_scene
from acousticswarms_speech_amd.search import INIT_WIDTH, MAX_BIG_PATCH
from tests.golden.surrogate import SurrogateSpot
from tests.lattice_nms_cases import chebyshev, coarse_by_hand, no_two_near, planted_scores

SMALL_ROI = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
SMALL_ROI_CUBES = 509                     # width 8, array of make_scene(1010, 5, 7, 24000)
G7_CUBES = 3364


def _array(mics, roi, **kw):
    with redirect_stdout(io.StringIO()):
        return MicArray(np.asarray(mics), Spk_Range=list(roi), **kw)


# ---------------------------------------------------------------- the statement
def test_table_counted_by_hand():
    """Eleven cubes on a line.  Cube 7 (score 1) has the near cubes 6, 7 and 8 with scores 5, 1, 0, so its best is
    cube 6 -- cube 5 holds the same score but lies two cells away, and ``best[i]`` is a near cube by definition."""
    cells = np.arange(-5, 6, dtype=np.int32)[:, None]
    scores = np.array([0, 1, 3, 2, 2, 5, 5, 1, 0, 4, 4], dtype=np.float64)
    best, degree = lattice_local_maxima(cells, scores, 1)
    assert best.dtype == degree.dtype == np.int32
    assert best.tolist() == [1, 2, 2, 2, 5, 5, 5, 6, 9, 9, 9]
    assert np.flatnonzero(best == np.arange(11)).tolist() == [2, 5, 9]
    assert degree.tolist() == [1] + [2] * 9 + [1]
    best, degree = lattice_local_maxima(cells, scores, 10)
    assert best.tolist() == [5] * 11 and degree.tolist() == [10] * 11
    # -0.0 ties with 0.0: the lower index stays
    best, _ = lattice_local_maxima(cells[:3], np.array([-1.0, 0.0, -0.0]), 1)
    assert best.tolist() == [1, 1, 1]
    best, _ = lattice_local_maxima(cells[:3], np.array([-1.0, -0.0, 0.0]), 1)
    assert best.tolist() == [1, 1, 1]


def test_empty_table_and_refusals():
    best, degree = lattice_local_maxima(np.zeros((0, 6), np.int32), np.zeros(0))
    assert best.shape == degree.shape == (0,) and best.dtype == degree.dtype == np.int32
    cells = np.arange(4, dtype=np.int32)[:, None]
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            lattice_local_maxima(cells, np.array([0.0, bad, 1.0, 2.0]))
    with pytest.raises(ValueError, match="radius"):
        lattice_local_maxima(cells, np.zeros(4), 0)
    with pytest.raises(ValueError, match="scores"):
        lattice_local_maxima(cells, np.zeros(3))


@pytest.fixture(scope="module")
def g7_cells(golden):
    g7 = golden("g7_srp_map")
    cells = coarse_lattice(_array(g7["mics"], g7["roi"]).SRP_node, INIT_WIDTH).cells
    assert cells.shape == (G7_CUBES, 6)
    return cells


@pytest.mark.parametrize("radius, figures", [(1, (10, 57, 110)), (2, (26, 194, 327))])
def test_invariants_on_the_g7_lattice(g7_cells, radius, figures):
    cells = g7_cells
    N = cells.shape[0]
    scores = np.random.default_rng(radius).permutation(N).astype(np.float64)          # distinct
    best, degree = lattice_local_maxima(cells, scores, radius)
    idx = np.arange(N)
    assert np.all(chebyshev(cells, idx, best) <= radius) and np.all(scores[best] >= scores[idx])
    maxima = np.flatnonzero(best == idx)
    assert 1 <= len(maxima) < N and no_two_near(cells, maxima, radius)
    assert (int(degree.min()), int(np.median(degree)), int(degree.max())) == figures
    # a cube that is no maximum has a strictly better near cube; the best of a maximum's neighbourhood is itself
    assert np.all(scores[best[best != idx]] > scores[idx[best != idx]])


def test_equal_scores_keep_the_lowest_near_index(g7_cells):
    cells = g7_cells
    N = cells.shape[0]
    best, degree = lattice_local_maxima(cells, np.full(N, 0.25), 1)
    near = np.max(np.abs(cells[:, None, :].astype(np.int64) - cells[None, :, :]), axis=2) <= 1
    np.testing.assert_array_equal(best, np.argmax(near, axis=1))
    np.testing.assert_array_equal(degree, near.sum(axis=1) - 1)
    assert int(np.sum(best == np.arange(N))) == 7
    best, degree = lattice_local_maxima(cells, np.full(N, 0.25), 64)
    assert np.all(best == 0) and np.all(degree == N - 1)


def test_chunked_statement_equals_brute_force():
    sc = make_scene(1010, 5, 7, 24000)
    cells = coarse_lattice(_array(sc.mic_positions, SMALL_ROI).SRP_node, INIT_WIDTH).cells
    N = cells.shape[0]
    assert N == SMALL_ROI_CUBES
    rng = np.random.default_rng(5)
    for scores in (rng.standard_normal(N), rng.integers(0, 2, N).astype(np.float64)):
        for radius in (1, 2):
            near = np.max(np.abs(cells[:, None, :].astype(np.int64) - cells[None, :, :]), axis=2) <= radius
            want_best = np.array([min(np.flatnonzero(near[i]), key=lambda j: (-scores[j], j)) for i in range(N)])
            for chunk in (1, 1000, 1 << 22):                 # one row at a time, ragged chunks, one chunk
                best, degree = lattice_local_maxima(cells, scores, radius, chunk=chunk)
                np.testing.assert_array_equal(best, want_best)
                np.testing.assert_array_equal(degree, near.sum(axis=1) - 1)


# ---------------------------------------------------------------- planted talkers: the capability
class PlantedSpot(object):
    """Stand-in scorer: the energy of a candidate is the planted score of the cube its offsets name."""

    def __init__(self, cells, scores, width):
        self.table = {tuple(int(v) for v in c): float(s) for c, s in zip(cells, scores)}
        self.width = width

    def shift_and_score(self, mix, patch_list, Strict=0, keep_waveforms=False):
        s = [self.table[tuple(int(v) for v in np.rint(np.asarray(p.sample_offset) / self.width))] for p in patch_list]
        return np.stack([np.array(s), np.array(s)], axis=1)


@pytest.fixture(scope="module")
def g7_arrays(golden):
    g7 = golden("g7_srp_map")
    return {m: _array(g7["mics"], g7["roi"], Prone_method=m) for m in ("DENSE", "DENSE_NMS")}


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("sigma", [1.5, 3.0])
@pytest.mark.parametrize("seed", [100, 101, 102, 103])
def test_planted_talkers_are_all_found(g7_arrays, monkeypatch, seed, sigma, radius):
    nms, dense = g7_arrays["DENSE_NMS"], g7_arrays["DENSE"]
    cells = nms.SRP_node.lattice.cells
    picks, scores = planted_scores(cells, seed, sigma)
    spot = PlantedSpot(cells, scores, INIT_WIDTH)
    mix = np.zeros((7, 100), dtype=np.float32)
    monkeypatch.setattr(search, "LATTICE_NMS_RADIUS", radius)          # read at call time
    with redirect_stdout(io.StringIO()):
        p1, _ = nms.Apply_SRP_PHAT(mix)
        kept = nms.Spotform_Big_Patch(mix, p1, spot)
        d1, _ = dense.Apply_SRP_PHAT(mix)
        dense_kept = dense.Spotform_Big_Patch(mix, d1, spot)
    assert nms.trace["coarse_kept"] == picks                           # exactly the planted cubes, loudest first
    assert [p1.index(p) for p in kept] == picks
    assert nms.lattice_nms["radius"] == radius and nms.lattice_nms["best"].shape == (G7_CUBES,)
    want_best, want_degree = lattice_local_maxima(cells, scores, radius)
    np.testing.assert_array_equal(nms.lattice_nms["best"], want_best)
    np.testing.assert_array_equal(nms.lattice_nms["degree"], want_degree)
    # without the suppression the 30 kept cubes crowd around the loudest talkers
    got = dense.trace["coarse_kept"]
    assert len(got) == len(dense_kept) == MAX_BIG_PATCH and dense.lattice_nms is None
    nearest = {int(np.argmin([chebyshev(cells, i, j) for j in picks])) for i in got}
    assert len(nearest) <= 3


# ---------------------------------------------------------------- the mode
@pytest.fixture(scope="module")
def small():
    sc = make_scene(1010, 5, 7, 24000)
    mix_t = torch.from_numpy(sc.mix)
    ma = _array(sc.mic_positions, SMALL_ROI)
    spot = SurrogateSpot()
    with redirect_stdout(io.StringIO()):
        lat = coarse_lattice(ma.SRP_node, INIT_WIDTH)
        p1 = lattice_patches(ma.SRP_node, lat)
        kept = coarse_by_hand(ma, mix_t, p1, spot, lat.cells, 1)
        ma.big_spotforming_times = len(p1)
        ma.trace = {"coarse_kept": list(kept), "fine_clusters": {}, "final_clusters": []}
        pairs = ma.Spotform_Small_Patch_Parallel(mix_t, [p1[i] for i in kept], spot)
        _audio, final, spot_times, _ = ma.Clustering_new(pairs)
    by_hand = {"kept": kept, "names": [p[3] for p in final], "powers": np.array([p[2] for p in final]),
               "centres": np.array([p[0].center_pos() for p in final]).reshape(-1, 3), "spot_times": int(spot_times),
               "trace": ma.trace, "calls": list(spot.calls), "cells": lat.cells}
    return sc, mix_t, by_hand


def test_dense_nms_forward_equals_the_stages_driven_by_hand(small):
    sc, mix_t, want = small
    spot = SurrogateSpot()
    jm = JointModel(spot)
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, SMALL_ROI, prone_method="DENSE_NMS")
        patches, _audio_loc, audio, d0, d1, spot_times = jm.forward(mix_t)
    ma = jm.Mic_processor
    assert ma.Prone_method == "DENSE_NMS" and jm.previous_config.endswith("|DENSE_NMS")
    assert ma.SRP_node.lattice.n_cubes == SMALL_ROI_CUBES and ma.SRP_node.lattice.width == INIT_WIDTH
    assert len(want["names"]) >= 1 and len(want["kept"]) >= 1
    assert spot.calls == want["calls"] and spot.calls[0] == (SMALL_ROI_CUBES, 0)
    assert [p[3] for p in patches] == want["names"] and int(spot_times) == want["spot_times"]
    assert ma.trace == want["trace"] and set(ma.trace) == {"coarse_kept", "fine_clusters", "final_clusters"}
    np.testing.assert_array_equal(np.array([p[0].center_pos() for p in patches]).reshape(-1, 3), want["centres"])
    np.testing.assert_array_equal(np.array([p[2] for p in patches]), want["powers"])
    assert audio is None and (d0, d1) == (0, 0)
    kept = ma.trace["coarse_kept"]
    assert kept == want["kept"] and no_two_near(want["cells"], kept, 1)
    assert ma.lattice_nms["radius"] == 1 and np.all(ma.lattice_nms["best"][kept] == kept)

    # DENSE on the same mixture: the same first cube (the global maximum is a local one), and near cubes among the 30
    dense = SurrogateSpot()
    jd = JointModel(dense)
    with redirect_stdout(io.StringIO()):
        jd.setup(sc.mic_positions, SMALL_ROI, prone_method="DENSE")
        p1, _ = jd.Mic_processor.Apply_SRP_PHAT(mix_t)
        jd.Mic_processor.Spotform_Big_Patch(mix_t, p1, dense)
    dense_kept = jd.Mic_processor.trace["coarse_kept"]
    assert dense_kept[0] == kept[0] and jd.Mic_processor.lattice_nms is None
    assert jd.previous_config.endswith("|DENSE")


def test_views_share_the_lattice_and_own_their_record(small):
    from acousticswarms_speech_amd.batching import mixture_view
    sc, mix_t, want = small
    ma = _array(sc.mic_positions, SMALL_ROI, Prone_method="DENSE_NMS")
    view = mixture_view(ma)
    spot = SurrogateSpot()
    with redirect_stdout(io.StringIO()):
        p1, _ = view.Apply_SRP_PHAT(mix_t)
        view.Spotform_Big_Patch(mix_t, p1, spot)
    assert view.trace["coarse_kept"] == want["kept"] and view.lattice_nms is not None
    assert ma.lattice_nms is None and ma.trace["coarse_kept"] == []
    assert view.SRP_node.lattice is ma.SRP_node.lattice


def test_a_patch_list_that_is_not_the_lattice_is_refused(small):
    sc, mix_t, _ = small
    ma = _array(sc.mic_positions, SMALL_ROI, Prone_method="DENSE_NMS")
    with redirect_stdout(io.StringIO()):
        p1, _ = ma.Apply_SRP_PHAT(mix_t)
    spot = PlantedSpot(ma.SRP_node.lattice.cells, np.ones(SMALL_ROI_CUBES), INIT_WIDTH)
    with pytest.raises(ValueError, match="one value per cube"):
        ma.Spotform_Big_Patch(mix_t, p1[:100], spot)


def test_nms_entry_points_reject_bad_arguments_without_a_gpu():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    buf = np.zeros(64)
    p = c_void_p(buf.ctypes.data)
    assert L.asw_lattice_nms_workspace_bytes(-1, 6) == -1
    assert b"lattice_nms_workspace_bytes" in L.asw_last_error()
    assert L.asw_lattice_nms_workspace_bytes(100, 0) == -1 and L.asw_lattice_nms_workspace_bytes(100, 32) == -1
    assert L.asw_lattice_nms_workspace_bytes(0, 6) == 0
    need = L.asw_lattice_nms_workspace_bytes(G7_CUBES, 6)
    assert need >= 2 * 4 * G7_CUBES

    def nms(cells=p, N=8, P=6, scores=p, radius=1, ws=p, ws_bytes=1 << 20, best=p, degree=p):
        return L.asw_lattice_nms(cells, N, P, scores, radius, ws, ws_bytes, best, degree, None)
    for name in ("cells", "scores", "ws"):
        assert nms(**{name: None}) == -1 and b"lattice_nms: null pointer" in L.asw_last_error(), name
    for name in ("best", "degree"):
        assert nms(**{name: None}) == -1 and b"null output" in L.asw_last_error(), name
    assert nms(N=-1) == -1 and b"N = -1" in L.asw_last_error()
    assert nms(P=0) == -1 and nms(P=32) == -1 and b"outside 1..31" in L.asw_last_error()
    assert nms(radius=0) == -1 and nms(radius=-3) == -1 and b"radius" in L.asw_last_error()
    assert nms(N=G7_CUBES, ws_bytes=need - 1) == -1 and b"too small" in L.asw_last_error()
    assert nms(N=0, cells=None, scores=None, ws=None, ws_bytes=0, best=None, degree=None) == 0      # launches nothing


# ---------------------------------------------------------------- coarse stage on two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _coarse_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from acousticswarms_speech_amd.shard import ShardedSpotModel
        sc = make_scene(1010, 5, 7, 24000)
        mix_t = torch.from_numpy(sc.mix)
        ma = _array(sc.mic_positions, SMALL_ROI, Prone_method="DENSE_NMS")
        inner = SurrogateSpot()
        spot = ShardedSpotModel(inner)
        with redirect_stdout(io.StringIO()):
            p1, _ = ma.Apply_SRP_PHAT(mix_t)
            p2 = ma.Spotform_Big_Patch(mix_t, p1, spot)
        kept = [int(np.flatnonzero([x is p for x in p1])[0]) for p in p2]
        q.put((rank, len(p1), kept, list(ma.trace["coarse_kept"]), [n for n, _s in inner.calls],
               ma.lattice_nms["best"].tolist()))
    finally:
        dist.destroy_process_group()


def test_two_rank_dense_nms_coarse_stage_matches_single_rank(small):
    """Every rank holds all energies after the all-gather and runs the same suppression: the single-rank set in the
    single-rank order on both."""
    import torch.multiprocessing as mp
    want = small[2]["kept"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_coarse_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for _rank, n1, kept, traced, _calls, _best in res:
        assert n1 == SMALL_ROI_CUBES and kept == want and traced == want
    assert res[0][5] == res[1][5]
    assert [r[4] for r in res] == [[255], [254]]             # each rank scored its slice of the 509 cubes
