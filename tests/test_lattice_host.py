"""CPU only: the coarse TDoA lattice stated in numpy (``dense_grid.coarse_lattice`` / ``lattice_patches``) and the
search mode built on it, ``Prone_method="DENSE"`` -- stage 1 without a pruner.

The lattice has no counterpart in the reference (it only names the configuration), so it is checked by its own
invariants, by a two-microphone array whose cubes can be counted by hand, and by cube counts recorded when the
statement was written.  The mode is checked against the stages driven by hand with the surrogate scorer, and its
coarse stage on two gloo ranks against one rank."""
import io
import os
import socket
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd.dense_grid import coarse_lattice, lattice_keep_mask, lattice_patches
from acousticswarms_speech_amd.joint import JointModel
from acousticswarms_speech_amd.mic_array import FREQ_BINS, MicArray
from acousticswarms_speech_amd.scenes import make_scene
from acousticswarms_speech_amd.search import INIT_WIDTH
from acousticswarms_speech_amd.srp import SRPPhat
from tests.golden.surrogate import SurrogateSpot

SMALL_ROI = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
SMALL_ROI_CUBES = 509                     # width 8, array of make_scene(1010, 5, 7, 24000)


def _array(mics, roi, **kw):
    with redirect_stdout(io.StringIO()):
        return MicArray(np.asarray(mics), Spk_Range=list(roi), **kw)


# ---------------------------------------------------------------- the statement
@pytest.fixture(scope="module")
def g7_node(golden):
    g7 = golden("g7_srp_map")
    return _array(g7["mics"], g7["roi"]).SRP_node


@pytest.mark.parametrize("width, n_cubes", [(8, 3364), (4, 15970)])
def test_coarse_lattice_invariants(g7_node, width, n_cubes):
    node = g7_node
    lat = coarse_lattice(node, width)
    cells, bounds, members, centres = lat
    P = node.num_mic - 1
    planes = node._planes_1.reshape(P, -1)
    n_points = planes.shape[1]
    assert cells.dtype == bounds.dtype == members.dtype == np.int32 and centres.dtype == np.float64
    assert lat.width == width and lat.n_cubes == cells.shape[0]
    assert cells.shape == (n_cubes, P) and bounds.shape == (n_cubes + 1,) and centres.shape == (n_cubes, 3)
    assert (n_points, members.shape[0]) == (460800, 358464)

    # every kept point is in exactly one cube, keep-out points are in none
    keep = lattice_keep_mask(node)
    np.testing.assert_array_equal(np.sort(members), np.flatnonzero(keep))
    pos = np.asarray(node.Pos_1).reshape(-1, 3)
    b = node.array_border
    inside = (pos[:, 0] > b[0]) & (pos[:, 0] < b[2]) & (pos[:, 1] > b[1]) & (pos[:, 1] < b[3])
    assert inside.any() and not inside[members].any() and inside.sum() + members.shape[0] == n_points
    assert bounds[0] == 0 and bounds[-1] == members.shape[0] and np.all(np.diff(bounds) >= 1)

    # every member's TDoA is within width/2 of the cube's offsets on every pair
    cube_of = np.repeat(np.arange(n_cubes), np.diff(bounds))
    dev = np.abs(planes[:, members].T - cells[cube_of].astype(np.float64) * width)
    assert dev.max() <= width / 2

    # cubes strictly increasing lexicographically (pair 0 most significant), members ascending within a cube
    d = cells[1:].astype(np.int64) - cells[:-1]
    first = np.argmax(d != 0, axis=1)
    assert np.all(np.any(d != 0, axis=1)) and np.all(d[np.arange(n_cubes - 1), first] > 0)
    step = np.diff(members.astype(np.int64))
    step[bounds[1:-1] - 1] = 1                               # the steps from one cube to the next do not count
    assert np.all(step > 0)

    # centres: the members' positions summed one after the other, divided by their number
    for g in (0, n_cubes // 2, n_cubes - 1, int(np.argmax(np.diff(bounds)))):
        s = np.zeros(3)
        for k, i in enumerate(members[bounds[g]:bounds[g + 1]]):
            s = pos[i].copy() if k == 0 else s + pos[i]
        np.testing.assert_array_equal(centres[g], s / float(bounds[g + 1] - bounds[g]))


def test_two_microphones_on_a_line():
    """Microphones at x = 0.003 and 0.103 on the line y = z = 0, lookup points x = -1 + 0.01 k (k = 0..199) on that
    line.  Left of both microphones the TDoA is +0.1 m = 13.99 samples, right of both -13.99: width 8 gives the cells
    +2 and -2, width 4 gives +3 and -3 (13.99 / 4 = 3.498).  The keep-out is the open interval (-0.197, 0.303) in x
    (y = 0 lies inside its y range), so k = 0..80 (x <= -0.2) and k = 131..199 (x >= 0.31) remain: two cubes, the
    negative cell first."""
    mics = np.array([[0.003, 0.0, 0.0], [0.103, 0.0, 0.0]])
    roi = [-1.0, 1.0, 0.0, 0.01, 0.0, 0.1]
    node = SRPPhat(mic_pos=mics, freq_bins=FREQ_BINS, Range_spk=roi, grid_size=0.05, FS=48000, n_fft=2048)
    assert node._planes_1.shape == (1, 1, 200, 1)
    for width, cell in ((8, 2), (4, 3)):
        cells, bounds, members, centres = coarse_lattice(node, width)
        assert cells.tolist() == [[-cell], [cell]]
        assert bounds.tolist() == [0, 69, 150]
        assert members.tolist() == list(range(131, 200)) + list(range(0, 81))
        np.testing.assert_allclose(centres, [[-1 + 0.01 * 165, 0, 0], [-1 + 0.01 * 40, 0, 0]], atol=1e-12)
        patches = lattice_patches(node, coarse_lattice(node, width))
        assert [p.sample_offset.tolist() for p in patches] == [[-cell * width], [cell * width]]
        assert [p.area_size() for p in patches] == [69, 81]


# ---------------------------------------------------------------- the mode
@pytest.fixture(scope="module")
def small():
    """The small-ROI array in DENSE mode, its scene, and the search driven by hand: an array in the default mode,
    ``lattice_patches(coarse_lattice(...))`` as the stage-1 list, then the three later stages (surrogate scorer)."""
    sc = make_scene(1010, 5, 7, 24000)
    mix_t = torch.from_numpy(sc.mix)
    dense = _array(sc.mic_positions, SMALL_ROI, Prone_method="DENSE")
    ma = _array(sc.mic_positions, SMALL_ROI)
    spot = SurrogateSpot()
    with redirect_stdout(io.StringIO()):
        p1 = lattice_patches(ma.SRP_node, coarse_lattice(ma.SRP_node, INIT_WIDTH))
        p2 = ma.Spotform_Big_Patch(mix_t, p1, spot)
        kept = [int(np.flatnonzero([q is p for q in p1])[0]) for p in p2]
        pairs = ma.Spotform_Small_Patch_Parallel(mix_t, p2, spot)
        _audio, final, spot_times, _ = ma.Clustering_new(pairs)
    by_hand = {"kept": kept, "names": [p[3] for p in final], "powers": np.array([p[2] for p in final]),
               "centres": np.array([p[0].center_pos() for p in final]).reshape(-1, 3), "spot_times": int(spot_times),
               "trace": ma.trace, "calls": list(spot.calls)}
    return sc, mix_t, dense, by_hand


def test_dense_stage_one_is_the_lattice_and_reads_no_mixture(small):
    sc, _mix_t, dense, _ = small
    node = dense.SRP_node
    assert dense.Prone_method == "DENSE" and node.lattice.n_cubes == SMALL_ROI_CUBES and node.lattice.width == INIT_WIDTH
    nan_mix = np.full((7, 100), np.nan, dtype=np.float32)    # too short for any pruning window, and never read
    a, drop = dense.Apply_SRP_PHAT(nan_mix)
    b, _ = dense.Apply_SRP_PHAT(torch.from_numpy(nan_mix))
    assert drop.shape == (3, 3) and not drop.any()
    want = lattice_patches(node, coarse_lattice(node, INIT_WIDTH))
    assert len(a) == len(b) == len(want) == SMALL_ROI_CUBES
    for pa, pb, pw in zip(a, b, want):
        assert pa is not pb and pa.sample_offset is not pb.sample_offset and pa.width_list is not pb.width_list
        for x, y in ((pa, pb), (pa, pw)):
            np.testing.assert_array_equal(x.sample_offset, y.sample_offset)
            np.testing.assert_array_equal(x.width_list, y.width_list)
            np.testing.assert_array_equal(x.area_points, y.area_points)
            np.testing.assert_array_equal(x.peak_pos, y.peak_pos)
        assert pa.sample_offset.dtype == np.float64 and pa.peak_pos is not None
        assert np.all(pa.width_list == INIT_WIDTH) and pa.area_points.shape[0] == 3
    # a patch is the caller's to mutate (check_out does): the next call is not affected
    a[0].sample_offset[0] += 1000.0
    a[0].peak_pos[0] += 1.0
    c, _ = dense.Apply_SRP_PHAT(nan_mix)
    np.testing.assert_array_equal(c[0].sample_offset, want[0].sample_offset)
    np.testing.assert_array_equal(c[0].peak_pos, want[0].peak_pos)


def test_dense_forward_equals_the_stages_driven_by_hand(small):
    sc, mix_t, _dense, want = small
    spot = SurrogateSpot()
    jm = JointModel(spot)
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, SMALL_ROI, prone_method="DENSE")
        patches, _audio_loc, audio, d0, d1, spot_times = jm.forward(mix_t)
    assert jm.Mic_processor.Prone_method == "DENSE" and jm.previous_config.endswith("|DENSE")
    assert len(want["names"]) >= 1 and len(want["kept"]) >= 1
    assert spot.calls == want["calls"] and spot.calls[0] == (SMALL_ROI_CUBES, 0)
    assert [p[3] for p in patches] == want["names"] and int(spot_times) == want["spot_times"]
    assert jm.Mic_processor.trace == want["trace"]
    np.testing.assert_array_equal(np.array([p[0].center_pos() for p in patches]).reshape(-1, 3), want["centres"])
    np.testing.assert_array_equal(np.array([p[2] for p in patches]), want["powers"])
    assert audio is None and (d0, d1) == (0, 0)


def test_refusals(small):
    sc = small[0]
    with pytest.raises(ValueError, match="Prone_method"):
        _array(sc.mic_positions, SMALL_ROI, Prone_method="GRID")
    with pytest.raises(ValueError, match="Prone_method"), redirect_stdout(io.StringIO()):
        JointModel(None).setup(sc.mic_positions, SMALL_ROI, prone_method="dense")
    b = small[2].SRP_node.array_border                       # a region of interest inside the keep-out box
    inside = [b[0] + 0.05, b[2] - 0.05, b[1] + 0.05, b[3] - 0.05, 0.1, 0.5]
    with pytest.raises(RuntimeError, match="keep-out"):
        _array(sc.mic_positions, inside, Prone_method="DENSE")


def test_lattice_entry_points_reject_bad_arguments_without_a_gpu():
    from ctypes import c_int, c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    buf = np.zeros(64)
    p = c_void_p(buf.ctypes.data)
    counts = (c_int * 2)()
    assert L.asw_geom_lattice_workspace_bytes(0, 6) == -1
    assert b"geom_lattice_workspace_bytes" in L.asw_last_error()
    assert L.asw_geom_lattice_workspace_bytes(1000, 0) == -1 and L.asw_geom_lattice_workspace_bytes(1000, 32) == -1

    def lattice(planes=p, P=6, ny=4, nx=4, nz=2, width=8.0, ws_bytes=1 << 20, cells=p, counts=counts):
        return L.asw_geom_lattice(planes, P, ny, nx, nz, p, p, p, p, width, p, ws_bytes, cells, p, p, p, counts, None)
    assert lattice(planes=None) == -1 and b"geom_lattice: null" in L.asw_last_error()
    assert lattice(cells=None) == -1 and b"null output" in L.asw_last_error()
    assert lattice(counts=None) == -1
    assert lattice(ny=0) == -1 and b"bad grid" in L.asw_last_error()
    assert lattice(ny=1 << 12, nx=1 << 12, nz=1 << 8) == -1 and b"bad grid" in L.asw_last_error()
    assert lattice(P=0) == -1 and lattice(P=32) == -1 and b"outside 1..31" in L.asw_last_error()
    assert lattice(width=0.0) == -1 and lattice(width=float("nan")) == -1 and b"width" in L.asw_last_error()


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
        ma = _array(sc.mic_positions, SMALL_ROI, Prone_method="DENSE")
        inner = SurrogateSpot()
        spot = ShardedSpotModel(inner)
        with redirect_stdout(io.StringIO()):
            p1, _ = ma.Apply_SRP_PHAT(mix_t)
            p2 = ma.Spotform_Big_Patch(mix_t, p1, spot)
        kept = [int(np.flatnonzero([x is p for x in p1])[0]) for p in p2]
        q.put((rank, len(p1), kept, list(ma.trace["coarse_kept"]), [n for n, _s in inner.calls]))
    finally:
        dist.destroy_process_group()


def test_two_rank_dense_coarse_stage_matches_single_rank(small):
    """ShardedSpotModel's contiguous coarse split gives each rank a slice of the lattice; the energies are
    all-gathered and every rank keeps the single-rank set in the single-rank order."""
    import torch.multiprocessing as mp
    want = small[3]["kept"]
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
    for _rank, n1, kept, traced, _calls in res:
        assert n1 == SMALL_ROI_CUBES and kept == want and traced == want
    assert [c for _r, _n, _k, _t, c in res] == [[255], [254]]          # each rank scored its slice of the 509 cubes
