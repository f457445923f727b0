"""GPU: non-maximum suppression over the lattice on the device (``asw_lattice_nms`` in csrc/geometry_kernels.hip,
``torch.ops.asw.lattice_nms``) and the search mode made of it (``Prone_method="DENSE_NMS"``).

1. the op against its numpy statement (``dense_grid.lattice_local_maxima``), exactly, on the smallest shapes that
   reach each path of the kernel, under score patterns with and without ties, at radius 1, 2 and 64;
2. two calls are bit-identical, and the result does not depend on what the workspace held;
3. a device-built array runs the op on the cells tensor its lattice build left on the GPU: only the scores go up;
4. the whole search in DENSE_NMS mode on a device-built array against the stages driven by hand on a host-built one;
5. a batch of mixtures in DENSE_NMS mode: the plain loop exactly, the concurrent form by its invariants.
There is no tolerance anywhere: integer compares and exact float64 compares on both sides.  Needs an MI355X."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests.lattice_nms_cases import coarse_by_hand, no_two_near, planted_scores

pytestmark = pytest.mark.gpu

SMALL_ROI = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
LINE = np.arange(-5, 6, dtype=np.int32)[:, None]
LINE_SCORES = np.array([0, 1, 3, 2, 2, 5, 5, 1, 0, 4, 4], dtype=np.float64)


def _array(mics, roi, geometry, **kw):
    from acousticswarms_speech_amd.mic_array import MicArray
    with redirect_stdout(io.StringIO()):
        return MicArray(np.asarray(mics), Spk_Range=list(roi), device="cuda", geometry=geometry, **kw)


def _op(cells, scores, radius):
    from acousticswarms_speech_amd.dense_grid import lattice_local_maxima_device
    dev = torch.from_numpy(np.ascontiguousarray(cells, dtype=np.int32)).cuda()
    return lattice_local_maxima_device(dev, scores, radius)


# ---------------------------------------------------------------- shapes
_TABLES = {}


def _cells(name, golden):
    """int32 [N,P] tables, each made once: lattices of host-built arrays (the numpy statement of the lattice) and,
    for the wide arrays, the cubes ``dense_tdoa_candidates`` enumerates -- sorted, distinct rows either way."""
    if name in _TABLES:
        return _TABLES[name]
    from acousticswarms_speech_amd.dense_grid import coarse_lattice, dense_tdoa_candidates
    from acousticswarms_speech_amd.scenes import make_scene
    if name == "single cube":
        cells = np.array([[3]], dtype=np.int32)
    elif name == "line":
        cells = LINE
    elif name == "7 mics":
        cells = coarse_lattice(_array(make_scene(1010, 5, 7, 24000).mic_positions, SMALL_ROI, "host").SRP_node, 8).cells
    elif name in ("g7 width 8", "g7 width 4"):
        g7 = golden("g7_srp_map")
        node = _array(g7["mics"], g7["roi"], "host").SRP_node
        _TABLES["g7 width 8"], _TABLES["g7 width 4"] = coarse_lattice(node, 8).cells, coarse_lattice(node, 4).cells
        return _TABLES[name]
    else:
        M = {"16 mics": 16, "32 mics": 32}[name]
        if M == 16:
            mics = make_scene(1010, 5, 16, 4000).mic_positions
        else:
            rng = np.random.default_rng(32)
            mics = np.stack([rng.uniform(-0.3, 0.3, 32), rng.uniform(0.0, 0.4, 32), rng.uniform(0.0, 0.05, 32)], axis=1)
        offsets, _counts, _ = dense_tdoa_candidates(mics, SMALL_ROI, width=8, step=0.02, with_points=False)
        cells = (offsets // 8).astype(np.int32)
        assert np.array_equal(cells.astype(np.int64) * 8, offsets) and cells.shape[1] == M - 1
    _TABLES[name] = cells
    return cells


def _pattern(name, cells, N):
    rng = np.random.default_rng(N)
    if name == "distinct":
        return rng.permutation(N).astype(np.float64) - N // 2
    if name == "equal":
        return np.full(N, 0.25)
    if name == "two-valued":
        return rng.integers(0, 2, N).astype(np.float64)
    if name == "zeros":                                      # +0.0, -0.0 and negative values, in equal parts
        return rng.choice(np.array([0.0, -0.0, -1.5]), N)
    return planted_scores(cells, 100, 1.5)[1]               # "planted"


SHAPES = [("single cube", 1, 1, (1, 2, 64)),                 # smallest input
          ("line", 11, 1, (1, 2, 64)),                       # the table counted by hand
          ("7 mics", 509, 6, (1, 2, 64)),                    # a ragged second row block
          ("g7 width 8", 3364, 6, (1, 2, 64)),               # several j splits
          ("g7 width 4", 15970, 6, (1,)),                    # many tiles per split
          ("16 mics", None, 15, (1, 2, 64)),                 # more than 8 pair fields: the 16-field kernel
          ("32 mics", None, 31, (1, 2, 64))]                 # the LDS maximum: the 31-field kernel
PATTERNS = ("distinct", "equal", "two-valued", "zeros")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name, N, P, radii", SHAPES, ids=[s[0] for s in SHAPES])
def test_op_equals_the_statement(golden, name, N, P, radii, pattern):
    from acousticswarms_speech_amd.dense_grid import lattice_local_maxima
    cells = _cells(name, golden)
    assert cells.dtype == np.int32 and cells.shape[1] == P and (N is None or cells.shape[0] == N)
    N = cells.shape[0]
    if name == "7 mics":
        assert N > 256 and N % 256 != 0
    scores = _pattern(pattern, cells, N)
    for radius in radii:
        best, degree = _op(cells, scores, radius)
        want_best, want_degree = lattice_local_maxima(cells, scores, radius)
        maxima = int(np.sum(want_best == np.arange(N)))
        print(f"{name} ({N} x {P}), {pattern}, radius {radius}: {maxima} maxima, degree up to {int(want_degree.max())}")
        assert best.dtype == degree.dtype == np.int32
        np.testing.assert_array_equal(best, want_best, err_msg=f"{name}, {pattern}, radius {radius}: best")
        np.testing.assert_array_equal(degree, want_degree, err_msg=f"{name}, {pattern}, radius {radius}: degree")


def test_the_line_counted_by_hand():
    best, degree = _op(LINE, LINE_SCORES, 1)
    assert best.tolist() == [1, 2, 2, 2, 5, 5, 5, 6, 9, 9, 9] and degree.tolist() == [1] + [2] * 9 + [1]
    best, degree = _op(LINE, LINE_SCORES, 10)
    assert best.tolist() == [5] * 11 and degree.tolist() == [10] * 11


@pytest.mark.parametrize("radius", [1, 2, 64])
def test_planted_bumps_on_g7(golden, radius):
    from acousticswarms_speech_amd.dense_grid import lattice_local_maxima
    cells = _cells("g7 width 8", golden)
    N = cells.shape[0]
    picks, scores = planted_scores(cells, 100, 1.5)
    best, degree = _op(cells, scores, radius)
    want_best, want_degree = lattice_local_maxima(cells, scores, radius)
    np.testing.assert_array_equal(best, want_best)
    np.testing.assert_array_equal(degree, want_degree)
    if radius == 64:                                         # every cube is near every other: one survivor
        assert np.all(best == picks[0]) and np.all(degree == N - 1)
    else:
        assert set(picks) <= set(np.flatnonzero(best == np.arange(N)).tolist())


def test_empty_table_through_the_op():
    from acousticswarms_speech_amd import native
    ops = native.torch_ops()
    best, degree = ops.lattice_nms(torch.zeros((0, 6), dtype=torch.int32, device="cuda"),
                                   torch.zeros(0, dtype=torch.float64, device="cuda"), 1)
    assert tuple(best.shape) == tuple(degree.shape) == (0,) and best.dtype == degree.dtype == torch.int32


def test_wrapper_refusals(golden):
    from acousticswarms_speech_amd.dense_grid import lattice_local_maxima_device
    cells = torch.from_numpy(LINE.copy()).cuda()
    with pytest.raises(ValueError, match="finite"):
        lattice_local_maxima_device(cells, np.where(np.arange(11) == 4, np.nan, LINE_SCORES), 1)
    with pytest.raises(ValueError, match="radius"):
        lattice_local_maxima_device(cells, LINE_SCORES, 0)
    with pytest.raises(ValueError, match="non-decreasing"):
        lattice_local_maxima_device(torch.flip(cells, dims=[0]).contiguous(), LINE_SCORES, 1)


def test_two_calls_are_bit_identical_whatever_the_workspace_held(golden):
    """Through the C ABI, where the workspace is the caller's: pre-filled with 0xFF bytes, zeroed, and again."""
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    from acousticswarms_speech_amd.dense_grid import lattice_local_maxima
    L = native.lib()
    cells = _cells("g7 width 8", golden)
    N, P = cells.shape
    scores = _pattern("two-valued", cells, N)
    cells_d, scores_d = torch.from_numpy(cells).cuda(), torch.from_numpy(scores).cuda()
    ws_bytes = L.asw_lattice_nms_workspace_bytes(N, P)
    assert ws_bytes >= 2 * 2 * 4 * N                        # at least two splits of (best, degree)
    got = []
    for fill in (0xFF, 0x00, 0xFF):
        ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device="cuda")
        best = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        degree = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        native.check(L.asw_lattice_nms(c_void_p(cells_d.data_ptr()), N, P, c_void_p(scores_d.data_ptr()), 1,
                                       c_void_p(ws.data_ptr()), ws_bytes, c_void_p(best.data_ptr()),
                                       c_void_p(degree.data_ptr()), native.current_stream()))
        torch.cuda.synchronize()
        got.append((best.cpu().numpy().tobytes(), degree.cpu().numpy().tobytes()))
    assert got[0] == got[1] == got[2]
    want_best, want_degree = lattice_local_maxima(cells, scores, 1)
    assert got[0] == (want_best.tobytes(), want_degree.tobytes())


def test_the_op_reads_the_cells_left_on_the_device(monkeypatch):
    """A device-built DENSE_NMS array keeps the cells tensor of its lattice build (its own N x P x 4 bytes); a
    suppression uploads the N scores and nothing else, and the op reads that tensor."""
    from acousticswarms_speech_amd import native
    from acousticswarms_speech_amd.dense_grid import lattice_local_maxima
    from acousticswarms_speech_amd.scenes import make_scene
    ops = native.torch_ops()
    built, read, uploads = [], [], []

    class Spy(object):
        def __getattr__(self, name):
            fn = getattr(ops, name)
            if name == "geom_lattice":
                return lambda *a: (built.append(fn(*a)), built[-1])[1]
            if name == "lattice_nms":
                return lambda cells, *a: (read.append(cells), fn(cells, *a))[1]
            return fn
    from_numpy = torch.from_numpy
    monkeypatch.setattr(native, "torch_ops", lambda: Spy())
    node = _array(make_scene(1010, 5, 7, 4000).mic_positions, SMALL_ROI, "device", Prone_method="DENSE_NMS").SRP_node
    N, P = node.lattice.cells.shape
    kept = node._geom_dev["cells"]
    assert len(built) == 1 and kept.is_cuda and tuple(kept.shape) == (N, P) == (509, 6)
    assert torch.equal(kept, built[0][0]) and kept.untyped_storage().nbytes() == N * P * 4
    np.testing.assert_array_equal(kept.cpu().numpy(), node.lattice.cells)
    scores = np.random.default_rng(3).standard_normal(N)
    monkeypatch.setattr(torch, "from_numpy", lambda a: (uploads.append(int(a.size)), from_numpy(a))[1])
    best, degree = node.lattice_local_maxima(scores, 1)
    monkeypatch.undo()
    assert len(read) == 1 and read[0] is kept
    assert uploads == [N] and N < N * P                      # the scores; nothing as large as the cell table
    want_best, want_degree = lattice_local_maxima(node.lattice.cells, scores, 1)
    np.testing.assert_array_equal(best, want_best)
    np.testing.assert_array_equal(degree, want_degree)


# ------------------------------------------------------------------------------ with the spot network
@pytest.fixture(scope="module")
def spot():
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    return SpotModel(SMALL, make_spot_state_dict(SMALL, 21), batch_size=32).to("cuda")


def _summary(patches, spot_times):
    return (np.array([p[0].center_pos() for p in patches]).reshape(-1, 3), np.array([p[2] for p in patches]),
            [p[3] for p in patches], int(spot_times))


def _trace(ma):
    tr = ma.trace
    return {"coarse_kept": list(tr["coarse_kept"]), "fine_clusters": {g: dict(c) for g, c in tr["fine_clusters"].items()},
            "final_clusters": [list(c) for c in tr["final_clusters"]]}


def _forward(jm, mix_t):
    with redirect_stdout(io.StringIO()):
        patches, _al, _a, _d0, _d1, spot_times = jm.forward(mix_t)
    return _summary(patches, spot_times), _trace(jm.Mic_processor)


def test_whole_dense_nms_search_on_a_device_built_array_equals_the_stages_by_hand(spot):
    """JointModel in DENSE_NMS mode on a device-built array against a host-built array in the default mode driven
    through the stages, its coarse stage written out with the numpy statement.  Bit-equal, the quantities of
    test_whole_dense_search_on_a_device_built_array_equals_the_stages_by_hand."""
    from acousticswarms_speech_amd.dense_grid import coarse_lattice, lattice_patches
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.search import INIT_WIDTH
    sc = make_scene(1001, 3, 7, 24000)
    mix_t = torch.from_numpy(sc.mix)
    jm = JointModel(spot, None, device="cuda", geometry="device")
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, SMALL_ROI, prone_method="DENSE_NMS")
    mp = jm.Mic_processor
    assert mp.SRP_node.geometry == "device" and mp.Prone_method == "DENSE_NMS"
    got, trace_got = _forward(jm, mix_t)

    ma = _array(sc.mic_positions, SMALL_ROI, "host")
    with redirect_stdout(io.StringIO()):
        lat = coarse_lattice(ma.SRP_node, INIT_WIDTH)
        p1 = lattice_patches(ma.SRP_node, lat)
        final, spot_times = [], 0
        kept = coarse_by_hand(ma, mix_t, p1, spot, lat.cells, 1)
        ma.big_spotforming_times = len(p1)
        ma.trace = {"coarse_kept": list(kept), "fine_clusters": {}, "final_clusters": []}
        if len(kept) > 0:
            pairs = ma.Spotform_Small_Patch_Parallel(mix_t, [p1[i] for i in kept], spot)
            if len(pairs) > 0:
                _audio, final, spot_times, _ = ma.Clustering_new(pairs)
    want, trace_want = _summary(final, spot_times), _trace(ma)
    print(f"DENSE_NMS search: {len(p1)} cubes, {len(kept)} kept, {want[3]} spot evaluations, {len(want[2])} talkers")
    assert len(p1) == mp.big_spotforming_times and len(kept) >= 1 and no_two_near(lat.cells, kept, 1)
    assert mp.lattice_nms["radius"] == 1 and np.all(mp.lattice_nms["best"][kept] == kept)
    assert got[2] == want[2] and got[3] == want[3]                     # names, spot_times
    assert trace_got == trace_want                                     # every hard decision
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_dense_nms_batch(spot, monkeypatch):
    """Four mixtures recorded with one array.  ``concurrent=1`` is the per-mixture loop and equals it exactly.  With
    ``concurrent=2`` a candidate's energy moves by about 1e-6 with the internal batch it lands in, and a decision
    between two near-equal neighbours may differ, so only the invariants hold: one result per mixture, at least one
    kept cube each, no two kept cubes near each other."""
    from acousticswarms_speech_amd import batching
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.shard import localize_batch
    a = make_scene(1001, 3, 7, 24000)
    scenes = [a] + [make_scene(1001 + k, 3, 7, 24000, mic_positions=a.mic_positions) for k in (2, 3, 4)]
    mixes = [torch.from_numpy(s.mix) for s in scenes]
    jm = JointModel(spot, None, device="cuda", geometry="device")
    with redirect_stdout(io.StringIO()):
        jm.setup(a.mic_positions, SMALL_ROI, prone_method="DENSE_NMS")
    want = [_forward(jm, m)[0] for m in mixes]
    with redirect_stdout(io.StringIO()):
        got = localize_batch(jm, mixes, concurrent=1)
    assert len(got) == 4
    for r, w in zip(got, want):
        assert list(r["names"]) == w[2] and int(r["spot_times"]) == w[3]
        np.testing.assert_array_equal(r["centres"], w[0])
        np.testing.assert_array_equal(r["powers"], w[1])

    views = []
    view_of = batching.mixture_view
    monkeypatch.setattr(batching, "mixture_view", lambda m: (views.append(view_of(m)), views[-1])[1])
    with redirect_stdout(io.StringIO()):
        got = localize_batch(jm, mixes, concurrent=2)
    monkeypatch.undo()
    cells = jm.Mic_processor.SRP_node.lattice.cells
    assert len(got) == 4 and all(r is not None for r in got) and len(views) == 4
    for v in views:
        kept = v.trace["coarse_kept"]
        assert v.lattice_nms is not None and v.lattice_nms["radius"] == 1
        assert len(kept) >= 1 and np.all(v.lattice_nms["best"][kept] == kept) and no_two_near(cells, kept, 1)
        assert v.SRP_node._geom_dev["cells"] is jm.Mic_processor.SRP_node._geom_dev["cells"]
