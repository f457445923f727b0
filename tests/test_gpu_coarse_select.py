"""GPU: the lattice coarse stage's decision on the device (``asw_coarse_select`` in csrc/cluster_kernels.hip,
``torch.ops.asw.coarse_select``) and the search mode made of it (``MicArray(coarse="device")``).

1. the op against its numpy statement (``search.coarse_select_f64``) in every output byte -- kept, counts, thr -- on the
   sizes around the cap, the wavefront, the workgroup and the kernel's slice of 1024 cubes, on the lattice sizes
   3 364, 15 970 and 70 001, at cap 1, 30 and 64, with the relative threshold on and off, under the generated kinds of
   tests/coarse_select_cases.py (none / exactly cap / cap + 1 / all pass, winners in the first or the last slice, runs
   of equal powers across the slice boundaries, two values, signed zeros, NaN and Inf, a ``best`` that removes the top);
2. the C entry point on outputs and a workspace filled with 0xFF, and two calls compared;
3. the adapter's refusals;
4. the whole search, ``coarse="device"`` against ``coarse="host"``: DENSE and DENSE_NMS on host- and device-built
   arrays, the calls counted, and a batch of four mixtures.
There is no tolerance anywhere.  Needs an MI355X."""
import contextlib
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests import coarse_select_cases as cases

pytestmark = pytest.mark.gpu

SMALL_ROI = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
SMALL_ROI_CUBES = 509


def _op(case):
    from acousticswarms_speech_amd import native
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    best = None if case["best"] is None else up(case["best"].astype(np.int32))
    return native.torch_ops().coarse_select(up(case["energies"]), up(case["dis1"]), best, case["thr1"], case["relative"],
                                            case["rel"], case["cap"])


def _bytes(triple):
    return tuple(np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).tobytes() for t in triple)


def _check(case, what):
    from acousticswarms_speech_amd.search import coarse_select_f64
    got = _op(case)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float64
    assert tuple(got[0].shape) == (case["cap"],) and tuple(got[1].shape) == (2,) and tuple(got[2].shape) == (2,)
    want = cases.expected(case, coarse_select_f64)
    g, w = _bytes(got), _bytes(want)
    assert g[1] == w[1], (what, "counts", got[1].tolist(), want[1].tolist())
    assert g[2] == w[2], (what, "thr", got[2].tolist(), want[2].tolist())
    assert g[0] == w[0], (what, "kept", got[0].tolist(), want[0].tolist())
    return want


# ---------------------------------------------------------------- the op against the statement
@pytest.mark.parametrize("N", cases.SIZES)
def test_op_equals_the_statement(N):
    seen = set()
    for cap in cases.CAPS:
        for kind in cases.KINDS:
            for relative in (False, True):
                case = cases.make_case(N, cap, kind, relative)
                kept, counts, _thr = _check(case, (N, cap, kind, relative))
                seen.add((kind, int(counts[0]) > cap, int(counts[0]) == 0))
    if N > 64:
        assert {k for k, over, _ in seen if over} >= {"cap_plus_1", "all", "ties", "two_valued", "zeros"}
        assert ("none", False, True) in seen


def test_cases_written_out():
    from acousticswarms_speech_amd.search import coarse_select_f64
    S = cases.SLICE
    nan = float("nan")
    base = {"best": None, "thr1": 0.008, "relative": False, "rel": 0.4, "cap": 30}

    def case(pw, dis1=None, **kw):
        pw = np.asarray(pw, dtype=np.float64)
        return dict(base, energies=np.stack([np.full(pw.shape[0], 7.0), pw], axis=1),
                    dis1=np.ones(pw.shape[0]) if dis1 is None else np.asarray(dis1, dtype=np.float64), **kw)
    # the hand case of the host test
    pw = [0.5, 0.02, 0.5, nan, -0.0, 0.0, 0.001, 0.9]
    d1 = [1, 1, 1, 1, 1, 1, 10, 1]
    kept, counts, thr = _check(case(pw, d1), "hand")
    assert kept[:7].tolist() == [7, 0, 2, 1, 6, 3, -1] and counts.tolist() == [6, 1] and thr.tolist() == [0.008, 0.9]
    kept, counts, thr = _check(case(pw, d1, thr1=1.0, relative=True, cap=3), "hand relative")
    assert kept.tolist() == [7, 0, 2] and counts.tolist() == [4, 1] and thr.tolist() == [0.4 * 0.9, 0.9]
    kept, counts, _ = _check(case(pw, d1, thr1=0.0), "hand zeros")
    assert kept[:9].tolist() == [7, 0, 2, 1, 6, 4, 5, 3, -1]
    # every power NaN: thr1 stays, the maximum is the quiet NaN, index order, in one slice and across four
    for N in (5, 3 * S + 17):
        for relative in (False, True):
            kept, counts, thr = _check(case(np.full(N, nan), relative=relative, cap=64), ("all NaN", N, relative))
            assert kept.tolist() == list(range(min(N, 64))) + [-1] * (64 - min(N, 64)) and counts.tolist() == [N, N]
            assert thr[0] == 0.008 and np.isnan(thr[1])
    # one value everywhere: the first cap indices, whatever the number of slices
    for N in (S - 1, S, S + 1, 2 * S, 5 * S + 3):
        kept, counts, _ = _check(case(np.full(N, 0.25), cap=64), ("constant", N))
        assert kept.tolist() == list(range(64)) and counts.tolist() == [N, 0]
    # the winners are the last cube of every slice, then equal powers on both sides of every boundary
    N = 4 * S
    pw = np.full(N, 0.01)
    pw[S - 1::S] = [4.0, 3.0, 2.0, 1.0]
    pw[S - 3:S + 3] = 0.5
    pw[S - 1] = 4.0
    kept, counts, _ = _check(case(pw, cap=30), "boundaries")
    assert kept[:9].tolist() == [S - 1, 2 * S - 1, 3 * S - 1, 4 * S - 1, S - 3, S - 2, S, S + 1, S + 2]
    # a best that keeps only every 1000th cube, values outside the table included
    N = 15970
    rng = np.random.default_rng(5)
    pw = 0.01 + rng.random(N)
    best = rng.integers(-5, N + 5, size=N).astype(np.int32)
    best[::1000] = np.arange(0, N, 1000)
    c = case(pw, best=best)
    kept, counts, _ = _check(c, "sparse best")
    alive = np.flatnonzero(best == np.arange(N))
    assert counts[0] == alive.shape[0] <= 30 and sorted(kept[:counts[0]].tolist()) == alive.tolist()
    assert coarse_select_f64(pw, np.ones(N), best == np.arange(N))[1] == counts[0]


def test_empty_table_through_the_op():
    from acousticswarms_speech_amd import native
    ops = native.torch_ops()
    for relative in (False, True):
        for best in (None, torch.zeros(0, dtype=torch.int32, device="cuda")):
            kept, counts, thr = ops.coarse_select(torch.zeros(0, 2, dtype=torch.float64, device="cuda"),
                                                  torch.zeros(0, dtype=torch.float64, device="cuda"), best, 0.125, relative, 0.4, 7)
            assert kept.tolist() == [-1] * 7 and counts.tolist() == [0, 0]
            assert thr[0].item() == 0.125 and thr.cpu().numpy().tobytes() == np.array([0.125, np.nan]).tobytes()


def test_energies_are_read_in_place_with_the_defaults_of_the_schema():
    """Column 1 of the [N,2] tensor is what counts; column 0 may hold anything; the schema's defaults are the search's
    constants."""
    from acousticswarms_speech_amd import native, search
    from acousticswarms_speech_amd.search import coarse_select_f64
    rng = np.random.default_rng(11)
    N = 3364
    pw, dis1 = rng.random(N) * 0.01, 1 + rng.random(N) * 4
    outs = []
    for col0 in (np.zeros(N), np.full(N, np.nan), rng.random(N) * 100):
        en = torch.from_numpy(np.stack([col0, pw], axis=1)).cuda()
        outs.append(_bytes(native.torch_ops().coarse_select(en, torch.from_numpy(dis1).cuda())))
    assert outs[0] == outs[1] == outs[2]
    kept, n_pass, thr = coarse_select_f64(pw, dis1, thr1=search.SPOT_POWER_THRESHOLD1, relative=False, cap=search.MAX_BIG_PATCH)
    assert np.frombuffer(outs[0][0], dtype=np.int32).tolist() == kept.tolist() and n_pass > 30
    assert np.frombuffer(outs[0][1], dtype=np.int32).tolist() == [n_pass, 0]


# ---------------------------------------------------------------- the C entry point on dirty buffers
@pytest.mark.parametrize("N, cap, kind, relative", [(3364, 30, "random", True), (2 * cases.SLICE + 1, 64, "ties", False),
                                                    (70001, 30, "nan_inf", True), (257, 1, "best_removes_top", False),
                                                    (31, 64, "all", True)])
def test_two_calls_are_bit_identical_whatever_the_buffers_held(N, cap, kind, relative):
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    from acousticswarms_speech_amd.search import coarse_select_f64
    L = native.lib()
    case = cases.make_case(N, cap, kind, relative)
    want = _bytes(cases.expected(case, coarse_select_f64))
    en = torch.from_numpy(case["energies"]).cuda()
    dis1 = torch.from_numpy(case["dis1"]).cuda()
    best = None if case["best"] is None else torch.from_numpy(case["best"].astype(np.int32)).cuda()
    need = L.asw_coarse_select_workspace_bytes(N, cap)
    assert need > 0 and need % 8 == 0
    results = []
    for fill in (0xFF, 0x00, 0x5A):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        kept = torch.full((cap * 4,), fill, dtype=torch.uint8, device="cuda")
        counts = torch.full((8,), fill, dtype=torch.uint8, device="cuda")
        thr = torch.full((16,), fill, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 8 == 0
        torch.cuda.synchronize()
        stream = c_void_p(torch.cuda.current_stream().cuda_stream)
        native.check(L.asw_coarse_select(c_void_p(en.data_ptr()), c_void_p(dis1.data_ptr()),
                                         None if best is None else c_void_p(best.data_ptr()), N, case["thr1"],
                                         int(case["relative"]), case["rel"], cap, c_void_p(ws.data_ptr()), need,
                                         c_void_p(kept.data_ptr()), c_void_p(counts.data_ptr()), c_void_p(thr.data_ptr()), stream))
        torch.cuda.synchronize()
        results.append(tuple(t.cpu().numpy().tobytes() for t in (kept, counts, thr)))
    assert results[0] == want and results[1] == want and results[2] == want
    # and the refusals leave the outputs alone: a workspace one byte short
    kept = torch.full((cap,), 123, dtype=torch.int32, device="cuda")
    rc = L.asw_coarse_select(c_void_p(en.data_ptr()), c_void_p(dis1.data_ptr()), None, N, 0.008, 0, 0.4, cap,
                             c_void_p(ws.data_ptr()), need - 1, c_void_p(kept.data_ptr()), c_void_p(counts.data_ptr()),
                             c_void_p(thr.data_ptr()), stream)
    torch.cuda.synchronize()
    assert rc == -1 and b"too small" in L.asw_last_error() and kept.tolist() == [123] * cap


def test_adapter_refusals():
    from acousticswarms_speech_amd import native
    op = native.torch_ops().coarse_select
    N = 100
    en = torch.rand(N, 2, dtype=torch.float64, device="cuda")
    dis1 = torch.ones(N, dtype=torch.float64, device="cuda")
    best = torch.arange(N, dtype=torch.int32, device="cuda")
    op(en, dis1, best)                                          # the good call
    bad = [
        ("energies must be Double", (en.float(), dis1, None)),
        ("dis1 must be Double", (en, dis1.float(), None)),
        ("best must be Int", (en, dis1, best.long())),
        ("energies must have 2 dimensions", (en.reshape(-1), dis1, None)),
        (r"energies must be \[N, 2\]", (torch.rand(N, 3, dtype=torch.float64, device="cuda"), dis1, None)),
        (r"dis1 must be \[N\]", (en, dis1[:-1], None)),
        ("dis1 must have 1 dimensions", (en, dis1.reshape(N, 1), None)),
        (r"best must be \[N\]", (en, dis1, best[:-1])),
        ("energies must be a HIP", (en.cpu(), dis1, None)),
        ("dis1 must be a HIP", (en, dis1.cpu(), None)),
        ("best must be a HIP", (en, dis1, best.cpu())),
        ("energies must be contiguous", (torch.rand(2 * N, 2, dtype=torch.float64, device="cuda")[::2], dis1, None)),
        ("energies must be contiguous", (torch.rand(2, N, dtype=torch.float64, device="cuda").t(), dis1, None)),
        ("dis1 must be contiguous", (en, torch.ones(2 * N, dtype=torch.float64, device="cuda")[::2], None)),
        ("best must be contiguous", (en, dis1, torch.arange(2 * N, dtype=torch.int32, device="cuda")[::2])),
    ]
    for msg, args in bad:
        with pytest.raises(RuntimeError, match=msg):
            op(*args)
    for cap in (0, 65, -1):
        with pytest.raises(RuntimeError, match="cap must lie in 1..64"):
            op(en, dis1, None, 0.008, False, 0.4, cap)


# ------------------------------------------------------------------------------ with the spot network
@pytest.fixture(scope="module")
def spot():
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    return SpotModel(SMALL, make_spot_state_dict(SMALL, 21), batch_size=32).to("cuda")


@pytest.fixture(scope="module")
def scene():
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 7, 24000)
    return sc, torch.from_numpy(sc.mix)


@contextlib.contextmanager
def _counting(model, names):
    """Counts the calls of ``names`` on ``model`` (instance attributes over the bound methods, taken off again)."""
    count = {n: 0 for n in names}

    def wrap(n, fn):
        def inner(*a, **kw):
            count[n] += 1
            return fn(*a, **kw)
        return inner
    for n in names:
        setattr(model, n, wrap(n, getattr(model, n)))
    try:
        yield count
    finally:
        for n in names:
            delattr(model, n)


def _summary(patches, spot_times):
    return (np.array([p[0].center_pos() for p in patches]).reshape(-1, 3), np.array([p[2] for p in patches]),
            [p[3] for p in patches], int(spot_times))


def _forward(spot, sc, mix_t, method, geometry, coarse, **modes):
    from acousticswarms_speech_amd.joint import JointModel
    jm = JointModel(spot, None, device="cuda", geometry=geometry, coarse=coarse, **modes)
    out = io.StringIO()
    with redirect_stdout(out), _counting(spot, ("shift_and_score", "score_offsets", "coarse_select")) as count:
        jm.setup(sc.mic_positions, SMALL_ROI, prone_method=method)
        patches, _al, _a, _d0, _d1, spot_times = jm.forward(mix_t)
    ma = jm.Mic_processor
    return {"summary": _summary(patches, spot_times), "trace": ma.trace, "thr": ma.Relative_Threshold, "nms": ma.lattice_nms,
            "count": dict(count), "stdout": out.getvalue(), "ma": ma, "jm": jm}


_HOST_RUNS = {}                          # (method, geometry) -> the host-mode search, made once


def _host_run(spot, sc, mix_t, method, geometry):
    key = (method, geometry)
    if key not in _HOST_RUNS:
        _HOST_RUNS[key] = _forward(spot, sc, mix_t, method, geometry, "host")
    return _HOST_RUNS[key]


def _same_search(got, want):
    assert got["trace"] == want["trace"] and got["thr"] == want["thr"]
    assert got["summary"][2] == want["summary"][2] and got["summary"][3] == want["summary"][3]
    np.testing.assert_array_equal(got["summary"][0], want["summary"][0])
    np.testing.assert_array_equal(got["summary"][1], want["summary"][1])
    assert got["stdout"] == want["stdout"]


@pytest.mark.parametrize("geometry", ["host", "device"])
@pytest.mark.parametrize("method", ["DENSE", "DENSE_NMS"])
def test_whole_search_device_mode_equals_host_mode(spot, scene, method, geometry):
    from acousticswarms_speech_amd.dense_grid import LatticePatches
    sc, mix_t = scene
    want = _host_run(spot, sc, mix_t, method, geometry)
    got = _forward(spot, sc, mix_t, method, geometry, "device")
    ma = got["ma"]
    assert ma.coarse == "device" and ma.SRP_node.geometry == geometry and ma.SRP_node.lattice.n_cubes == SMALL_ROI_CUBES
    assert got["jm"].previous_config == want["jm"].previous_config + "|coarse=device"
    kept = want["trace"]["coarse_kept"]
    print(f"{method}/{geometry}: {SMALL_ROI_CUBES} cubes, {len(kept)} kept, {want['summary'][3]} spot evaluations, "
          f"{len(want['summary'][2])} talkers")
    assert 1 <= len(kept) <= 30
    _same_search(got, want)
    assert want["count"] == {"shift_and_score": 1, "score_offsets": 0, "coarse_select": 0}
    assert got["count"] == {"shift_and_score": 0, "score_offsets": 1, "coarse_select": 1}
    if method == "DENSE_NMS":
        assert got["nms"]["radius"] == want["nms"]["radius"] == 1
        np.testing.assert_array_equal(got["nms"]["best"], want["nms"]["best"])
        np.testing.assert_array_equal(got["nms"]["degree"], want["nms"]["degree"])
    else:
        assert got["nms"] is None and want["nms"] is None
    # the tables live on the device once, and on a device-built node the cells are the ones its build left there
    node = ma.SRP_node
    tables = node.lattice_tables_device("cuda")
    assert tables is node.lattice_tables_device(spot.device) and tables["offsets"].is_cuda and tables["dis1"].is_cuda
    np.testing.assert_array_equal(tables["offsets"].cpu().numpy(), node.lattice_tables()[0])
    assert tables["dis1"].cpu().numpy().tobytes() == node.lattice_tables()[1].tobytes()
    if geometry == "device":
        assert tables["cells"] is node._geom_dev["cells"]
    # stage 1 of the mode builds nothing, the coarse stage only what it keeps
    with redirect_stdout(io.StringIO()):
        p1, _ = ma.Apply_SRP_PHAT(mix_t)
        assert isinstance(p1, LatticePatches) and p1.built == 0
        kept_patches = ma.Spotform_Big_Patch(mix_t.cuda(), p1, spot)
    assert p1.built == len(kept_patches) == len(kept) and ma.trace["coarse_kept"] == kept


def test_device_mode_composes_with_the_other_device_modes(spot, scene):
    sc, mix_t = scene
    modes = {"segments": "device", "clustering": "device", "global_clustering": "device"}
    want = _forward(spot, sc, mix_t, "DENSE_NMS", "device", "host", **modes)
    got = _forward(spot, sc, mix_t, "DENSE_NMS", "device", "device", **modes)
    _same_search(got, want)
    assert got["jm"].previous_config.endswith("|segments=device|clustering=device|global_clustering=device|coarse=device")
    assert got["count"] == {"shift_and_score": 0, "score_offsets": 1, "coarse_select": 1}


def test_coarse_stage_through_the_batcher(spot, scene):
    """One search through a ``CandidateBatcher``: its lone request is launched as it is, so the energies of the two
    modes are the same numbers and the decisions must be equal.  Device mode sends the host table to ``request``."""
    from acousticswarms_speech_amd import batching
    from acousticswarms_speech_amd.mic_array import MicArray
    sc, mix_t = scene
    stack = torch.stack([mix_t.float(), mix_t.float().flip(1)]).cuda().contiguous()
    torch.cuda.synchronize()
    runs = {}
    for coarse in ("host", "device"):
        with redirect_stdout(io.StringIO()):
            ma = MicArray(np.asarray(sc.mic_positions), Spk_Range=list(SMALL_ROI), Prone_method="DENSE_NMS", device="cuda",
                          geometry="device", coarse=coarse)
            batcher = batching.CandidateBatcher(spot, stack, 1)
            view, scorer = batching.mixture_view(ma), batcher.proxy(1)
            p1, _ = view.Apply_SRP_PHAT(mix_t)
            kept = view.Spotform_Big_Patch(stack[1], p1, scorer)
            batcher.worker_done()
        torch.cuda.synchronize()
        runs[coarse] = (view.trace["coarse_kept"], view.Relative_Threshold, view.lattice_nms, batcher.requests, batcher.sizes,
                        [p.sample_offset.tolist() for p in kept])
        assert ma.lattice_nms is None and ma.trace["coarse_kept"] == []
    h, d = runs["host"], runs["device"]
    assert len(h[0]) >= 1 and d[0] == h[0] and d[1] == h[1] and d[5] == h[5]
    np.testing.assert_array_equal(d[2]["best"], h[2]["best"])
    np.testing.assert_array_equal(d[2]["degree"], h[2]["degree"])
    assert d[3] == h[3] == 1 and d[4] == h[4] == [SMALL_ROI_CUBES]


def _batch_scenes():
    from acousticswarms_speech_amd.scenes import make_scene
    a = make_scene(1010, 5, 7, 24000)
    scenes = [a] + [make_scene(1010 + k, 3, 7, 24000, mic_positions=a.mic_positions) for k in (2, 3, 4)]
    return a, [torch.from_numpy(s.mix) for s in scenes]


def test_batch_of_four_mixtures(spot):
    """Four mixtures recorded with one array, ``concurrent=1``: the per-mixture loop, where device mode equals host mode
    exactly."""
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.shard import localize_batch
    a, mixes = _batch_scenes()
    res = {}
    for coarse in ("host", "device"):
        jm = JointModel(spot, None, device="cuda", geometry="device", coarse=coarse)
        with redirect_stdout(io.StringIO()):
            jm.setup(a.mic_positions, SMALL_ROI, prone_method="DENSE")
            res[coarse] = localize_batch(jm, mixes, concurrent=1)
    assert len(res["device"]) == len(res["host"]) == 4
    for r, w in zip(res["device"], res["host"]):
        assert list(r["names"]) == list(w["names"]) and int(r["spot_times"]) == int(w["spot_times"])
        np.testing.assert_array_equal(r["centres"], w["centres"])
        np.testing.assert_array_equal(r["powers"], w["powers"])
    assert sum(len(w["names"]) for w in res["host"]) >= 1


def test_concurrent_searches_share_the_batcher(spot):
    """Two mixtures, ``concurrent=2``: a candidate's energy moves by about 1e-6 with the internal batch it lands in, so a
    decision between near-equal cubes may differ from the loop's and only the invariants hold: one result per mixture,
    every search decided by one ``coarse_select`` call, at most 30 cubes kept and only those built."""
    from acousticswarms_speech_amd import batching
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.shard import localize_batch
    a, mixes = _batch_scenes()
    mixes = mixes[:2]
    jm = JointModel(spot, None, device="cuda", geometry="device", coarse="device")
    with redirect_stdout(io.StringIO()):
        jm.setup(a.mic_positions, SMALL_ROI, prone_method="DENSE")
    views = []
    view_of = batching.mixture_view

    def spy(m):
        v = view_of(m)
        stage1 = v.Apply_SRP_PHAT

        def apply(mix, v=v, stage1=stage1):                  # keeps the stage-1 list of this view's search
            v.stage1_list = stage1(mix)
            return v.stage1_list
        v.Apply_SRP_PHAT = apply
        views.append(v)
        return v
    batching.mixture_view = spy
    try:
        with redirect_stdout(io.StringIO()), _counting(spot, ("coarse_select",)) as count:
            got = localize_batch(jm, mixes, concurrent=2)
    finally:
        batching.mixture_view = view_of
    assert len(got) == 2 and all(r is not None for r in got) and len(views) == 2 and count["coarse_select"] == 2
    for v in views:
        p1, kept = v.stage1_list[0], v.trace["coarse_kept"]
        assert 1 <= len(kept) <= 30 and len(set(kept)) == len(kept) and p1.built == len(kept)
        assert v.big_spotforming_times == SMALL_ROI_CUBES
