"""GPU: the global clustering's decisions on the device (``asw_global_clusters`` in csrc/cluster_kernels.hip,
``torch.ops.asw.global_clusters``) and the search mode made of it (``MicArray(global_clustering="device")``).

1. the op against its numpy statement (``global_cluster.global_clusters_f64``) at sizes around a wavefront of k-lanes
   and a workgroup of k-threads, with a head list longer than the workgroup, and on the degenerate inputs;
2. two calls are identical, and the result does not depend on what the outputs or the workspace held;
3. the whole search and a batch of four mixtures with ``global_clustering="device"`` against ``"host"``, and what the
   global stage calls in device mode.
The bound is equality everywhere: ``label`` and ``merge`` byte for byte.  Needs an MI355X."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests.global_cluster_cases import hand_case, make_case, statement, unmerged_case

pytestmark = pytest.mark.gpu


def _ops():
    from acousticswarms_speech_amd import native
    return native.torch_ops()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(case, tag="", want=None, seg_dev=None):
    """The op on one case's inputs against the statement: every byte of label and merge, with and without the merge
    output."""
    label_w, merge_w = statement(case) if want is None else want
    n = case["full"].shape[0]
    args = (_dev(case["full"]), _dev(case["seg"]) if seg_dev is None else seg_dev, _dev(case["counts"]), _dev(case["near"]))
    label, merge = _ops().global_clusters(*args, -1.0, -2.0, -7.0, -1.0, -5.0, True)
    assert label.dtype == torch.int32 and merge.dtype == torch.uint8
    assert tuple(label.shape) == (n,) and tuple(merge.shape) == (n, n)
    label, merge = label.cpu().numpy(), merge.cpu().numpy()
    heads = int(np.sum(label == np.arange(n)))
    print(f"{tag} n={n} K={case['seg'].shape[2]}: {heads} heads, {int(np.sum(label >= 0)) - heads} joined, "
          f"{int(np.sum(label == -1))} discarded, {int(np.sum(label == -2))} shadowed, {int(merge.sum())} merge bits")
    assert merge.tobytes() == merge_w.tobytes(), f"{tag}: merge differs in {np.count_nonzero(merge != merge_w)} of {merge.size}"
    np.testing.assert_array_equal(label, label_w)
    label2, merge2 = _ops().global_clusters(*args)                     # the defaults: no merge output
    assert merge2.numel() == 0 and torch.equal(label2.cpu(), torch.from_numpy(label_w))
    return label_w, merge_w


# ---------------------------------------------------------------- the op against the statement
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_sizes_around_the_wavefront_and_the_workgroup(n):
    """K = 1, 47, 63, 64, 65, 257: fewer slots than lanes, one short of a wavefront, one each, one more, and more than
    the 256 threads that stride over k in the walk.  At K = 65 and 257 a second case lets only the window test merge,
    so that many heads stand when the second test runs."""
    for K in (1, 47, 63, 64, 65, 257):
        case = make_case(1000 * n + K, n, K)
        _check(case, tag="uniform")
        if K >= 65 and n > 2:
            case["full"] = unmerged_case(n, K, seed=K)["full"]
            case["near"][:] = 0
            label, _m = _check(case, tag="window only")
            assert np.sum(label == np.arange(n)) >= 3


def test_case_counted_by_hand():
    case, label_w, merge_w = hand_case()
    _check(case, tag="by hand", want=(label_w, merge_w))


def test_more_heads_than_the_workgroup_has_threads():
    """300 rows that neither merge nor shadow each other: 300 heads, scanned in two strides of 256 threads.  Row 300
    is near the LAST head only -- position 299, found in the second stride --; row 301 is near the heads at positions
    260 and 70: the lower position wins although another thread found the higher one first."""
    case = unmerged_case(302, 5, seed=3)
    case["near"][300, 299] = 1
    case["near"][301, 260] = 1
    case["near"][301, 70] = 1
    label, _m = _check(case, tag="300 heads")
    assert np.array_equal(label[:300], np.arange(300)) and label[300] == 299 and label[301] == 70


def test_degenerate_inputs():
    rng = np.random.default_rng(8)
    # every row merges into row 0
    case = make_case(1, 70, 6)
    case["full"][:] = 5.0
    case["counts"][:] = np.maximum(case["counts"], 1)
    label, merge = _check(case, tag="all into 0")
    assert np.all(label == 0) and np.all(merge == 1)
    # all counts zero: everyone is discarded, the merge matrix is full and near alone
    case = make_case(2, 70, 6)
    case["counts"][:] = 0
    label, merge = _check(case, tag="no segments")
    assert np.all(label == -1) and np.array_equal(merge != 0, (case["full"] > -1) | (case["near"] != 0))
    # counts above K and below 0 are clamped: the decisions of K and 0
    case = make_case(3, 70, 6)
    want = statement(case)
    case["counts"] = np.where(case["counts"] == 6, 2 ** 31 - 1, np.where(case["counts"] == 0, -2 ** 31, case["counts"])).astype(np.int32)
    assert case["counts"].max() > 6 and case["counts"].min() < 0
    _check(case, tag="counts out of range", want=want)
    # NaN and +-Inf among the used slots and in full
    case = make_case(4, 70, 9)
    for arr in (case["seg"], case["full"]):
        flat = arr.reshape(-1)
        idx = rng.integers(0, flat.size, size=flat.size // 10)
        flat[idx] = rng.choice([np.nan, np.inf, -np.inf], size=idx.size)
    label, _m = _check(case, tag="NaN and Inf")
    assert len(set(label.tolist())) >= 4


def test_unused_slots_may_hold_anything():
    """The C entry point leaves the slots from a row's count on untouched: here they hold finite values that would
    flip decisions, and then whatever ``torch.rand`` left on the device."""
    want = statement(make_case(5, 65, 9))
    _check(make_case(5, 65, 9, garbage="finite"), tag="finite garbage", want=want)
    case = make_case(6, 65, 9)
    seg_dev = torch.rand((65, 65, 9), dtype=torch.float64, device="cuda") * 14.0 - 12.0
    case["seg"] = seg_dev.cpu().numpy()
    used = np.arange(9)[None, None, :] < case["counts"][:, None, None]
    nan_fill = dict(case, seg=np.where(used, case["seg"], np.nan))
    _check(case, tag="torch.rand", want=statement(nan_fill), seg_dev=seg_dev)


# ---------------------------------------------------------------- what the buffers held
def test_outputs_and_workspace_may_hold_anything_and_two_calls_are_identical():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    case = make_case(7, 130, 11)
    label_w, merge_w = statement(case)
    n, K = 130, 11
    full, seg, cnt, near = _dev(case["full"]), _dev(case["seg"]), _dev(case["counts"]), _dev(case["near"])
    ws_bytes = L.asw_global_clusters_workspace_bytes(n)
    assert ws_bytes == (4 * n + n * n + 7) // 8 * 8
    got = []
    for fill, with_merge in ((0xFF, True), (0x00, True), (0xFF, False), (0xFF, True)):
        label = torch.full((n * 4,), fill, dtype=torch.uint8, device="cuda").view(torch.int32)
        merge = torch.full((n * n,), fill, dtype=torch.uint8, device="cuda")
        ws = torch.full((ws_bytes + 8,), fill, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 8 == 0
        native.check(L.asw_global_clusters(c_void_p(full.data_ptr()), c_void_p(seg.data_ptr()), c_void_p(cnt.data_ptr()),
                                           c_void_p(near.data_ptr()), n, K, -1.0, -2.0, -7.0, -1.0, -5.0,
                                           c_void_p(ws.data_ptr()), ws_bytes, c_void_p(label.data_ptr()),
                                           c_void_p(merge.data_ptr()) if with_merge else None, native.current_stream()))
        torch.cuda.synchronize()
        assert ws[ws_bytes:].cpu().numpy().tolist() == [fill] * 8      # nothing is written past the stated size
        if with_merge:
            got.append((label.cpu().numpy().tobytes(), merge.cpu().numpy().tobytes()))
        else:                                                          # the merge matrix lives in the workspace then
            assert label.cpu().numpy().tobytes() == label_w.tobytes()
            assert ws[4 * n:4 * n + n * n].cpu().numpy().tobytes() == merge_w.tobytes()
    assert got[0] == got[1] == got[2] == (label_w.tobytes(), merge_w.tobytes())


def test_empty_calls_and_adapter_checks():
    ops = _ops()
    f64 = dict(dtype=torch.float64, device="cuda")
    label, merge = ops.global_clusters(torch.zeros((0, 0), **f64), torch.zeros((0, 0, 3), **f64),
                                       torch.zeros(0, dtype=torch.int32, device="cuda"),
                                       torch.zeros((0, 0), dtype=torch.uint8, device="cuda"), -1.0, -2.0, -7.0, -1.0, -5.0, True)
    assert tuple(label.shape) == (0,) and tuple(merge.shape) == (0, 0) and label.is_cuda and label.dtype == torch.int32
    full, seg = torch.zeros((3, 3), **f64), torch.zeros((3, 3, 2), **f64)
    cnt = torch.ones(3, dtype=torch.int32, device="cuda")
    near = torch.zeros((3, 3), dtype=torch.uint8, device="cuda")
    ops.global_clusters(full, seg, cnt, near)
    with pytest.raises(RuntimeError, match="full must be Double"):
        ops.global_clusters(full.float(), seg, cnt, near)
    with pytest.raises(RuntimeError, match="seg must be Double"):
        ops.global_clusters(full, seg.float(), cnt, near)
    with pytest.raises(RuntimeError, match="counts must be Int"):
        ops.global_clusters(full, seg, cnt.long(), near)
    with pytest.raises(RuntimeError, match="near must be Byte"):
        ops.global_clusters(full, seg, cnt, near.bool())
    with pytest.raises(RuntimeError, match=r"full must be \[n, n\]"):
        ops.global_clusters(torch.zeros((3, 4), **f64), seg, cnt, near)
    with pytest.raises(RuntimeError, match="full must have 2 dimensions"):
        ops.global_clusters(full.reshape(-1), seg, cnt, near)
    with pytest.raises(RuntimeError, match=r"seg must be \[n, n, K\]"):
        ops.global_clusters(full, torch.zeros((3, 2, 2), **f64), cnt, near)
    with pytest.raises(RuntimeError, match=r"seg must be \[n, n, K\]"):
        ops.global_clusters(full, torch.zeros((3, 3, 0), **f64), cnt, near)
    with pytest.raises(RuntimeError, match=r"counts must be \[n\]"):
        ops.global_clusters(full, seg, cnt[:2].contiguous(), near)
    with pytest.raises(RuntimeError, match=r"near must be \[n, n\]"):
        ops.global_clusters(full, seg, cnt, near[:2].contiguous())
    with pytest.raises(RuntimeError, match="near must be a HIP"):
        ops.global_clusters(full, seg, cnt, near.cpu())
    with pytest.raises(RuntimeError, match="counts must be a HIP"):
        ops.global_clusters(full, seg, cnt.cpu(), near)
    with pytest.raises(RuntimeError, match="full must be contiguous"):
        ops.global_clusters(torch.zeros((3, 3), **f64).t(), seg, cnt, near)
    with pytest.raises(RuntimeError, match="seg must be contiguous"):
        ops.global_clusters(full, torch.zeros((3, 3, 4), **f64)[:, :, :2], cnt, near)


def test_spot_model_surface_returns_device_tensors():
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.spot import SpotModel
    m = SpotModel(SMALL)                                     # the SI-SDR ops and the clustering need no weights
    rng = np.random.default_rng(12)
    src = rng.standard_normal((2, 9000))
    rows = np.stack([src[k % 2] * (1.0 + 0.1 * k) + 0.3 * rng.standard_normal(9000) for k in range(6)]).astype(np.float32)
    rows[:, 3000:4500] *= 1e-3                               # a pause: more than one segment per row
    rows[5] *= 1e-4                                          # below the quiet bound: no voiced segment, discarded
    waves = torch.from_numpy(rows - rows.mean(axis=1, keepdims=True)).cuda()
    seg_tab, cnt = m.voiced_segments(waves)
    full = m.pair_sisdr_device(waves)
    seg = m.segment_sisdr_resident(waves, seg_tab, cnt)
    near = np.zeros((6, 6), dtype=np.uint8)
    label = m.global_clusters(full, seg, cnt, near)
    assert full.is_cuda and seg.is_cuda and label.is_cuda
    assert tuple(full.shape) == (6, 6) and tuple(seg.shape) == (6, 6, 9) and tuple(label.shape) == (6,)
    assert full.dtype == seg.dtype == torch.float64 and label.dtype == torch.int32
    # the same values as the methods that read back
    assert full.cpu().numpy().tobytes() == m.pair_sisdr(waves).tobytes()
    seg_host, cnt_host = m.segment_sisdr_device(waves, seg_tab, cnt)
    kmax = seg_host.shape[2]
    assert kmax == max(1, int(cnt_host.max())) and int(cnt_host.max()) >= 2
    assert np.array_equal(seg.cpu().numpy()[:, :, :kmax], seg_host, equal_nan=True)
    assert np.all(np.isnan(seg.cpu().numpy()[:, :, kmax:]))
    label_w, _m = statement({"full": full.cpu().numpy(), "seg": seg.cpu().numpy(), "counts": cnt_host, "near": near})
    np.testing.assert_array_equal(label.cpu().numpy(), label_w)
    print(cnt_host.tolist(), label_w.tolist())
    assert label_w.tolist() == [0, 1, 0, 1, 0, -1] and int(cnt_host[5]) == 0      # two sources and their noisy copies


# ---------------------------------------------------------------- the search
@pytest.fixture(scope="module")
def spot():
    from acousticswarms_speech_amd.config import FULL
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    return SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")


def _forward(jm, mix_t):
    with redirect_stdout(io.StringIO()):
        patches, _al, _a, _d0, _d1, spot_times = jm.forward(mix_t)
    tr = jm.Mic_processor.trace
    trace = {"coarse_kept": list(tr["coarse_kept"]), "fine_clusters": {g: dict(c) for g, c in tr["fine_clusters"].items()},
             "final_clusters": [list(c) for c in tr["final_clusters"]]}
    return (np.array([p[0].center_pos() for p in patches]).reshape(-1, 3), np.array([p[2] for p in patches]),
            [p[3] for p in patches], int(spot_times)), trace


def _count_calls(monkeypatch):
    """Calls the scorer receives from inside the global stage."""
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.spot import SpotModel
    names = ("pair_sisdr", "segment_sisdr", "segment_sisdr_device", "voiced_segments", "pair_sisdr_device",
             "segment_sisdr_resident", "global_clusters")
    counts = dict({k: 0 for k in names}, inside=0, heads=0)
    stage = MicArray.Clustering_new

    def global_stage(self, output_pair, *a, **kw):
        counts["inside"] += 1
        counts["heads"] = len(output_pair)
        try:
            return stage(self, output_pair, *a, **kw)
        finally:
            counts["inside"] -= 1
    monkeypatch.setattr(MicArray, "Clustering_new", global_stage)
    for name in names:
        def counted(self, *a, _inner=getattr(SpotModel, name), _name=name, **kw):
            counts[_name] += 1 if counts["inside"] else 0
            return _inner(self, *a, **kw)
        monkeypatch.setattr(SpotModel, name, counted)
    return counts, names


@pytest.mark.parametrize("clustering", ["host", "device"])
def test_whole_search_with_device_global_clustering_equals_host(spot, monkeypatch, clustering):
    """The configs[2] scene (seed 1010, 5 talkers, 7 mics, 48 000 samples, reverberant), both modes with
    ``segments="device"``.  The decisions are the same comparisons of the same float64 values: trace, talkers, positions,
    powers and spot_times are equal outright.  In device mode the global stage reads nothing back through
    ``pair_sisdr`` / ``segment_sisdr`` / ``segment_sisdr_device`` and makes exactly one ``global_clusters`` call."""
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    counts, names = _count_calls(monkeypatch)
    sc = make_scene(1010, 5, 7, 48000, reverb=True)
    mix_t = torch.from_numpy(sc.mix)
    jm = JointModel(spot, None, device="cuda", segments="device", clustering=clustering)
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, sc.speaker_range)
    assert jm.Mic_processor.global_clustering == "host"
    want, trace_want = _forward(jm, mix_t)
    assert counts["global_clusters"] == counts["pair_sisdr_device"] == counts["segment_sisdr_resident"] == 0
    assert counts["pair_sisdr"] == counts["segment_sisdr_device"] == counts["voiced_segments"] == 1
    n_heads = counts["heads"]
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, sc.speaker_range, global_clustering="device")
    mp = jm.Mic_processor
    assert mp.global_clustering == "device" and mp.segments == "device" and mp.clustering == clustering
    for k in names:
        counts[k] = 0
    got, trace_got = _forward(jm, mix_t)
    print(f"{n_heads} cluster heads into the global stage, {len(want[2])} talkers in "
          f"{sum(len(c) for c in trace_want['final_clusters'])} clustered heads")
    assert {k: counts[k] for k in names} == {"pair_sisdr": 0, "segment_sisdr": 0, "segment_sisdr_device": 0, "voiced_segments": 1,
                                             "pair_sisdr_device": 1, "segment_sisdr_resident": 1, "global_clusters": 1}
    assert counts["heads"] == n_heads >= 10 and len(want[2]) >= 1
    assert trace_got == trace_want
    assert got[2] == want[2] and got[3] == want[3]
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_batch_of_four_mixtures_with_device_global_clustering(spot):
    """``localize_batch`` with global_clustering="device" against the same batch with "host", both with
    ``segments="device"``.  The plain loop (``concurrent=1``) runs the same arithmetic in both and must be equal; with
    ``concurrent=2`` a candidate's energy moves by about 1e-6 with the internal batch it lands in, the bar of
    test_config3_mixture_batch_equals_plain_loop."""
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.shard import localize_batch
    first = make_scene(2000, 5, 7, 24000)
    scenes = [make_scene(2000 + k, 5, 7, 24000, mic_positions=first.mic_positions) for k in range(4)]
    mixes = [torch.from_numpy(s.mix) for s in scenes]
    jh = JointModel(spot, None, device="cuda", segments="device")
    jd = JointModel(spot, None, device="cuda", segments="device", global_clustering="device")
    with redirect_stdout(io.StringIO()):
        jh.setup(first.mic_positions, first.speaker_range)
        want = localize_batch(jh, mixes, concurrent=1)
        jd.setup(first.mic_positions, first.speaker_range)
        plain = localize_batch(jd, mixes, concurrent=1)
        batched = localize_batch(jd, mixes, concurrent=2)
    assert jd.Mic_processor.global_clustering == "device" and len(want) == len(plain) == len(batched) == 4
    for k in range(4):
        r, w = plain[k], want[k]
        assert list(r["names"]) == list(w["names"]) and int(r["spot_times"]) == int(w["spot_times"]) and len(w["names"]) >= 1
        np.testing.assert_array_equal(r["centres"], w["centres"])
        np.testing.assert_array_equal(r["powers"], w["powers"])
        r = batched[k]
        assert list(r["names"]) == list(w["names"]) and int(r["spot_times"]) == int(w["spot_times"])
        np.testing.assert_allclose(r["centres"], w["centres"], atol=1e-6)
        np.testing.assert_allclose(r["powers"], w["powers"], rtol=1e-5)
