"""CPU only: the statement of the global clustering's decisions (``global_cluster.global_clusters_f64``), which
``asw_global_clusters`` reproduces on the GPU (tests/test_gpu_global_clusters.py).

The statement is checked on a case counted by hand and against the shipped ``MicArray.Clustering_new``
(``segments="device"``, a stand-in scorer that serves generated tensors) on 200 generated cases; then the same cases
through ``global_clustering="device"`` with a stand-in ``global_clusters`` that evaluates the statement, the keyword
through every layer, and the C entry points' refusals through ctypes.  Every bound is equality."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from acousticswarms_speech_amd.global_cluster import MAX_ROWS, clusters_of_labels, global_clusters_f64
from tests.global_cluster_cases import hand_case, make_case, near_of, statement, unmerged_case


# ---------------------------------------------------------------- counted by hand
def test_case_counted_by_hand():
    case, label_w, merge_w = hand_case()
    label, merge = statement(case)
    assert label.dtype == np.int32 and merge.dtype == np.uint8 and merge.shape == (11, 11)
    np.testing.assert_array_equal(label, label_w)
    np.testing.assert_array_equal(merge, merge_w)
    assert clusters_of_labels(label) == {0: [0, 7], 2: [2, 5, 8], 3: [3, 6], 9: [9, 10]}
    assert list(clusters_of_labels(label)) == [0, 2, 3, 9]
    # the thresholds are parameters: with a window that nothing passes and a similarity nothing reaches, only the
    # distance merges, and with the second test out of reach too nobody is shadowed
    label2, merge2 = statement(case, sim_db=50.0, win_hi=50.0, best_hi=50.0)
    assert label2.tolist() == [0, -1, 2, 3, 4, 3, 3, 7, 8, 9, 10] and int(merge2.sum()) == 2


def test_unused_slots_are_never_read():
    """The slots from a row's count on may hold anything: NaN (what the torch adapter fills), finite values that would
    flip decisions, or Inf -- the decisions are the same."""
    for seed in range(6):
        a = make_case(seed, 30, 9)
        b = make_case(seed, 30, 9, garbage="finite")
        assert np.array_equal(a["counts"], b["counts"]) and not np.array_equal(np.nan_to_num(a["seg"]), np.nan_to_num(b["seg"]))
        la, ma = statement(a)
        lb, mb = statement(b)
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ma, mb)
    # counts outside 0..K are clamped
    c = make_case(3, 12, 4)
    lw, mw = statement(c)
    c2 = dict(c, counts=np.where(c["counts"] == 4, 1000, np.where(c["counts"] == 0, -7, c["counts"])).astype(np.int32))
    l2, m2 = statement(c2)
    np.testing.assert_array_equal(lw, l2)
    np.testing.assert_array_equal(mw, m2)


def test_shapes_are_checked():
    c = make_case(0, 5, 3)
    with pytest.raises(ValueError, match=r"full must be \[n, n\]"):
        global_clusters_f64(c["full"][:4], c["seg"], c["counts"], c["near"])
    with pytest.raises(ValueError, match="seg must be"):
        global_clusters_f64(c["full"], c["seg"][:, :4], c["counts"], c["near"])
    with pytest.raises(ValueError, match="seg must be"):
        global_clusters_f64(c["full"], c["seg"][:, :, :0], c["counts"], c["near"])
    with pytest.raises(ValueError, match="counts must be"):
        global_clusters_f64(c["full"], c["seg"], c["counts"][:4], c["near"])
    label, merge = global_clusters_f64(np.zeros((0, 0)), np.zeros((0, 0, 2)), np.zeros(0, np.int32), np.zeros((0, 0), np.uint8))
    assert label.shape == (0,) and merge.shape == (0, 0) and clusters_of_labels(label) == {}
    assert MAX_ROWS == 8192


# ---------------------------------------------------------------- against Clustering_new
class _Patch(object):
    def __init__(self, c):
        self.c = None if c is None else np.asarray(c, dtype=np.float64)

    def center_pos(self):
        return self.c


class _Scorer(object):
    """The device surface ``Clustering_new`` uses with ``segments="device"``, on CPU tensors: it serves the tensors of
    one generated case, as the HIP model would have computed them from the waveforms.  ``segment_sisdr_device`` returns
    what the shipped method returns: the tensor cut to the largest count, NaN beyond a row's count.  ``calls`` counts."""
    device = "cpu"

    def __init__(self, case, with_global):
        self.case = case
        self.calls = {k: 0 for k in ("voiced_segments", "pair_sisdr", "segment_sisdr", "segment_sisdr_device",
                                     "pair_sisdr_device", "segment_sisdr_resident", "global_clusters")}
        if not with_global:
            self.global_clusters = None                      # hasattr stays true, but host mode must never call it

    def voiced_segments(self, waves):
        import torch
        self.calls["voiced_segments"] += 1
        n, K = self.case["seg"].shape[0], self.case["seg"].shape[2]
        assert waves.shape[0] == n
        tab = np.zeros((n, K, 2), dtype=np.int32)
        tab[:, :, 1] = 1000 * (np.arange(K)[None, :] < self.case["counts"][:, None])
        return torch.from_numpy(tab), torch.from_numpy(self.case["counts"].copy())

    def pair_sisdr(self, waves):
        self.calls["pair_sisdr"] += 1
        return self.case["full"].copy()

    def segment_sisdr(self, waves, segments):
        raise AssertionError('segments="device" never passes host segment lists')

    def segment_sisdr_device(self, waves, seg_dev, cnt_dev):
        self.calls["segment_sisdr_device"] += 1
        cnt = cnt_dev.numpy()
        kmax = max(1, int(cnt.max()) if cnt.size else 1)
        used = np.arange(kmax)[None, None, :] < cnt[:, None, None]
        return np.where(used, self.case["seg"][:, :, :kmax], np.nan), cnt

    def pair_sisdr_device(self, waves):
        import torch
        self.calls["pair_sisdr_device"] += 1
        return torch.from_numpy(self.case["full"].copy())

    def segment_sisdr_resident(self, waves, seg_dev, cnt_dev):
        import torch
        self.calls["segment_sisdr_resident"] += 1
        assert seg_dev.shape[1] == self.case["seg"].shape[2]               # sized by the table's own width
        return torch.from_numpy(self.case["seg"].copy())

    def global_clusters(self, full_dev, seg_dev, cnt_dev, near):
        import torch
        self.calls["global_clusters"] += 1
        assert isinstance(near, np.ndarray) and near.dtype == np.uint8
        label, _merge = global_clusters_f64(full_dev.numpy(), seg_dev.numpy(), cnt_dev.numpy(), near)
        return torch.from_numpy(label)


def _array(mode, scorer):
    from acousticswarms_speech_amd.mic_array import MicArray

    class Array(MicArray):
        def __init__(self):                                  # no geometry tables: the clustering needs none
            self.segments, self.clustering, self.global_clustering = "device", "host", mode
            self._device_scorer = scorer
            self._seg_cache, self._dev_cache = {}, {}
            self.trace = {"coarse_kept": [], "fine_clusters": {}, "final_clusters": []}
            self.big_spotforming_times, self.spotforming_times = 3, 40
    return Array()


def _candidates(case, rng, centres=None):
    """The output tuples of the fine stage for one case, already by descending power, with ground-truth labels on a
    third of them so that the ``wrong`` list is formed; handed over in a shuffled order."""
    n = case["full"].shape[0]
    centres = case["centres"] if centres is None else centres
    cands = []
    for i in range(n):
        big_label = int(rng.integers(-1, 2)) if rng.random() < 0.6 else -1
        cands.append((_Patch(centres[i]), np.full(8, float(i), dtype=np.float32), 100.0 - i, f"g{i}_{i % 3}",
                      {"audio_offset": rng.integers(-20, 20, 6), "localization_offset": None}, big_label))
    order = rng.permutation(n)
    return cands, [cands[k] for k in order]


def _run(mode, case, cands_shuffled, sample_gt, with_global=None):
    scorer = _Scorer(case, mode == "device" if with_global is None else with_global)
    ma = _array(mode, scorer)
    out = io.StringIO()
    with redirect_stdout(out):
        audio, patches, times, wrong = ma.Clustering_new(cands_shuffled, sample_gt=sample_gt)
    return audio, patches, times, wrong, ma.trace["final_clusters"], out.getvalue(), scorer.calls


def _generated(k):
    rng = np.random.default_rng(9000 + k)
    n = 1 + k % 40
    K = int(rng.integers(1, 13))
    case = make_case(500 + k, n, K, area=6.0 if k % 4 else 2.0)
    if k % 5 == 4:                                           # NaN and Inf among the used slots and in full
        for arr in (case["seg"], case["full"]):
            flat = arr.reshape(-1)
            idx = rng.integers(0, flat.size, size=max(1, flat.size // 15))
            flat[idx] = rng.choice([np.nan, np.inf, -np.inf], size=idx.size)
    if k % 7 == 6:                                           # only the window merges: more heads for the second test
        case["full"] = unmerged_case(n, K, seed=k)["full"]
        case["centres"] = case["centres"] * np.array([50.0, 50.0, 1.0])
        case["near"] = near_of(case["centres"])
    return case, rng


def _same_wrong(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and x[3] == y[3]


def test_statement_equals_clustering_new_on_generated_cases():
    """200 cases, n = 1 .. 40: the clusters the shipped host walk builds from the read-back tensors are those rebuilt
    from the statement's labels -- trace, returned patches, and the number of discards it prints."""
    seen = {"discarded": 0, "shadowed": 0, "joined": 0, "heads": 0, "wrong": 0}
    for k in range(200):
        case, rng = _generated(k)
        cands, shuffled = _candidates(case, rng)
        sample_gt = rng.integers(-20, 20, (6, 2))
        _audio, patches, times, wrong, trace, text, calls = _run("host", case, shuffled, sample_gt)
        n = len(cands)
        assert calls["global_clusters"] == 0 and calls["voiced_segments"] == 1
        assert calls["pair_sisdr"] == calls["segment_sisdr_device"] == (1 if n > 1 else 0)
        near = _array("host", None)._near_matrix([c[0].center_pos() for c in cands]).astype(np.uint8)
        np.testing.assert_array_equal(near, case["near"])
        label, _merge = global_clusters_f64(case["full"], case["seg"], case["counts"], near)
        clusters = clusters_of_labels(label)
        assert trace == [[cands[i][3] for i in clusters[h]] for h in clusters], k
        assert len(patches) == len(clusters) and all(p is cands[h] for p, h in zip(patches, clusters)), k
        assert text.count("discard because no invalid split!!!") == int(np.sum(label == -1))
        assert text.rstrip().endswith(f"final speaker number is  {len(clusters)}") and times == 43
        seen["discarded"] += int(np.sum(label == -1))
        seen["shadowed"] += int(np.sum(label == -2))
        seen["joined"] += int(np.sum((label >= 0) & (label != np.arange(n))))
        seen["heads"] += len(clusters)
        seen["wrong"] += len(wrong)
    print(seen)
    assert min(seen.values()) >= 50                          # every outcome was compared many times


def test_device_mode_equals_host_mode_on_the_same_cases():
    """The same 200 cases through ``global_clustering="device"`` with a stand-in ``global_clusters`` that evaluates the
    statement: everything ``Clustering_new`` returns, records and prints equals host mode's, from one ``global_clusters``
    call and none of the reading methods."""
    for k in range(200):
        case, rng = _generated(k)
        cands, shuffled = _candidates(case, rng)
        sample_gt = rng.integers(-20, 20, (6, 2)) if k % 3 else None
        host = _run("host", case, shuffled, sample_gt)
        dev = _run("device", case, shuffled, sample_gt)
        assert dev[6] == {"voiced_segments": 1, "pair_sisdr": 0, "segment_sisdr": 0, "segment_sisdr_device": 0,
                          "pair_sisdr_device": 1, "segment_sisdr_resident": 1, "global_clusters": 1}, k
        assert len(dev[0]) == len(host[0]) and all(a is b for a, b in zip(dev[0], host[0]))
        assert len(dev[1]) == len(host[1]) and all(a is b for a, b in zip(dev[1], host[1]))
        assert dev[2] == host[2] and dev[4] == host[4] and dev[5] == host[5], k
        _same_wrong(dev[3], host[3])


def test_device_mode_without_candidates_or_without_a_centre():
    """No candidate: nothing is enqueued.  A candidate whose patch has no centre: the per-pair host loop, as in host
    mode (it compares waveforms on the host, so the case is tiny and its audio real)."""
    case = make_case(1, 3, 2)
    empty = _run("device", case, [], None)
    assert empty[0] == [] and empty[1] == [] and empty[4] == [] and sum(empty[6].values()) == 0
    res = {}
    for mode in ("host", "device"):
        rng = np.random.default_rng(4)
        cands = [(_Patch(None if i == 1 else [float(i), 0.0, 0.0]), rng.standard_normal(4000).astype(np.float32), 9.0 - i,
                  f"g{i}", {"audio_offset": np.zeros(6)}, -1) for i in range(3)]
        res[mode] = _run(mode, case, cands, None)
    assert res["device"][6]["global_clusters"] == 0 and res["device"][6] == res["host"][6]
    assert res["device"][4] == res["host"][4] and res["device"][5] == res["host"][5]


# ---------------------------------------------------------------- the keyword
def test_global_clustering_keyword_and_config_key():
    from acousticswarms_speech_amd import batching
    from acousticswarms_speech_amd.joint import JointModel, config_key
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 7, 4000)
    roi = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
    assert config_key(sc.mic_positions, roi) == config_key(sc.mic_positions, roi, global_clustering="host")
    assert config_key(sc.mic_positions, roi, segments="device", global_clustering="device") \
        == config_key(sc.mic_positions, roi) + "|segments=device|global_clustering=device"
    assert config_key(sc.mic_positions, roi, segments="device", clustering="device", global_clustering="device") \
        .endswith("|segments=device|clustering=device|global_clustering=device")
    with pytest.raises(ValueError, match="global_clustering"):
        JointModel(None, segments="device", global_clustering="gpu")
    with pytest.raises(ValueError, match='needs segments="device"'):
        JointModel(None, global_clustering="device")
    with redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="global_clustering"):
            MicArray(sc.mic_positions, Spk_Range=roi, segments="device", global_clustering="gpu")
        with pytest.raises(ValueError, match='needs segments="device"'):
            MicArray(sc.mic_positions, Spk_Range=roi, global_clustering="device")
        assert MicArray(sc.mic_positions, Spk_Range=roi).global_clustering == "host"
        jm = JointModel(None, segments="device", global_clustering="device")
        jm.setup(sc.mic_positions, roi)
        mp = jm.Mic_processor
        assert mp.global_clustering == "device" and mp.segments == "device" and mp.clustering == "host"
        assert jm.previous_config.endswith("|segments=device|global_clustering=device")
        assert batching.mixture_view(mp).global_clustering == "device"
        assert jm.mic_array_for(sc.mic_positions, roi).global_clustering == "device"
        jm.use_geometry(sc.mic_positions, roi)
        assert jm.Mic_processor.global_clustering == "device" and jm.previous_config.endswith("|global_clustering=device")
        jm.setup(sc.mic_positions, roi, global_clustering="host")
        assert jm.Mic_processor.global_clustering == "host" and "global_clustering" not in jm.previous_config
        with pytest.raises(ValueError, match='needs segments="device"'):
            jm.setup(sc.mic_positions, roi, segments="host", global_clustering="device")
        plain = JointModel(None)
        plain.setup(sc.mic_positions, roi)
        assert plain.global_clustering == "host" and plain.Mic_processor.global_clustering == "host"


def test_device_mode_needs_a_scorer_that_clusters():
    """A scorer without ``global_clusters`` cannot serve global_clustering="device": RuntimeError, no quiet fall-back to
    the host walk; one without ``voiced_segments`` fails as ``segments="device"`` does."""
    case = make_case(2, 4, 3)
    cands, shuffled = _candidates(case, np.random.default_rng(0))

    class NoGlobal(object):
        device = "cpu"

        def voiced_segments(self, waves):
            raise AssertionError("not reached")
    ma = _array("device", NoGlobal())
    with pytest.raises(RuntimeError, match="global_clusters"):
        ma.Clustering_new(shuffled)
    ma = _array("device", None)
    with pytest.raises(RuntimeError, match="voiced_segments"):
        ma.Clustering_new(shuffled)


def test_scorer_pass_through():
    from acousticswarms_speech_amd.batching import MixtureScorer

    class Model:
        device, batch_size = None, 4

        def pair_sisdr_device(self, *a):
            return ("pair",) + a

        def segment_sisdr_resident(self, *a):
            return ("seg",) + a

        def global_clusters(self, *a):
            return ("glob",) + a

    class Batcher:
        model = Model()
    s = MixtureScorer(Batcher(), 0)
    assert s.pair_sisdr_device("w") == ("pair", "w")
    assert s.segment_sisdr_resident("w", "t", "c") == ("seg", "w", "t", "c")
    assert s.global_clusters("f", "s", "c", "n") == ("glob", "f", "s", "c", "n")


# ---------------------------------------------------------------- the C entry points
def test_entry_points_reject_bad_arguments_without_a_gpu():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    buf = np.zeros(1 << 12)
    p = c_void_p(buf.ctypes.data)
    assert L.asw_global_clusters_workspace_bytes(0) == 0
    assert L.asw_global_clusters_workspace_bytes(1) == 8                       # 4 + 1, rounded up
    assert L.asw_global_clusters_workspace_bytes(10) == 144                    # 40 + 100, rounded up
    assert L.asw_global_clusters_workspace_bytes(8192) == 4 * 8192 + 8192 * 8192
    assert L.asw_global_clusters_workspace_bytes(-1) == 0 and b"n = -1" in L.asw_last_error()
    assert L.asw_global_clusters_workspace_bytes(8193) == 0 and b"n = 8193" in L.asw_last_error()

    def call(full=p, seg=p, counts=p, near=p, n=10, K=3, ws=p, ws_bytes=144, label=p, merge=None):
        return L.asw_global_clusters(full, seg, counts, near, n, K, -1.0, -2.0, -7.0, -1.0, -5.0, ws, ws_bytes, label, merge,
                                     None)
    for name in ("full", "seg", "counts", "near", "ws"):
        assert call(**{name: None}) == -1 and b"global_clusters: null pointer" in L.asw_last_error(), name
    assert call(label=None) == -1 and b"null output" in L.asw_last_error()
    assert call(n=-1) == -1 and b"n = -1" in L.asw_last_error()
    assert call(n=8193, ws_bytes=1 << 40) == -1 and b"n = 8193" in L.asw_last_error()
    assert call(K=0) == -1 and call(K=-3) == -1 and b"K = -3" in L.asw_last_error()
    assert call(ws_bytes=143) == -1 and b"too small, 144 needed" in L.asw_last_error()
    assert call(ws=c_void_p(buf.ctypes.data + 4), ws_bytes=1 << 10) == -1 and b"aligned" in L.asw_last_error()
    # nothing to do: no launch, whatever the pointers are -- but K is still checked
    assert call(n=0, full=None, seg=None, counts=None, near=None, ws=None, ws_bytes=0, label=None) == 0
    assert call(n=0, K=0) == -1
