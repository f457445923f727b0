"""CPU only: the float64 statement of the fine stage's per-coarse-patch clustering (``fine_cluster.fine_clusters_f64``),
which ``asw_fine_clusters`` reproduces bit for bit on the GPU (tests/test_gpu_fine_clusters.py).

The statement is checked on a case counted by hand, on the order of its sums, and against ``MicArray._cluster_group``
driven with the float32 ``hostdsp.si_sdr`` on 120 generated groups; then the ``clustering=`` keyword of the search, the
device-mode bookkeeping with a stand-in scorer, and the C entry points' refusals through ctypes."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from acousticswarms_speech_amd.fine_cluster import (GRAM_MAX_ELEMS, clusters_of_group, fine_cluster_margin_db,
                                                    fine_clusters_f64)
from acousticswarms_speech_amd.hostdsp import si_sdr
from tests.fine_cluster_cases import energies_of, gram_entry, hand_case, make_call, make_group, statement

MARGIN_DB = 1e-3          # float32 si_sdr and the float64 statement part by 3e-6 dB at most: three hundred times that
MAX_LEFT_OUT = 0.05


# ---------------------------------------------------------------- counted by hand
def test_case_counted_by_hand():
    call, order_w, label_w, gram_w = hand_case()
    order, label, gram = statement(call)
    assert order.dtype == label.dtype == np.int32 and gram.dtype == np.float64
    np.testing.assert_array_equal(order, order_w)           # closed group ordered too; equal powers by ascending index
    np.testing.assert_array_equal(label, label_w)           # closed, all-ineligible, alone, second head only
    assert gram.tobytes() == gram_w.tobytes() and gram.shape == (4 + 4 + 1 + 16,)
    assert clusters_of_group(order, label, 5, 4) == {0: [0, 3], 1: [1, 2]}
    assert clusters_of_group(order, label, 0, 2) == {} and clusters_of_group(order, label, 4, 1) == {0: [0]}
    # the threshold is a parameter: at +20 dB nothing but a copy is the same talker
    _o, label20, _g = statement(call, sim_db=20.0)
    assert label20[5:].tolist() == [5, 6, 7, 8]


def test_margin_is_the_distance_of_the_closest_comparison():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(2000).astype(np.float32)
    b = (0.5 * a + 0.7 * rng.standard_normal(2000)).astype(np.float32)
    call = make_call(0, None, 2000, groups=[np.stack([a, b])])
    call["gate"][:] = 0.0
    call["min_trigger"] = 0.0
    k, h = (1, 0) if call["energies"][0, 0] >= call["energies"][1, 0] else (0, 1)
    w = call["waves"].astype(np.float64)
    want = abs(float(si_sdr(w[k], w[h])) + 4.0)
    got = fine_cluster_margin_db(call["waves"], call["bounds"], call["energies"], call["gate"], call["group_gate"], 0.0)
    assert got == pytest.approx(want, abs=1e-9) and got > MARGIN_DB
    one = make_call(0, None, 2000, groups=[a[None]])
    assert fine_cluster_margin_db(one["waves"], one["bounds"], one["energies"], one["gate"], one["group_gate"], 0.0) == np.inf


def test_the_order_of_the_sums_is_the_statement():
    """The Gram entries are not merely close to the inner products: they are the stated order's values, which differ
    from ``np.dot`` in the last bits, and do not depend on the size of the group or on the partner rows."""
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((3, 1000)).astype(np.float32)
    call = make_call(0, None, 1000, groups=[rows[:2], rows])
    _o, _l, gram = statement(call)
    g2, g3 = gram[:4].reshape(2, 2), gram[4:].reshape(3, 3)
    want = np.array([[gram_entry(rows[a], rows[b]) for b in range(3)] for a in range(3)])
    assert g3.tobytes() == want.tobytes() and g2.tobytes() == want[:2, :2].copy().tobytes()
    assert np.array_equal(g3, g3.T)
    dots = rows.astype(np.float64) @ rows.astype(np.float64).T
    np.testing.assert_allclose(g3, dots, rtol=1e-12, atol=1e-12)
    assert np.any(g3 != dots)
    # T below 256 and no multiple of it: the partials that get no sample stay 0.0
    short = rng.standard_normal((2, 77)).astype(np.float32)
    _o, _l, g = statement(make_call(0, None, 77, groups=[short]))
    assert g[1] == gram_entry(short[0], short[1]) and g[0] == gram_entry(short[0], short[0])


def test_bounds_are_checked():
    call = make_call(1, [2, 3], 64)
    for bad in ([1, 2, 5], [0, 3, 2, 5], [0, 2, 4]):
        with pytest.raises(ValueError, match="bounds"):
            fine_clusters_f64(call["waves"], np.array(bad), call["energies"], call["gate"], call["group_gate"][:len(bad) - 1], 0.0)
    with pytest.raises(ValueError, match="fit"):
        fine_clusters_f64(call["waves"], call["bounds"], call["energies"][:4], call["gate"], call["group_gate"], 0.0)
    assert GRAM_MAX_ELEMS == 1 << 27


# ---------------------------------------------------------------- against _cluster_group
class _Patch(object):
    def __init__(self, c):
        self.c = np.asarray(c, dtype=np.float64)
        self.sample_offset = np.zeros(6)

    def center_pos(self):
        return self.c


def _host_clusters(ma, g, big, patches, waves, en, thr_new, T_len):
    """``_cluster_group`` as the fine stage drives it on the host, with the float32 ``si_sdr``; -> its clusters dict, or
    None for a closed group.  The output tuples (geometry of real patches) are not formed: the shared tail records
    the trace entry and returns."""
    ma.trace = {"fine_clusters": {}}
    ma._cluster_group(g, big, patches, list(en[:, 0]), list(en[:, 1]), None, None, T_len, thr_new, None,
                      lambda k, h: si_sdr(waves[k], waves[h]), lambda heads: [waves[h] for h in heads])
    return ma.trace["fine_clusters"].get(g)


@pytest.fixture(scope="module")
def stub_array():
    from acousticswarms_speech_amd.mic_array import MicArray

    class Array(MicArray):
        def __init__(self):                                  # no geometry tables: the clustering needs none
            self.MIN_TRIGGER_POWER = 0.5
            self.mic_positions = np.zeros((7, 3))
            self.segments = self.clustering = "host"
            self.trace = {"fine_clusters": {}}

        def _cluster_outputs(self, g, patches, powers, clusters, area, centre, big_label, audio_of):
            self.trace["fine_clusters"][int(g)] = {int(h): [int(k) for k in m] for h, m in clusters.items()}
            return []
    return Array()


def test_statement_equals_cluster_group_on_generated_groups(stub_array):
    """120 groups of 2-39 rows at T = 12 000 with the thresholds of the search formed from stand-in patch positions:
    the statement's clusters are those of ``_cluster_group`` wherever no comparison lies within MARGIN_DB of -4 dB."""
    ma, T = stub_array, 12000
    rng = np.random.default_rng(2024)
    left_out, n_clusters, joined, closed = 0, [], 0, 0
    for g in range(120):
        n = int(rng.integers(2, 40))
        waves = make_group(rng, n, T)
        en = energies_of(waves)
        patches = [_Patch(rng.uniform(-1.5, 1.5, 3)) for _ in range(n)]
        big = _Patch(rng.uniform(-1.5, 1.5, 3))
        # a threshold among the gated levels, so that both outcomes of the gates occur
        dist = np.array([np.linalg.norm(p.center_pos()) for p in patches])
        thr_new = float(np.quantile(en[:, 1] * (1 + dist), rng.uniform(0.0, 0.5)))
        if g % 10 == 9:
            thr_new = float(np.max(en[:, 1])) * (1 + np.linalg.norm(big.center_pos())) * 1.01      # closes the group
        gate = np.array([thr_new / (1 + np.linalg.norm(p.center_pos() - ma.mic_positions[0])) for p in patches])
        group_gate = np.array([ma._group_gate(big, thr_new)])
        min_trigger = ma.MIN_TRIGGER_POWER / (3 * 48000) * T
        bounds = np.array([0, n], dtype=np.int32)
        args = (waves, bounds, en, gate, group_gate, min_trigger)
        if fine_cluster_margin_db(*args) < MARGIN_DB:
            left_out += 1
            continue
        order, label, _gram = fine_clusters_f64(*args)
        want = _host_clusters(ma, g, big, patches, waves, en, thr_new, T)
        if want is None:
            closed += 1
            assert np.all(label == -1) and sorted(order.tolist()) == list(range(n))
            continue
        got = clusters_of_group(order, label, 0, n)
        assert got == want and list(got) == list(want), g            # heads in creation order, members in visiting order
        n_clusters.append(len(got))
        joined += sum(len(m) - 1 for m in got.values())
    print(f"{left_out} of 120 within {MARGIN_DB} dB; {closed} closed; clusters per group {min(n_clusters)}..{max(n_clusters)}; "
          f"{joined} joins")
    assert left_out <= MAX_LEFT_OUT * 120
    assert closed >= 10 and max(n_clusters) >= 10 and joined >= 100           # every branch was compared


# ---------------------------------------------------------------- the keyword
def test_clustering_keyword_and_config_key():
    from acousticswarms_speech_amd import batching
    from acousticswarms_speech_amd.joint import JointModel, config_key
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 7, 4000)
    roi = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
    assert config_key(sc.mic_positions, roi) == config_key(sc.mic_positions, roi, clustering="host")
    assert config_key(sc.mic_positions, roi, clustering="device") == config_key(sc.mic_positions, roi) + "|clustering=device"
    assert config_key(sc.mic_positions, roi, segments="device", clustering="device").endswith("|segments=device|clustering=device")
    with pytest.raises(ValueError, match="clustering"):
        JointModel(None, clustering="gpu")
    with redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="clustering"):
            MicArray(sc.mic_positions, Spk_Range=roi, clustering="gpu")
        assert MicArray(sc.mic_positions, Spk_Range=roi).clustering == "host"
        jm = JointModel(None, clustering="device")
        jm.setup(sc.mic_positions, roi)
        assert jm.Mic_processor.clustering == "device" and jm.previous_config.endswith("|clustering=device")
        assert jm.Mic_processor.segments == "host"
        assert batching.mixture_view(jm.Mic_processor).clustering == "device"
        assert jm.mic_array_for(sc.mic_positions, roi).clustering == "device"
        jm.setup(sc.mic_positions, roi, clustering="host")
        assert jm.Mic_processor.clustering == "host" and "clustering" not in jm.previous_config


def test_device_clustering_needs_a_scorer_that_clusters():
    """A duck-typed model without ``fine_clusters`` cannot serve clustering="device": RuntimeError, no quiet fall-back
    to the host path."""
    import torch
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    from tests.golden.surrogate import SurrogateSpot
    sc = make_scene(1010, 5, 7, 4000)
    with redirect_stdout(io.StringIO()):
        ma = MicArray(sc.mic_positions, Spk_Range=[-0.5, 0.5, 1.0, 2.0, 0.1, 0.5], clustering="device")
        ma.Relative_Threshold = 1.0
        with pytest.raises(RuntimeError, match="fine_clusters"):
            ma.Spotform_Small_Patch_Parallel(torch.from_numpy(sc.mix), [], SurrogateSpot())

        class Resident(SurrogateSpot):                      # resident, but still without the method
            def shift_and_sep_resident(self, *a, **kw):
                raise AssertionError("not reached")
        with pytest.raises(RuntimeError, match="fine_clusters"):
            ma.Spotform_Small_Patch_Parallel(torch.from_numpy(sc.mix), [], Resident())


def test_scorer_pass_through():
    from acousticswarms_speech_amd.batching import MixtureScorer

    class Model:
        device, batch_size = None, 4

        def fine_clusters(self, *a):
            return a

    class Batcher:
        model = Model()
    s = MixtureScorer(Batcher(), 0)
    assert s.fine_clusters("w", "b", "e", "g", "gg", 0.25) == ("w", "b", "e", "g", "gg", 0.25)


# ---------------------------------------------------------------- the fine stage, with a stand-in scorer
class _CpuSpot(object):
    """The resident surface the fine stage uses, on CPU tensors: fixed waveforms per candidate (keyed by the patch's
    tag), what the HIP model computes stated with numpy.  ``calls`` counts."""
    device = None

    def __init__(self, table, with_clusters):
        self.table, self.calls = table, {"pair_sisdr": 0, "fine_clusters": 0}
        if not with_clusters:
            self.fine_clusters = None                        # hasattr stays true, but host mode must never call it

    def shift_and_sep_resident(self, mix, patch_list, Strict=0, window=12000, device_energies=False):
        import torch
        waves = np.stack([self.table[p.tag] for p in patch_list])
        en = energies_of(waves)
        return torch.from_numpy(waves), (torch.from_numpy(en) if device_energies else en)

    def pair_sisdr(self, waves):
        self.calls["pair_sisdr"] += 1
        w = waves.numpy()
        return np.array([[si_sdr(a, b) for b in w] for a in w])

    def segment_sisdr(self, waves, segments):
        raise AssertionError("the fine stage compares whole waveforms only")

    def fine_clusters(self, waves, bounds, en_dev, gate, group_gate, min_trigger):
        import torch
        self.calls["fine_clusters"] += 1
        order, label, _g = fine_clusters_f64(waves.numpy(), bounds, en_dev.numpy(), gate, group_gate, min_trigger)
        return torch.from_numpy(order), torch.from_numpy(label)


def test_fine_stage_with_device_clustering_equals_host_clustering(monkeypatch):
    """``Spotform_Small_Patch_Parallel`` (the plain resident loop) over two coarse patches of a real array, their
    subdivisions given generated waveforms: device mode makes ONE ``fine_clusters`` call and no ``pair_sisdr`` call and
    returns the output tuples of host mode -- names, powers, waveforms, merged offsets, trace."""
    import torch
    from acousticswarms_speech_amd import mic_array
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 7, 24000)
    res = {}
    for mode in ("host", "device"):
        with redirect_stdout(io.StringIO()):
            ma = MicArray(sc.mic_positions, Spk_Range=sc.speaker_range, Prone_method="DENSE", clustering=mode)
            patch_list, _ = ma.Apply_SRP_PHAT(torch.from_numpy(sc.mix))      # the lattice: no map, no GPU
        bigs = patch_list[len(patch_list) // 2:len(patch_list) // 2 + 2]
        assert len(bigs) == 2
        # tag every fine candidate as the stage meets it and give it a waveform of its group
        table, rng, tags = {}, np.random.default_rng(77), iter(range(10 ** 6))
        inner_subdivide = MicArray._subdivide

        def subdivide(self, big, table=table, rng=rng, tags=tags):
            fine, c = inner_subdivide(self, big)
            rows = make_group(rng, len(fine), 4000)
            for p, row in zip(fine, rows):
                p.tag = next(tags)
                table[p.tag] = row
            return fine, c
        monkeypatch.setattr(MicArray, "_subdivide", subdivide)
        monkeypatch.setattr(mic_array, "SPOT_POWER_THRESHOLD2", 0.02)
        ma.Relative_Threshold = 0.02
        spot = _CpuSpot(table, mode == "device")
        with redirect_stdout(io.StringIO()):
            pairs = ma.Spotform_Small_Patch_Parallel(torch.from_numpy(sc.mix), bigs, spot)
        monkeypatch.setattr(MicArray, "_subdivide", inner_subdivide)
        res[mode] = (pairs, dict(ma.trace["fine_clusters"]), dict(spot.calls), ma)
    host, dev = res["host"], res["device"]
    assert host[2]["fine_clusters"] == 0 and host[2]["pair_sisdr"] >= 1
    assert dev[2] == {"pair_sisdr": 0, "fine_clusters": 1}
    assert dev[1] == host[1] and sum(len(c) for c in host[1].values()) >= 2
    assert len(dev[0]) == len(host[0]) >= 2
    for a, b in zip(dev[0], host[0]):
        assert a[3] == b[3] and a[2] == b[2] and a[5] == b[5]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[0].sample_offset, b[0].sample_offset)
        np.testing.assert_array_equal(a[4]["localization_offset"], b[4]["localization_offset"])
        np.testing.assert_array_equal(a[4]["audio_offset"], b[4]["audio_offset"])
    ma = dev[3]
    assert len(ma._dev_cache) == len(dev[0]) == len(ma._seg_cache)
    for p in dev[0]:
        assert ma._dev_cache[id(p[1])][0] is p[1] and np.array_equal(ma._dev_cache[id(p[1])][1].numpy(), p[1])


def test_chunk_whose_only_open_patch_has_no_head():
    """One coarse patch, far from the array, whose two candidates sit at the reference microphone: the best candidate
    passes the patch's gate (thr / 10) and none passes its own (thr), so the patch is open and has no cluster head.
    Both clustering modes return no output tuple and the energies, record the empty trace entry, copy no row and
    register nothing -- device mode from one ``fine_clusters`` call, host mode without a ``pair_sisdr`` call."""
    import torch
    from acousticswarms_speech_amd.mic_array import MicArray

    class Array(MicArray):
        def __init__(self, mode):                            # no geometry tables: the clustering needs none
            self.MIN_TRIGGER_POWER = 0.5
            self.mic_positions = np.zeros((7, 3))
            self.segments, self.clustering = "host", mode
            self.trace = {"fine_clusters": {}}
            self._seg_cache, self._dev_cache = {}, {}

    T, thr_new, g = 4000, 1.0, 5
    big = _Patch([9.0, 0.0, 0.0])
    big.area_points = None
    fine = [_Patch([0.0, 0.0, 0.0]), _Patch([0.0, 0.0, 0.0])]
    waves = torch.from_numpy(make_group(np.random.default_rng(3), 2, T))
    energies = np.array([[40.0, 0.5], [30.0, 0.25]])                         # (power, windowed power) per candidate
    for mode in ("host", "device"):
        ma = Array(mode)
        spot = _CpuSpot({}, mode == "device")
        gates = ma._fine_gates([big], [fine], thr_new) if mode == "device" else None
        if gates is not None:
            assert gates[1].tolist() == [1.0, 1.0] and gates[2].tolist() == [0.1]
        out, back = ma._cluster_chunk([g], [big], [fine], [None], waves, torch.from_numpy(energies), gates, T, thr_new,
                                      None, spot)
        assert out == [] and back.dtype == np.float64 and back.tobytes() == energies.tobytes() and back.shape == (2, 2)
        assert ma.trace["fine_clusters"] == {g: {}}
        assert ma._seg_cache == {} and ma._dev_cache == {}
        assert spot.calls == {"pair_sisdr": 0, "fine_clusters": int(mode == "device")}


# ---------------------------------------------------------------- the C entry points
def test_entry_points_reject_bad_arguments_without_a_gpu():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    buf = np.zeros(1 << 16)
    p = c_void_p(buf.ctypes.data)

    def b(*v):
        a = np.array(v, dtype=np.int32)
        return a, c_void_p(a.ctypes.data)
    keep, good = b(0, 3, 3, 12)                              # n = 3, 0, 9: 90 Gram elements; tiles 1 + 0 + 3
    need = 90 * 8 + (2 * 4 + 2 * 4 + 12) * 4
    assert L.asw_fine_clusters_workspace_bytes(good, 3) == need
    _k0, zero = b(0)
    assert L.asw_fine_clusters_workspace_bytes(zero, 0) == 8
    assert L.asw_fine_clusters_workspace_bytes(None, 3) == 0 and b"null bounds" in L.asw_last_error()
    assert L.asw_fine_clusters_workspace_bytes(good, -1) == 0 and b"G = -1" in L.asw_last_error()
    assert L.asw_fine_clusters_workspace_bytes(good, 65536) == 0 and b"65535" in L.asw_last_error()
    _k1, bad0 = b(1, 3, 3, 12)
    assert L.asw_fine_clusters_workspace_bytes(bad0, 3) == 0 and b"bounds[0] = 1" in L.asw_last_error()
    _k2, down = b(0, 5, 3, 12)
    assert L.asw_fine_clusters_workspace_bytes(down, 3) == 0 and b"decrease at group 1" in L.asw_last_error()
    _k3, huge = b(0, 11586)                                  # 11586 ** 2 > 2 ** 27 >= 11585 ** 2
    assert L.asw_fine_clusters_workspace_bytes(huge, 1) == 0 and b"cap" in L.asw_last_error()
    _k4, fits = b(0, 11585)
    assert L.asw_fine_clusters_workspace_bytes(fits, 1) > 11585 ** 2 * 8

    def call(y=p, N=12, T=100, bounds=good, G=3, en=p, gate=p, ggate=p, ws=p, ws_bytes=1 << 19, order=p, label=p, gram=None):
        return L.asw_fine_clusters(y, N, T, bounds, G, en, gate, ggate, 0.5, 0.398, ws, ws_bytes, order, label, gram, None)
    for name in ("y", "en", "gate", "ggate", "ws"):
        assert call(**{name: None}) == -1 and b"fine_clusters: null pointer" in L.asw_last_error(), name
    for name in ("order", "label"):
        assert call(**{name: None}) == -1 and b"null output" in L.asw_last_error(), name
    assert call(bounds=None) == -1 and b"null bounds" in L.asw_last_error()
    assert call(N=-1) == -1 and b"N = -1" in L.asw_last_error()
    assert call(T=0) == -1 and call(T=-5) == -1 and b"T = -5" in L.asw_last_error()
    assert call(G=-1) == -1 and call(G=65536) == -1 and b"G = 65536" in L.asw_last_error()
    assert call(bounds=bad0) == -1 and b"bounds[0] = 1" in L.asw_last_error()
    assert call(bounds=down) == -1 and b"decrease" in L.asw_last_error()
    assert call(N=13) == -1 and b"not N = 13" in L.asw_last_error()
    assert call(bounds=huge, G=1, N=11586) == -1 and b"cap" in L.asw_last_error()
    assert call(ws_bytes=need - 1) == -1 and b"too small" in L.asw_last_error()
    assert call(ws=c_void_p(buf.ctypes.data + 4)) == -1 and b"aligned" in L.asw_last_error()
    # nothing to do: no launch, whatever the other pointers are
    _k5, empty = b(0, 0, 0, 0)
    assert call(N=0, bounds=empty, y=None, en=None, gate=None, ggate=None, ws=None, ws_bytes=0, order=None, label=None) == 0
    assert call(N=0, bounds=zero, G=0, y=None, en=None, gate=None, ggate=None, ws=None, ws_bytes=0, order=None, label=None) == 0
    assert call(N=0, bounds=good) == -1 and b"not N = 0" in L.asw_last_error()
    del keep
