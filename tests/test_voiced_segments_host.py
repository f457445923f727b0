"""CPU only: the float64 statement of the voiced segments (``hostdsp.voiced_segments_f64``), which
``asw_voiced_segments`` reproduces bit for bit on the GPU (tests/test_gpu_voiced_segments.py).

The statement is checked on waveforms whose segments are counted by hand, by its structure, and against ``split_wav``
(float32 pairwise sums and ``log10``) on 288 scene waveforms; then the ``segments=`` keyword of the search and the C
entry points' refusals through ctypes."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from acousticswarms_speech_amd.hostdsp import (VOICED_Q, frame_rms, split_wav, voiced_margin_db,
                                               voiced_segments_f64)
from tests.voiced_segments_cases import check_structure, clipped_wave, envelope_wave, scene_waves, statement_tables

MARGIN_DB = 1e-3          # the host's float32 sums and log10 move a level by less than 2e-5 dB: fifty times that
MAX_LEFT_OUT = 0.02


def _lists(segs):
    return [[int(a), int(b)] for a, b in segs]


# ---------------------------------------------------------------- counted by hand
def test_envelope_counted_by_hand():
    y, want = envelope_wave()
    segs, ms = voiced_segments_f64(y)
    assert ms.dtype == np.float64 and ms.shape == (1 + y.shape[0] // 256,)
    assert segs == want                       # 768 dropped; 1792 and 4096 whole; 8192 in two; the last clipped to T
    assert ms.max() == 1.0 and ms[6] == 1.0   # the four blocks of magnitude 1.0
    voiced = np.flatnonzero(ms > 10.0 ** -1.8)
    assert voiced.tolist() == (list(range(3, 10)) + list(range(16, 19)) + list(range(26, 42)) + list(range(50, 82))
                               + list(range(90, 97)))
    check_structure(segs, y.shape[0])
    assert _lists(split_wav(y)) == want       # far from every threshold: split_wav agrees


@pytest.mark.parametrize("length, n_seg", [(999, 0), (1000, 1), (4000, 1), (4001, 1), (7999, 1), (8000, 2), (12345, 3)])
def test_interval_lengths_around_the_splitting_rule(length, n_seg):
    y, want = clipped_wave(length)
    segs, _ = voiced_segments_f64(y)
    assert segs == want and len(segs) == n_seg
    if n_seg:
        assert segs[0][0] == 1024 and segs[-1][1] == y.shape[0]                     # the run reaches the end: clipped to T
        assert all(b - a == 4000 for a, b in segs[:-1]) and 1000 <= segs[-1][1] - segs[-1][0] < 8000
    check_structure(segs, y.shape[0])


def test_zero_wave_and_constant_wave():
    for T in (1, 255, 5000):
        segs, ms = voiced_segments_f64(np.zeros(T, dtype=np.float32))
        assert segs == [] and not ms.any() and ms.shape == (1 + T // 256,)
        assert voiced_margin_db(np.zeros(T, dtype=np.float32)) > 50.0
    segs, ms = voiced_segments_f64(np.full(5000, 0.5, dtype=np.float32))
    assert segs == [[0, 5000]] and ms[2] == 0.25                                   # one run over all 20 frames, 5000 // 4000 = 1
    segs, _ = voiced_segments_f64(np.full(9000, 0.5, dtype=np.float32))
    assert segs == [[0, 4000], [4000, 9000]]
    assert voiced_segments_f64(np.full(999, 0.5, dtype=np.float32))[0] == []


def test_both_sides_of_the_quiet_bound():
    """Below Q the reference level is Q itself: a wave of magnitude 0.039 (peak 0.00152 < 0.0016) is judged against
    thr * Q, one of 0.041 against thr * its own peak.  A second half of magnitude 0.0051 lies between the two
    thresholds (0.04 and 0.041 times 10 ** -0.9 = 0.00504 and 0.00516): voiced beside the quiet wave only."""
    for mag, quiet in ((0.039, True), (0.041, False)):
        y = np.full(8192, mag, dtype=np.float32)
        y[4096:] = 0.0051
        segs, ms = voiced_segments_f64(y)
        assert (ms.max() < VOICED_Q) == quiet
        # quiet: every frame with four whole blocks, 0 .. 30 (the zero padding thins out frames 31 and 32); loud: frames
        # 0 .. 17 hold one of the blocks 0 .. 15.  [0, 7936) and [0, 4608): both // 4000 = 1
        assert segs == ([[0, 7936]] if quiet else [[0, 4608]]), (mag, segs)
        assert voiced_margin_db(y) > 0.05 and _lists(split_wav(y)) == segs


def test_the_order_of_the_sums_is_the_statement():
    """ms is not merely close to the mean square: it is the butterfly's value, and differs from a plain float64 sum."""
    rng = np.random.default_rng(3)
    y = rng.standard_normal(4001).astype(np.float32)
    _, ms = voiced_segments_f64(y)
    q = np.zeros(16 * 256)
    q[:4001] = y.astype(np.float64) ** 2
    lanes = q.reshape(16, 64, 4)
    p = ((lanes[:, :, 0] + lanes[:, :, 1]) + lanes[:, :, 2]) + lanes[:, :, 3]
    for s in (32, 16, 8, 4, 2, 1):
        p = p[:, :s] + p[:, s:2 * s]
    b = np.concatenate([[0.0, 0.0], p[:, 0], [0.0, 0.0]])
    want = np.array([((b[f] + b[f + 1]) + b[f + 2]) + b[f + 3] for f in range(16)]) / 1024.0
    assert ms.tobytes() == want.tobytes()
    np.testing.assert_allclose(ms, frame_rms(y.astype(np.float64), 1024, 256)[0] ** 2, rtol=1e-12)


# ---------------------------------------------------------------- against split_wav
def test_statement_equals_split_wav_on_scene_waveforms():
    waves = scene_waves(range(2000, 2012))
    assert len(waves) == 288 and all(w.dtype == np.float32 and w.shape == (48000,) for w in waves)
    left_out, quiet = 0, 0
    for w in waves:
        segs, ms = voiced_segments_f64(w)
        check_structure(segs, 48000)
        quiet += bool(ms.max() < VOICED_Q)
        if voiced_margin_db(w) < MARGIN_DB:
            left_out += 1
            continue
        assert _lists(split_wav(w)) == segs
    print(f"{left_out} of 288 within {MARGIN_DB} dB of a decision; {quiet} judged against the quiet bound")
    assert left_out <= MAX_LEFT_OUT * len(waves)
    assert 50 <= quiet <= 238                              # both branches of the reference level are compared


def test_statement_tables_layout():
    y, want = envelope_wave()
    seg, cnt, ms, lists = statement_tables(np.stack([y, np.zeros_like(y)]))
    assert seg.shape == (2, 24, 2) and seg.dtype == cnt.dtype == np.int32 and ms.shape == (2, 97)
    assert cnt.tolist() == [5, 0] and seg[0, :5].tolist() == want and not seg[0, 5:].any() and not seg[1].any()
    assert lists == [want, []]


# ---------------------------------------------------------------- the keyword
def test_segments_keyword_and_config_key():
    from acousticswarms_speech_amd import batching
    from acousticswarms_speech_amd.joint import JointModel, config_key
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 7, 4000)
    roi = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
    assert config_key(sc.mic_positions, roi) == config_key(sc.mic_positions, roi, segments="host")
    assert config_key(sc.mic_positions, roi, segments="device") == config_key(sc.mic_positions, roi) + "|segments=device"
    with pytest.raises(ValueError, match="segments"):
        JointModel(None, segments="gpu")
    with redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="segments"):
            MicArray(sc.mic_positions, Spk_Range=roi, segments="gpu")
        assert MicArray(sc.mic_positions, Spk_Range=roi).segments == "host"
        jm = JointModel(None, segments="device")
        jm.setup(sc.mic_positions, roi)
        assert jm.Mic_processor.segments == "device" and jm.previous_config.endswith("|segments=device")
        assert batching.mixture_view(jm.Mic_processor).segments == "device"
        assert jm.mic_array_for(sc.mic_positions, roi).segments == "device"
        jm.setup(sc.mic_positions, roi, segments="host")
        assert jm.Mic_processor.segments == "host" and "segments" not in jm.previous_config


def test_device_segments_need_a_scorer_that_finds_them():
    """A duck-typed model without ``voiced_segments`` cannot serve segments="device": RuntimeError, no quiet fall-back
    to the host path."""
    import torch
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    from tests.golden.surrogate import SurrogateSpot
    sc = make_scene(1010, 5, 7, 4000)
    with redirect_stdout(io.StringIO()):
        ma = MicArray(sc.mic_positions, Spk_Range=[-0.5, 0.5, 1.0, 2.0, 0.1, 0.5], segments="device")
        ma.Relative_Threshold = 1.0
        with pytest.raises(RuntimeError, match="voiced_segments"):
            ma.Spotform_Small_Patch_Parallel(torch.from_numpy(sc.mix), [], SurrogateSpot())
        with pytest.raises(RuntimeError, match="voiced_segments"):
            ma.Clustering_new([])


def test_scorer_pass_throughs():
    from acousticswarms_speech_amd.batching import MixtureScorer

    class Model:
        device, batch_size = None, 4

        def voiced_segments(self, waves):
            return ("seg", waves)

        def segment_sisdr_device(self, waves, seg, cnt):
            return (waves, seg, cnt)

    class Batcher:
        model = Model()
    s = MixtureScorer(Batcher(), 0)
    assert s.voiced_segments("w") == ("seg", "w") and s.segment_sisdr_device("w", "s", "c") == ("w", "s", "c")


# ---------------------------------------------------------------- the C entry points
def test_entry_points_reject_bad_arguments_without_a_gpu():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    buf = np.zeros(1 << 16)
    p = c_void_p(buf.ctypes.data)
    thr, Q = 10.0 ** -1.8, 0.04 * 0.04
    assert L.asw_voiced_segments_workspace_bytes(3, 48000) == 3 * 188 * 8
    assert L.asw_voiced_segments_workspace_bytes(2, 257) == 2 * 2 * 8 and L.asw_voiced_segments_workspace_bytes(0, 100) == 0
    assert L.asw_voiced_segments_workspace_bytes(-1, 100) == 0 and b"voiced_segments_workspace_bytes" in L.asw_last_error()
    assert L.asw_voiced_segments_workspace_bytes(4, 0) == 0 and L.asw_voiced_segments_workspace_bytes(65536, 100) == 0

    def call(y=p, n=4, T=5000, seg=p, kcap=5, cnt=p, ms=None, ws=p, ws_bytes=1 << 19):
        return L.asw_voiced_segments(y, n, T, thr, Q, seg, kcap, cnt, ms, ws, ws_bytes, None)
    for name in ("y", "ws"):
        assert call(**{name: None}) == -1 and b"voiced_segments: null pointer" in L.asw_last_error(), name
    for name in ("seg", "cnt"):
        assert call(**{name: None}) == -1 and b"null output" in L.asw_last_error(), name
    assert call(n=-1) == -1 and b"n = -1" in L.asw_last_error()
    assert call(n=65536) == -1 and b"65535" in L.asw_last_error()
    assert call(T=0) == -1 and call(T=-5) == -1 and b"T = -5" in L.asw_last_error()
    assert call(kcap=4) == -1 and b"kcap = 4" in L.asw_last_error()
    assert call(T=999, kcap=0) == -1 and b"kcap = 0" in L.asw_last_error()          # max(1, T // 1000) = 1
    need = L.asw_voiced_segments_workspace_bytes(4, 5000)
    assert need == 4 * 20 * 8
    assert call(ws_bytes=need - 1) == -1 and b"too small" in L.asw_last_error()
    assert call(n=0, y=None, seg=None, cnt=None, ws=None, ws_bytes=0) == 0             # launches nothing


# ---------------------------------------------------------------- the clustering, with a stand-in scorer
class _CpuScorer(object):
    """The scorer surface ``Clustering_new`` uses, in numpy on CPU tensors: what the HIP model computes, stated with
    ``hostdsp``.  ``calls`` records the order."""
    device = "cpu"

    def __init__(self, device_segments):
        self.calls = []
        if not device_segments:
            self.voiced_segments = None          # hasattr stays true, but host mode must never call it
            self.segment_sisdr_device = None

    def pair_sisdr(self, waves):
        from acousticswarms_speech_amd.hostdsp import si_sdr
        self.calls.append("pair_sisdr")
        w = waves.numpy().astype(np.float64)
        return np.array([[si_sdr(a, b) for b in w] for a in w])

    def segment_sisdr(self, waves, segments):
        from acousticswarms_speech_amd.hostdsp import si_sdr
        self.calls.append("segment_sisdr")
        w = waves.numpy().astype(np.float64)
        cnt = np.array([len(s) for s in segments], dtype=np.int32)
        out = np.full((len(w), len(w), max(1, int(cnt.max()))), np.nan)
        for i, segs in enumerate(segments):
            for j in range(len(w)):
                for k, (a, b) in enumerate(segs):
                    out[i, j, k] = si_sdr(w[i, a:b], w[j, a:b])
        return out, cnt

    def voiced_segments(self, waves):
        import torch
        self.calls.append("voiced_segments")
        seg, cnt, _ms, _lists = statement_tables(waves.numpy())
        return torch.from_numpy(seg), torch.from_numpy(cnt)

    def segment_sisdr_device(self, waves, seg_dev, cnt_dev):
        self.calls.append("segment_sisdr_device")
        seg, cnt = seg_dev.numpy(), cnt_dev.numpy()
        out, cnt2 = self.segment_sisdr(waves, [seg[i, :cnt[i]].tolist() for i in range(len(cnt))])
        self.calls.pop()
        return out, cnt2


class _Spot(object):
    def __init__(self, c):
        self.c = np.asarray(c, dtype=np.float64)

    def center_pos(self):
        return self.c


def test_clustering_with_device_segments_equals_host_segments(monkeypatch):
    """``Clustering_new`` on twelve scene waveforms (and a faint one, which has no segment and is discarded) spread
    over the room: device mode makes one ``voiced_segments`` call, no ``split_wav`` call, and reaches the decisions
    of host mode."""
    from acousticswarms_speech_amd import mic_array
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(2003, 5, T=24000, reverb=True)
    faint = (1e-7 * np.random.default_rng(0).standard_normal(24000)).astype(np.float32)     # under the floor A2
    waves = [w for w in scene_waves([2003], T=24000, gains=False)] + [faint]
    assert min(voiced_margin_db(w) for w in waves) >= MARGIN_DB
    pairs = [(_Spot([0.6 * (i % 4), 0.6 * (i // 4), 0.3]), w, float(np.sum(w.astype(np.float64) ** 2)), f"0_{i}", {}, -1)
             for i, w in enumerate(waves)]
    split_calls = []
    monkeypatch.setattr(mic_array, "split_wav", lambda w, *a, **kw: (split_calls.append(1), split_wav(w, *a, **kw))[1])
    res = {}
    for mode in ("host", "device"):
        with redirect_stdout(io.StringIO()):
            ma = MicArray(sc.mic_positions, Spk_Range=[-0.5, 0.5, 1.0, 2.0, 0.1, 0.5], segments=mode)
            ma._device_scorer = _CpuScorer(mode == "device")
            del split_calls[:]
            _audio, final, _n, _wrong = ma.Clustering_new(list(pairs))
        res[mode] = ([p[3] for p in final], ma.trace["final_clusters"], list(ma._device_scorer.calls), len(split_calls))
    assert res["host"][2] == ["pair_sisdr", "segment_sisdr"] and res["host"][3] == 13
    assert res["device"][2] == ["voiced_segments", "pair_sisdr", "segment_sisdr_device"] and res["device"][3] == 0
    assert res["device"][:2] == res["host"][:2]
    assert 2 <= len(res["host"][0]) <= 12 and "0_12" not in sum(res["host"][1], [])     # the faint one is in no cluster
    # one candidate: no SI-SDR launch, but its segments still decide whether it is kept
    for pair, kept in ((pairs[0], 1), (pairs[12], 0)):
        with redirect_stdout(io.StringIO()):
            ma._device_scorer = _CpuScorer(True)
            _audio, final, _n, _wrong = ma.Clustering_new([pair])
        assert len(final) == kept and ma._device_scorer.calls == ["voiced_segments"]
