"""GPU: the voiced segments found on the device (``asw_voiced_segments`` in csrc/misc_kernels.hip,
``torch.ops.asw.voiced_segments``) and the search mode made of them (``MicArray(segments="device")``).

1. the op against its numpy statement (``hostdsp.voiced_segments_f64``) on the smallest shapes that reach each path of
   the two kernels -- fewer samples than a block, rows that are not 16-byte aligned, more waveforms than fit one
   launch row, more frames than one chunk of the scan --, on the waveforms counted by hand and on scene waveforms;
2. two calls are bit-identical, and the result does not depend on what the outputs or the workspace held;
3. ``segment_sisdr_device`` on the op's tables against ``segment_sisdr`` on the statement's lists;
4. the whole search and a batch of four mixtures with ``segments="device"`` against ``segments="host"``.
The bound is equality everywhere: ``ms`` bit for bit, whole tables including the zeroed tail, counts.  Needs an MI355X."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd.hostdsp import VOICED_Q, voiced_margin_db
from tests.voiced_segments_cases import clipped_wave, envelope_wave, scene_waves, statement_tables

pytestmark = pytest.mark.gpu

MARGIN_DB = 1e-3          # as in tests/test_voiced_segments_host.py: fifty times what float32 rounding moves a level by


def _ops():
    from acousticswarms_speech_amd import native
    return native.torch_ops()


def _bursts(n, T, seed):
    """float32 [n, T]: noise gated in stretches of 700 samples at random levels, so that runs of every length occur."""
    rng = np.random.default_rng(seed)
    k = -(-T // 700)
    env = np.repeat((rng.uniform(size=(n, k)) > 0.4) * rng.uniform(0.05, 1.0, (n, k)), 700, axis=1)[:, :T]
    return (rng.standard_normal((n, T)) * env * 0.3).astype(np.float32)


def _check(waves, y_dev=None, label=""):
    """The op on ``waves`` (or on the device tensor that holds them) against the statement: every byte."""
    waves = np.ascontiguousarray(waves, dtype=np.float32)
    n, T = waves.shape
    seg_w, cnt_w, ms_w, lists = statement_tables(waves)
    y = torch.from_numpy(waves).cuda() if y_dev is None else y_dev
    seg, cnt, ms = _ops().voiced_segments(y, 18.0, True)
    assert seg.dtype == torch.int32 and cnt.dtype == torch.int32 and ms.dtype == torch.float64
    assert tuple(seg.shape) == (n, max(1, T // 1000), 2) and tuple(cnt.shape) == (n,) and tuple(ms.shape) == (n, 1 + T // 256)
    seg, cnt, ms = seg.cpu().numpy(), cnt.cpu().numpy(), ms.cpu().numpy()
    print(f"{label} n={n} T={T}: counts {cnt_w.tolist()[:8]}")
    assert ms.tobytes() == ms_w.tobytes(), f"{label}: ms differs in {np.count_nonzero(ms != ms_w)} of {ms.size} frames"
    np.testing.assert_array_equal(cnt, cnt_w)
    assert seg.tobytes() == seg_w.tobytes(), label
    seg2, cnt2, ms2 = _ops().voiced_segments(y)                         # the defaults: top_db 18, no ms
    assert ms2.numel() == 0 and seg2.cpu().numpy().tobytes() == seg_w.tobytes() and torch.equal(cnt2.cpu(), torch.from_numpy(cnt_w))
    return lists


# ---------------------------------------------------------------- the op against the statement
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 1023, 1024, 4001])
def test_small_shapes(T, n):
    """One sample; one sample short of a block, a block, one more; the first T with a segment slot of its own; odd T
    with three rows: rows 1 and 2 start at addresses that are no multiple of 16."""
    _check(_bursts(n, T, 100 * T + n), label="bursts")


def test_more_rows_than_one_wavefront_of_blocks():
    lists = _check(_bursts(65, 2048, 7), label="65 rows")
    assert sum(len(s) for s in lists) >= 20


def test_aligned_length_on_a_misaligned_base():
    """T % 4 == 0 but the tensor starts 4 bytes into its allocation: the kernel must not take the 16-byte loads."""
    waves = _bursts(3, 4000, 11)
    buf = torch.zeros(3 * 4000 + 4, device="cuda")
    y = buf[1:1 + 3 * 4000].view(3, 4000)
    y.copy_(torch.from_numpy(waves))
    assert y.is_contiguous() and y.data_ptr() % 16 == 4
    _check(waves, y_dev=y, label="base + 4")


def test_waveforms_counted_by_hand():
    y, want = envelope_wave()
    assert _check(y[None], label="envelope") == [want]
    for length in (1000, 4000):
        y, want = clipped_wave(length)
        assert _check(y[None], label=f"clipped {length}") == [want]


def test_zero_wave_constant_wave_and_both_sides_of_the_quiet_bound():
    waves = np.zeros((5, 8192), dtype=np.float32)
    waves[1] = 0.5
    waves[2, :4096], waves[2, 4096:] = 0.039, 0.0051                    # below Q: judged against Q, all of it voiced
    waves[3, :4096], waves[3, 4096:] = 0.041, 0.0051                    # above: against its own peak, the loud half only
    waves[4] = 1e-6                                                     # under the floor A2 altogether
    lists = _check(waves, label="levels")
    assert lists == [[], [[0, 4000], [4000, 8192]], [[0, 7936]], [[0, 4608]], []]
    ms = statement_tables(waves)[2]
    assert ms[2].max() < VOICED_Q < ms[3].max()


def test_a_run_longer_than_one_chunk_of_frames():
    """300 frames: the scan's carries take a run and its segment count from one chunk of 256 frames into the next."""
    waves = np.full((2, 76800), 0.5, dtype=np.float32)
    waves[1, 256 * 250:256 * 262] = 0.0                                 # a gap across the chunk boundary
    lists = _check(waves, label="two chunks")
    assert len(lists[0]) == 19 and lists[0][-1] == [72000, 76800]


_SCENE = {}


def _scene(T):
    """Scene waveforms and the statement's tables for them, made once: 24 at T = 48 000 (the 12 of one scene at gain
    1 and at a quiet gain), 4 at T = 144 000."""
    if T not in _SCENE:
        waves = np.stack(scene_waves([2000]) if T == 48000 else scene_waves([2001], T=T, gains=False)[:4])
        _SCENE[T] = (waves, statement_tables(waves))
    return _SCENE[T]


@pytest.mark.parametrize("T, n", [(48000, 24), (144000, 4)])
def test_scene_waveforms(T, n):
    waves, (_seg, cnt, ms, _lists) = _scene(T)
    assert waves.shape == (n, T) and cnt.max() >= 4
    if T == 48000:
        assert (ms.max(axis=1) < VOICED_Q).any() and (ms.max(axis=1) >= VOICED_Q).any()
    _check(waves, label="scene")


# ---------------------------------------------------------------- what the buffers held
def test_outputs_and_workspace_may_hold_anything_and_two_calls_are_identical():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    waves, (seg_w, cnt_w, ms_w, _lists) = _scene(48000)
    n, T = waves.shape
    y = torch.from_numpy(waves).cuda()
    ws_bytes = L.asw_voiced_segments_workspace_bytes(n, T)
    assert ws_bytes == n * 188 * 8
    thr, Q = 10.0 ** (-18.0 / 10.0), 0.04 * 0.04
    got = []
    for fill in (0xFF, 0x00, 0xFF):
        seg = torch.full((n, 48, 2), fill, dtype=torch.uint8, device="cuda").repeat(1, 1, 4).view(torch.int32)
        cnt = torch.full((n * 4,), fill, dtype=torch.uint8, device="cuda").view(torch.int32)
        ms = torch.full((n, 188 * 8), fill, dtype=torch.uint8, device="cuda").view(torch.float64)
        ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device="cuda")
        assert tuple(seg.shape) == (n, 48, 2) and tuple(ms.shape) == (n, 188)
        native.check(L.asw_voiced_segments(c_void_p(y.data_ptr()), n, T, thr, Q, c_void_p(seg.data_ptr()), 48,
                                           c_void_p(cnt.data_ptr()), c_void_p(ms.data_ptr()), c_void_p(ws.data_ptr()),
                                           ws_bytes, native.current_stream()))
        torch.cuda.synchronize()
        got.append((seg.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes(), ms.cpu().numpy().tobytes()))
    assert got[0] == got[1] == got[2] == (seg_w.tobytes(), cnt_w.tobytes(), ms_w.tobytes())
    # a table wider than needed: the tail is zeroed all the way
    seg = torch.full((n, 60, 2), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    native.check(L.asw_voiced_segments(c_void_p(y.data_ptr()), n, T, thr, Q, c_void_p(seg.data_ptr()), 60,
                                       c_void_p(cnt.data_ptr()), None, c_void_p(ws.data_ptr()), ws_bytes,
                                       native.current_stream()))
    seg = seg.cpu().numpy()
    assert np.array_equal(seg[:, :48], seg_w) and not seg[:, 48:].any() and np.array_equal(cnt.cpu().numpy(), cnt_w)


def test_no_waveforms_and_adapter_checks():
    ops = _ops()
    seg, cnt, ms = ops.voiced_segments(torch.zeros((0, 5000), device="cuda"), 18.0, True)
    assert tuple(seg.shape) == (0, 5, 2) and tuple(cnt.shape) == (0,) and tuple(ms.shape) == (0, 20)
    y = torch.zeros((3, 5000), device="cuda")
    with pytest.raises(RuntimeError, match="must be Float"):
        ops.voiced_segments(y.double())
    with pytest.raises(RuntimeError, match="2 dimensions"):
        ops.voiced_segments(y[0])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.voiced_segments(torch.zeros((5000, 3), device="cuda").t())
    with pytest.raises(RuntimeError, match="at least one sample"):
        ops.voiced_segments(torch.zeros((3, 0), device="cuda"))
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.voiced_segments(torch.zeros((3, 5000)))


# ---------------------------------------------------------------- into the segment SI-SDR
def test_segment_sisdr_device_equals_segment_sisdr_on_the_statements_lists():
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.spot import SpotModel
    m = SpotModel(SMALL)                                     # the SI-SDR helpers need no weights
    waves, (_seg, cnt_w, _ms, lists) = _scene(48000)
    y = torch.from_numpy(waves).cuda()
    want, want_cnt = m.segment_sisdr(y, lists)
    seg_dev, cnt_dev = m.voiced_segments(y)
    assert seg_dev.is_cuda and cnt_dev.is_cuda and tuple(seg_dev.shape) == (24, 48, 2)
    got, got_cnt = m.segment_sisdr_device(y, seg_dev, cnt_dev)
    assert got.shape == want.shape == (24, 24, int(cnt_w.max())) and got.dtype == np.float64
    np.testing.assert_array_equal(got_cnt, want_cnt)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any() and not np.isnan(want).all()
    np.testing.assert_array_equal(got, want)                # NaN positions included


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


def _record_heads(monkeypatch):
    """Every waveform the global clustering compares, per Clustering_new call."""
    from acousticswarms_speech_amd.mic_array import MicArray
    calls, inner = [], MicArray.Clustering_new

    def recording(self, output_pair, *a, **kw):
        calls.append([np.asarray(p[1]) for p in output_pair])
        return inner(self, output_pair, *a, **kw)
    monkeypatch.setattr(MicArray, "Clustering_new", recording)
    return calls


def test_whole_search_with_device_segments_equals_host_segments(spot, monkeypatch):
    """Same talker names, trace, spot_times, positions and powers, on a scene none of whose cluster heads lies within
    MARGIN_DB of a decision (there float32 ``split_wav`` and the float64 statement may part): seed 1010, else 1011,
    else 1012; no qualifying seed is a failure."""
    from acousticswarms_speech_amd import hostdsp, mic_array
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    calls = _record_heads(monkeypatch)
    tried = []
    for seed in (1010, 1011, 1012):
        sc = make_scene(seed, 5, 7, 48000, reverb=True)
        mix_t = torch.from_numpy(sc.mix)
        jm = JointModel(spot, None, device="cuda")
        with redirect_stdout(io.StringIO()):
            jm.setup(sc.mic_positions, sc.speaker_range)
        del calls[:]
        want, trace_want = _forward(jm, mix_t)
        heads = calls[0] if calls else []
        margin = min([voiced_margin_db(h) for h in heads], default=0.0)
        tried.append((seed, len(heads), margin))
        print(f"seed {seed}: {len(heads)} cluster heads, smallest margin {margin:.3g} dB, {len(want[2])} talkers")
        if len(heads) < 2 or margin < MARGIN_DB:
            continue
        with redirect_stdout(io.StringIO()):
            jm.setup(sc.mic_positions, sc.speaker_range, segments="device")
        mp = jm.Mic_processor
        assert mp.segments == "device"
        split_calls = []
        monkeypatch.setattr(mic_array, "split_wav", lambda w, *a, **kw: (split_calls.append(1), hostdsp.split_wav(w, *a, **kw))[1])
        got, trace_got = _forward(jm, mix_t)
        assert split_calls == [] and mp._seg_cache == {} and len(mp._dev_cache) == len(heads)
        assert len(want[2]) >= 1
        assert got[2] == want[2] and got[3] == want[3]                     # names, spot_times
        assert trace_got == trace_want                                     # every hard decision
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        return
    raise AssertionError(f"no scene whose cluster heads all keep {MARGIN_DB} dB from a decision: {tried}")


def test_batch_of_four_mixtures_with_device_segments(spot, monkeypatch):
    """``localize_batch`` with segments="device" against the per-mixture loop with segments="host".  The plain loop
    (``concurrent=1``) is the same arithmetic and must be equal; with ``concurrent=2`` a candidate's energy moves by
    about 1e-6 with the internal batch it lands in, the bar of test_config3_mixture_batch_equals_plain_loop.  A
    mixture with a cluster head within MARGIN_DB of a decision is left out, as in the single search; at least two of
    the four must remain."""
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.shard import localize_batch
    first = make_scene(2000, 5, 7, 24000)
    scenes = [make_scene(2000 + k, 5, 7, 24000, mic_positions=first.mic_positions) for k in range(4)]
    mixes = [torch.from_numpy(s.mix) for s in scenes]
    calls = _record_heads(monkeypatch)
    jm = JointModel(spot, None, device="cuda")
    with redirect_stdout(io.StringIO()):
        jm.setup(first.mic_positions, first.speaker_range)
    want = [_forward(jm, m)[0] for m in mixes]
    assert len(calls) == 4
    compared = [k for k in range(4) if min(voiced_margin_db(h) for h in calls[k]) >= MARGIN_DB]
    print(f"heads per mixture {[len(c) for c in calls]}, compared {compared}")
    assert len(compared) >= 2

    jd = JointModel(spot, None, device="cuda", segments="device")
    with redirect_stdout(io.StringIO()):
        jd.setup(first.mic_positions, first.speaker_range)
        plain = localize_batch(jd, mixes, concurrent=1)
        batched = localize_batch(jd, mixes, concurrent=2)
    assert jd.Mic_processor.segments == "device" and len(plain) == len(batched) == 4
    for k in compared:
        r, w = plain[k], want[k]
        assert list(r["names"]) == w[2] and int(r["spot_times"]) == w[3] and len(w[2]) >= 1
        np.testing.assert_array_equal(r["centres"], w[0])
        np.testing.assert_array_equal(r["powers"], w[1])
        r = batched[k]
        assert list(r["names"]) == w[2] and int(r["spot_times"]) == w[3]
        np.testing.assert_allclose(r["centres"], w[0], atol=1e-6)
        np.testing.assert_allclose(r["powers"], w[1], rtol=1e-5)
