"""CPU only: the host side of the batched joint separation -- the packing rule of ``SepModel.infer_batch``, its argument
checks (made before any device work), ``localize_batch(..., separate=True)`` with stand-in models, and the refusals of
the two ragged kernel entry points (no HIP call is made)."""
import ctypes

import numpy as np
import pytest

from acousticswarms_speech_amd import native
from acousticswarms_speech_amd.joint import JointModel
from acousticswarms_speech_amd.sep import MAX_SEQUENCES, SepModel, pack_items
from acousticswarms_speech_amd.shard import localize_batch


# ---------------------------------------------------------------- pack_items
def test_pack_items_cases_worked_out_by_hand():
    assert MAX_SEQUENCES == 64
    assert pack_items([5] * 13, 64) == [(0, 12), (12, 13)]             # 12 x 5 = 60; the 13th would make 65
    assert pack_items([5] * 13) == [(0, 12), (12, 13)]                 # the default cap is the library's limit
    assert pack_items([], 64) == []
    assert pack_items([3, 0, 2], 64) == [(0, 3)]                       # an empty item rides along
    assert pack_items([0, 0], 64) == [(0, 2)]
    assert pack_items([64], 64) == [(0, 1)]                            # exactly the limit
    assert pack_items([64, 1, 63, 0, 1], 64) == [(0, 1), (1, 4), (4, 5)]
    assert pack_items([60, 0, 5], 64) == [(0, 2), (2, 3)]
    with pytest.raises(RuntimeError, match="65"):
        pack_items([3, 65], 64)
    with pytest.raises(ValueError):
        pack_items([3, -1], 64)


def test_pack_items_properties():
    rng = np.random.default_rng(7)
    for _ in range(300):
        cap = int(rng.integers(1, 70))
        counts = [int(c) for c in rng.integers(0, cap + 1, int(rng.integers(0, 40)))]
        calls = pack_items(counts, cap)
        # order kept, every item exactly once, no empty call
        assert [k for a, b in calls for k in range(a, b)] == list(range(len(counts)))
        assert all(b > a for a, b in calls)
        for i, (a, b) in enumerate(calls):
            assert sum(counts[a:b]) <= cap
            if i + 1 < len(calls):                                      # greedy: the next item did not fit
                assert sum(counts[a:b]) + counts[b] > cap


# ---------------------------------------------------------------- argument errors before any device work
def test_infer_batch_checks_its_arguments_before_any_device_work():
    from acousticswarms_speech_amd.config import SEP_SMALL
    model = SepModel(SEP_SMALL)                    # no weights, no device: whatever got past the checks would raise RuntimeError
    mixes = [np.zeros((7, 4000), dtype=np.float32) for _ in range(3)]
    one = [np.zeros(6)]
    with pytest.raises(ValueError, match="2 sample lists for 3 mixtures"):
        model.infer_batch(mixes, [one, one])
    with pytest.raises(ValueError, match="share M and T"):
        model.infer_batch(mixes[:2] + [np.zeros((7, 4004), dtype=np.float32)], [one] * 3)
    with pytest.raises(ValueError, match="share M and T"):
        model.infer_batch(mixes[:2] + [np.zeros((6, 4000), dtype=np.float32)], [one] * 3)
    with pytest.raises(ValueError, match=r"\[M, T\]"):
        model.infer_batch([np.zeros(4000, dtype=np.float32)], [one])
    with pytest.raises(RuntimeError, match="65 speakers in one item"):
        model.infer_batch(mixes, [one, [np.zeros(6)] * 65, one])
    with pytest.raises(RuntimeError, match="offsets"):
        model.infer_batch(mixes, [one, [np.zeros(5)], one])
    # no talker anywhere: nothing to launch, so not even a device is needed
    out = model.infer_batch(mixes, [[], [], []])
    assert [o.shape for o in out] == [(0, 4000)] * 3 and all(o.dtype == np.float32 for o in out)
    assert model.infer_batch([], []) == []


def test_joint_model_forwards_the_sample_offsets():
    class Patch:
        def __init__(self, o):
            self.sample_offset = o

    class Sep:
        def infer_batch(self, mixes, sample_lists):
            return ("batch", mixes, sample_lists)

        def infer_sample(self, mix, sample_list):
            return ("sample", mix, sample_list)
    jm = JointModel(None, Sep())
    got = jm.separate_batch(["m0", "m1"], [[(Patch(1), "a", 0.5, "n")], []])
    assert got == ("batch", ["m0", "m1"], [[1], []])
    assert jm.separate_by_localization_by_sample("m", [[1, 2]]) == ("sample", "m", [[1, 2]])
    assert jm.separate_by_localization_by_sample("m", []) is None       # the reference's early return (:207-208)
    with pytest.raises(RuntimeError, match="separation model"):
        JointModel(None).separate_batch(["m0"], [[]])


# ---------------------------------------------------------------- localize_batch(separate=...) with stand-in models
class _Patch:
    def __init__(self, pos):
        self.pos = np.asarray(pos, dtype=np.float64)

    def center_pos(self):
        return self.pos


def _stand_in(sep_model):
    """A JointModel whose forward is a stand-in: mixture k (its first sample is k) has k talkers."""
    jm = JointModel(None, sep_model)
    made = {}

    def forward(mix):
        k = int(mix[0, 0])
        patches = [(_Patch([k, s, 0]), None, 0.25 * (s + 1), f"{k}_{s}") for s in range(k)]
        audio = None if k == 0 else np.full((k, mix.shape[1]), float(k), dtype=np.float32)
        made[k] = audio
        jm.times = [1, 2, 3, 4, 5]
        return patches, None, audio, 0, 0, 7
    jm.forward = forward
    return jm, made


def _mixes(n, T=40):
    return [np.full((7, T), float(k), dtype=np.float32) for k in range(n)]


def test_plain_loop_returns_the_audio_of_forward():
    jm, made = _stand_in(sep_model=object())
    out = localize_batch(jm, _mixes(3), concurrent=1, separate=True)
    assert len(out) == 3
    for k, r in enumerate(out):
        assert set(r) == {"centres", "powers", "names", "spot_times", "times", "audio"}
        assert r["names"] == [f"{k}_{s}" for s in range(k)] and r["audio"].shape == (k, 40)
        assert r["audio"].dtype == np.float32
    assert out[0]["audio"].shape == (0, 40)
    assert out[1]["audio"] is made[1] and out[2]["audio"] is made[2]


def test_without_separate_the_result_has_exactly_the_keys_it_had():
    jm, _made = _stand_in(sep_model=object())
    for kw in ({}, {"separate": False}):
        out = localize_batch(jm, _mixes(3), concurrent=1, **kw)
        assert [set(r) for r in out] == [{"centres", "powers", "names", "spot_times", "times"}] * 3


def test_separate_needs_a_separation_model():
    from acousticswarms_speech_amd.batching import search_batched
    jm, made = _stand_in(sep_model=None)
    for concurrent in (1, 2):
        with pytest.raises(RuntimeError, match="separation model"):
            localize_batch(jm, _mixes(3), concurrent=concurrent, separate=True)
    with pytest.raises(RuntimeError, match="separation model"):
        search_batched(jm, _mixes(3), separate=True)
    assert made == {}                                                   # refused before any search


# ---------------------------------------------------------------- C entry points: refused on the host
def test_ragged_kernel_entry_points_reject_bad_arguments_without_a_gpu():
    L = native.lib()
    buf = np.zeros(64)
    p = ctypes.c_void_p(buf.ctypes.data)                               # never dereferenced: every call below is refused

    def table(*v):
        return (ctypes.c_int32 * len(v))(*v)
    assert L.asw_inter_attention_groups(None, table(0, 2), 1, 5, 128, 8, p, None) == -1
    assert b"inter_attention_groups: null" in L.asw_last_error()
    assert L.asw_inter_attention_groups(p, table(0, 2), -1, 5, 128, 8, p, None) == -1
    assert L.asw_inter_attention_groups(p, table(1, 2), 1, 5, 128, 8, p, None) == -1
    assert b"bounds[0]" in L.asw_last_error()
    assert L.asw_inter_attention_groups(p, table(0, 2, 2), 2, 5, 128, 8, p, None) == -1      # an empty group
    assert b"group 1 holds 0" in L.asw_last_error()
    assert L.asw_inter_attention_groups(p, table(0, 2, 1), 2, 5, 128, 8, p, None) == -1      # decreasing
    assert L.asw_inter_attention_groups(p, table(0, 65), 1, 5, 128, 8, p, None) == -1
    assert b"65 sequences" in L.asw_last_error()
    assert L.asw_inter_attention_groups(p, table(*range(66)), 65, 5, 128, 8, p, None) == -1
    assert b"G=65" in L.asw_last_error()
    assert L.asw_inter_attention_groups(p, table(0, 2), 1, 5, 130, 8, p, None) == -1
    assert L.asw_inter_attention_groups(p, table(0, 2), 1, 5, 1024, 8, p, None) == -1         # head_dim 128
    assert L.asw_inter_attention_groups(p, table(0), 0, 5, 128, 8, p, None) == 0              # no group: nothing to launch

    ok = (p, 7, 4000, p, table(0, 2), 1, table(0), p, p, p, None)
    assert L.asw_joint_shift_stats_groups(None, *ok[1:]) == -1
    assert b"joint_shift_stats_groups: null" in L.asw_last_error()
    assert L.asw_joint_shift_stats_groups(p, 7, 1, *ok[3:]) == -1                              # T < 2
    assert L.asw_joint_shift_stats_groups(p, 7, 4000, p, table(0, 2, 2), 2, table(0, 1), p, p, p, None) == -1
    assert L.asw_joint_shift_stats_groups(p, 7, 4000, p, table(0, 2), 1, table(-1), p, p, p, None) == -1
    assert b"mixture -1" in L.asw_last_error()
    assert L.asw_joint_shift_stats_groups(p, 40, 4000, p, table(0, 64), 1, table(0), p, p, p, None) == -1   # 64 * 40 channels
    assert b"S*M" in L.asw_last_error()
    assert L.asw_joint_shift_stats_groups(p, 7, 4000, p, table(0), 0, table(0), p, p, p, None) == 0
    # the model entry refuses a handle that is not ready before it looks at anything else
    assert L.asw_sep_infer_batch(None, p, 1, 7, 4000, p, table(2), p, None) != 0
