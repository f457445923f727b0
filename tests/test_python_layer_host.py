"""Host: the shared pieces of the Python layer -- ``device_model.DeviceModel`` under both handle classes (no GPU: the
refusals only), ``mic_array.run_search`` under its two callers on a stub array, ``hostdsp.mean_removed_energies`` and
``batching.result_record``.  The expected messages are written out as they were before the pieces were shared."""
import numpy as np
import pytest

from acousticswarms_speech_amd import batching, joint
from acousticswarms_speech_amd.batching import result_record, search_one
from acousticswarms_speech_amd.config import SEP_SMALL, TINY, sep_param_shapes, spot_param_shapes
from acousticswarms_speech_amd.device_model import DeviceModel
from acousticswarms_speech_amd.hostdsp import max_avg_power, mean_removed_energies
from acousticswarms_speech_amd.joint import JointModel
from acousticswarms_speech_amd.mic_array import SEARCH_STAGES, run_search
from acousticswarms_speech_amd.sep import SepModel
from acousticswarms_speech_amd.spot import SpotModel
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict

PRECISIONS = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3_safe": 3}
MODELS = {
    "SpotModel": (SpotModel, TINY, make_spot_state_dict, spot_param_shapes, "the spot hot path",
                  lambda m: m.shift_and_sep(np.zeros((7, 4000), dtype=np.float32), [np.zeros(6)])),
    "SepModel": (SepModel, SEP_SMALL, make_sep_state_dict, sep_param_shapes, "the separation network",
                 lambda m: m.infer_sample(np.zeros((7, 4000), dtype=np.float32), [np.zeros(6)])),
}


# ---------------------------------------------------------------- the two handle classes, without a GPU
@pytest.mark.parametrize("name", sorted(MODELS))
def test_both_models_refuse_in_their_own_words(name):
    cls, cfg, make_sd, shapes, _hot, infer = MODELS[name]
    assert issubclass(cls, DeviceModel)
    assert cls.PRECISIONS == PRECISIONS and SpotModel.PRECISIONS is SepModel.PRECISIONS
    unknown = "precision must be one of ['f32', 'f16x3', 'f16', 'f16x3_safe']"
    with pytest.raises(RuntimeError) as err:
        cls(cfg, precision="bf16")
    assert str(err.value) == unknown
    model = cls(cfg)
    with pytest.raises(RuntimeError) as err:
        model.set_precision("fp32")
    assert str(err.value) == unknown and model.precision == "f32"
    model.set_precision("f16x3")                                       # no handle yet: remembered for to()
    assert model.precision == "f16x3" and model.eval() is model and model.to(None) is model

    sd = make_sd(cfg, 1)
    keys = list(sd)
    assert keys == [k for k, _shape in shapes(cfg)]
    dropped = {k: v for k, v in sd.items() if k != keys[2]}
    with pytest.raises(RuntimeError) as err:
        model.load_state_dict(dropped)
    assert str(err.value) == f"Error(s) in loading state_dict: missing ['{keys[2]}'] unexpected []"
    added = dict(sd, **{"extra.weight": np.zeros(3, dtype=np.float32)})
    with pytest.raises(RuntimeError) as err:
        model.load_state_dict(added)
    assert str(err.value) == "Error(s) in loading state_dict: missing [] unexpected ['extra.weight']"
    want_shape = tuple(sd[keys[0]].shape)
    reshaped = dict(sd, **{keys[0]: sd[keys[0]].reshape(-1, 1)})
    with pytest.raises(RuntimeError) as err:
        model.load_state_dict(reshaped)
    assert str(err.value) == f"size mismatch for {keys[0]}: {(sd[keys[0]].size, 1)} vs {want_shape}"
    assert model._sd is None                                           # a refused dict leaves nothing behind
    with pytest.raises(RuntimeError) as err:
        model.load_state_dict(dict(dropped, **{keys[0]: reshaped[keys[0]]}), strict=False)   # not strict: sizes still count
    assert str(err.value).startswith(f"size mismatch for {keys[0]}: ")

    with pytest.raises(RuntimeError) as err:
        model.to("cpu")
    assert str(err.value) == f"{name} runs only on an MI355X (device 'cuda'); there is no CPU path"
    with pytest.raises(RuntimeError) as err:
        infer(model)
    assert str(err.value) == f"{name}.to('cuda') must be called before inference"
    assert model.load_state_dict(sd) is model and list(model._sd) == keys
    model._h = object()                                                # a handle without weights: the second refusal
    model._sd = None
    try:
        with pytest.raises(RuntimeError) as err:
            model._need()
        assert str(err.value) == f"{name} has no weights: call load_state_dict()"
    finally:
        model._h = None


def test_no_device_message_names_the_hot_path(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as err:
        SpotModel(TINY).to("cuda")
    assert str(err.value) == "no HIP device visible: the spot hot path has no CPU fallback"
    with pytest.raises(RuntimeError) as err:
        SepModel(SEP_SMALL).to("cuda:0")
    assert str(err.value) == "no HIP device visible: the separation network has no CPU fallback"


# ---------------------------------------------------------------- the search driver under its two callers
class _Patch:
    def __init__(self, pos):
        self.pos = np.asarray(pos, dtype=np.float64)

    def center_pos(self):
        return self.pos


class _StubArray:
    """The four stage methods with scripted results; ``empty_at`` names the stage that comes back with nothing."""

    def __init__(self, empty_at=None):
        self.empty_at, self.calls = empty_at, []

    def _out(self, stage, value):
        return [] if self.empty_at == stage else value

    def Apply_SRP_PHAT(self, mix):
        self.calls.append(("srp", mix))
        return self._out(0, ["p0", "p1", "p2"]), np.zeros((3, 3))

    def Spotform_Big_Patch(self, mix, patch_list, spot_model):
        self.calls.append(("coarse", mix, list(patch_list), spot_model))
        return self._out(1, ["p0", "p2"])

    def Spotform_Small_Patch_Parallel(self, mix, kept, spot_model):
        self.calls.append(("fine", mix, list(kept), spot_model))
        return self._out(2, ["pair0", "pair1"])

    def Clustering_new(self, pairs):
        self.calls.append(("cluster", list(pairs)))
        final = [(_Patch([1, 2, 3]), "a0", 0.5, "0_1"), (_Patch([4, 5, 6]), "a1", 0.25, "1_0")]
        return [[1.0, 2.0], [3.0, 4.0]], self._out(3, final), 17, None


class _Clock:
    """stands in for the ``time`` module of a caller: every reading is one second after the last"""

    def __init__(self):
        self.now = 0.0

    def time(self):
        self.now += 1.0
        return self.now

    perf_counter = time


CASES = [(0, "No spk picked in SRP-PHAT\n"), (1, "No spk picked in Spotform_Big_Patch\n"),
         (2, "No spk picked in Spotform_Small_Patch\n"), (3, "No spk picked in Clustering\n"), (None, "")]


@pytest.mark.parametrize("empty_at,line", CASES)
def test_one_search_driver_under_both_callers(empty_at, line, monkeypatch, capsys):
    assert SEARCH_STAGES == ("SRP-PHAT", "Spotform_Big_Patch", "Spotform_Small_Patch", "Clustering")
    n_stages = 4 if empty_at is None else empty_at + 1
    # the driver itself, with a timer that only records
    stub, slots = _StubArray(empty_at), []

    def timed(slot, fn, *args):
        slots.append(slot)
        return fn(*args)
    patches, audio, spot_times, empty = run_search(stub, "model", timed, "mix")
    assert slots == list(range(n_stages)) and [c[0] for c in stub.calls] == ["srp", "coarse", "fine", "cluster"][:n_stages]
    assert all(c[1] == "mix" for c in stub.calls[:3]) and all(c[3] == "model" for c in stub.calls[1:3])
    assert empty == (None if empty_at is None else SEARCH_STAGES[empty_at])
    if empty_at is None:
        assert [p[3] for p in patches] == ["0_1", "1_0"] and audio == [[1.0, 2.0], [3.0, 4.0]] and spot_times == 17
    else:
        assert (patches, audio, spot_times) == ([], [], 0)
    # the scoring stages read stage_mix(), asked for after stage 0
    stub2, order = _StubArray(empty_at), []
    run_search(stub2, "model", lambda slot, fn, *a: (order.append(slot), fn(*a))[1], "host mix",
               lambda: (order.append("stage_mix"), "device mix")[1])
    assert order[:2] == [0, "stage_mix"] and stub2.calls[0][1] == "host mix"
    assert all(c[1] == "device mix" for c in stub2.calls[1:3])
    assert capsys.readouterr().out == ""

    # JointModel.localize_by_separation: the five-tuple, the filled slots, the printed line
    monkeypatch.setattr(joint, "time", _Clock())
    jm = JointModel(None)
    jm.Mic_processor, jm.previous_config = _StubArray(empty_at), "stub"
    got = jm.localize_by_separation("mix")
    assert capsys.readouterr().out == line
    if empty_at is None:
        assert got[0] is not None and [p[3] for p in got[0]] == ["0_1", "1_0"]
        assert isinstance(got[1], np.ndarray) and got[1].tolist() == audio and got[2:] == (0, 0, 17)
    else:
        assert got == ([], [], 0, 0, 0)
    assert jm.times == [1.0] * n_stages + [0] * (5 - n_stages)
    assert [c[0] for c in jm.Mic_processor.calls] == [c[0] for c in stub.calls]

    # a search of a batch: the same patches in the record, the same slots, not a word
    monkeypatch.setattr(batching, "time", _Clock())
    view = _StubArray(empty_at)
    finals, record = search_one(view, "scorer", "host mix", "device row")
    assert capsys.readouterr().out == ""
    assert [p[3] for p in finals] == [p[3] for p in got[0]] and record["names"] == [p[3] for p in got[0]]
    assert record["spot_times"] == got[4] and record["times"] == [1.0] * n_stages + [0.0] * (5 - n_stages)
    assert view.calls[0] == ("srp", "host mix")
    assert all(c[1] == "device row" and c[3] == "scorer" for c in view.calls[1:3])


# ---------------------------------------------------------------- the host energy loop
def test_mean_removed_energies_in_and_out_of_place():
    rng = np.random.default_rng(5)
    sep = (rng.standard_normal((3, 257)) + 0.75).astype(np.float32)
    sep[1] = 0.5                                                       # a constant row
    sep[2] = 0.0                                                       # a row of zeros
    before = sep.copy()
    want_p, want_p2, centred = [], [], []
    for i in range(3):
        x = before[i, :] - np.mean(before[i, :])
        centred.append(x)
        want_p.append(np.sum(x ** 2))
        want_p2.append(max_avg_power(x))
    p, p2 = mean_removed_energies(sep)
    assert sep.tobytes() == before.tobytes()                           # left alone
    assert len(p) == len(p2) == 3 and all(v.dtype == np.float32 for v in p) and all(type(v) is float for v in p2)
    assert np.array(p).tobytes() == np.array(want_p).tobytes() and p2 == want_p2
    assert p[1] == 0.0 and p[2] == 0.0 and p2[1] == 0.0 and p2[2] == 0.0 and p[0] > 0 and p2[0] > 0
    view = sep[0:3]                                                    # the fine stage hands in a slice of its table
    q, q2 = mean_removed_energies(view, in_place=True)
    assert np.array(q).tobytes() == np.array(p).tobytes() and q2 == p2
    assert sep.tobytes() == np.stack(centred).tobytes() and sep.tobytes() != before.tobytes()
    assert mean_removed_energies(np.zeros((0, 9), dtype=np.float32)) == ([], [])


# ---------------------------------------------------------------- the per-mixture record
def test_result_record_of_zero_and_two_patches():
    times = [0.1, 0.2, 0.3, 0.4, 0.0]
    r = result_record([], 0, times)
    assert set(r) == {"centres", "powers", "names", "spot_times", "times"}
    assert r["centres"].shape == (0, 3) and r["powers"].shape == (0,) and r["names"] == []
    assert r["spot_times"] == 0 and r["times"] is times
    patches = [(_Patch([1, 2, 3]), "audio0", 0.5, "0_1"), (_Patch([4, 5, 6]), "audio1", 0.25, "1_0")]
    r = result_record(patches, 17, times)
    assert r["centres"].dtype == np.float64 and r["centres"].tolist() == [[1, 2, 3], [4, 5, 6]]
    assert r["powers"].dtype == np.float64 and r["powers"].tolist() == [0.5, 0.25]
    assert r["names"] == ["0_1", "1_0"] and r["spot_times"] == 17 and "audio" not in r
