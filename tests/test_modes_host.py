"""Host: the pieces the search's "host" | "device" modes share -- ``modes.check_modes`` and ``joint.config_key`` over the
mode list, ``native.read_back`` on CPU tensors, and ``batching.MixtureScorer`` forwarding its device helpers by name."""
import itertools

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import modes
from acousticswarms_speech_amd.batching import MixtureScorer
from acousticswarms_speech_amd.joint import JointModel, config_key
from acousticswarms_speech_amd.native import read_back
from tests.read_back_cases import make_cases, check

NAMES = ("geometry", "segments", "clustering", "global_clustering", "coarse")


# ---------------------------------------------------------------- the mode list
def test_names_and_defaults():
    assert modes.MODE_NAMES == NAMES
    assert modes.check_modes() == ("host",) * 5
    assert modes.check_modes(Prone_method="SRP") == ("host",) * 5
    got = modes.check_modes("device", "device", "host", "device", "device", Prone_method="DENSE_NMS")
    assert got == ("device", "device", "host", "device", "device")
    assert modes.check_modes(coarse="device") == ("host",) * 4 + ("device",)          # no method known yet: no rule
    jm = JointModel(None)
    assert [getattr(jm, n) for n in NAMES] == ["host"] * 5
    jm = JointModel(None, segments="device", coarse="device")
    assert [getattr(jm, n) for n in NAMES] == ["host", "device", "host", "host", "device"]


def test_every_refusal_by_its_text():
    for name in NAMES:
        with pytest.raises(ValueError) as err:
            modes.check_modes(**{name: "gpu"})
        assert str(err.value) == f'{name} must be "host" or "device", got \'gpu\''
        with pytest.raises(ValueError, match=f'{name} must be "host" or "device", got None'):
            modes.check_modes(**{name: None})
        with pytest.raises(ValueError, match=f'{name} must be "host" or "device"'):
            JointModel(None, **{name: "Device"})
    with pytest.raises(ValueError) as err:
        modes.check_modes(global_clustering="device")
    assert str(err.value) == 'global_clustering="device" needs segments="device"'
    with pytest.raises(ValueError, match='needs segments="device"'):
        JointModel(None, global_clustering="device", clustering="device")
    for method in ("SRP", "MUSIC", "TOPS"):
        with pytest.raises(ValueError) as err:
            modes.check_modes(coarse="device", Prone_method=method)
        assert str(err.value) == (f'coarse="device" needs a lattice search (Prone_method in '
                                  f"('DENSE', 'DENSE_NMS')), got {method!r}")
    for method in ("DENSE", "DENSE_NMS"):
        modes.check_modes(coarse="device", Prone_method=method)
    # a value that is no mode is refused before a combination is looked at
    with pytest.raises(ValueError, match="segments must be"):
        modes.check_modes(segments="gpu", global_clustering="device")


def test_need_methods_names_what_is_missing():
    class Half(object):
        def score_offsets(self):
            pass
    modes.need_methods(Half(), 'coarse="device"', "score_offsets")
    with pytest.raises(RuntimeError) as err:
        modes.need_methods(Half(), 'coarse="device"', "score_offsets", "coarse_select")
    assert str(err.value) == 'coarse="device" needs a spot model with score_offsets() and coarse_select() (the HIP SpotModel)'
    with pytest.raises(RuntimeError) as err:
        modes.need_methods(None, 'segments="device"', "voiced_segments")
    assert str(err.value) == 'segments="device" needs a spot model with voiced_segments() (the HIP SpotModel)'


def test_config_key_over_all_combinations():
    """The rule of the key, written out: the base key, the pruning method when it is not "SRP", then ``|<name>=device``
    for each mode that is not at its default, in the order of the list."""
    mics = np.array([[0.0, 0.0, 0.02], [0.12, 0.03, 0.02], [-0.07, 0.1, 0.0]])
    roi = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
    base = '~'.join(f"{x:.05f}" for x in mics.flatten()) + '|' + '~'.join(f"{x:.05f}" for x in roi)
    assert config_key(mics, roi) == base
    seen = set()
    for method in ("SRP", "DENSE_NMS"):
        for values in itertools.product(("host", "device"), repeat=5):
            want = base + ("" if method == "SRP" else "|" + method)
            for name, value in zip(NAMES, values):
                if value != "host":
                    want += "|" + name + "=device"
            assert config_key(mics, roi, method, **dict(zip(NAMES, values))) == want
            assert config_key(mics, roi, method, *values) == want                      # positional, in the list's order
            seen.add(want)
    assert len(seen) == 64


# ---------------------------------------------------------------- the one blocking copy
def test_read_back_on_cpu_tensors():
    cases = make_cases()
    sizes = {(str(t.dtype), t.numel()) for t in cases}
    for dtype in ("torch.uint8", "torch.int32", "torch.float32", "torch.float64"):
        assert {n for d, n in sizes if d == dtype} >= {0, 1, 3, 5}, dtype
    offsets = np.cumsum([0] + [t.numel() * t.element_size() for t in cases])
    assert any(o % 8 for o in offsets[:-1]) and any(o % 4 for o in offsets[:-1])    # pieces start off their alignment
    check(read_back(*cases), cases)
    check(read_back(*cases[::-1]), cases[::-1])
    for t in cases:
        check(read_back(t), [t])
    assert read_back() == []
    # the pieces are copies: writing one changes neither its tensor nor its neighbours
    a, b = torch.arange(3, dtype=torch.int32), torch.arange(3, dtype=torch.int32)
    pa, pb = read_back(a, b)
    pa[:] = 9
    assert a.tolist() == [0, 1, 2] and pb.tolist() == [0, 1, 2]


# ---------------------------------------------------------------- the scorer of a batched search
def test_mixture_scorer_forwards_by_name():
    class Model(object):
        device, batch_size = None, 4
        secret = "the model's own"

        def fine_clusters(self, *a, **kw):
            return ("fine", a, kw)

        def coarse_select(self, *a, **kw):
            return ("select", a, kw)

        def shift_and_sep_device_multi(self, *a):
            raise AssertionError("not reached")

    class Batcher(object):
        model = Model()
    s = MixtureScorer(Batcher(), 0)
    assert set(MixtureScorer.FORWARDED) == {"pair_sisdr", "segment_sisdr", "voiced_segments", "segment_sisdr_device",
                                            "fine_clusters", "pair_sisdr_device", "segment_sisdr_resident",
                                            "global_clusters", "coarse_select"}
    assert s.fine_clusters(1, 2, x=3) == ("fine", (1, 2), {"x": 3})
    assert s.coarse_select("e", "d", None, cap=7) == ("select", ("e", "d", None), {"cap": 7})
    for name in MixtureScorer.FORWARDED:
        assert hasattr(s, name) == (name in ("fine_clusters", "coarse_select")), name
    # a name outside the tuple is not forwarded, whatever the model has
    assert not hasattr(s, "secret") and not hasattr(s, "shift_and_sep_device_multi")
    with pytest.raises(AttributeError, match="secret"):
        s.secret
    # the methods that do their own work are the scorer's
    for name in ("shift_and_score", "shift_and_sep_resident", "shift_and_sep", "score_offsets", "host_offsets"):
        assert name in vars(MixtureScorer) and name not in MixtureScorer.FORWARDED
    # the capability checks see the model through the scorer
    with pytest.raises(RuntimeError, match=r"voiced_segments\(\)"):
        modes.need_methods(s, 'segments="device"', "voiced_segments")
    modes.need_methods(s, 'clustering="device"', "fine_clusters")
