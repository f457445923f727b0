"""BSS-eval SDR on the device, the parts that need no GPU: the packing rule, the Python layer's errors, the route back
to the host statement for items the device marks, and the refusals of the C entry point (all of which happen before the
first launch)."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import evalkit, native

from tests import bss_eval_cases as cases
from tests.bss_sources_cases import c_bytes as _c_bytes, c_call, stand_in as _stand_in

MB = 1 << 20


def test_workspace_formula_equals_the_library():
    rng = np.random.default_rng(4)
    shapes = [([5], 2, 48000, 512), ([2], 2, 16000, 512), ([1], 1, 64, 64), ([0, 2, 0], 2, 257, 21), ([3, 1, 2], 3, 4099, 43),
              ([], 2, 100, 10), ([0], 1, 100, 10), ([16], 2, 9000, 512)]
    for _ in range(40):
        flen = int(rng.integers(1, 200))
        shapes.append(([int(c) for c in rng.integers(0, 9, rng.integers(1, 6))], int(rng.integers(1, 4)),
                       int(flen + rng.integers(0, 5000)), flen))
    for counts, R, T, flen in shapes:
        assert evalkit.bss_workspace_bytes(counts, R, T, flen) == _c_bytes(counts, R, T, flen), (counts, R, T, flen)
    # the dense systems dominate: 5 talkers of 512 taps are 2560^2 + 5 * 512^2 doubles
    assert evalkit.bss_workspace_bytes([5], 2, 48000, 512) > 8 * (2560 ** 2 + 5 * 512 ** 2)
    assert evalkit.bss_workspace_bytes([5], 2, 48000, 512) < 80 * MB


def test_packing_cases_by_hand():
    one = evalkit.bss_workspace_bytes([2], 2, 1000, 64)
    two = evalkit.bss_workspace_bytes([2, 2], 2, 1000, 64)
    three = evalkit.bss_workspace_bytes([2, 2, 2], 2, 1000, 64)
    assert one < two < three
    pack = evalkit.pack_bss_items
    assert pack([], [], 2, 64) == []
    assert pack([2, 2, 2], [1000] * 3, 2, 64) == [(0, 3)]                          # the default budget holds them all
    assert pack([2, 2, 2], [1000] * 3, 2, 64, budget=three) == [(0, 3)]            # exactly full is full, not over
    assert pack([2, 2, 2], [1000] * 3, 2, 64, budget=three - 1) == [(0, 2), (2, 3)]
    assert pack([2, 2, 2], [1000] * 3, 2, 64, budget=two - 1) == [(0, 1), (1, 2), (2, 3)]
    assert pack([2, 2, 2], [1000, 1000, 1001], 2, 64) == [(0, 2), (2, 3)]          # one length per call
    assert pack([2, 0, 2], [1000, 1000, 1000], 2, 64, budget=two - 1) == [(0, 2), (2, 3)]      # an empty item rides along
    assert pack([0, 0], [64, 64], 1, 64) == [(0, 2)]
    with pytest.raises(RuntimeError, match="alone needs"):
        pack([2], [1000], 2, 64, budget=one - 1)
    with pytest.raises(ValueError, match="talkers"):
        pack([17], [100000], 2, 64)
    with pytest.raises(ValueError, match="flen = 1025"):
        pack([1], [100000], 2, 1025)
    with pytest.raises(ValueError, match="talkers"):
        pack([9], [100000], 2, 1000)                                               # 9000 > 8192
    with pytest.raises(ValueError, match="fewer than flen"):
        pack([1], [63], 2, 64)
    with pytest.raises(ValueError, match="lengths"):
        pack([1, 1], [64], 2, 64)
    with pytest.raises(ValueError, match="R = 0"):
        pack([1], [64], 0, 64)


def test_packing_properties():
    rng = np.random.default_rng(20261019)
    for _ in range(200):
        K = int(rng.integers(0, 12))
        counts = [int(c) for c in rng.integers(0, 5, K)]
        lengths = [int(t) for t in rng.choice([600, 700], K, p=[0.8, 0.2])]
        R, flen = int(rng.integers(1, 3)), int(rng.integers(1, 65))
        alone = max([evalkit.bss_workspace_bytes([c], R, t, flen) for c, t in zip(counts, lengths)] + [1])
        budget = int(alone * rng.uniform(1.0, 4.0))
        calls = evalkit.pack_bss_items(counts, lengths, R, flen, budget)
        assert [k for a, b in calls for k in range(a, b)] == list(range(K))       # whole, in order, once
        for a, b in calls:
            assert b > a and len(set(lengths[a:b])) == 1
            assert evalkit.bss_workspace_bytes(counts[a:b], R, lengths[a], flen) <= budget
        for (a, b), (c, d) in zip(calls, calls[1:]):                               # greedy: the next item did not fit
            assert lengths[c] != lengths[a] or evalkit.bss_workspace_bytes(counts[a:c + 1], R, lengths[a], flen) > budget
        assert evalkit.pack_bss_items(counts, lengths, R, flen, budget) == calls   # pure


def test_metrics_values_and_missing_gpu(monkeypatch):
    ref = np.ones((1, 600))
    for fn, args in ((evalkit.compute_metrics, (ref, ref, ref)), (evalkit.evaluate_sample, (None, {}, ref, ref)),
                     (evalkit.evaluate_dataset, (None, "/nonexistent"))):
        with pytest.raises(ValueError, match="metrics must be one of"):
            fn(*args, metrics="gpu")
    # "device" without a GPU is an error, not the host metric
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        evalkit.compute_metrics(ref, ref, ref, metrics="device")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        evalkit.bss_eval_sdr_device(ref, ref[None], flen=8)
    # ... and without the built adapter library too
    monkeypatch.setattr(native, "_ops", None)
    monkeypatch.setattr(native, "OPS_PATH", "/nonexistent/libasw_torch_ops.so")
    with pytest.raises(RuntimeError, match="is missing"):
        evalkit.bss_eval_sdr_device(ref, ref[None], flen=8)


def test_host_default_is_untouched_by_the_option():
    rng = np.random.default_rng(1)
    gt = cases.references(rng, 2, 900)
    est = cases.estimates(rng, gt, "noisy")
    inp = cases.estimates(rng, gt, "mixture")
    a = evalkit.compute_metrics(inp, est, gt)
    b = evalkit.compute_metrics(inp, est, gt, metrics="host")
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    np.testing.assert_array_equal(a[0], evalkit.bss_eval_sdr(gt, inp))


def test_marked_items_are_recomputed_on_the_host():
    refs, ests = cases.make_batch(5, [2, 1, 0, 3], 400)
    want = [np.stack([evalkit.bss_eval_sdr(r, e[s], 16) for s in range(2)]) if r.shape[0] else np.zeros((2, 0))
            for r, e in zip(refs, ests)]
    seen = []
    got, redone = evalkit.bss_eval_sdr_batch(refs, ests, flen=16, op=_stand_in({1, 3}, seen))
    assert redone == [1, 3] and len(seen) == 1
    assert seen[0] == ((6, 400), (2, 6, 400), [2, 1, 0, 3], 16)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == np.float64 and g.tobytes() == w.tobytes()
    # several calls: the marks are per call, the reported items per batch
    seen = []
    budget = evalkit.bss_workspace_bytes([2, 1, 0, 3], 2, 400, 16) - 1
    got, redone = evalkit.bss_eval_sdr_batch(refs, ests, flen=16, op=_stand_in({0}, seen), budget=budget)
    assert [s[2] for s in seen] == [[2, 1, 0], [3]] and redone == [0, 3]
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    # nothing marked, one sample
    one = evalkit.bss_eval_sdr_device(refs[3], ests[3], flen=16, op=_stand_in(set(), []))
    assert one.tobytes() == want[3].tobytes()
    assert evalkit.bss_eval_sdr_batch([], []) == ([], [])


def test_batch_shape_errors():
    refs, ests = cases.make_batch(5, [2, 1], 400)
    op = _stand_in(set(), [])
    with pytest.raises(ValueError, match="estimate sets for"):
        evalkit.bss_eval_sdr_batch(refs, ests[:1], op=op)
    with pytest.raises(ValueError, match="do not go with"):
        evalkit.bss_eval_sdr_batch(refs, [ests[0], ests[1][:1]], flen=16, op=op)       # another R
    with pytest.raises(ValueError, match="do not go with"):
        evalkit.bss_eval_sdr_batch(refs, [ests[0], ests[1][:, :, :399]], flen=16, op=op)
    with pytest.raises(ValueError, match="do not go with"):
        evalkit.bss_eval_sdr_batch(refs, [ests[0][0], ests[1][0]], flen=16, op=op)     # [S, T] is not [R, S, T]
    with pytest.raises(ValueError, match="fewer than flen"):
        evalkit.bss_eval_sdr_batch(refs, ests, flen=512, op=op)


# ---- the C entry point refuses on the host, before the first launch: host memory stands in for every pointer ---------
_call = functools.partial(c_call, "asw_bss_eval_sdr")


@pytest.mark.parametrize("kw,message", [
    (dict(null="ref"), "null pointer"), (dict(null="est"), "null pointer"), (dict(null="sdr"), "null pointer"),
    (dict(null="ws"), "null pointer"), (dict(null="status"), "null status"), (dict(null="counts"), "null counts"),
    (dict(K=-1), "K = -1 < 0"), (dict(R=0), "R = 0 < 1"),
    (dict(flen=0), "flen = 0 outside"), (dict(flen=1025, T=2000, counts=(1,)), "flen = 1025 outside"),
    (dict(T=7), "T = 7 outside flen = 8"),
    (dict(counts=(2, -1)), r"counts\[1\] = -1 outside 0..16"), (dict(counts=(17,)), r"counts\[0\] = 17 outside 0..16"),
    (dict(counts=(1, 9), flen=1000, T=1000), "item 1: 9 references of 1000 taps make a system of order 9000 > 8192"),
    (dict(ws_delta=-1), "too small"), (dict(ws_shift=4), "not 8-byte aligned"),
])
def test_c_refusals(kw, message):
    rc, msg, need = _call(**kw)
    assert rc == -1
    assert re.search(message, msg), msg


def test_c_workspace_query_refuses_like_the_call():
    L = native.lib()
    c = (ctypes.c_int32 * 2)(2, 17)
    assert L.asw_bss_eval_sdr_workspace_bytes(c, 2, 2, 100, 8) == 0
    assert "counts[1] = 17" in L.asw_last_error().decode()
    assert L.asw_bss_eval_sdr_workspace_bytes(c, 1, 2, 100, 8) > 0


def test_c_empty_batch_launches_nothing():
    rc, _msg, need = _call(counts=(), K=0)
    assert rc == 0 and need == 0
    # K = 0 looks at no pointer at all
    assert native.lib().asw_bss_eval_sdr(None, None, None, 0, 1, 10, 5, None, None, None, 0, None) == 0
