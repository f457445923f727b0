"""GPU: the fine stage's clustering on the device (``asw_fine_clusters`` in csrc/cluster_kernels.hip,
``torch.ops.asw.fine_clusters``) and the search mode made of it (``MicArray(clustering="device")``).

1. the op against its numpy statement (``fine_cluster.fine_clusters_f64``) on the smallest shapes that reach each path
   of the two kernels -- fewer samples than threads, group sizes around the 8 x 8 tile, more heads than a wavefront
   has lanes, hundreds of groups, rows that are not 16-byte aligned, the full length --, and on the case counted by hand;
2. two calls are bit-identical, and the result does not depend on what the outputs or the workspace held;
3. the whole search and a batch of four mixtures with ``clustering="device"`` against ``clustering="host"``, and what
   the fine stage calls in device mode.
The bound is equality everywhere: ``order``, ``label`` and ``gram`` byte for byte.  Needs an MI355X."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests.fine_cluster_cases import hand_case, make_call, statement

pytestmark = pytest.mark.gpu

R = 8                     # the Gram kernel's tile edge (GR in csrc/cluster_kernels.hip)


def _ops():
    from acousticswarms_speech_amd import native
    return native.torch_ops()


def _check(call, y_dev=None, label="", want=None):
    """The op on one call's inputs (or on the device tensor that holds its waveforms) against the statement: every
    byte of order, label and gram."""
    order_w, label_w, gram_w = statement(call) if want is None else want
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    y = dev(call["waves"]) if y_dev is None else y_dev
    args = (y, torch.from_numpy(call["bounds"]), dev(call["energies"]), dev(call["gate"]), dev(call["group_gate"]),
            float(call["min_trigger"]))
    order, lab, gram = _ops().fine_clusters(*args, -4.0, True)
    N = call["waves"].shape[0]
    assert order.dtype == lab.dtype == torch.int32 and gram.dtype == torch.float64
    assert tuple(order.shape) == tuple(lab.shape) == (N,) and tuple(gram.shape) == gram_w.shape
    order, lab, gram = order.cpu().numpy(), lab.cpu().numpy(), gram.cpu().numpy()
    heads = int(np.sum(lab == np.arange(N)))
    print(f"{label} N={N} T={call['waves'].shape[1]} G={len(call['bounds']) - 1}: {heads} heads, "
          f"{int(np.sum(lab >= 0)) - heads} joined, {int(np.sum(lab < 0))} skipped")
    assert gram.tobytes() == gram_w.tobytes(), f"{label}: gram differs in {np.count_nonzero(gram != gram_w)} of {gram.size}"
    np.testing.assert_array_equal(order, order_w)
    np.testing.assert_array_equal(lab, label_w)
    order2, lab2, gram2 = _ops().fine_clusters(*args)                  # the defaults: -4 dB, no gram
    assert gram2.numel() == 0 and torch.equal(order2.cpu(), torch.from_numpy(order_w)) and torch.equal(lab2.cpu(), torch.from_numpy(label_w))
    return order_w, label_w, gram_w


# ---------------------------------------------------------------- the op against the statement
@pytest.mark.parametrize("T", [1, 255, 256, 257, 1000])
def test_shapes_around_the_tile_and_the_workgroup(T):
    """Group sizes 0, 1, 2, R, R + 1 (the tile edge) and 2 R + 1 in one call, one group closed; one sample, one short of
    a sample per thread, one each, one more, and some.  (T = 1: every mean-removed row is 0 and every power equal -- the
    order is the index order, and the 0 / 0 similarities compare false on both sides, so everyone is a head.)"""
    call = make_call(10 + T, [0, 1, 2, R, 0, R + 1, 2 * R + 1, 3], T, closed=(3,))
    _o, lab, _g = _check(call, label="tile edges")
    if T >= 255:
        assert np.all(lab[3:3 + R] == -1) and np.any(lab >= 0) and np.any(lab[3 + R:] == -1)


def test_case_counted_by_hand():
    call, order_w, label_w, gram_w = hand_case()
    _check(call, label="by hand", want=(order_w, label_w, gram_w))


def test_more_heads_than_a_wavefront_has_lanes():
    """70 rows of independent noise: about -30 dB against each other, 70 heads -- the candidates from the 65th on
    are tested against the heads in two rounds of 64 lanes."""
    rng = np.random.default_rng(70)
    rows = rng.standard_normal((70, 1000)).astype(np.float32)
    rows -= rows.mean(axis=1, keepdims=True)
    call = make_call(70, None, 1000, groups=[rows])
    call["gate"][:] = 0.0
    call["min_trigger"] = 0.0
    _o, lab, _g = _check(call, label="70 heads")
    assert np.array_equal(lab, np.arange(70))
    # ... and a 71st row that copies the LAST head created: found in the second round only
    last = int(np.argmin(call["energies"][:, 0]))
    copy = (0.5 * rows[last] + 0.01 * rng.standard_normal(1000)).astype(np.float32)
    call = make_call(70, None, 1000, groups=[np.concatenate([rows, (copy - copy.mean())[None]])])
    call["gate"][:] = 0.0
    call["min_trigger"] = 0.0
    _o, lab, _g = _check(call, label="70 heads and a copy")
    assert lab[70] == last and np.array_equal(lab[:70], np.arange(70))


def test_degenerate_groups():
    """40 noisy copies of one source that all join the loudest; a closed group between two open ones; duplicated rows
    (equal powers: visited by ascending index, the first of each pair is the head or joins first)."""
    rng = np.random.default_rng(40)
    src = rng.standard_normal(1500)
    copies = np.stack([(g * src + 0.05 * rng.standard_normal(1500)).astype(np.float32) for g in rng.uniform(0.3, 1.0, 40)])
    copies -= copies.mean(axis=1, keepdims=True)
    other = rng.standard_normal((5, 1500)).astype(np.float32)
    other -= other.mean(axis=1, keepdims=True)
    dup = np.concatenate([other[:3], other[:3], other[3:]])            # rows 0-2 twice
    call = make_call(41, None, 1500, groups=[copies, other, dup], closed=(1,))
    call["gate"][:] = 0.0
    call["min_trigger"] = 0.0
    order, lab, _g = _check(call, label="degenerate")
    loudest = int(np.argmax(call["energies"][:40, 0]))
    assert np.all(lab[:40] == loudest) and np.all(lab[40:45] == -1)
    assert lab[45:].tolist() == [45, 46, 47, 45, 46, 47, 51, 52]
    pos = {int(k): r for r, k in enumerate(order[45:])}
    assert all(pos[45 + i] + 1 == pos[48 + i] for i in range(3))       # each duplicate right after its original


def test_many_small_groups():
    rng = np.random.default_rng(300)
    sizes = [int(n) for n in rng.integers(1, 6, 300)]
    _o, lab, _g = _check(make_call(300, sizes, 300, closed=tuple(range(0, 300, 7))), label="300 groups")
    assert np.sum(lab >= 0) > 100


@pytest.mark.parametrize("T", [257, 1001])
def test_odd_lengths_misalign_every_row_but_the_first(T):
    _check(make_call(T, [3, R + 2, 5], T), label="odd T")


def test_aligned_length_on_a_misaligned_base():
    """T % 4 == 0 but the tensor starts 4 bytes into its allocation: no row is 16-byte aligned."""
    call = make_call(12, [4, R + 3, 2], 1000)
    N = call["waves"].shape[0]
    buf = torch.zeros(N * 1000 + 4, device="cuda")
    y = buf[1:1 + N * 1000].view(N, 1000)
    y.copy_(torch.from_numpy(call["waves"]))
    assert y.is_contiguous() and y.data_ptr() % 16 == 4
    _check(call, y_dev=y, label="base + 4")


_FULL = {}


def _full_length():
    """One call at the search's length, made once: T = 48 000, three groups of about 24 rows."""
    if not _FULL:
        call = make_call(48, [23, 24, 26], 48000)
        _FULL["call"], _FULL["want"] = call, statement(call)
    return _FULL["call"], _FULL["want"]


def test_full_length():
    call, want = _full_length()
    _o, lab, _g = _check(call, label="full length", want=want)
    assert np.sum(lab == np.arange(len(lab))) >= 3 and np.sum(lab >= 0) > np.sum(lab == np.arange(len(lab)))


# ---------------------------------------------------------------- what the buffers held
def test_outputs_and_workspace_may_hold_anything_and_two_calls_are_identical():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    call, (order_w, label_w, gram_w) = _full_length()
    N, T = call["waves"].shape
    G = len(call["bounds"]) - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    y, en, gate, ggate = dev(call["waves"]), dev(call["energies"]), dev(call["gate"]), dev(call["group_gate"])
    bounds = np.ascontiguousarray(call["bounds"], dtype=np.int32)
    ws_bytes = L.asw_fine_clusters_workspace_bytes(c_void_p(bounds.ctypes.data), G)
    assert ws_bytes >= gram_w.size * 8 + (2 * (G + 1) + N) * 4
    ratio = 10.0 ** (-4.0 / 10.0)
    got = []
    for fill, with_gram in ((0xFF, True), (0x00, True), (0xFF, False), (0xFF, True)):
        order = torch.full((N * 4,), fill, dtype=torch.uint8, device="cuda").view(torch.int32)
        lab = torch.full((N * 4,), fill, dtype=torch.uint8, device="cuda").view(torch.int32)
        gram = torch.full((gram_w.size * 8,), fill, dtype=torch.uint8, device="cuda").view(torch.float64)
        ws = torch.full((ws_bytes + 8,), fill, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 8 == 0
        native.check(L.asw_fine_clusters(c_void_p(y.data_ptr()), N, T, c_void_p(bounds.ctypes.data), G,
                                         c_void_p(en.data_ptr()), c_void_p(gate.data_ptr()), c_void_p(ggate.data_ptr()),
                                         float(call["min_trigger"]), ratio, c_void_p(ws.data_ptr()), ws_bytes,
                                         c_void_p(order.data_ptr()), c_void_p(lab.data_ptr()),
                                         c_void_p(gram.data_ptr()) if with_gram else None, native.current_stream()))
        torch.cuda.synchronize()
        assert ws[ws_bytes:].cpu().numpy().tolist() == [fill] * 8      # nothing is written past the stated size
        if with_gram:
            got.append((order.cpu().numpy().tobytes(), lab.cpu().numpy().tobytes(), gram.cpu().numpy().tobytes()))
        else:                                                          # the Gram matrix lives in the workspace then
            assert (order.cpu().numpy().tobytes(), lab.cpu().numpy().tobytes()) == (order_w.tobytes(), label_w.tobytes())
            assert ws[:gram_w.size * 8].view(torch.float64).cpu().numpy().tobytes() == gram_w.tobytes()
    assert got[0] == got[1] == got[2] == (order_w.tobytes(), label_w.tobytes(), gram_w.tobytes())


def test_empty_calls_and_adapter_checks():
    ops = _ops()
    f64 = dict(dtype=torch.float64, device="cuda")
    y0 = torch.zeros((0, 500), device="cuda")
    for bounds, G in (([0, 0, 0, 0], 3), ([0], 0)):
        order, lab, gram = ops.fine_clusters(y0, torch.tensor(bounds, dtype=torch.int32), torch.zeros((0, 2), **f64),
                                             torch.zeros(0, **f64), torch.zeros(G, **f64), 0.1, -4.0, True)
        assert tuple(order.shape) == tuple(lab.shape) == tuple(gram.shape) == (0,) and order.is_cuda
    y = torch.zeros((3, 500), device="cuda")
    b = torch.tensor([0, 1, 3], dtype=torch.int32)
    en, gate, gg = torch.zeros((3, 2), **f64), torch.zeros(3, **f64), torch.zeros(2, **f64)
    ops.fine_clusters(y, b, en, gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="must be Float"):
        ops.fine_clusters(y.double(), b, en, gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="must be Double"):
        ops.fine_clusters(y, b, en.float(), gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.fine_clusters(torch.zeros((500, 3), device="cuda").t(), b, en, gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="CPU Int"):
        ops.fine_clusters(y, b.cuda(), en, gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="CPU Int"):
        ops.fine_clusters(y, b.long(), en, gate, gg, 0.1)
    with pytest.raises(RuntimeError, match=r"energies must be \[N, 2\]"):
        ops.fine_clusters(y, b, en[:2].contiguous(), gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="gate must be"):
        ops.fine_clusters(y, b, en, gate[:2].contiguous(), gg, 0.1)
    with pytest.raises(RuntimeError, match="group_gate must be"):
        ops.fine_clusters(y, b, en, gate, gate, 0.1)
    with pytest.raises(RuntimeError, match="end at the number of rows"):
        ops.fine_clusters(y, torch.tensor([0, 1, 2], dtype=torch.int32), en, gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="decrease"):
        ops.fine_clusters(y, torch.tensor([0, 4, 3], dtype=torch.int32), en, gate, gg, 0.1)
    with pytest.raises(RuntimeError, match="at least one sample"):
        ops.fine_clusters(torch.zeros((3, 0), device="cuda"), b, en, gate, gg, 0.1)


def test_spot_model_surface_returns_device_tensors():
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.spot import SpotModel
    m = SpotModel(SMALL)                                     # the clustering needs no weights
    call, order_w, label_w, _gram = hand_case()
    y, en = torch.from_numpy(call["waves"]).cuda(), torch.from_numpy(call["energies"]).cuda()
    order, lab = m.fine_clusters(y, call["bounds"], en, call["gate"], call["group_gate"], call["min_trigger"])
    assert order.is_cuda and lab.is_cuda
    np.testing.assert_array_equal(order.cpu().numpy(), order_w)
    np.testing.assert_array_equal(lab.cpu().numpy(), label_w)


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
    """Calls of the scorer's ``pair_sisdr`` made from inside the fine stage, and of ``fine_clusters``."""
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.spot import SpotModel
    counts = {"pair_sisdr_fine": 0, "fine_clusters": 0, "in_fine": 0}
    fine, pair, clus = MicArray.Spotform_Small_Patch_Parallel, SpotModel.pair_sisdr, SpotModel.fine_clusters

    def fine_stage(self, *a, **kw):
        counts["in_fine"] += 1
        try:
            return fine(self, *a, **kw)
        finally:
            counts["in_fine"] -= 1

    def pair_sisdr(self, waves):
        counts["pair_sisdr_fine"] += 1 if counts["in_fine"] else 0
        return pair(self, waves)

    def fine_clusters(self, *a, **kw):
        counts["fine_clusters"] += 1
        return clus(self, *a, **kw)
    monkeypatch.setattr(MicArray, "Spotform_Small_Patch_Parallel", fine_stage)
    monkeypatch.setattr(SpotModel, "pair_sisdr", pair_sisdr)
    monkeypatch.setattr(SpotModel, "fine_clusters", fine_clusters)
    return counts


@pytest.mark.parametrize("segments", ["host", "device"])
def test_whole_search_with_device_clustering_equals_host_clustering(spot, monkeypatch, segments):
    """The configs[2] scene (seed 1010, 5 talkers, 7 mics, 48 000 samples, reverberant).  The two modes differ by the
    order of the Gram sums and the missing logarithm, about 1e-12 dB on similarities that lie whole decibels from the
    threshold: every hard decision, the talkers, their positions and powers and spot_times are equal outright.  In
    device mode the fine stage never calls ``pair_sisdr`` and makes at most one ``fine_clusters`` call per chunk."""
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.mic_array import FINE_CHUNK_EDGES
    from acousticswarms_speech_amd.scenes import make_scene
    counts = _count_calls(monkeypatch)
    sc = make_scene(1010, 5, 7, 48000, reverb=True)
    mix_t = torch.from_numpy(sc.mix)
    jm = JointModel(spot, None, device="cuda", segments=segments)
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, sc.speaker_range)
    want, trace_want = _forward(jm, mix_t)
    assert counts["fine_clusters"] == 0 and counts["pair_sisdr_fine"] >= 3
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, sc.speaker_range, clustering="device")
    mp = jm.Mic_processor
    assert mp.clustering == "device" and mp.segments == segments
    counts["pair_sisdr_fine"] = 0
    got, trace_got = _forward(jm, mix_t)
    print(f"{len(trace_want['fine_clusters'])} open coarse patches, "
          f"{sum(len(c) for c in trace_want['fine_clusters'].values())} cluster heads, {len(want[2])} talkers, "
          f"{counts['fine_clusters']} fine_clusters calls")
    assert counts["pair_sisdr_fine"] == 0
    assert 1 <= counts["fine_clusters"] <= len(FINE_CHUNK_EDGES) - 1
    assert len(want[2]) >= 1 and sum(len(c) for c in trace_want["fine_clusters"].values()) >= 10
    assert trace_got["fine_clusters"] == trace_want["fine_clusters"]
    assert [list(c) for c in trace_got["fine_clusters"].values()] == [list(c) for c in trace_want["fine_clusters"].values()]
    assert trace_got == trace_want
    assert got[2] == want[2] and got[3] == want[3]
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert len(mp._dev_cache) == sum(len(c) for c in trace_want["fine_clusters"].values())


def test_batch_of_four_mixtures_with_device_clustering(spot):
    """``localize_batch`` with clustering="device" against the per-mixture loop with clustering="host".  The plain loop
    (``concurrent=1``) is the same arithmetic and must be equal; with ``concurrent=2`` a candidate's energy moves by
    about 1e-6 with the internal batch it lands in, the bar of test_config3_mixture_batch_equals_plain_loop."""
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.shard import localize_batch
    first = make_scene(2000, 5, 7, 24000)
    scenes = [make_scene(2000 + k, 5, 7, 24000, mic_positions=first.mic_positions) for k in range(4)]
    mixes = [torch.from_numpy(s.mix) for s in scenes]
    jm = JointModel(spot, None, device="cuda")
    with redirect_stdout(io.StringIO()):
        jm.setup(first.mic_positions, first.speaker_range)
    want = [_forward(jm, m)[0] for m in mixes]
    jd = JointModel(spot, None, device="cuda", clustering="device")
    with redirect_stdout(io.StringIO()):
        jd.setup(first.mic_positions, first.speaker_range)
        plain = localize_batch(jd, mixes, concurrent=1)
        batched = localize_batch(jd, mixes, concurrent=2)
    assert jd.Mic_processor.clustering == "device" and len(plain) == len(batched) == 4
    for k in range(4):
        r, w = plain[k], want[k]
        assert list(r["names"]) == w[2] and int(r["spot_times"]) == w[3] and len(w[2]) >= 1
        np.testing.assert_array_equal(r["centres"], w[0])
        np.testing.assert_array_equal(r["powers"], w[1])
        r = batched[k]
        assert list(r["names"]) == w[2] and int(r["spot_times"]) == w[3]
        np.testing.assert_allclose(r["centres"], w[0], atol=1e-6)
        np.testing.assert_allclose(r["powers"], w[1], rtol=1e-5)
