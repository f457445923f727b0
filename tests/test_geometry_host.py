"""CPU only: the host-side pieces of the device-built geometry (``geometry="device"``) and of the per-mixture
arrays of the batch path (``geometries=``) -- the lazy cluster sequence and the generated lookup positions against a
host-built node, argument validation of the batch interface, the small LRU of per-mixture arrays, and the argument
checks of the new C entry points (no HIP call is made)."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from acousticswarms_speech_amd import native
from acousticswarms_speech_amd.batching import check_geometries, search_batched
from acousticswarms_speech_amd.joint import JointModel, config_key
from acousticswarms_speech_amd.mic_array import MicArray
from acousticswarms_speech_amd.shard import localize_batch
from acousticswarms_speech_amd.srp import ClusterSeq, LookupPositions, SRPPhat


@pytest.fixture(scope="module")
def host_node(golden):
    g7 = golden("g7_srp_map")
    with redirect_stdout(io.StringIO()):
        ma = MicArray(g7["mics"], Spk_Range=list(g7["roi"]))
    return ma.SRP_node


def _csr_of(node):
    """The CSR arrays a device build hands to ClusterSeq, taken from a host-built node."""
    order = np.argsort(node._valid_cid, kind="stable")
    members = node._valid_flat[order]
    bounds = np.searchsorted(node._valid_cid[order], np.arange(len(node.clusters) + 1))
    offsets = np.stack([c.sample_offset for c in node.clusters])
    return offsets.astype(np.int32), bounds.astype(np.int32), members.astype(np.int32)


def test_lazy_cluster_sequence_equals_the_host_list(host_node):
    node = host_node
    offsets, bounds, members = _csr_of(node)
    seq = ClusterSeq(offsets, bounds, members, node.x_grids, node.y_grids, node.z_grids)
    assert len(seq) == len(node.clusters) == node.grids.shape[0]
    np.testing.assert_array_equal(seq.sizes(), [c.cluster_size() for c in node.clusters])
    n = 0
    for lazy, want in zip(seq, node.clusters):                       # iteration
        np.testing.assert_array_equal(lazy.sample_offset, want.sample_offset)
        assert lazy.sample_offset.dtype == want.sample_offset.dtype
        np.testing.assert_array_equal(lazy.grids, want.grids)        # member points: same values, same order
        np.testing.assert_array_equal(lazy.index, want.index)
        assert lazy.cluster_size() == want.cluster_size()
        np.testing.assert_array_equal(lazy.center_pos(), want.center_pos())
        n += 1
    assert n == len(seq)
    np.testing.assert_array_equal(seq[-1].index, node.clusters[-1].index)
    np.testing.assert_array_equal(seq[np.int64(3)].grids, node.clusters[3].grids)
    assert [c.cluster_size() for c in seq[2:5]] == [c.cluster_size() for c in node.clusters[2:5]]
    with pytest.raises(IndexError):
        seq[len(seq)]


def test_generated_lookup_positions_equal_the_stored_table(host_node):
    node = host_node
    r = node.Range_spk
    for step, stored in ((0.05, node.Pos_5), (0.01, node.Pos_1)):
        pos = LookupPositions(np.arange(r[0], r[1], step), np.arange(r[2], r[3], step), np.arange(r[4], r[5], 0.1))
        assert pos.shape == stored.shape
        idx = np.random.default_rng(0).integers(0, stored.size // 3, 500).astype(np.int32)
        np.testing.assert_array_equal(pos.reshape(-1, 3)[idx], stored.reshape(-1, 3)[idx])
        np.testing.assert_array_equal(pos.reshape(-1, 3)[idx[:0]], stored.reshape(-1, 3)[idx[:0]])
    np.testing.assert_array_equal(np.asarray(LookupPositions(np.arange(r[0], r[1], 0.05), np.arange(r[2], r[3], 0.05),
                                                             np.arange(r[4], r[5], 0.1))), node.Pos_5)


def test_geometry_argument(golden):
    g7 = golden("g7_srp_map")
    with pytest.raises(ValueError):
        SRPPhat(g7["mics"], np.arange(2, 200), list(g7["roi"]), geometry="gpu")
    with pytest.raises(ValueError):
        JointModel(None, geometry="gpu")
    import torch
    if not torch.cuda.is_available():                               # like the maps: no host fallback
        with pytest.raises(RuntimeError), redirect_stdout(io.StringIO()):
            MicArray(g7["mics"], Spk_Range=list(g7["roi"]), geometry="device")
        jm = JointModel(None, geometry="device")
        with pytest.raises(RuntimeError), redirect_stdout(io.StringIO()):
            jm.setup(g7["mics"], list(g7["roi"]))
        assert jm.Mic_processor is None and jm.previous_config is None
    assert config_key(g7["mics"], g7["roi"]) + "|geometry=device" == config_key(g7["mics"], g7["roi"], geometry="device")


def test_batch_interface_rejects_bad_geometries(golden):
    g7 = golden("g7_srp_map")
    geo = (g7["mics"], list(g7["roi"]))
    mixes = [np.zeros((7, 4000), dtype=np.float32) for _ in range(3)]

    class NoDevice:                          # any touch of the model would be device work: there must be none
        def __getattr__(self, name):
            raise AssertionError(f"the model was used ({name}) before the arguments were checked")

    for call in (lambda m, g: localize_batch(NoDevice(), m, geometries=g),
                 lambda m, g: localize_batch(NoDevice(), m, concurrent=1, geometries=g),
                 lambda m, g: search_batched(NoDevice(), m, geometries=g)):
        with pytest.raises(ValueError, match="2 entries for 3 mixtures"):
            call(mixes, [geo, geo])
        with pytest.raises(ValueError, match="share M and T"):
            call(mixes[:2] + [np.zeros((7, 4004), dtype=np.float32)], [geo] * 3)
        with pytest.raises(ValueError, match="share M and T"):
            call(mixes[:2] + [np.zeros((6, 4000), dtype=np.float32)], [geo] * 3)
        with pytest.raises(ValueError, match="mic_positions"):
            call(mixes, [geo, geo, (g7["mics"][:6], list(g7["roi"]))])
        with pytest.raises(ValueError, match="speaker_range"):
            call(mixes, [geo, geo, (g7["mics"], list(g7["roi"])[:4])])
    check_geometries(mixes, None)
    check_geometries(mixes, [geo] * 3)


def test_per_mixture_arrays_come_from_a_small_lru(golden, monkeypatch):
    """mic_array_for builds an array once while it stays cached, evicts the least recently used one, and never runs
    the collector; the plain loop of localize_batch searches each mixture on its own array and hands the model back."""
    import gc
    from acousticswarms_speech_amd import joint
    g7 = golden("g7_srp_map")
    roi = list(g7["roi"])
    built = []

    class FakeArray:
        Prone_method = "SRP"

        def __init__(self, mic_positions, **kw):
            built.append((float(mic_positions[1, 0]), kw["geometry"]))
            self.mics = mic_positions
    monkeypatch.setattr(joint, "MicArray", FakeArray)
    monkeypatch.setattr(joint, "GEOMETRY_CACHE_SIZE", 2)
    monkeypatch.setattr(gc, "collect", lambda *a: pytest.fail("gc.collect() in a per-mixture build"))
    monkeypatch.setattr(gc, "freeze", lambda: pytest.fail("gc.freeze() in a per-mixture build"))
    jm = JointModel(None)
    arrays = [g7["mics"] + np.array([0.01 * k, 0, 0]) for k in range(3)]
    a0 = jm.mic_array_for(arrays[0], roi)
    assert jm.mic_array_for(arrays[0], roi) is a0
    a1 = jm.mic_array_for(arrays[1], roi)
    assert jm.mic_array_for(arrays[0], roi) is a0                    # 0 is now the most recent
    jm.mic_array_for(arrays[2], roi)                                 # evicts 1
    assert jm.mic_array_for(arrays[0], roi) is a0
    assert jm.mic_array_for(arrays[1], roi) is not a1
    assert jm.geometry_stats == {"builds": 4, "hits": 3}
    assert [g for _x, g in built] == ["host"] * 4

    # the plain loop: forward() of mixture k sees the array of geometries[k]
    seen = []
    jm2 = JointModel(None)
    jm2.forward = lambda mix: (seen.append(jm2.Mic_processor.mics), ([], None, None, 0, 0, 0))[1]
    of_setup = FakeArray(g7["mics"] + 1.0, geometry="host")          # stands for the array of setup()
    jm2.Mic_processor, jm2.previous_config = of_setup, "its key"
    mixes = [np.zeros((7, 4000), dtype=np.float32)] * 4
    thr = gc.get_threshold()
    out = localize_batch(jm2, mixes, concurrent=1, geometries=[(arrays[k], roi) for k in (0, 1, 0, 2)])
    assert len(out) == 4 and gc.get_threshold() == thr
    for got, k in zip(seen, (0, 1, 0, 2)):
        np.testing.assert_array_equal(got, arrays[k])
    assert jm2.geometry_stats == {"builds": 3, "hits": 1}
    assert jm2.Mic_processor is of_setup and jm2.previous_config == "its key"


def test_geometry_entry_points_reject_bad_arguments_without_a_gpu():
    from ctypes import byref, c_int, c_void_p
    L = native.lib()
    buf = np.zeros(64)
    p = c_void_p(buf.ctypes.data)                                    # never dereferenced: every call below is refused
    assert L.asw_geom_lookup_planes(None, 4, p, 4, p, 2, p, 7, 343.0, 16000.0, p, None) == -1
    assert b"geom_lookup_planes: null" in L.asw_last_error()
    assert L.asw_geom_lookup_planes(p, 0, p, 4, p, 2, p, 7, 343.0, 16000.0, p, None) == -1
    assert L.asw_geom_lookup_planes(p, 1 << 12, p, 1 << 12, p, 1 << 8, p, 7, 343.0, 16000.0, p, None) == -1
    assert b"int32" in L.asw_last_error()
    assert L.asw_geom_lookup_planes(p, 4, p, 4, p, 2, p, 1, 343.0, 16000.0, p, None) == -1
    assert b"M = 1" in L.asw_last_error()
    assert L.asw_geom_lookup_planes(p, 4, p, 4, p, 2, p, 7, 0.0, 16000.0, p, None) == -1

    assert L.asw_geom_voxel_map(p, 4, p, 4, p, 2, p, 7, p, p, 343.0, 16000.0, 4.0, None, p, p, None) == -1
    assert b"geom_voxel_map: null" in L.asw_last_error()
    assert L.asw_geom_voxel_map(p, 4, p, -4, p, 2, p, 7, p, p, 343.0, 16000.0, 4.0, p, p, p, None) == -1
    assert b"lattice" in L.asw_last_error()
    assert L.asw_geom_voxel_map(p, 4, p, 4, p, 2, p, 7, p, p, 343.0, 16000.0, 0.5, p, p, p, None) == -1
    assert b"resolution" in L.asw_last_error()
    assert L.asw_geom_voxel_map(p, 1 << 10, p, 1 << 10, p, 1 << 10, p, 7, p, p, 343.0, 16000.0, 4.0, p, p, p, None) == -1

    sweeps = c_int()
    assert L.asw_geom_label(p, None, 4, 4, 2, 6, p, p, p, byref(sweeps), None) == -1
    assert b"geom_label: null" in L.asw_last_error()
    assert L.asw_geom_label(p, p, 4, 4, 2, 0, p, p, p, byref(sweeps), None) == -1
    assert b"P = 0" in L.asw_last_error()
    assert L.asw_geom_label(p, p, 4, 0, 2, 6, p, p, p, None, None) == -1

    assert L.asw_geom_workspace_bytes(0) == -1
    assert b"geom_workspace_bytes" in L.asw_last_error()
    assert L.asw_geom_workspace_bytes((1 << 24) + 1) == -1

    counts = (c_int * 2)()
    args = [p, p, p, 4, p, 4, p, 2, p, 7, p, 343.0, p, 1 << 20, p, p, p, p, p, p, p, p, p, counts, None]

    def compact(**change):
        a = list(args)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.asw_geom_compact(*a)
    assert compact(_0=None) == -1 and b"geom_compact: null" in L.asw_last_error()
    assert compact(_20=None) == -1 and b"null output" in L.asw_last_error()
    assert compact(_23=None) == -1
    assert compact(_9=40) == -1 and b"M = 40" in L.asw_last_error()
    assert compact(_3=0) == -1 and b"lattice" in L.asw_last_error()
    assert compact(_13=16) == -1 and b"too small" in L.asw_last_error()
    assert compact(_11=0.0) == -1
