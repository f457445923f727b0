"""GPU: geometry tables built on the device (csrc/geometry_kernels.hip, ``geometry="device"``) and the per-mixture
arrays of the batch path (``geometries=``).

1. against the reference's own tables (fixture g7);
2. against the host build on g7, four desk arrays (seeds 2000-2003), the 16-microphone array of configs[4] and the
   full region of interest: every integer table equal, every float table bit-identical (``MAX_ULP``);
3. the reference's patches (fixture g8) from a device-built node;
4. the whole search on the five-speaker reverberant scene, device-built against host-built;
5. a batch of mixtures recorded with different arrays against the per-mixture setup + forward loop;
6. two device builds of one geometry are bit-identical.
Needs an MI355X."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FULL_ROI = [-2.2, 2.25, 0.0, 6.2, 0.0, 0.9]
# The float tables are expected bit-identical to numpy's: same float64 expression order, IEEE sqrt and divide, no fma.
# Measured on the MI355X: 0 ulp on every table of every geometry below.
MAX_ULP = 0
FLOAT_TABLES = ("_planes_5", "_planes_1", "Offset_5", "Offset_1", "tau", "tops_delta", "grids", "dis_matrix")
INT_TABLES = ("POWER_INDEX", "_valid_flat", "_valid_cid")


def _array(mics, roi, geometry):
    from acousticswarms_speech_amd.mic_array import MicArray
    with redirect_stdout(io.StringIO()):
        return MicArray(np.asarray(mics), Spk_Range=list(roi), device="cuda", geometry=geometry)


def _ulps(got, want):
    """largest difference in units of the last place of the larger magnitude"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    d = np.abs(got - want)
    if not d.any():
        return 0.0
    return float(np.max(d / np.spacing(np.maximum(np.abs(got), np.abs(want)))))


def _geometries(golden):
    from acousticswarms_speech_amd.scenes import make_scene
    g7 = golden("g7_srp_map")
    out = [("g7", g7["mics"], list(g7["roi"]))]
    for seed in range(2000, 2004):
        sc = make_scene(seed, 5, 7, 4000)
        out.append((f"seed {seed}", sc.mic_positions, sc.speaker_range))
    sc16 = make_scene(1010, 5, 16, 4000)
    out.append(("16 mics", sc16.mic_positions, sc16.speaker_range))
    out.append(("full ROI", make_scene(1010, 5, 7, 4000).mic_positions, FULL_ROI))
    return out


def _assert_same_node(dev, host, name):
    for t in INT_TABLES:
        a, b = getattr(dev, t), getattr(host, t)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, t)
        np.testing.assert_array_equal(a, b, err_msg=f"{name}: {t}")
    assert len(dev.clusters) == len(host.clusters) == dev.SRP_times == host.SRP_times
    np.testing.assert_array_equal(dev.clusters.offsets, np.stack([c.sample_offset for c in host.clusters]))
    np.testing.assert_array_equal(dev.clusters.sizes(), [c.cluster_size() for c in host.clusters])
    # the CSR member lists: ascending voxel index within a cluster, which is the host's member order
    want = np.concatenate([np.ravel_multi_index(tuple(c.index.T), (host.Lx, host.Ly, host.Lz)) for c in host.clusters])
    np.testing.assert_array_equal(dev.clusters.members, want)
    for g in (0, len(host.clusters) // 2, len(host.clusters) - 1):
        np.testing.assert_array_equal(dev.clusters[g].grids, host.clusters[g].grids)
        np.testing.assert_array_equal(dev.clusters[g].index, host.clusters[g].index)
    worst = {t: _ulps(getattr(dev, t), getattr(host, t)) for t in FLOAT_TABLES}
    print(f"{name}: G = {len(host.clusters)}, label sweeps {dev.label_sweeps}, ulp differences {worst}, "
          f"build split {dev.build_times}")
    for t, u in worst.items():
        assert u <= MAX_ULP, f"{name}: {t} differs from the host build by {u} ulp"
    np.testing.assert_array_equal(np.asarray(dev.Pos_5), host.Pos_5)
    assert dev.POWER_MAP.shape == host.POWER_MAP.shape and not dev.POWER_MAP.any()


def test_device_tables_match_the_reference(golden):
    g7 = golden("g7_srp_map")
    node = _array(g7["mics"], g7["roi"], "device").SRP_node
    np.testing.assert_array_equal(node.clusters.offsets, g7["cluster_offsets"])
    np.testing.assert_array_equal(np.stack([c.sample_offset for c in node.clusters]), g7["cluster_offsets"])
    np.testing.assert_array_equal(np.array([c.cluster_size() for c in node.clusters]), g7["cluster_sizes"])
    np.testing.assert_array_equal(node.POWER_INDEX, g7["power_index"])
    assert node.grids.shape == g7["grids"].shape
    np.testing.assert_allclose(node.grids, g7["grids"], rtol=0, atol=1e-12)       # the host build's own bar


def test_device_tables_equal_the_host_build(golden):
    for name, mics, roi in _geometries(golden):
        _assert_same_node(_array(mics, roi, "device").SRP_node, _array(mics, roi, "host").SRP_node, name)


def test_device_tables_stay_on_the_device(golden):
    """tau / tops_delta of a device-built node are not uploaded again; the twiddles are uploaded once per device."""
    g7 = golden("g7_srp_map")
    a, b = _array(g7["mics"], g7["roi"], "device").SRP_node, _array(g7["mics"], g7["roi"], "host").SRP_node
    ta, tb = a._device_tables(torch.device("cuda")), b._device_tables(torch.device("cuda"))
    assert ta["tau"] is a._geom_dev["tau"] and ta["delta"] is a._geom_dev["delta"]
    assert ta["tw"] is tb["tw"]
    assert torch.equal(ta["tau"], tb["tau"]) and torch.equal(ta["delta"], tb["delta"])


def test_reference_patches_from_a_device_built_node(golden):
    g7, g8 = golden("g7_srp_map"), golden("g8_srp_patches")
    node = _array(g7["mics"], g7["roi"], "device").SRP_node
    node.set_map(g7["srp_map"])
    with redirect_stdout(io.StringIO()):
        peaks = node.find_valid_peak_new()
        patches = node.local_source_adaptive()
    assert peaks == g8["peak_index"].tolist()
    assert len(patches) == g8["offsets"].shape[0]
    np.testing.assert_array_equal(np.stack([p.sample_offset for p in patches]), g8["offsets"])
    np.testing.assert_array_equal(np.stack([p.width_list for p in patches]), g8["widths"])
    np.testing.assert_array_equal(np.array([p.area_size() for p in patches]), g8["npoints"])
    np.testing.assert_allclose(np.stack([p.peak_pos for p in patches]), g8["peaks"], atol=1e-12)
    np.testing.assert_allclose(np.stack([p.area_points.mean(1) for p in patches]), g8["centroid"], atol=1e-9)


def test_two_device_builds_are_bit_identical(golden):
    _name, mics, roi = _geometries(golden)[2]
    a, b = _array(mics, roi, "device").SRP_node, _array(mics, roi, "device").SRP_node
    for t in INT_TABLES + FLOAT_TABLES:
        assert getattr(a, t).tobytes() == getattr(b, t).tobytes(), t
    for t in ("offsets", "bounds", "members"):
        assert getattr(a.clusters, t).tobytes() == getattr(b.clusters, t).tobytes(), t
    assert torch.equal(a._geom_dev["tau"], b._geom_dev["tau"]) and torch.equal(a._geom_dev["delta"], b._geom_dev["delta"])


# ------------------------------------------------------------------------------ with the spot network
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


def test_whole_search_device_built_equals_host_built(spot):
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 7, 24000, reverb=True)
    mix_t = torch.from_numpy(sc.mix)
    res = {}
    for mode in ("device", "host"):
        jm = JointModel(spot, None, device="cuda")
        with redirect_stdout(io.StringIO()):
            jm.setup(sc.mic_positions, sc.speaker_range, geometry=mode)
        assert jm.Mic_processor.SRP_node.geometry == mode
        res[mode] = _forward(jm, mix_t)
    (got, trace_got), (want, trace_want) = res["device"], res["host"]
    assert len(want[2]) >= 1
    assert got[2] == want[2] and got[3] == want[3]                     # names, spot_times
    assert trace_got == trace_want                                     # every hard decision
    np.testing.assert_array_equal(got[0], want[0])                     # bit-equal, as the tables are
    np.testing.assert_array_equal(got[1], want[1])


def _same_search_result(got, want):
    """the bar of test_config3_mixture_batch_equals_plain_loop: names and spot counts exact, positions 1e-6 m,
    powers 1e-5"""
    assert got[2] == want[2] and got[3] == want[3]
    np.testing.assert_allclose(got[0], want[0], atol=1e-6)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-5)


def test_batch_with_one_array_per_mixture_equals_the_plain_loop(spot):
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.shard import localize_batch
    scenes = [make_scene(2000 + k, 5, 7, 24000) for k in range(4)]
    scenes.append(scenes[1])                                           # the array (and mixture) of entry 1 again
    assert len({s.mic_positions.tobytes() for s in scenes}) == 4
    mixes = [torch.from_numpy(s.mix) for s in scenes]
    geometries = [(s.mic_positions, s.speaker_range) for s in scenes]

    loop = JointModel(spot, None, device="cuda")                       # the per-mixture setup + forward loop, host tables
    want = []
    for s, m in zip(scenes, mixes):
        with redirect_stdout(io.StringIO()):
            loop.setup(s.mic_positions, s.speaker_range)
        want.append(_forward(loop, m)[0])
    assert all(len(w[2]) >= 1 for w in want)

    def summary(out):
        return [(r["centres"], r["powers"], list(r["names"]), int(r["spot_times"])) for r in out]

    for mode in ("device", "host"):
        jm = JointModel(spot, None, device="cuda", geometry=mode)
        with redirect_stdout(io.StringIO()):
            got = summary(localize_batch(jm, mixes, geometries=geometries, concurrent=2))
        assert len(got) == 5
        for g, w in zip(got, want):
            _same_search_result(g, w)
        assert jm.geometry_stats == {"builds": 4, "hits": 1}, jm.geometry_stats      # the repeated array is built once
        assert jm.Mic_processor is None                                # no setup() was needed, none was faked
        with redirect_stdout(io.StringIO()):
            plain = summary(localize_batch(jm, mixes, geometries=geometries, concurrent=1))
        for g, w in zip(plain, want):
            _same_search_result(g, w)
        assert jm.geometry_stats == {"builds": 4, "hits": 6}, jm.geometry_stats      # all five found in the LRU
        assert jm.Mic_processor is None and jm.previous_config is None
