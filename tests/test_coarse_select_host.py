"""CPU only: the statement of the lattice coarse stage's decision (``search.coarse_select_f64``), which
``asw_coarse_select`` reproduces on the GPU (tests/test_gpu_coarse_select.py), the lattice tables and the lazy patch
sequence of ``coarse="device"``, and the mode itself driven by a stand-in scorer that evaluates the statement on CPU
tensors.  Every bound is equality."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import batching, search
from acousticswarms_speech_amd.dense_grid import (LatticePatches, lattice_dis1, lattice_offsets_i32,
                                                  lattice_patches)
from acousticswarms_speech_amd.hostdsp import max_avg_power
from acousticswarms_speech_amd.joint import JointModel, config_key
from acousticswarms_speech_amd.mic_array import FREQ_BINS, LATTICE_METHODS, MicArray
from acousticswarms_speech_amd.scenes import make_scene
from acousticswarms_speech_amd.search import INIT_WIDTH, MAX_BIG_PATCH, binary_search_baseline, coarse_select_f64
from acousticswarms_speech_amd.spot import offsets_from_patches
from acousticswarms_speech_amd.srp import SRPPhat
from tests import coarse_select_cases as cases
from tests.golden.surrogate import SurrogateSpot

SMALL_ROI = [-0.5, 0.5, 1.0, 2.0, 0.1, 0.5]
SMALL_ROI_CUBES = 509                     # width 8, array of make_scene(1010, 5, 7, 24000)
G7_CUBES = 3364


def _array(mics, roi, **kw):
    with redirect_stdout(io.StringIO()):
        return MicArray(np.asarray(mics), Spk_Range=list(roi), **kw)


# ---------------------------------------------------------------- the statement, counted by hand
NAN = float("nan")
HAND_PW = np.array([0.5, 0.02, 0.5, NAN, -0.0, 0.0, 0.001, 0.9])
HAND_DIS1 = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 10.0, 1.0])      # wd = pw except wd[6] = 0.01


def test_case_counted_by_hand():
    sel = lambda **kw: coarse_select_f64(HAND_PW, HAND_DIS1, **{"thr1": 0.008, "relative": False, **kw})
    # the zeros fail (0 < 0.008); cube 6 passes by its distance; the NaN passes and sorts last; 0 before 2 by index
    kept, n_pass, thr = sel(cap=30)
    assert kept.dtype == np.int32 and kept.tolist() == [7, 0, 2, 1, 6, 3] and n_pass == 6 and thr == 0.008
    # cap + 1 pass: the caller's warning condition, and the list is cut
    kept, n_pass, _ = sel(cap=5)
    assert kept.tolist() == [7, 0, 2, 1, 6] and n_pass == 6 and n_pass > 5
    kept, n_pass, _ = sel(cap=6)
    assert kept.tolist() == [7, 0, 2, 1, 6, 3] and not n_pass > 6
    # the best cube masked out: it neither is kept nor counts
    alive = np.array([1, 1, 1, 1, 1, 1, 1, 0])
    kept, n_pass, _ = sel(cap=5, alive=alive)
    assert kept.tolist() == [0, 2, 1, 6, 3] and n_pass == 5
    kept, n_pass, _ = sel(cap=5, alive=alive.astype(bool))
    assert kept.tolist() == [0, 2, 1, 6, 3] and n_pass == 5
    # thr1 = 0: both zeros pass (neither is < 0) and -0.0 at 4 equals 0.0 at 5, so the index decides
    kept, n_pass, thr = sel(cap=30, thr1=0.0)
    assert kept.tolist() == [7, 0, 2, 1, 6, 4, 5, 3] and n_pass == 8 and thr == 0.0
    kept, _, _ = coarse_select_f64(HAND_PW[[0, 5, 4, 1]], np.ones(4), thr1=0.0, relative=False)
    assert kept.tolist() == [0, 3, 1, 2]
    # relative: 0.4 * max wd = 0.36 (the maximum skips the NaN) lies above thr1 = 0.008, so nothing changes ...
    assert sel(cap=30, relative=True)[0].tolist() == [7, 0, 2, 1, 6, 3] and sel(relative=True)[2] == 0.008
    # ... and below thr1 = 1.0, where it is the threshold: 0.02 and 0.01 fail
    stats = {}
    kept, n_pass, thr = sel(cap=30, relative=True, thr1=1.0, stats=stats)
    assert kept.tolist() == [7, 0, 2, 3] and n_pass == 4 and thr == 0.4 * 0.9 and thr != 0.36
    assert stats == {"max_wd": 0.9, "non_finite": 1}
    # without relative the same thr1 keeps only the NaN
    assert sel(cap=30, thr1=1.0)[0].tolist() == [3]
    # every wd NaN: thr = thr1 with and without relative, everything passes in index order
    for rel in (False, True):
        stats = {}
        kept, n_pass, thr = coarse_select_f64([NAN, NAN, NAN], [1.0, 2.0, 3.0], thr1=0.5, relative=rel, cap=2, stats=stats)
        assert kept.tolist() == [0, 1] and n_pass == 3 and thr == 0.5 and np.isnan(stats["max_wd"])
    # +Inf leads, -Inf fails the threshold, both count as not finite
    stats = {}
    kept, n_pass, _ = coarse_select_f64([1.0, np.inf, -np.inf, 2.0], np.ones(4), thr1=0.5, relative=False, stats=stats)
    assert kept.tolist() == [1, 3, 0] and n_pass == 3 and stats["non_finite"] == 2 and stats["max_wd"] == np.inf
    # the sign of a zero maximum does not depend on the order
    for order in ([0.0, -0.0], [-0.0, 0.0]):
        stats = {}
        coarse_select_f64(order, [1.0, 1.0], thr1=0.5, relative=True, stats=stats)
        assert stats["max_wd"] == 0 and not np.signbit(stats["max_wd"])
    # nothing at all
    kept, n_pass, thr = coarse_select_f64(np.zeros(0), np.zeros(0), thr1=0.25, relative=True)
    assert kept.shape == (0,) and kept.dtype == np.int32 and n_pass == 0 and thr == 0.25
    # the defaults are the loop's constants
    assert coarse_select_f64([1.0], [1.0])[2] == search.SPOT_POWER_THRESHOLD1
    assert coarse_select_f64(np.ones(40), np.ones(40))[0].tolist() == list(range(MAX_BIG_PATCH))
    with pytest.raises(ValueError, match="one shape"):
        coarse_select_f64(np.ones(3), np.ones(4))
    with pytest.raises(ValueError, match="one flag per candidate"):
        coarse_select_f64(np.ones(3), np.ones(3), np.ones(2))
    with pytest.raises(ValueError, match="cap"):
        coarse_select_f64(np.ones(3), np.ones(3), cap=0)


# ---------------------------------------------------------------- against binary_search_baseline
class _Cube(object):
    def __init__(self, c):
        self.c = c

    def center_pos(self):
        return self.c


class _Energies(object):
    """``stage_energies`` finds ``shift_and_score`` and gets the generated energies."""

    def __init__(self, en):
        self.en = en

    def shift_and_score(self, mix, patch_list, Strict=0, keep_waveforms=False):
        assert Strict == 0 and len(patch_list) == self.en.shape[0]
        return self.en


def test_statement_equals_the_host_loop_on_generated_cases(monkeypatch):
    """320 tie-free cases, N = 1..399: the kept indices, ``thr * 1.2`` and the bytes of ``with_dis``.  A third carries a
    ``survivors`` mask, half run with the relative threshold; the scale of the powers varies so that some keep
    nothing, many reach the cap and some end just around it."""
    rng = np.random.default_rng(20261018)
    mic = rng.normal(size=(4, 3))
    tally = {"capped": 0, "empty": 0, "masked": 0, "relative": 0}
    for k in range(320):
        N = int(rng.integers(1, 400))
        scale = [0.0005, 0.004, 0.01, 0.05, 1.0][k % 5]
        pw = rng.permutation(N).astype(np.float64) / N * scale + rng.random() * 1e-4       # distinct by construction
        assert np.unique(pw).shape[0] == N
        centres = rng.normal(size=(N, 3)) * 2.0
        cubes = [_Cube(centres[i]) for i in range(N)]
        alive = (rng.random(N) < 0.6) if k % 3 == 0 else None
        relative = bool(k % 2)
        monkeypatch.setattr(search, "USE_RELATIVE_SPOT_POWER", relative)
        out = io.StringIO()
        with redirect_stdout(out):
            kept_w, with_dis, thr12 = binary_search_baseline(
                None, _Energies(np.stack([pw * 3, pw], axis=1)), cubes, mic,
                survivors=None if alive is None else (lambda p, alive=alive: alive))
        dis1 = np.array([np.linalg.norm(c - mic[0]) + 1 for c in centres])
        kept, n_pass, thr = coarse_select_f64(pw, dis1, alive, relative=relative)
        where = {id(c): i for i, c in enumerate(cubes)}
        assert [where[id(c)] for c in kept_w] == kept.tolist(), k
        assert thr * 1.2 == thr12, k
        assert np.asarray(with_dis, dtype=np.float64).tobytes() == (pw * dis1).tobytes(), k
        assert ("warning too many patch remaining" in out.getvalue()) == (n_pass > MAX_BIG_PATCH), k
        tally["capped"] += n_pass > MAX_BIG_PATCH
        tally["empty"] += n_pass == 0
        tally["masked"] += alive is not None
        tally["relative"] += relative
    assert tally["capped"] >= 100 and tally["empty"] >= 1 and tally["masked"] >= 100 and tally["relative"] == 160, tally


def test_generated_cases_cover_what_they_claim():
    """The generator of the GPU test: the kinds give the counts they are named for (relative off)."""
    for N in (1, 31, 257, 2 * cases.SLICE, 3364):
        for cap in cases.CAPS:
            n_pass = {}
            for kind in cases.KINDS:
                c = cases.make_case(N, cap, kind, False)
                kept, cnt, thr = cases.expected(c, coarse_select_f64)
                assert kept.shape == (cap,) and kept.dtype == cnt.dtype == np.int32 and thr.dtype == np.float64
                assert np.all(kept[min(cap, cnt[0]):] == -1) and np.all(kept[:min(cap, cnt[0])] >= 0)
                n_pass[kind] = int(cnt[0])
                if kind == "nan_inf":
                    assert cnt[1] >= 2 or N < 4
                if kind == "first_slice" and cnt[0]:
                    assert kept[:min(cap, cnt[0])].max() < cases.SLICE
                if kind == "last_slice" and cnt[0]:
                    assert kept[:min(cap, cnt[0])].min() >= ((N - 1) // cases.SLICE) * cases.SLICE
                if kind == "best_removes_top" and N > cap + 1:
                    top = np.argsort(-c["energies"][:, 1], kind="stable")[:cap]
                    assert not set(top.tolist()) & set(kept.tolist())
            assert n_pass["none"] == 0 and n_pass["exact"] == min(N, cap) and n_pass["cap_plus_1"] == min(N, cap + 1)
            assert n_pass["all"] == n_pass["ties"] == n_pass["two_valued"] == n_pass["zeros"] == N
    # with relative the threshold moves with the maximum
    c = cases.make_case(257, 30, "none", True)
    _, cnt, thr = cases.expected(c, coarse_select_f64)
    assert cnt[0] >= 1 and thr[0] == 0.4 * thr[1] and thr[0] < cases.THR1


# ---------------------------------------------------------------- the tables and the lazy sequence
@pytest.fixture(scope="module")
def g7(golden):
    g = golden("g7_srp_map")
    ma = _array(g["mics"], g["roi"], Prone_method="DENSE")
    return ma, ma.SRP_node, ma.SRP_node.lattice


def _same_patch(a, b):
    assert a is not b
    np.testing.assert_array_equal(a.sample_offset, b.sample_offset)
    np.testing.assert_array_equal(a.width_list, b.width_list)
    np.testing.assert_array_equal(a.area_points, b.area_points)
    np.testing.assert_array_equal(a.peak_pos, b.peak_pos)
    assert a.sample_offset.dtype == b.sample_offset.dtype and a.width_list.dtype == b.width_list.dtype
    assert a.area_points.shape == b.area_points.shape and a.num_pair == b.num_pair
    np.testing.assert_array_equal(a.center_pos(), b.center_pos())


def test_tables_and_lazy_patches_on_the_g7_lattice(g7):
    ma, node, lat = g7
    assert lat.n_cubes == G7_CUBES
    want = lattice_patches(node, lat)
    seq = LatticePatches(node, lat)
    assert len(seq) == G7_CUBES and seq.lattice is lat and seq.built == 0 and seq.dis1 is None
    # offsets_i32: what the scorer's own conversion makes of the patch list
    off = lattice_offsets_i32(lat)
    assert off.dtype == np.int32 and off.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(off, offsets_from_patches(want, lat.cells.shape[1]))
    np.testing.assert_array_equal(seq.offsets_i32, off)
    # dis1: the loop's expression per patch, bit for bit
    dis1 = lattice_dis1(lat, ma.mic_positions)
    loop = np.array([np.linalg.norm(p.center_pos() - ma.mic_positions[0]) + 1 for p in want])
    assert dis1.dtype == np.float64 and dis1.tobytes() == loop.tobytes()
    # the node keeps both, built once
    t_off, t_dis1 = node.lattice_tables(ma.mic_positions)
    assert t_off.tobytes() == off.tobytes() and t_dis1.tobytes() == dis1.tobytes()
    assert node.lattice_tables()[0] is t_off and node.lattice_tables()[1] is t_dis1
    # every patch, field by field
    for g, p in enumerate(seq):
        _same_patch(p, want[g])
    assert seq.built == G7_CUBES
    for g in (0, 17, G7_CUBES - 1, -1, -G7_CUBES):
        _same_patch(seq[g], want[g])
    sl = seq[5:40:7]
    assert isinstance(sl, list) and len(sl) == 5
    for p, q in zip(sl, want[5:40:7]):
        _same_patch(p, q)
    assert seq[G7_CUBES:] == [] and seq.built == G7_CUBES + 10
    for bad in (G7_CUBES, -G7_CUBES - 1):
        with pytest.raises(IndexError):
            seq[bad]
    # check_out mutates a patch: the next access is a fresh one, and so are its arrays
    a = seq[0]
    a.check_out(np.zeros(lat.cells.shape[1]))
    assert not np.array_equal(a.width_list, want[0].width_list) or not np.array_equal(a.sample_offset, want[0].sample_offset)
    a.peak_pos[:] = 99.0
    _same_patch(seq[0], want[0])
    np.testing.assert_array_equal(seq.offsets_i32, off)


def test_lazy_patches_on_two_microphones_on_a_line():
    mics = np.array([[0.003, 0.0, 0.0], [0.103, 0.0, 0.0]])
    node = SRPPhat(mic_pos=mics, freq_bins=FREQ_BINS, Range_spk=[-1.0, 1.0, 0.0, 0.01, 0.0, 0.1], grid_size=0.05, FS=48000,
                   n_fft=2048, lattice_width=INIT_WIDTH)
    lat = node.lattice
    want = lattice_patches(node, lat)
    off, dis1 = node.lattice_tables()
    seq = LatticePatches(node, lat, off, dis1)
    assert len(seq) == 2 and off.tolist() == [[-16], [16]] and seq.dis1 is dis1
    for g in range(2):
        _same_patch(seq[g], want[g])
    assert [p.area_size() for p in seq] == [69, 81]
    assert dis1.tobytes() == np.array([np.linalg.norm(p.center_pos() - mics[0]) + 1 for p in want]).tobytes()


# ---------------------------------------------------------------- the mode, with a stand-in scorer
_COARSE_ENERGIES = {}                   # offsets bytes -> energies [N,2]: the surrogate's coarse call is computed once


class _StatementSpot(SurrogateSpot):
    """The surrogate with the two methods of ``coarse="device"`` on CPU tensors: ``score_offsets`` gives the energies the
    host loop (``search.stage_energies``) forms from the surrogate's waveforms, ``coarse_select`` evaluates the
    statement.  ``shift_and_sep`` remembers the coarse energies too, so that host mode and device mode share one
    evaluation of the 509 cubes.  ``count`` counts the calls."""
    device = None

    def __init__(self):
        super().__init__()
        self.count = {"score_offsets": 0, "coarse_select": 0, "coarse_shift_and_sep": 0}

    @staticmethod
    def _energies(sep):
        out = np.empty((sep.shape[0], 2))
        for i in range(sep.shape[0]):
            x = sep[i, :] - np.mean(sep[i, :])
            out[i] = np.sum(x ** 2), max_avg_power(x)
        return out

    def shift_and_sep(self, input_channels, patch_list, Strict=0, save_input=False):
        if Strict != 0:
            return super().shift_and_sep(input_channels, patch_list, Strict, save_input)
        self.count["coarse_shift_and_sep"] += 1
        key = offsets_from_patches(patch_list, len(patch_list[0].sample_offset)).tobytes()
        if key not in _COARSE_ENERGIES:
            sep = super().shift_and_sep(input_channels, patch_list, Strict, save_input)
            _COARSE_ENERGIES[key] = (sep, self._energies(sep))
        else:
            self.calls.append((len(patch_list), Strict))
        return _COARSE_ENERGIES[key][0].copy()

    def score_offsets(self, input_channels, offsets, Strict=0, window=12000):
        self.count["score_offsets"] += 1
        assert Strict == 0 and isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int32
        off = offsets.numpy()
        key = np.ascontiguousarray(off).tobytes()
        if key not in _COARSE_ENERGIES:
            sep = SurrogateSpot.shift_and_sep(self, input_channels, [_Offsets(r) for r in off], 0)
            _COARSE_ENERGIES[key] = (sep, self._energies(sep))
        else:
            self.calls.append((off.shape[0], 0))
        return torch.from_numpy(_COARSE_ENERGIES[key][1].copy())

    def coarse_select(self, en_dev, dis1_dev, best_dev=None, thr1=None, relative=None, rel=0.4, cap=None):
        self.count["coarse_select"] += 1
        N = en_dev.shape[0]
        alive = None if best_dev is None else best_dev.numpy() == np.arange(N)
        stats = {}
        kept, n_pass, thr = coarse_select_f64(
            en_dev.numpy()[:, 1], dis1_dev.numpy(), alive, thr1=search.SPOT_POWER_THRESHOLD1 if thr1 is None else thr1,
            relative=search.USE_RELATIVE_SPOT_POWER if relative is None else relative, rel=rel,
            cap=MAX_BIG_PATCH if cap is None else cap, stats=stats)
        out = np.full(MAX_BIG_PATCH if cap is None else cap, -1, dtype=np.int32)
        out[:kept.shape[0]] = kept
        return (torch.from_numpy(out), torch.tensor([n_pass, stats["non_finite"]], dtype=torch.int32),
                torch.tensor([thr, stats["max_wd"]], dtype=torch.float64))


class _Offsets(object):
    def __init__(self, row):
        self.sample_offset = row


@pytest.fixture(scope="module")
def small():
    sc = make_scene(1010, 5, 7, 24000)
    return sc, torch.from_numpy(sc.mix)


def _search(sc, mix_t, method, coarse):
    spot = _StatementSpot()
    jm = JointModel(spot, coarse=coarse)
    out = io.StringIO()
    with redirect_stdout(out):
        jm.setup(sc.mic_positions, SMALL_ROI, prone_method=method)
        built = []
        ma = jm.Mic_processor
        stage1 = ma.Apply_SRP_PHAT

        def spy(m):                                          # keeps the stage-1 list the forward hands on
            r = stage1(m)
            built.append(r[0])
            return r
        ma.Apply_SRP_PHAT = spy
        patches, _loc, audio, d0, d1, spot_times = jm.forward(mix_t)
    return {"jm": jm, "ma": ma, "spot": spot, "stage1": built[0], "patches": patches, "spot_times": spot_times,
            "stdout": out.getvalue()}


@pytest.mark.parametrize("method", LATTICE_METHODS)
def test_device_mode_equals_host_mode_on_the_small_scene(small, method):
    sc, mix_t = small
    host = _search(sc, mix_t, method, "host")
    dev = _search(sc, mix_t, method, "device")
    hm, dm = host["ma"], dev["ma"]
    assert hm.coarse == "host" and dm.coarse == "device" and dm.SRP_node.lattice.n_cubes == SMALL_ROI_CUBES
    assert isinstance(host["stage1"], list) and isinstance(dev["stage1"], LatticePatches)
    assert len(dev["stage1"]) == len(host["stage1"]) == SMALL_ROI_CUBES
    assert dev["jm"].previous_config == host["jm"].previous_config + "|coarse=device"
    # the coarse stage built the kept patches and nothing else; the decision is the host's
    kept = hm.trace["coarse_kept"]
    assert 1 <= len(kept) <= MAX_BIG_PATCH and dev["stage1"].built == len(kept)
    assert dm.trace == hm.trace and dm.Relative_Threshold == hm.Relative_Threshold
    assert dm.big_spotforming_times == hm.big_spotforming_times == SMALL_ROI_CUBES
    assert dev["spot"].count == {"score_offsets": 1, "coarse_select": 1, "coarse_shift_and_sep": 0}
    assert host["spot"].count == {"score_offsets": 0, "coarse_select": 0, "coarse_shift_and_sep": 1}
    assert dev["spot"].calls == host["spot"].calls
    if method == "DENSE_NMS":
        assert dm.lattice_nms["radius"] == hm.lattice_nms["radius"] == 1
        for k in ("best", "degree"):
            np.testing.assert_array_equal(dm.lattice_nms[k], hm.lattice_nms[k])
            assert dm.lattice_nms[k].dtype == hm.lattice_nms[k].dtype
    else:
        assert dm.lattice_nms is None and hm.lattice_nms is None
    # the warning and every later line of the search
    assert dev["stdout"] == host["stdout"]
    assert ("warning too many patch remaining" in host["stdout"]) == (method == "DENSE")
    # the talkers
    assert len(host["patches"]) >= 1 and int(dev["spot_times"]) == int(host["spot_times"])
    assert [p[3] for p in dev["patches"]] == [p[3] for p in host["patches"]]
    for p, q in zip(dev["patches"], host["patches"]):
        np.testing.assert_array_equal(p[0].center_pos(), q[0].center_pos())
        np.testing.assert_array_equal(p[1], q[1])
        assert p[2] == q[2]
    # the kept patches are the host's, field by field
    again = LatticePatches(dm.SRP_node, dm.SRP_node.lattice)
    want = lattice_patches(hm.SRP_node, hm.SRP_node.lattice)
    for g in kept:
        _same_patch(again[g], want[g])


def test_non_finite_scores_raise_as_in_host_mode(small):
    sc, mix_t = small

    class NanSpot(_StatementSpot):
        def score_offsets(self, *a, **kw):
            en = super().score_offsets(*a, **kw)
            en[7, 1] = float("nan")
            return en

    ma = _array(sc.mic_positions, SMALL_ROI, Prone_method="DENSE_NMS", coarse="device")
    with redirect_stdout(io.StringIO()):
        p1, _ = ma.Apply_SRP_PHAT(mix_t)
        with pytest.raises(ValueError, match="every score must be finite"):
            ma.Spotform_Big_Patch(mix_t, p1, NanSpot())
        # a maximum search that does not object (the GPU's does not look): coarse_select's count decides
        ma.SRP_node.lattice_local_maxima_resident = lambda s, radius=1: (torch.arange(len(p1), dtype=torch.int32),
                                                                         torch.zeros(len(p1), dtype=torch.int32))
        with pytest.raises(ValueError, match="every score must be finite"):
            ma.Spotform_Big_Patch(mix_t, p1, NanSpot())
    assert ma.lattice_nms is None and p1.built == 0


# ---------------------------------------------------------------- the keyword through every layer
def test_keyword_errors_config_key_and_views(small):
    sc, mix_t = small
    roi = SMALL_ROI
    with pytest.raises(ValueError, match='coarse must be "host" or "device"'):
        _array(sc.mic_positions, roi, Prone_method="DENSE", coarse="gpu")
    with pytest.raises(ValueError, match='coarse must be "host" or "device"'):
        JointModel(SurrogateSpot(), coarse="gpu")
    for method in ("SRP", "MUSIC", "TOPS"):
        with pytest.raises(ValueError, match='coarse="device" needs a lattice search'):
            _array(sc.mic_positions, roi, Prone_method=method, coarse="device")
    with pytest.raises(ValueError, match='coarse="device" needs a lattice search'):
        with redirect_stdout(io.StringIO()):
            JointModel(SurrogateSpot(), coarse="device").setup(sc.mic_positions, roi)
    assert config_key(sc.mic_positions, roi) == config_key(sc.mic_positions, roi, coarse="host")
    assert config_key(sc.mic_positions, roi, "DENSE", coarse="device") == config_key(sc.mic_positions, roi, "DENSE") + "|coarse=device"
    assert config_key(sc.mic_positions, roi, "DENSE_NMS", segments="device", clustering="device", global_clustering="device",
                      coarse="device").endswith("|DENSE_NMS|segments=device|clustering=device|global_clustering=device|coarse=device")

    jm = JointModel(_StatementSpot(), coarse="device", segments="device", clustering="device", global_clustering="device")
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, roi, prone_method="DENSE")
        ma = jm.Mic_processor
        assert (ma.coarse, ma.segments, ma.clustering, ma.global_clustering) == ("device",) * 4
        assert jm.previous_config.endswith("|coarse=device")
        jm.setup(sc.mic_positions, roi, prone_method="DENSE")                    # unchanged: reused
        assert jm.Mic_processor is ma
        jm.setup(sc.mic_positions, roi, prone_method="DENSE", coarse="host", segments="host", global_clustering="host")
        assert jm.Mic_processor is not ma and jm.Mic_processor.coarse == "host"
        assert "coarse" not in jm.previous_config
        own = jm.mic_array_for(sc.mic_positions, roi, "DENSE_NMS")
        assert own.coarse == "device" and jm.mic_array_for(sc.mic_positions, roi, "DENSE_NMS") is own
        jm.Mic_processor = own
        jm.use_geometry(sc.mic_positions, roi)
        assert jm.Mic_processor is own and jm.previous_config.endswith("|coarse=device")

    # a view shares the tables and owns what a search writes
    ma = _array(sc.mic_positions, roi, Prone_method="DENSE_NMS", coarse="device")
    view = batching.mixture_view(ma)
    assert view.coarse == "device" and view.SRP_node.lattice_tables()[0] is ma.SRP_node.lattice_tables()[0]
    assert view.SRP_node.lattice_tables_device("cpu") is ma.SRP_node.lattice_tables_device("cpu")
    spot = _StatementSpot()
    with redirect_stdout(io.StringIO()):
        p1, z = view.Apply_SRP_PHAT(mix_t)
        assert isinstance(p1, LatticePatches) and z.shape == (3, 3) and not z.any()
        kept = view.Spotform_Big_Patch(mix_t, p1, spot)
    assert len(kept) == len(view.trace["coarse_kept"]) >= 1 and view.lattice_nms is not None
    assert ma.lattice_nms is None and ma.trace["coarse_kept"] == []
    # the host mode of the same array type still returns the list
    with redirect_stdout(io.StringIO()):
        assert isinstance(_array(sc.mic_positions, roi, Prone_method="DENSE").Apply_SRP_PHAT(mix_t)[0], list)


def test_scorers_the_mode_refuses(small):
    sc, mix_t = small
    ma = _array(sc.mic_positions, SMALL_ROI, Prone_method="DENSE", coarse="device")
    with redirect_stdout(io.StringIO()):
        p1, _ = ma.Apply_SRP_PHAT(mix_t)
        with pytest.raises(RuntimeError, match=r"needs a spot model with score_offsets\(\) and coarse_select\(\)"):
            ma.Spotform_Big_Patch(mix_t, p1, SurrogateSpot())

        class Sharded(_StatementSpot):
            world = 2
        with pytest.raises(RuntimeError, match="runs on one GPU"):
            ma.Spotform_Big_Patch(mix_t, p1, Sharded())
        with pytest.raises(RuntimeError, match="takes the LatticePatches"):
            ma.Spotform_Big_Patch(mix_t, lattice_patches(ma.SRP_node, ma.SRP_node.lattice), _StatementSpot())
    assert p1.built == 0


def test_mixture_scorer_passes_both_methods_through():
    """``MixtureScorer.score_offsets`` sends the host table to the batcher's ``request``; ``coarse_select`` goes to the
    model."""
    seen = {}

    class Model(object):
        device, batch_size = None, 32

        def coarse_select(self, en, dis1, best=None, **kw):
            seen["select"] = (en, dis1, best, kw)
            return "decided"

    class Batcher(object):
        model = Model()
        mixes = torch.zeros(3, 7, 100)

        def request(self, k, offs, strict, window, want_wave):
            seen["request"] = (k, offs, strict, window, want_wave)
            return None, "energies"
    scorer = batching.MixtureScorer(Batcher(), 2)
    assert scorer.host_offsets is True
    table = np.arange(24, dtype=np.int32).reshape(4, 6)
    assert scorer.score_offsets(None, table, Strict=0, window=12000) == "energies"
    k, offs, strict, window, want_wave = seen["request"]
    assert (k, strict, window, want_wave) == (2, 0, 12000, False) and offs.dtype == np.int32
    np.testing.assert_array_equal(offs, table)
    scorer.score_offsets(None, torch.from_numpy(table))
    np.testing.assert_array_equal(seen["request"][1], table)
    with pytest.raises(RuntimeError, match="do not fit"):
        scorer.score_offsets(None, table[:, :5])
    assert scorer.coarse_select("e", "d", "b", cap=7) == "decided" and seen["select"] == ("e", "d", "b", {"cap": 7})


# ---------------------------------------------------------------- the C entry points' refusals
def test_coarse_select_entry_points_refuse_without_a_gpu():
    from ctypes import c_void_p
    from acousticswarms_speech_amd import native
    L = native.lib()
    buf = np.zeros(1 << 16)
    p = c_void_p(buf.ctypes.data)
    size = L.asw_coarse_select_workspace_bytes
    for N, cap in ((-1, 30), ((1 << 24) + 1, 30), (100, 0), (100, 65), (100, -3)):
        assert size(N, cap) == 0 and b"coarse_select_workspace_bytes" in L.asw_last_error(), (N, cap)
    slices = lambda N: (N + cases.SLICE - 1) // cases.SLICE
    for N, cap in ((0, 1), (1, 1), (cases.SLICE, 30), (cases.SLICE + 1, 64), (G7_CUBES, 30), (1 << 24, 64)):
        assert size(N, cap) == (((256 + slices(N)) * 8 + slices(N) * (2 + cap) * 4 + 7) // 8) * 8, (N, cap)
    need = size(G7_CUBES, 30)

    def select(energies=p, dis1=p, best=p, N=G7_CUBES, thr1=0.008, relative=0, rel=0.4, cap=30, ws=p, ws_bytes=1 << 19,
               kept=p, counts=p, thr=p):
        return L.asw_coarse_select(energies, dis1, best, N, thr1, relative, rel, cap, ws, ws_bytes, kept, counts, thr, None)
    assert select(N=-1) == -1 and b"N = -1" in L.asw_last_error()
    assert select(N=(1 << 24) + 1) == -1 and b"outside 0..16777216" in L.asw_last_error()
    for cap in (0, 65, -1):
        assert select(cap=cap) == -1 and b"outside 1..64" in L.asw_last_error(), cap
    for name in ("energies", "dis1", "ws"):
        assert select(**{name: None}) == -1 and b"coarse_select: null pointer" in L.asw_last_error(), name
    for name in ("kept", "counts", "thr"):
        assert select(**{name: None}) == -1 and b"null output" in L.asw_last_error(), name
        assert select(N=0, **{name: None}) == -1 and b"null output" in L.asw_last_error(), name
    assert select(ws_bytes=need - 1) == -1 and b"too small" in L.asw_last_error()
    assert select(ws=c_void_p(buf.ctypes.data + 4)) == -1 and b"not 8-byte aligned" in L.asw_last_error()
