"""GPU: the SI-SDR matrices of a ragged batch on the device (csrc/eval_kernels.hip) against
``evalkit.cross_sisdr_f64`` -- ``hostdsp.si_sdr`` in a loop -- on the same float32-rounded inputs, never against the
kernel itself; the metrics pass of a batch, device against host, on the same search results; and
``evaluate_dataset(batch=4, metrics="device")`` against the per-sample loop.  Needs an MI355X.

The bound.  MEASURED_DB is the largest |device - statement| in dB over the shape, level and status cases of this file
on an MI355X; the tests assert ten times it, the slack being for the change of summation order with the grid.  The
bound may not exceed 1e-9 dB: a two-pass kernel sits orders below that, a Gram-form kernel (sum est^2 - (sum ref est)^2 /
rr) breaks it from about 57 dB up, which the level sweep reaches.  Every test prints its figure before it asserts."""
import ctypes
import functools
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import evalkit, native
from tests import bss_eval_cases as cases

pytestmark = pytest.mark.gpu

MEASURED_DB = 2.700e-12
BOUND_DB = 10 * MEASURED_DB
assert BOUND_DB <= 1e-9
DEV = "cuda:0"
LEVELS = (30.0, 1.0, 1e-2, 1e-4, 1e-5, 1e-6)         # noise relative to the reference: -33 .. +104 dB


@functools.lru_cache(maxsize=None)
def _case(seed, counts, T, level=None):
    """(ests, refs, the statement per item) of one generated batch: made once, shared, read-only.  Item k has
    counts[k] = (P, S): speech-like references (tests/bss_eval_cases.py) and estimates that are random mixtures of them
    plus noise, or -- with ``level`` -- est_p = 0.7 ref_(p mod S) + level * rms(ref_(p mod S)) * noise."""
    rng = np.random.default_rng([seed, T] + [int(v) for c in counts for v in c])
    ests, refs = [], []
    for P, S in counts:
        ref = cases.references(rng, S, T) if S else np.zeros((0, T), dtype=np.float32)
        r64 = ref.astype(np.float64)
        if level is None or S == 0:
            rms = float(np.sqrt(np.mean(r64 ** 2))) if S else 0.05
            est = rng.uniform(-1, 1, (P, S)) @ r64 + 0.3 * rms * rng.standard_normal((P, T))
        else:
            own = r64[np.arange(P) % S]
            est = 0.7 * own + level * np.sqrt(np.mean(own ** 2, axis=1, keepdims=True)) * rng.standard_normal((P, T))
        ests.append(np.ascontiguousarray(est, dtype=np.float32))
        refs.append(ref)
    want = [evalkit.cross_sisdr_f64(e, r) for e, r in zip(ests, refs)]
    for a in ests + refs + want:
        a.setflags(write=False)
    return ests, refs, want


def _op(ests, refs):
    est = torch.from_numpy(np.concatenate(ests, axis=0)).to(DEV)
    ref = torch.from_numpy(np.concatenate(refs, axis=0)).to(DEV)
    out, status = native.torch_ops().cross_sisdr(est, ref, [e.shape[0] for e in ests], [r.shape[0] for r in refs])
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert out.dtype == np.float64 and status.dtype == np.int32
    mats, pos = [], 0
    for e, r in zip(ests, refs):
        mats.append(out[pos:pos + e.shape[0] * r.shape[0]].reshape(e.shape[0], r.shape[0]))
        pos += e.shape[0] * r.shape[0]
    assert pos == out.size
    return mats, status


def _check(tag, got, want):
    err = 0.0
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.all(np.isfinite(g)), tag
        if g.size:
            err = max(err, float(np.max(np.abs(g - w))))
    lo = min((float(w.min()) for w in want if w.size), default=0.0)
    hi = max((float(w.max()) for w in want if w.size), default=0.0)
    print(f"{tag}: max |device - statement| = {err:.3e} dB, statement {lo:.1f} .. {hi:.1f} dB (bound {BOUND_DB:.1e})")
    assert err <= BOUND_DB, (tag, err)
    return err


# ---------------------------------------------------------------- shapes
# the tile is 8 estimate rows x 8 reference rows: 7, 8 and 9 on both sides, 17 x 9 = 3 x 2 tiles, empty items riding along
COUNTS = [((1, 1),), ((3, 2),), ((0, 3), (2, 0), (3, 2)), ((9, 1), (1, 5)), ((17, 9),), ((7, 7), (8, 8), (9, 9))]


@pytest.mark.parametrize("counts", COUNTS)
def test_ragged_counts(counts):
    ests, refs, want = _case(21, counts, 1000)
    got, status = _op(ests, refs)
    assert status.tolist() == [0] * len(counts)
    _check(f"counts {counts}", got, want)


@pytest.mark.parametrize("T", [1, 2, 511, 512, 513, 1023, 1024, 1025, 4099])
def test_sample_lengths(T):
    """Below a chunk (512), a chunk, a chunk and a tail, several chunks (one run each), and nine chunks in eight runs."""
    ests, refs, want = _case(22, ((3, 2), (9, 9)), T)
    got, status = _op(ests, refs)
    assert status.tolist() == [0, 0]
    _check(f"T {T}", got, want)


def test_working_size():
    ests, refs, want = _case(23, ((55, 5),), 48000)
    got, status = _op(ests, refs)
    assert status.tolist() == [0]
    _check("P 55 S 5 T 48000", got, want)


@pytest.mark.parametrize("level", LEVELS)
def test_level_sweep(level):
    """est = 0.7 ref + noise: the matched pairs run from -33 dB (level 30) to about +100 dB (level 1e-6, where the
    1e-8 in the denominator takes over).  From 57 dB up (levels 1e-4 and below) a kernel that forms ne from the Gram
    sums misses the bound."""
    ests, refs, want = _case(24, ((3, 3), (2, 1)), 48000, level)
    got, status = _op(ests, refs)
    assert status.tolist() == [0, 0]
    matched = float(want[0][0, 0])
    print(f"level {level:g}: matched pair at {matched:.1f} dB")
    if level >= 1e-2:                                                   # 20 log10(0.7) = -3.1: the sweep is where it says
        assert abs(matched - (-20 * np.log10(level) - 3.1)) < 2.0
    else:
        assert matched > 57.0
    _check(f"level {level:g}", got, want)


# ---------------------------------------------------------------- bytes and status
def _c_call(est, ref, ec, rc, T, fill):
    """One call of the C entry point on the current stream with out, status and workspace pre-filled with ``fill``."""
    L = native.lib()
    ec_c, rc_c = (ctypes.c_int32 * len(ec))(*ec), (ctypes.c_int32 * len(rc))(*rc)
    n = L.asw_cross_sisdr_workspace_bytes(ec_c, rc_c, len(ec), T)
    assert n > 0 and n % 8 == 0
    out = torch.full((sum(p * s for p, s in zip(ec, rc)) * 8,), fill, dtype=torch.uint8, device=DEV)
    status = torch.full((len(ec) * 4,), fill, dtype=torch.uint8, device=DEV)
    ws = torch.full((n,), fill, dtype=torch.uint8, device=DEV)
    native.check(L.asw_cross_sisdr(native.ptr(est), native.ptr(ref), ec_c, rc_c, len(ec), T, native.ptr(out), native.ptr(status),
                                   native.ptr(ws), n, native.current_stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), status.cpu().numpy().tobytes()


def test_identical_bytes_whatever_the_buffers_held():
    counts = ((0, 3), (2, 0), (3, 2), (17, 9))
    ests, refs, want = _case(25, counts, 4099)
    est = torch.from_numpy(np.concatenate(ests, axis=0)).to(DEV)
    ref = torch.from_numpy(np.concatenate(refs, axis=0)).to(DEV)
    ec, rc = [c[0] for c in counts], [c[1] for c in counts]
    runs = [_c_call(est, ref, ec, rc, 4099, fill) for fill in (0xFF, 0x00, 0xFF)]
    assert runs[0] == runs[1] == runs[2]
    assert np.frombuffer(runs[0][1], dtype=np.int32).tolist() == [0, 0, 0, 0]
    vals = np.frombuffer(runs[0][0], dtype=np.float64)
    _check("C entry point", [vals[:6].reshape(3, 2), vals[6:].reshape(17, 9)], want[2:])
    # through the op: torch's allocator hands back the blocks just freed, whatever they hold
    a = native.torch_ops().cross_sisdr(est, ref, ec, rc)
    junk = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=DEV)
    del junk
    b = native.torch_ops().cross_sisdr(est, ref, ec, rc)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() == runs[0][0]
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes() == runs[0][1]


def test_status_marks_only_the_item_that_needs_the_host():
    ests, refs, want = _case(26, ((3, 2), (4, 3), (9, 9), (2, 2)), 1000)
    ests, refs = [e.copy() for e in ests], [r.copy() for r in refs]
    refs[1][2] = 0.0                                                    # a silent reference: rr == 0
    ests[2][8] = 0.0                                                    # an all-zero estimate: te == 0
    got, status = _op(ests, refs)
    assert status.tolist() == [0, 1, 1, 0]
    _check("neighbours of flagged items", [got[0], got[3]], [want[0], want[3]])
    # through cross_sisdr_batch the silent-reference item is the host statement's own result, warnings and all
    with np.errstate(all="ignore"):
        host = evalkit.cross_sisdr_f64(ests[1], refs[1])
        mats, recomputed = evalkit.cross_sisdr_batch(ests[:2] + ests[3:], refs[:2] + refs[3:])
    assert recomputed == [1]
    np.testing.assert_array_equal(mats[1], host)
    assert np.isnan(host[:, 2]).all() and np.isfinite(host[:, :2]).all()
    _check("cross_sisdr_batch", [mats[0], mats[2]], [want[0], want[3]])
    # the all-zero estimate raises, as the statement does
    with pytest.raises(ValueError, match="math domain"), np.errstate(all="ignore"):
        evalkit.cross_sisdr_batch(ests, refs)


def test_adapter_refusals():
    op = native.torch_ops().cross_sisdr
    est, ref = torch.zeros((3, 100), device=DEV), torch.ones((2, 100), device=DEV)
    with pytest.raises(RuntimeError, match="Float"):
        op(est.double(), ref, [3], [2])
    with pytest.raises(RuntimeError, match="Float"):
        op(est, ref.half(), [3], [2])
    with pytest.raises(RuntimeError, match="2 dimensions"):
        op(est[0], ref, [3], [2])
    with pytest.raises(RuntimeError, match="HIP"):
        op(est.cpu(), ref, [3], [2])
    with pytest.raises(RuntimeError, match="contiguous"):
        op(torch.zeros((100, 3), device=DEV).t(), ref, [3], [2])
    with pytest.raises(RuntimeError, match="differ in length"):
        op(est, ref[:, :99].contiguous(), [3], [2])
    with pytest.raises(RuntimeError, match="est_counts sum"):
        op(est, ref, [2], [2])
    with pytest.raises(RuntimeError, match="ref_counts sum"):
        op(est, ref, [3], [1])
    with pytest.raises(RuntimeError, match="ref_counts 1"):
        op(est, ref, [1, 2], [2])
    with pytest.raises(RuntimeError, match="outside 0..64"):
        op(est, torch.ones((65, 100), device=DEV), [3], [65])
    with pytest.raises(RuntimeError, match="outside 0..4096"):
        op(est, ref, [-1, 4], [1, 1])
    out, status = op(est[:0], ref[:0], [], [])                         # K = 0
    assert out.shape == (0,) and status.shape == (0,)
    out, status = op(ref, ref, [2], [2])                               # still works
    assert status.tolist() == [0] and out.shape == (4,)


# ---------------------------------------------------------------- the metrics pass, device against host
def synthetic_results(tmp_path):
    """Three samples (2, 3 and 5 talkers, 7 mics, T = 6000) as ``get_items`` reads them and a search result for each:
    the true positions moved by a few cm, separated audio = source + a leak of the next source + noise, localisation-
    stage audio = a noisier copy, two false positives, the predictions in shuffled order.  The waveforms are float64
    arrays of float32 values, so that the host matcher works in float64 like the statement.
    The seeds: per talker count the first one from 3100 on whose talkers all speak within the 6000 samples (energy
    above 0.5) and on which the host statement agrees with itself -- ``bss_eval_sdr`` with its LU solve against the same
    with a float64 Cholesky solve, on the CPU -- within 1e-13 dB, a quarter of the BSS bound.  (Seed 3103 with 5 talkers
    has a Gram matrix of condition 7.5e20, and the two host solves differ by 3.5e-12 dB there.)"""
    from acousticswarms_speech_amd.scenes import make_scene
    rng = np.random.default_rng(31)
    samples, results = [], []
    for k, (seed, S) in enumerate(((3100, 2), (3102, 3), (3100, 5))):
        sc = make_scene(seed, S, 7, 6000)
        assert np.all(np.sum(sc.sources.astype(np.float64) ** 2, axis=1) > 0.5)
        evalkit.write_scene_dir(sc, str(tmp_path / f"{k:05d}"))
        meta, mix, gt = evalkit.get_items(str(tmp_path / f"{k:05d}"))
        T, g64 = mix.shape[1], gt.astype(np.float64)
        rms = np.sqrt(np.mean(g64 ** 2, axis=1, keepdims=True))
        sep = g64 + 0.1 * np.roll(g64, 1, axis=0) + 0.05 * rms * rng.standard_normal((S, T))
        loc = sep + 0.3 * rms * rng.standard_normal((S, T))
        fp_audio = 0.02 * rng.standard_normal((2, T))
        pos = np.concatenate([sc.speaker_positions + rng.uniform(-0.04, 0.04, (S, 3)),
                              sc.speaker_positions[:2] + np.array([3.0, 2.5, 0.0])])
        offs = np.concatenate([np.round(sc.tdoa_samples()) + rng.integers(-1, 2, (S, 6)), rng.integers(-40, 40, (2, 6))])
        order = rng.permutation(S + 2)
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # noqa: E731
        results.append({"centres": pos[order], "offsets": offs[order], "audio_offsets": offs[order] + 0.25,
                        "audio_loc": f32(np.concatenate([loc, 1.5 * fp_audio]))[order],
                        "audio": f32(np.concatenate([sep, fp_audio]))[order]})
        samples.append((meta, mix, g64))
    return samples, results


def check_precondition(samples, results, db_margin, m_margin):
    """On host values only: no pair within ``db_margin`` of the -15 dB acceptance threshold, none within ``m_margin``
    of the 1 m range, no two matching costs tied.  -> the number of inlier pairs."""
    inliers = 0
    for (meta, _mix, gt), res in zip(samples, results):
        sep = res["audio_loc"] if res.get("audio") is None else res["audio"]
        if len(res["centres"]) == 0 or len(gt) == 0:
            continue
        M = evalkit.cross_sisdr_f64(sep, gt)
        gt_pos = evalkit.preprocess_metadata(meta)[3]
        dis = np.linalg.norm(np.asarray(res["centres"])[:, None, :2] - gt_pos[None, :, :2], axis=2)
        assert np.min(np.abs(M + 15.0)) > db_margin, ("threshold", float(np.min(np.abs(M + 15.0))))
        assert np.min(np.abs(dis - 1.0)) > m_margin, ("range", float(np.min(np.abs(dis - 1.0))))
        ok = (dis < 1) & (M > -15)
        cost = np.sort((dis - M)[ok])
        assert cost.size < 2 or np.min(np.diff(cost)) > 1e-9, "tied costs"
        inliers += int(ok.sum())
    return inliers


def test_metrics_pass_device_against_host(tmp_path):
    from tests.test_gpu_bss_eval import BOUND_DB as BSS_BOUND_DB
    samples, results = synthetic_results(tmp_path)
    assert check_precondition(samples, results, 1e-6, 1e-9) >= 10
    host = evalkit.records_from_results(samples, results, "host")
    dev = evalkit.records_from_results(samples, results, "device")
    assert [h[1:] for h in host] == [d[1:] for d in dev] == [(2, 2, 0), (3, 2, 0), (5, 2, 0)]
    worst = {"sisdr": 0.0, "bss": 0.0}
    for (rh, *_h), (rd, *_d) in zip(host, dev):
        assert rh.keys() == rd.keys() and rh["perm"] == rd["perm"]
        for key in rh:
            if key != "pred":
                assert rh[key] == rd[key], key
        assert len(rh["pred"]) == len(rd["pred"])
        for ph, pd in zip(rh["pred"], rd["pred"]):
            assert ph.keys() == pd.keys()
            for key in ph:
                if key in ("si_snr_in", "si_snri", "si_snr_in_old", "si_snri_old"):
                    worst["sisdr"] = max(worst["sisdr"], abs(ph[key] - pd[key]))
                elif key in ("si_snr_in_mir", "si_snri_mir"):
                    worst["bss"] = max(worst["bss"], abs(ph[key] - pd[key]))
                else:
                    assert ph[key] == pd[key], key
    print(f"records: SI-SDR fields |d| {worst['sisdr']:.3e} dB (bound {BOUND_DB:.1e}), "
          f"BSS fields |d| {worst['bss']:.3e} dB (bound {BSS_BOUND_DB:.1e})")
    assert worst["sisdr"] <= BOUND_DB and worst["bss"] <= BSS_BOUND_DB


# ---------------------------------------------------------------- the whole path
@pytest.fixture(scope="module")
def four_mixtures(tmp_path_factory):
    """The four-mixture configuration of test_gpu_sep_batch.py::test_localize_batch_with_separation (seeds 2000-2003, 5
    talkers, 7 mics, T = 24 000, the FULL spot net and SEP_SMALL in f16x3) as sample directories; the last two mixtures
    were recorded with a second array."""
    from acousticswarms_speech_amd.config import FULL, SEP_SMALL
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.sep import SepModel
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict
    arrays = [make_scene(2000, 5, 7, 24000).mic_positions, make_scene(2002, 5, 7, 24000).mic_positions]
    assert not np.array_equal(arrays[0], arrays[1])
    scs = [make_scene(2000 + k, 5, 7, 24000, mic_positions=arrays[k // 2]) for k in range(4)]
    root = tmp_path_factory.mktemp("four")
    for k, sc in enumerate(scs):
        evalkit.write_scene_dir(sc, str(root / "ds" / f"{k:05d}"))
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")
    sep = SepModel(SEP_SMALL, make_sep_state_dict(SEP_SMALL, 31), precision="f16x3").to("cuda")
    return JointModel(spot, sep, device="cuda"), root, scs


def test_evaluate_dataset_batched_against_the_loop(four_mixtures, monkeypatch):
    jm, root, _scs = four_mixtures
    seen = []
    build = evalkit.record_from_result

    def record(*args, **kw):
        seen.append(args)
        return build(*args, **kw)
    monkeypatch.setattr(evalkit, "record_from_result", record)
    with redirect_stdout(io.StringIO()):
        want = evalkit.evaluate_dataset(jm, str(root / "ds"), str(root / "loop"))
        got = evalkit.evaluate_dataset(jm, str(root / "ds"), str(root / "batched"), metrics="device", batch=4)
    assert len(seen) == 8
    # precondition, on the per-sample path's own values
    loop = seen[:4]
    check_precondition([a[:3] for a in loop], [a[3] for a in loop], 0.1, 1e-3)
    print(f"loop {want}, batched {got}")
    assert got == want and want["tp"] + want["fp"] >= 4               # talkers found (random weights: none matches)
    names = sorted(os.listdir(root / "loop"))
    assert names == [f"result_{k:05d}.json" for k in range(4)] == sorted(os.listdir(root / "batched"))
    for name in names:
        with open(root / "loop" / name) as f:
            a = json.load(f)
        with open(root / "batched" / name) as f:
            b = json.load(f)
        assert a.keys() == b.keys()
        for key in ("gt", "mic_pos", "speaker_pos", "perm", "est_offsets"):
            assert a[key] == b[key], (name, key)
        assert len(a["pred"]) == len(b["pred"]) and len(a["false_positive"]) == len(b["false_positive"])
        for pa, pb in zip(a["pred"], b["pred"]):
            assert pa.keys() == pb.keys()
            assert pa["voice_id"] == pb["voice_id"] and pa["shifts"] == pb["shifts"] and pa["sample_err"] == pb["sample_err"]
            np.testing.assert_allclose(pa["pos"], pb["pos"], atol=1e-6)
            assert abs(pa["dis_err"] - pb["dis_err"]) <= 2e-6
        for fa, fb in zip(a["false_positive"], b["false_positive"]):
            assert fa["sample"] == fb["sample"]
            np.testing.assert_allclose(fa["pos"], fb["pos"], atol=1e-6)


def test_localize_batch_details_batched_against_the_loop(four_mixtures):
    from acousticswarms_speech_amd.shard import localize_batch
    jm, _root, scs = four_mixtures
    mixes = [torch.from_numpy(s.mix) for s in scs]
    geo = [(s.mic_positions, list(s.speaker_range)) for s in scs]
    with redirect_stdout(io.StringIO()):
        loop = localize_batch(jm, mixes, concurrent=1, geometries=geo, separate=True, details=True)
        got = localize_batch(jm, mixes, concurrent=2, geometries=geo, separate=True, details=True)
    n_talkers = 0
    for k, (r, p) in enumerate(zip(got, loop)):
        assert set(r) == set(p) == {"centres", "powers", "names", "spot_times", "times", "audio", "offsets", "audio_offsets",
                                    "audio_loc"}
        K = len(r["names"])
        assert list(r["names"]) == list(p["names"]) and int(r["spot_times"]) == int(p["spot_times"])
        np.testing.assert_allclose(r["centres"], p["centres"], atol=1e-6)
        assert r["offsets"].shape == r["audio_offsets"].shape == (K, 6)
        np.testing.assert_array_equal(r["offsets"], p["offsets"])
        np.testing.assert_array_equal(r["audio_offsets"], p["audio_offsets"])
        assert r["audio_loc"].dtype == np.float32 and r["audio_loc"].shape == (K, 24000)
        if K:
            snr = 10 * np.log10(np.sum(p["audio_loc"].astype(np.float64) ** 2)
                                / max(np.sum((r["audio_loc"].astype(np.float64) - p["audio_loc"]) ** 2), 1e-300))
            print(f"details=True, mixture {k}: {K} talkers, audio_loc {snr:.1f} dB vs the plain loop")
            assert snr >= 74.0
        n_talkers += K
    assert n_talkers >= 4
