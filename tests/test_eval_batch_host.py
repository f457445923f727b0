"""No GPU: the pieces of the batched dataset evaluation -- the matcher fed a ready-made SI-SDR
matrix, the record built from a search result, the metrics pass of a batch with stand-in ops, the grouping rule,
``evaluate_dataset(batch=)`` on the surrogate model, ``localize_batch(details=True)`` in the plain loop, the refusals of
``asw_cross_sisdr`` through ctypes and the argument parser of the program."""
import ctypes
import io
import json
import os
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import evalkit, native
from acousticswarms_speech_amd.hostdsp import si_sdr
from tests.bss_sources_cases import stand_in


# ---------------------------------------------------------------- the matcher with a ready-made matrix
def _host_matrix(wav_pred, wav_gt):
    return np.array([[si_sdr(np.asarray(p), np.asarray(g)) for g in wav_gt] for p in wav_pred]).reshape(len(wav_pred), len(wav_gt))


def test_matcher_with_matrix_on_the_reference_cases(golden):
    g = golden("g12_best_permutation")
    for k in range(int(g["n_cases"])):
        gt, pred = g[f"wav_gt{k}"].astype(np.float64), g[f"wav_pred{k}"].astype(np.float64)
        want = evalkit.find_best_permutation(gt, pred, g[f"pos_gt{k}"], g[f"pos_pred{k}"])
        got = evalkit.find_best_permutation(gt, None, g[f"pos_gt{k}"], g[f"pos_pred{k}"], sisdr=_host_matrix(pred, gt))
        assert got == want, k


def test_matcher_with_matrix_on_random_cases():
    rng = np.random.default_rng(5)
    n_matched = 0
    for trial in range(200):
        n_gt, n_pred = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        wav_gt = rng.standard_normal((n_gt, 300))
        pos_gt = rng.uniform(-2, 2, (n_gt, 3))
        src = rng.integers(0, max(n_gt, 1), n_pred)
        wav_pred = (wav_gt[src] if n_gt else np.zeros((n_pred, 300))) \
            + rng.uniform(0.05, 3.0, (n_pred, 1)) * rng.standard_normal((n_pred, 300))
        pos_pred = (pos_gt[src] if n_gt else np.zeros((n_pred, 3))) \
            + rng.uniform(0.0, 0.9, (n_pred, 1)) * rng.standard_normal((n_pred, 3))
        want = evalkit.find_best_permutation(wav_gt, wav_pred, pos_gt, pos_pred)
        got = evalkit.find_best_permutation(wav_gt, None, pos_gt, pos_pred, sisdr=_host_matrix(wav_pred, wav_gt))
        assert got == want, trial
        n_matched += len(want)
    assert n_matched > 100


def test_cross_sisdr_f64_is_the_host_statement_in_a_loop():
    rng = np.random.default_rng(6)
    est, ref = rng.standard_normal((3, 500)).astype(np.float32), rng.standard_normal((2, 500)).astype(np.float32)
    got = evalkit.cross_sisdr_f64(est, ref)
    assert got.shape == (3, 2) and got.dtype == np.float64
    for p in range(3):
        for s in range(2):
            assert got[p, s] == si_sdr(est[p].astype(np.float64), ref[s].astype(np.float64))
    assert evalkit.cross_sisdr_f64(np.zeros((0, 5)), ref[:, :5]).shape == (0, 2)
    with pytest.raises(ValueError):                                     # the statement's own: log10(0)
        evalkit.cross_sisdr_f64(np.zeros((1, 500)), ref)


# ---------------------------------------------------------------- stand-in ops (the host statements on CPU tensors)
class _CrossOp:
    """``torch.ops.asw.cross_sisdr`` on CPU tensors; marks the items whose index (over all calls) is in ``mark``."""

    def __init__(self, mark=()):
        self.mark, self.calls, self.items = set(mark), 0, 0

    def __call__(self, est, ref, est_counts, ref_counts):
        est, ref = est.numpy(), ref.numpy()
        assert est.dtype == np.float32 and ref.dtype == np.float32
        self.calls += 1
        vals, status, e0, r0 = [], [], 0, 0
        for P, S in zip(est_counts, ref_counts):
            if self.items in self.mark:
                vals.append(np.full(P * S, np.nan))
                status.append(1)
            else:
                vals.append(evalkit.cross_sisdr_f64(est[e0:e0 + P], ref[r0:r0 + S]).reshape(-1))
                status.append(0)
            e0, r0, self.items = e0 + P, r0 + S, self.items + 1
        return torch.from_numpy(np.concatenate(vals)), torch.tensor(status, dtype=torch.int32)


_bss_op = stand_in()                                   # the BSS op: nothing marked


def test_cross_sisdr_batch_groups_by_length_and_recomputes_marked_items():
    rng = np.random.default_rng(7)
    shapes = [(3, 2, 300), (1, 1, 200), (0, 2, 300), (2, 0, 200), (4, 3, 300)]
    ests = [rng.standard_normal((P, T)) for P, _S, T in shapes]
    refs = [rng.standard_normal((S, T)) for _P, S, T in shapes]
    want = [evalkit.cross_sisdr_f64(e, r) for e, r in zip(ests, refs)]
    op = _CrossOp(mark=(1,))                                            # the second item the op sees: item 2 (T = 300)
    got, recomputed = evalkit.cross_sisdr_batch(ests, refs, op=op)
    assert op.calls == 2 and recomputed == [2]
    for g, w, (P, S, _T) in zip(got, want, shapes):
        assert g.shape == (P, S) and g.dtype == np.float64
        np.testing.assert_array_equal(g, w)
    assert evalkit.cross_sisdr_batch([], []) == ([], [])
    with pytest.raises(ValueError, match="reference sets"):
        evalkit.cross_sisdr_batch(ests, refs[:2], op=op)
    with pytest.raises(ValueError, match="item 0"):
        evalkit.cross_sisdr_batch([np.zeros((2, 10))], [np.zeros((2, 11))], op=op)
    with pytest.raises(ValueError, match="at most 64"):
        evalkit.cross_sisdr_batch([np.zeros((2, 10))], [np.zeros((65, 10))], op=op)


# ---------------------------------------------------------------- the surrogate model of test_evalkit.py
def _surrogate():
    """(JointModel on the CPU surrogate scorer whose arrays reuse the fixture's SRP map, metadata, mixture, ground truth):
    the scene and model of test_gpu_bss_eval.py::test_record_device_against_host."""
    from acousticswarms_speech_amd.joint import JointModel
    from tests.golden.make_golden_search import ROI, scene_in_roi
    from tests.golden.surrogate import SurrogateSpot
    mics, spk, mixr = scene_in_roi()
    g7 = np.load(os.path.join(os.path.dirname(__file__), "golden", "g7_srp_map.npz"))
    meta = {"ROI": list(ROI[:5]) + [ROI[5] - 0.02]}
    for m in range(mics.shape[0]):
        meta[f"mic{m:02d}"] = {"position": mics[m].tolist()}
    for s in range(spk.shape[0]):
        meta[f"voice{s:02d}"] = {"position": spk[s].tolist()}
    jm = JointModel(SurrogateSpot())

    def with_map(mp):
        node = mp.SRP_node
        node.SRP_Map_WINDOW_new = lambda signal, window=36000: node.set_map(g7["srp_map"])
        return mp
    orig_setup, orig_for = jm.setup, jm.mic_array_for

    def setup(mic_positions, speaker_range, **kw):
        orig_setup(mic_positions, speaker_range, **kw)
        with_map(jm.Mic_processor)
    jm.setup = setup
    jm.mic_array_for = lambda *a, **kw: with_map(orig_for(*a, **kw))
    gt = np.stack([mixr[0]] * spk.shape[0]).astype(np.float32)
    return jm, meta, np.asarray(mixr, dtype=np.float32), gt, (mics, spk)


@pytest.fixture(scope="module")
def surrogate_run():
    """One forward pass of the surrogate model, shared and read-only: (metadata, mix, gt, search result, the record of
    ``evaluate_sample`` on the same pass)."""
    jm, meta, mix, gt, _geo = _surrogate()

    class Once:
        out = None

        def setup(self, **kw):
            if self.out is None:
                jm.setup(**kw)

        def __call__(self, m):
            if self.out is None:
                self.out = jm(m)
            return self.out
    model = Once()
    with redirect_stdout(io.StringIO()):
        want = evalkit.evaluate_sample(model, meta, mix, gt)
        result = evalkit.search_result(model, meta, mix)
    return meta, mix, gt, result, want


def test_record_from_result_reproduces_evaluate_sample(surrogate_run):
    meta, mix, gt, result, want = surrogate_run
    assert len(want[0]["pred"]) >= 1
    got = evalkit.record_from_result(meta, mix, gt, result, metrics="host")
    assert json.dumps(got[0]) == json.dumps(want[0]) and got[1:] == want[1:]
    # the arrays of localize_batch(details=True) in place of the lists of search_result
    as_arrays = dict(result, offsets=np.array(result["offsets"]), audio_offsets=np.array(result["audio_offsets"]))
    got = evalkit.record_from_result(meta, mix, gt, as_arrays)
    assert json.dumps(got[0]) == json.dumps(want[0])


def _variants(surrogate_run):
    """Four samples from the one forward pass: as it is, with a second 'separated' audio (so that the third block of
    estimate rows exists), without talkers, and with a noisier ground truth."""
    meta, mix, gt, result, _want = surrogate_run
    rng = np.random.default_rng(8)
    K, T = result["audio_loc"].shape
    sep = (result["audio_loc"] + 0.05 * rng.standard_normal((K, T))).astype(np.float32)
    empty = {"centres": np.zeros((0, 3)), "offsets": np.zeros((0, 6)), "audio_offsets": np.zeros((0, 6)),
             "audio_loc": np.zeros((0, T), dtype=np.float32), "audio": np.zeros((0, T), dtype=np.float32)}
    gt2 = (gt + 0.1 * rng.standard_normal(gt.shape)).astype(np.float32)
    samples = [(meta, mix, gt), (meta, mix, gt), (meta, mix, gt), (meta, mix, gt2)]
    results = [result, dict(result, audio=sep), empty, result]
    return samples, results


def test_records_from_results_with_stand_in_ops_gives_the_host_records(surrogate_run):
    samples, results = _variants(surrogate_run)
    want = evalkit.records_from_results(samples, results, "host")
    assert [w[1] for w in want][2] == 0 and sum(w[1] for w in want) >= 3
    for k in range(4):
        one = evalkit.record_from_result(*samples[k], results[k], "host")
        assert json.dumps(one[0]) == json.dumps(want[k][0]) and one[1:] == want[k][1:]
    # one call, the op marking items 1 and 3 (they are recomputed by the host statement)
    op = _CrossOp(mark=(1, 3))
    got = evalkit.records_from_results(samples, results, "device", ops=(op, _bss_op))
    assert op.calls == 1 and op.items == 4
    assert json.dumps([g[0] for g in got]) == json.dumps([w[0] for w in want])
    assert [g[1:] for g in got] == [w[1:] for w in want]
    # two calls
    op = _CrossOp(mark=(0,))
    got = evalkit.records_from_results(samples[:1], results[:1], "device", ops=(op, _bss_op)) \
        + evalkit.records_from_results(samples[1:], results[1:], "device", ops=(op, _bss_op))
    assert op.calls == 2
    assert json.dumps([g[0] for g in got]) == json.dumps([w[0] for w in want])
    with pytest.raises(ValueError, match="metrics"):
        evalkit.records_from_results(samples, results, "gpu")
    with pytest.raises(ValueError, match="results for"):
        evalkit.records_from_results(samples, results[:2], "host")


# ---------------------------------------------------------------- grouping and evaluate_dataset
def test_grouping_rule():
    a, b = (7, 48000), (7, 24000)
    assert evalkit.group_samples([], 4) == []
    assert evalkit.group_samples([a] * 8, 4) == [(0, 4), (4, 8)]                       # an exact multiple
    assert evalkit.group_samples([a] * 9, 4) == [(0, 4), (4, 8), (8, 9)]
    assert evalkit.group_samples([a] * 3, 4) == [(0, 3)]
    assert evalkit.group_samples([a, a, b, b, b, a], 2) == [(0, 2), (2, 4), (4, 5), (5, 6)]   # a shape change mid-run
    assert evalkit.group_samples([a, a, a, b, a, a], 4) == [(0, 3), (3, 4), (4, 6)]
    assert evalkit.group_samples([a, (6, 48000), a], 4) == [(0, 1), (1, 2), (2, 3)]    # M counts too
    assert evalkit.group_samples([a, a, b], 1) == [(0, 1), (1, 2), (2, 3)]             # batch = 1
    for bad in (0, -1):
        with pytest.raises(ValueError, match="batch"):
            evalkit.group_samples([a], bad)


def test_evaluate_dataset_batched_writes_the_files_of_the_loop(tmp_path):
    jm, _meta, mix, gt, (mics, spk) = _surrogate()
    from tests.golden.make_golden_search import ROI
    roi = list(ROI[:5]) + [ROI[5] - 0.02]
    rng = np.random.default_rng(9)
    for k in range(3):                                                   # three samples; the last one is shorter
        T = mix.shape[1] if k < 2 else mix.shape[1] - 500
        noisy = (mix[:, :T] + (1e-3 * k) * rng.standard_normal((mix.shape[0], T))).astype(np.float32)
        scene = types.SimpleNamespace(speaker_range=roi, mic_positions=mics, speaker_positions=spk, fs=48000, mix=noisy,
                                      sources=gt[:, :T])
        evalkit.write_scene_dir(scene, str(tmp_path / "ds" / f"{k:05d}"))
    with redirect_stdout(io.StringIO()):
        want = evalkit.evaluate_dataset(jm, str(tmp_path / "ds"), str(tmp_path / "loop"), batch=1)
        stats = {}
        got = evalkit.evaluate_dataset(jm, str(tmp_path / "ds"), str(tmp_path / "batched"), batch=2, stats=stats)
    assert got == want and want["tp"] >= 2
    names = sorted(os.listdir(tmp_path / "loop"))
    assert names == [f"result_{k:05d}.json" for k in range(3)]
    assert sorted(os.listdir(tmp_path / "batched")) == names
    for name in names:
        assert (tmp_path / "batched" / name).read_bytes() == (tmp_path / "loop" / name).read_bytes(), name
    assert set(stats) == {"read_s", "search_s", "sisdr_s", "match_s", "bss_s", "record_s", "write_s"}
    for bad in (0, -3):
        with pytest.raises(ValueError, match="batch"):
            evalkit.evaluate_dataset(jm, str(tmp_path / "ds"), batch=bad)


# ---------------------------------------------------------------- localize_batch(details=) in the plain loop
def test_localize_batch_details_in_the_plain_loop():
    from acousticswarms_speech_amd.shard import localize_batch
    jm, meta, mix, _gt, (mics, _spk) = _surrogate()
    _m, mic_positions, _v, _gp, _og, roi = evalkit.preprocess_metadata(meta)
    mixes = [torch.from_numpy(mix), torch.zeros(mix.shape)]            # the second one is silent: no talker
    geo = [(mic_positions, roi)] * 2
    base = {"centres", "powers", "names", "spot_times", "times"}
    with redirect_stdout(io.StringIO()):
        plain = localize_batch(jm, mixes, concurrent=1, geometries=geo)
        got = localize_batch(jm, mixes, concurrent=1, geometries=geo, details=True)
    assert [set(r) for r in plain] == [base] * 2
    import inspect
    assert inspect.signature(localize_batch).parameters["details"].default is False
    M, T = mix.shape
    for r, p in zip(got, plain):
        assert set(r) == base | {"offsets", "audio_offsets", "audio_loc"}
        K = len(r["names"])
        assert list(r["names"]) == list(p["names"])
        assert r["offsets"].shape == (K, M - 1) and r["audio_offsets"].shape == (K, M - 1)
        assert r["audio_loc"].shape == (K, T) and r["audio_loc"].dtype == np.float32
    assert len(got[0]["names"]) >= 1 and len(got[1]["names"]) == 0
    with redirect_stdout(io.StringIO()):
        jm.use_geometry(mic_positions, roi)
        patches, audio_loc, _a, _d0, _d1, _st = jm.forward(mixes[0])
    np.testing.assert_array_equal(got[0]["audio_loc"], np.asarray(audio_loc))
    np.testing.assert_array_equal(got[0]["offsets"], np.array([p[4]["localization_offset"] for p in patches]))
    np.testing.assert_array_equal(got[0]["audio_offsets"], np.array([p[4]["audio_offset"] for p in patches]))


# ---------------------------------------------------------------- the C entry point: refused on the host
def _i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_cross_sisdr_entry_point_rejects_bad_arguments_without_a_gpu():
    L = native.lib()
    buf = np.zeros(4096)
    p = ctypes.c_void_p(buf.ctypes.data)                                # never dereferenced: every call below is refused
    one, n = _i32([1]), buf.nbytes

    def refused(message, est=p, ref=p, ec=one, rc=one, K=1, T=100, out=p, status=p, ws=p, ws_bytes=n):
        assert L.asw_cross_sisdr(est, ref, ec, rc, K, T, out, status, ws, ws_bytes, None) == -1
        assert message in L.asw_last_error(), L.asw_last_error()
    for null in ("est", "ref", "out", "status", "ws", "ec", "rc"):
        refused(b"cross_sisdr: null", **{null: None})
    refused(b"K = -1", K=-1)
    refused(b"K = 65536", K=65536)
    refused(b"T = 0", T=0)
    refused(b"T = 33554433", T=(1 << 25) + 1)
    refused(b"negative count", ec=_i32([-1]))
    refused(b"negative count", rc=_i32([-1]))
    refused(b"4097 estimates", ec=_i32([4097]))
    refused(b"65 references", rc=_i32([65]))
    need = L.asw_cross_sisdr_workspace_bytes(one, one, 1, 100)
    refused(b"too small", ws_bytes=need - 8)
    refused(b"not 8-byte aligned", ws=ctypes.c_void_p(buf.ctypes.data + 4))
    assert L.asw_cross_sisdr_workspace_bytes(_i32([-1]), one, 1, 100) == 0
    assert b"cross_sisdr_workspace_bytes: item 0: negative count" in L.asw_last_error()
    # K = 0 succeeds and touches nothing
    assert L.asw_cross_sisdr(None, None, None, None, 0, 100, None, None, None, 0, None) == 0
    assert not buf.any()


def test_cross_sisdr_workspace_formula():
    L = native.lib()
    rng = np.random.default_rng(10)
    for K in (1, 2, 5):
        for T in (1, 511, 512, 513, 4099, 48000, 1 << 25):
            ec = [int(v) for v in rng.integers(0, 60, K)]
            rc = [int(v) for v in rng.integers(0, 12, K)]
            n = L.asw_cross_sisdr_workspace_bytes(_i32(ec), _i32(rc), K, T)
            assert n > 0 and n % 8 == 0, (ec, rc, T, n)
            more = L.asw_cross_sisdr_workspace_bytes(_i32([c + 8 for c in ec]), _i32([c + 8 for c in rc]), K, T)
            assert more > n
    assert L.asw_cross_sisdr_workspace_bytes(_i32([4096]), _i32([64]), 1, 48000) % 8 == 0
    assert L.asw_cross_sisdr_workspace_bytes(_i32([0, 3]), _i32([2, 0]), 2, 100) > 0    # no pair at all: the lists only


# ---------------------------------------------------------------- the program
def test_program_argument_parser(capsys):
    import importlib
    mod = importlib.import_module("acousticswarms_speech_amd.evaluate")
    args = mod.build_parser().parse_args(["DS"])
    # the reference's defaults (sep/eval/eval_model.py:268-301)
    assert args.dataset == "DS" and args.spot_experiment_dir is None and args.sep_experiment_dir is None
    assert args.sr == 48000 and args.n_mics == 7 and args.use_cuda is False and args.spot_batch_size == 128
    assert args.cached_init is False and args.results_folder is None
    assert (args.batch, args.metrics, args.precision, args.geometry) == (1, "host", "f32", "host")
    args = mod.build_parser().parse_args(["DS", "--spot_experiment_dir", "a", "--sep_experiment_dir", "b", "--use_cuda",
                                          "--cached_init", "--batch", "16", "--metrics", "device", "--precision",
                                          "f16x3_safe", "--geometry", "device", "--results_folder", "out"])
    assert (args.batch, args.metrics, args.precision, args.geometry, args.results_folder) == \
        (16, "device", "f16x3_safe", "device", "out")
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(["DS", "--metrics", "gpu"])
    assert "invalid choice" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(["DS", "--precision", "f16"])
    help_text = mod.build_parser().format_help()
    assert help_text.count("no effect") == 2
    with pytest.raises(SystemExit, match="both needed"):
        mod.main(["DS"])
