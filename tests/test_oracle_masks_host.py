"""No GPU: the float64 statements of the STFT pair and of the oracle mask baselines (acousticswarms_speech_amd/
oracle_masks.py) against scipy -- the library the reference calls -- and against the reference's own
do_irm / do_ibm through the fixture g16; the batch route and the record with a CPU stand-in for the device op; the C entry
points' refusals through ctypes."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.signal
import torch

from acousticswarms_speech_amd import evalkit, native
from acousticswarms_speech_amd import oracle_masks as om
from acousticswarms_speech_amd.hostdsp import si_sdr
from tests.bss_sources_cases import stand_in
from tests.oracle_masks_cases import LENGTHS, eval_batch, sources, threshold_margin

BAR = 1e-13            # max abs difference over max abs value: measured 6e-16; the margin covers another FFT backend
EPS = np.finfo(np.float64).eps


def rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


# ---------------------------------------------------------------- the statements against scipy
def _scipy_masks(gt, mix, kind, alpha=1.0, theta=0.5):
    """do_irm / do_ibm spelled with scipy calls (the arithmetic of the issue, not the reference's text)."""
    N = mix.shape[0]
    X = scipy.signal.stft(mix.astype(np.float64), nperseg=2048)[2]
    P = np.abs(scipy.signal.stft(gt.astype(np.float64), nperseg=2048)[2]) ** alpha
    if kind == "irm":
        model = EPS
        for j in range(gt.shape[0]):
            model = model + P[j]
        mask = P / model
    else:
        mask = np.where(P / (EPS + np.abs(X) ** alpha) >= theta, 1.0, 0.0)
    return scipy.signal.istft(X[None] * mask)[1][..., :N]


@pytest.mark.parametrize("N", LENGTHS)
def test_stft_statement_against_scipy(N):
    x, _ = sources(N, 3, N)
    got = om.stft_f64(x)
    want = scipy.signal.stft(x.astype(np.float64), nperseg=2048)[2]
    assert got.shape == want.shape == (3, 1025, om.frame_count(N)) and got.dtype == np.complex128
    assert rel(got, want) <= BAR
    back = scipy.signal.istft(want)[1][..., :N]
    assert rel(om.istft_f64(want, N), back) <= BAR


@pytest.mark.parametrize("kind", om.KINDS)
@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("N", LENGTHS)
def test_mask_statements_against_scipy(N, S, kind):
    gt, mix = sources(100 * S + N, S, N)
    assert threshold_margin(gt, mix) > 1e-9
    got = om.masks_f64(gt, mix, kind)
    assert got.shape == (S, N) and got.dtype == np.float64
    assert rel(got, _scipy_masks(gt, mix, kind)) <= BAR


def test_mask_statements_against_the_reference_fixture():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g16_oracle_masks.npz"))
    gt, mix = g["gt"], g["mix"]
    assert gt.dtype == np.float32 and mix.dtype == np.float32 and gt.shape == (2, 4096) and g["irm"].dtype == np.float64
    assert threshold_margin(gt, mix, float(g["alpha"]), float(g["theta"])) > 1e-9
    assert rel(om.irm_f64(gt, mix, float(g["alpha"])), g["irm"]) <= BAR
    assert rel(om.ibm_f64(gt, mix, float(g["alpha"]), float(g["theta"])), g["ibm"]) <= BAR


def test_statement_refusals_and_frame_count():
    assert [om.frame_count(N) for N in (2048, 3072, 3073, 48000)] == [3, 4, 5, 48]
    x = np.zeros((2, 2047), dtype=np.float32)
    for call in (lambda: om.frame_count(2047), lambda: om.stft_f64(x), lambda: om.irm_f64(x, x[0]),
                 lambda: om.ibm_f64(x, x[0]),
                 lambda: om.irm_f64(np.zeros((0, 4096)), np.zeros(4096)),              # S = 0
                 lambda: om.ibm_f64(np.zeros((0, 4096)), np.zeros(4096)),
                 lambda: om.irm_f64(np.zeros((2, 4096)), np.zeros(4097)),              # shapes
                 lambda: om.ibm_f64(np.zeros((2, 4096)), np.zeros((1, 4096))),
                 lambda: om.irm_f64(np.zeros(4096), np.zeros(4096)),
                 lambda: om.istft_f64(np.zeros((1, 1024, 3)), 2048),
                 lambda: om.istft_f64(np.zeros((1, 1025, 3)), 2049),
                 lambda: om.masks_f64(np.zeros((1, 4096)), np.zeros(4096), "wiener")):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("N", LENGTHS)
def test_round_trip(N):
    x, _ = sources(7 + N, 2, N)
    assert rel(om.istft_f64(om.stft_f64(x), N), x.astype(np.float64)) <= 1e-13


def test_zero_rows_give_zero_estimates():
    gt, mix = sources(3, 3, 3073)
    gt[1] = 0.0
    for kind in om.KINDS:
        assert not om.masks_f64(gt, mix, kind)[1].any()
        assert not om.masks_f64(gt, np.zeros_like(mix), kind).any()


# ---------------------------------------------------------------- the batch route with a CPU stand-in
class _OracleOp:
    """``torch.ops.asw.oracle_masks`` on CPU tensors, from the statements."""

    def __init__(self):
        self.calls, self.items = 0, 0

    def __call__(self, mix, ref, counts, lengths, kind, alpha=1.0, theta=0.5):
        mix, ref = mix.numpy(), ref.numpy()
        assert mix.dtype == np.float32 and ref.dtype == np.float32 and mix.shape[0] == len(counts) == len(lengths)
        assert ref.shape == (sum(counts), mix.shape[1])
        self.calls += 1
        out, r0 = np.zeros(ref.shape), 0
        for k, (S, N) in enumerate(zip(counts, lengths)):
            if S:
                out[r0:r0 + S, :N] = om.masks_f64(ref[r0:r0 + S, :N], mix[k, :N], kind, alpha, theta)
            r0, self.items = r0 + S, self.items + 1
        return torch.from_numpy(out)


class _CrossOp:
    """``torch.ops.asw.cross_sisdr`` on CPU tensors, from the statement."""
    calls = 0

    def __call__(self, est, ref, est_counts, ref_counts):
        est, ref = est.numpy(), ref.numpy()
        self.calls += 1
        vals, e0, r0 = [], 0, 0
        for P, S in zip(est_counts, ref_counts):
            vals.append(evalkit.cross_sisdr_f64(est[e0:e0 + P], ref[r0:r0 + S]).reshape(-1))
            e0, r0 = e0 + P, r0 + S
        return torch.from_numpy(np.concatenate(vals)), torch.zeros(len(est_counts), dtype=torch.int32)


def test_oracle_masks_batch_groups_by_length_and_keeps_item_order():
    shapes = [(1, 2048), (3, 3073), (6, 2048), (0, 3073), (3, 2048)]
    data = [sources(20 + q, S, N) if S else (np.zeros((0, N), dtype=np.float32), sources(20 + q, 1, N)[1])
            for q, (S, N) in enumerate(shapes)]
    for kind in om.KINDS:
        op = _OracleOp()
        got = evalkit.oracle_masks_batch([g for g, _m in data], [m for _g, m in data], kind, op=op)
        assert op.calls == 2 and op.items == 4                      # one call per length; the empty item is not sent
        for (S, N), (gt, mix), rows in zip(shapes, data, got):
            assert rows.shape == (S, N) and rows.dtype == np.float64
            if S:
                np.testing.assert_array_equal(rows, om.masks_f64(gt, mix, kind))
    op = _OracleOp()
    assert evalkit.oracle_masks_batch([], [], "irm", op=op) == [] and op.calls == 0
    with pytest.raises(ValueError, match="mixtures for"):
        evalkit.oracle_masks_batch([data[0][0]], [], "irm", op=op)
    with pytest.raises(ValueError, match="item 0"):
        evalkit.oracle_masks_batch([np.zeros((2, 4096))], [np.zeros(4097)], "irm", op=op)
    with pytest.raises(ValueError, match="at most 64"):
        evalkit.oracle_masks_batch([np.zeros((65, 4096))], [np.zeros(4096)], "irm", op=op)
    with pytest.raises(ValueError, match="fewer than the window"):
        evalkit.oracle_masks_batch([np.zeros((1, 2047))], [np.zeros(2047)], "ibm", op=op)
    with pytest.raises(ValueError, match="must be one of"):
        evalkit.oracle_masks_batch([data[0][0]], [data[0][1]], "wiener", op=op)


# ---------------------------------------------------------------- the record
@pytest.fixture(scope="module")
def batch():
    return eval_batch()


FIELDS = ("si_snri_irm", "si_snri_mir_irm", "si_snri_ibm", "si_snri_mir_ibm")


def test_record_is_unchanged_without_oracle(batch):
    samples, results = batch
    plain = evalkit.record_from_result(*samples[0], results[0])
    assert [p["voice_id"] for p in plain[0]["pred"]] == [0, 2] and plain[1:] == (2, 1, 1)
    assert not any(f in p for p in plain[0]["pred"] for f in FIELDS)
    off = evalkit.record_from_result(*samples[0], results[0], oracle=())
    assert json.dumps(off[0]) == json.dumps(plain[0]) and off[1:] == plain[1:]
    many = evalkit.records_from_results(samples, results)
    many_off = evalkit.records_from_results(samples, results, oracle=())
    assert json.dumps([m[0] for m in many_off]) == json.dumps([m[0] for m in many]) and json.dumps(many[0][0]) == json.dumps(plain[0])


def test_record_with_oracle_on_the_host(batch):
    samples, results = batch
    meta, mix, gt = samples[0]
    plain = evalkit.record_from_result(meta, mix, gt, results[0])[0]
    rec, tp, fp, fn = evalkit.record_from_result(meta, mix, gt, results[0], oracle=("irm", "ibm"))
    assert (tp, fp, fn) == (2, 1, 1) and len(rec["pred"]) == 2
    voices = [p["voice_id"] for p in rec["pred"]]
    assert voices == [0, 2]                                              # talker 1 is not matched and not reported
    for name in ("irm", "ibm"):
        est = om.masks_f64(gt, mix[0], name).astype(np.float32).astype(np.float64)
        sdr = evalkit.bss_eval_sdr(gt[voices].astype(np.float64), est[voices])
        for i, (p, s) in enumerate(zip(rec["pred"], voices)):
            assert p[f"si_snri_{name}"] == si_sdr(est[s], gt[s].astype(np.float64)) - p["si_snr_in"]
            assert p[f"si_snri_mir_{name}"] == float(sdr[i]) - p["si_snr_in_mir"]
            assert p[f"si_snri_{name}"] > 0.0                            # a mask of the truth improves on the mixture
    for p, q in zip(rec["pred"], plain["pred"]):                          # everything else as without
        assert {k: v for k, v in p.items() if k not in FIELDS} == q and list(p)[-4:] == list(FIELDS)
    one = evalkit.record_from_result(meta, mix, gt, results[0], oracle=("ibm",))[0]
    assert [k for k in one["pred"][0] if k in FIELDS] == ["si_snri_ibm", "si_snri_mir_ibm"]
    assert one["pred"][0]["si_snri_ibm"] == rec["pred"][0]["si_snri_ibm"]
    for call in (lambda: evalkit.record_from_result(meta, mix, gt, results[0], oracle=("wiener",)),
                 lambda: evalkit.records_from_results(samples, results, oracle=("irm", "psm")),
                 lambda: evalkit.compute_metrics(mix[:1], mix[:1], gt[:1], oracle=("x",)),
                 lambda: evalkit.evaluate_sample(None, meta, mix, gt, oracle="iam"),
                 lambda: evalkit.evaluate_dataset(None, "nowhere", oracle=("irm", "x"))):
        with pytest.raises(ValueError, match="oracle baselines"):
            call()


def test_records_with_oracle_through_stand_in_ops_give_the_host_records(batch):
    samples, results = batch
    want = evalkit.records_from_results(samples, results, "host", oracle=("irm", "ibm"))
    cross, oracle, stats = _CrossOp(), _OracleOp(), {}
    got = evalkit.records_from_results(samples, results, "device", ops=(cross, stand_in(), oracle), stats=stats,
                                       oracle=("irm", "ibm"))
    assert cross.calls == 1 and oracle.calls == 2 and oracle.items == 4 and "oracle_s" in stats
    assert [g[1:] for g in got] == [w[1:] for w in want]
    for (g, *_g), (w, *_w) in zip(got, want):
        assert len(g["pred"]) == len(w["pred"]) == 2
        for p, q in zip(g["pred"], w["pred"]):
            assert list(p) == list(q)
            for key in FIELDS + ("si_snri", "si_snri_mir"):
                assert abs(p[key] - q[key]) <= 1e-6, (key, p[key], q[key])


def test_program_parses_oracle(capsys):
    import importlib
    mod = importlib.import_module("acousticswarms_speech_amd.evaluate")
    assert mod.build_parser().parse_args(["DS"]).oracle == ()
    assert mod.build_parser().parse_args(["DS", "--oracle", "irm,ibm"]).oracle == ("irm", "ibm")
    assert mod.build_parser().parse_args(["DS", "--oracle", "ibm"]).oracle == ("ibm",)
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(["DS", "--oracle", "irm,wiener"])
    assert "oracle baselines" in capsys.readouterr().err


# ---------------------------------------------------------------- the C entry points: refused on the host
def _i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_oracle_masks_workspace_bytes():
    L = native.lib()
    for counts, lengths in (([1], [2048]), ([1, 3, 6], [2048, 3073, 5000]), ([64], [2048]), ([5] * 16, [48000] * 16)):
        K = len(counts)
        n = L.asw_oracle_masks_workspace_bytes(_i32(counts), _i32(lengths), K)
        frames = sum(S * om.frame_count(N) for S, N in zip(counts, lengths))
        assert n >= frames * 2048 * 8 and n % 8 == 0
        if max(counts) < 64:
            assert L.asw_oracle_masks_workspace_bytes(_i32([c + 1 for c in counts]), _i32(lengths), K) > n      # monotone
        assert L.asw_oracle_masks_workspace_bytes(_i32(counts), _i32([v + 1024 for v in lengths]), K) > n
        assert L.asw_oracle_masks_workspace_bytes(_i32(counts), _i32([v + 1 for v in lengths]), K) >= n
    for counts, lengths, message in (([-1], [2048], b"-1 references"), ([65], [2048], b"65 references"),
                                     ([1], [2047], b"2047 samples"), ([1, 1], [4096, 100], b"item 1: 100 samples"),
                                     ([1], [(1 << 25) + 1], b"33554433 samples")):
        assert L.asw_oracle_masks_workspace_bytes(_i32(counts), _i32(lengths), len(counts)) == 0
        assert b"oracle_masks_workspace_bytes" in L.asw_last_error() and message in L.asw_last_error(), L.asw_last_error()
    assert L.asw_oracle_masks_workspace_bytes(None, None, 1) == 0
    assert L.asw_oracle_masks_workspace_bytes(_i32([1]), _i32([2048]), 65536) == 0
    assert L.asw_oracle_masks_workspace_bytes(_i32([0]), _i32([2048]), 1) % 8 == 0      # no row at all: the table only


def test_entry_points_reject_bad_arguments_without_a_gpu():
    L = native.lib()
    buf = np.zeros(4096)
    p = ctypes.c_void_p(buf.ctypes.data)                                # never dereferenced: every call below is refused
    one, n2048, big = _i32([1]), _i32([2048]), 1 << 30

    def refused(message, mix=p, ref=p, c=one, n=n2048, K=1, stride=2048, kind=0, alpha=1.0, theta=0.5, out=p, ws=p,
                ws_bytes=big):
        assert L.asw_oracle_masks(mix, ref, c, n, K, stride, kind, alpha, theta, out, ws, ws_bytes, None) == -1
        assert message in L.asw_last_error(), L.asw_last_error()
    for null in ("mix", "ref", "out", "ws", "c", "n"):
        refused(b"oracle_masks: null", **{null: None})
    refused(b"K = -1", K=-1)
    refused(b"65 references", c=_i32([65]))
    refused(b"2047 samples", n=_i32([2047]))
    refused(b"exceed the stride", n=_i32([4096]))
    refused(b"neither IRM", kind=2)
    refused(b"not a number", alpha=float("nan"))
    refused(b"too small", ws_bytes=L.asw_oracle_masks_workspace_bytes(one, n2048, 1) - 8)
    refused(b"not 16-byte aligned", ws=ctypes.c_void_p(buf.ctypes.data + 8))
    assert L.asw_oracle_masks(None, None, None, None, 0, 2048, 0, 1.0, 0.5, None, None, 0, None) == 0    # K = 0
    # the two primitives
    assert L.asw_stft(None, 2, 4096, p, None) == -1 and b"stft: null pointer" in L.asw_last_error()
    assert L.asw_stft(p, 2, 2047, p, None) == -1 and b"stft: bad shape" in L.asw_last_error()
    assert L.asw_stft(None, 0, 4096, None, None) == 0
    assert L.asw_istft_workspace_bytes(2, 1) == 0 and b"istft_workspace_bytes" in L.asw_last_error()
    need = L.asw_istft_workspace_bytes(2, 5)
    assert need >= 2 * 5 * 2048 * 8 and need % 8 == 0
    assert L.asw_istft(None, 2, 5, 4096, p, p, need, None) == -1 and b"istft: null pointer" in L.asw_last_error()
    assert L.asw_istft(p, 2, 5, 4097, p, p, need, None) == -1 and b"what 5 frames cover" in L.asw_last_error()
    assert L.asw_istft(p, 2, 5, 4096, p, p, need - 8, None) == -1 and b"too small" in L.asw_last_error()
    assert L.asw_istft(None, 0, 5, 4096, None, None, 0, None) == 0
    assert not buf.any()
