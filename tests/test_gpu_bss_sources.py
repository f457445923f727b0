"""Full BSS-eval on the device (csrc/bss_kernels.hip: asw_bss_eval_sources) against
``evalkit.bss_eval_sources`` / ``evalkit.bss_eval_matrices`` on the same float32-rounded inputs -- the repository's own
float64 statement (mir_eval is absent: parity with it stays unpinned) -- never the device against itself.

The bounds.  MEASURED_DB holds the largest |device - statement| in dB over the cases of this file on an MI355X, separately
for SDR, SIR and SAR (perfect-estimate and +inf entries excluded); the tests assert ten times it, the slack being for the
change of summation order with the grid.  The SDR bound is the one tests/test_gpu_bss_eval.py asserts (3.864e-14 dB
measured in matched mode, here again); the off-diagonal entries of all-pairs mode, estimates scored against a
reference they hold nothing of, come to 2.984e-13 dB and sit under the same 3.864e-13 dB.  SIR: 9.052e-12 dB (S = 3,
flen = 512, T = 16 000); SAR: 5.684e-14 dB (S = 5, flen = 16).  No bound may exceed 1e-6 dB.  Every test prints its
figures before it asserts."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import evalkit, native
from tests import bss_sources_cases as sc
from tests.bss_sources_cases import Once as _Once

pytestmark = pytest.mark.gpu

MEASURED_DB = {"sdr": 3.864e-14, "sir": 9.052e-12, "sar": 5.684e-14}
BOUND_DB = {k: 10 * v for k, v in MEASURED_DB.items()}
assert all(b <= 1e-6 for b in BOUND_DB.values())
NAMES = ("sdr", "sir", "sar")
DEV = "cuda:0"


def _op(refs, ests, flen, all_pairs=False):
    ref, est, counts = sc.pack(refs, ests)
    *vals, status = native.torch_ops().bss_eval_sources(torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV), counts, flen,
                                                        all_pairs)
    return np.stack([v.cpu().numpy() for v in vals]), status.cpu().numpy()


def _check(tag, got, want):
    """got, want [3, ...]: sdr, sir, sar.  +inf must sit at the same places; the rest within the bounds."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    errs = []
    for q, name in enumerate(NAMES):
        g, w = got[q], want[q]
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.all(g[np.isinf(g)] > 0), (tag, name)
        fin = np.isfinite(w)
        assert np.all(np.isfinite(g[fin])), (tag, name)
        errs.append(float(np.max(np.abs(g[fin] - w[fin]))) if fin.any() else 0.0)
    print(f"{tag}: max |device - statement| sdr {errs[0]:.3e} sir {errs[1]:.3e} sar {errs[2]:.3e} dB over {got[0].size} rows "
          f"(bounds {BOUND_DB['sdr']:.1e} / {BOUND_DB['sir']:.1e} / {BOUND_DB['sar']:.1e})")
    for err, name in zip(errs, NAMES):
        assert err <= BOUND_DB[name], (tag, name, err)


@pytest.mark.parametrize("case", sc.MATCHED, ids=str)
def test_matched_mode(case):
    """Ragged counts; orders 63, 64, 65, 129, 128 of the full system (tile 64) and one- and two-tap filters; one chunk, a
    chunk tail, several chunks with a tail; three kinds of estimate; the working size."""
    refs, ests, want = sc.matched(*case)
    got, status = _op(refs, ests, case[3])
    assert status.tolist() == [0] * len(case[1])
    _check(f"matched {case[1:4]}", got, want)


@pytest.mark.parametrize("case", sc.PAIRS, ids=str)
def test_all_pairs_matrices(case):
    refs, ests, want = sc.pairs(*case)
    got, status = _op(refs, ests, case[3], all_pairs=True)
    assert status.tolist() == [0] * len(case[1])
    _check(f"all pairs {case[1:4]}", got, want)
    # the diagonal of every block is the matched call, bytes included: the same solves, the same sums
    matched, _ = _op(refs, ests, case[3])
    q0 = n0 = 0
    for S in case[1]:
        for j in range(S):
            assert got[:, :, q0 + j * S + j].tobytes() == matched[:, :, n0 + j].tobytes()
        q0, n0 = q0 + S * S, n0 + S


@pytest.mark.parametrize("case", sc.SHUFFLED, ids=str)
def test_batch_finds_the_known_permutations(case):
    refs, ests, perms, mats = sc.shuffled(*case)
    got, redone = evalkit.bss_eval_sources_batch(refs, ests, flen=case[3], compute_permutation=True, device=DEV)
    assert redone == [] and len(got) == len(refs)
    for k, (g, perm, m) in enumerate(zip(got, perms, mats)):
        S = perm.shape[1]
        assert g[3].dtype == np.int64 and g[3].tolist() == perm.tolist()
        idx = np.arange(S)
        want = np.stack([np.stack([m[r, q][perm[r], idx] for r in range(2)]) for q in range(3)])
        _check(f"shuffled {case[1:]} item {k}", np.stack(g[:3]), want)
    one = evalkit.bss_eval_sources_device(refs[0], ests[0], flen=case[3], compute_permutation=True, device=DEV)
    for a, b in zip(one, got[0]):
        assert a.tobytes() == b.tobytes()


def _c_call(d_ref, d_est, counts, flen, all_pairs, fill, want_all=True, ws_bytes=None):
    L, K, (R, N, T) = native.lib(), len(counts), d_est.shape
    c = (ctypes.c_int32 * K)(*counts)
    need = L.asw_bss_eval_sources_workspace_bytes(c, K, R, T, flen, all_pairs)
    assert need == evalkit.bss_sources_workspace_bytes(counts, R, T, flen, bool(all_pairs))
    if ws_bytes is not None:
        need = ws_bytes
    ncol = sum(S * S for S in counts) if all_pairs else N
    ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    outs = [torch.full((R * ncol * 8,), fill, dtype=torch.uint8, device=DEV) for _ in range(3)]
    status = torch.full((K * 4,), fill, dtype=torch.uint8, device=DEV)
    native.check(L.asw_bss_eval_sources(native.ptr(d_ref), native.ptr(d_est), c, K, R, T, flen, all_pairs, native.ptr(outs[0]),
                                        native.ptr(outs[1]) if want_all else None, native.ptr(outs[2]) if want_all else None,
                                        native.ptr(status), native.ptr(ws), need, native.current_stream()))
    torch.cuda.synchronize()
    return [o.cpu().numpy().tobytes() for o in outs], status.cpu().numpy().tobytes()


@pytest.mark.parametrize("all_pairs", [0, 1])
def test_prefilled_outputs_and_workspace_give_equal_bytes(all_pairs):
    """The C entry point on buffers filled with 0xFF, then with 0x00: every output slot is written, nothing that is
    read was left from before; and the op gives the same bytes call after call."""
    case = sc.PAIRS[0]
    refs, ests, want = (sc.pairs if all_pairs else sc.matched)(*case)
    ref, est, counts = sc.pack(refs, ests)
    d_ref, d_est = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    runs = [_c_call(d_ref, d_est, counts, 16, all_pairs, fill) for fill in (0xFF, 0x00, 0xFF)]
    assert runs[0] == runs[1] == runs[2]
    got = np.stack([np.frombuffer(b, dtype=np.float64).reshape(want.shape[1:]) for b in runs[0][0]])
    _check(f"prefilled, all_pairs {all_pairs}", got, want)
    assert np.frombuffer(runs[0][1], dtype=np.int32).tolist() == [0, 0, 0]
    a, sa = _op(refs, ests, 16, bool(all_pairs))
    b, sb = _op(refs, ests, 16, bool(all_pairs))
    assert a.tobytes() == b.tobytes() == got.tobytes() and sa.tobytes() == sb.tobytes() == runs[0][1]


@pytest.mark.parametrize("all_pairs", [0, 1])
def test_sdr_bytes_with_and_without_sir_and_sar(all_pairs):
    """sir = sar = null: the SDR alone, in the smaller workspace, untouched sir / sar buffers; matched, its bytes are those
    of ``torch.ops.asw.bss_eval_sdr``; and with sir and sar wanted the sdr bytes are still the same: the same two sums."""
    case = sc.PAIRS[0]
    refs, ests, _want = sc.matched(*case)
    ref, est, counts = sc.pack(refs, ests)
    d_ref, d_est = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    small = evalkit.bss_sources_workspace_bytes(counts, est.shape[0], est.shape[2], 16, bool(all_pairs), sdr_only=True)
    (sdr0, sir0, sar0), st0 = _c_call(d_ref, d_est, counts, 16, all_pairs, 0xFF, want_all=False, ws_bytes=small)
    (sdr1, _sir1, _sar1), st1 = _c_call(d_ref, d_est, counts, 16, all_pairs, 0x00)
    assert sdr0 == sdr1 and st0 == st1
    assert sir0 == sar0 == b"\xff" * len(sir0)
    if not all_pairs:
        assert small == evalkit.bss_workspace_bytes(counts, est.shape[0], est.shape[2], 16)
        old, status = native.torch_ops().bss_eval_sdr(d_ref, d_est, counts, 16)
        assert old.cpu().numpy().tobytes() == sdr0 and status.cpu().numpy().tobytes() == st0


def test_both_ops_give_the_same_sdr_and_status_bytes():
    """The two registered ops are one adapter: on the same inputs ``bss_eval_sdr`` (null sir / sar, the smaller workspace)
    and matched ``bss_eval_sources`` answer the same ``sdr`` and ``status``, byte for byte."""
    refs, ests = sc.cases.make_batch(19, [2, 0, 3, 1], 257)
    ref, est, counts = sc.pack(refs, ests)
    assert est.shape[0] == 2
    d_ref, d_est = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    sdr, status = native.torch_ops().bss_eval_sdr(d_ref, d_est, counts, 21)
    full, _sir, _sar, full_status = native.torch_ops().bss_eval_sources(d_ref, d_est, counts, 21, False)
    assert tuple(sdr.shape) == (2, 6) and status.cpu().tolist() == [0, 0, 0, 0]
    assert sdr.cpu().numpy().tobytes() == full.cpu().numpy().tobytes()
    assert status.cpu().numpy().tobytes() == full_status.cpu().numpy().tobytes()


def _degenerate():
    refs, ests = sc.cases.make_batch(16, [2, 3, 1, 2], 600)
    refs, ests = [r.copy() for r in refs], [e.copy() for e in ests]
    refs[1][2] = refs[1][0]                                            # a duplicated reference
    refs[3][1] = 0.0                                                   # an all-zero reference
    return refs, ests


@pytest.mark.parametrize("permute", [False, True])
def test_degenerate_items_are_marked_spare_their_neighbours_and_come_out_as_the_host(permute):
    refs, ests = _degenerate()
    got, status = _op(refs, ests, 20, all_pairs=permute)
    assert status.tolist() == [0, 1, 0, 1]
    with np.errstate(all="ignore"):
        want = [tuple(np.stack(v) for v in zip(*[evalkit.bss_eval_sources(r, e[s], 20, permute) for s in range(2)]))
                for r, e in zip(refs, ests)]
        mats = [np.stack([np.stack(evalkit.bss_eval_matrices(refs[k], ests[k][s], 20)) for s in range(2)]) for k in (0, 2)]
        batch, redone = evalkit.bss_eval_sources_batch(refs, ests, flen=20, compute_permutation=permute, device=DEV)
    assert redone == [1, 3]
    for k in redone:
        for a, b in zip(batch[k], want[k]):
            assert a.tobytes() == b.tobytes()
    for k in (0, 2):
        assert batch[k][3].tolist() == want[k][3].tolist()
        _check(f"batch, sound item {k}, permute {permute}", np.stack(batch[k][:3]), np.stack(want[k][:3]))
    # the op's own columns of the sound items: 0..1 and 5 matched, the blocks at 0 and 13 all pairs
    if permute:
        _check("neighbours, all pairs", np.concatenate([got[:, :, 0:4], got[:, :, 13:14]], axis=2),
               np.concatenate([mats[0].transpose(1, 0, 2, 3).reshape(3, 2, 4), mats[1].transpose(1, 0, 2, 3).reshape(3, 2, 1)], axis=2))
    else:
        _check("neighbours, matched", np.concatenate([got[:, :, 0:2], got[:, :, 5:6]], axis=2),
               np.concatenate([np.stack(want[0][:3]), np.stack(want[2][:3])], axis=2))


def test_one_talker_has_infinite_sir_on_both_sides():
    refs, ests, want = sc.matched(*sc.RAGGED[0])
    assert np.all(want[1] == np.inf)
    for all_pairs in (False, True):
        got, status = _op(refs, ests, 16, all_pairs)
        assert status.tolist() == [0] and np.all(got[1] == np.inf)
        assert got[0].tobytes() == got[2].tobytes()                       # e_interf is exactly 0: sar is the sdr
        _check(f"one talker, all_pairs {all_pairs}", got, want)


def test_adapter_refusals():
    op = native.torch_ops().bss_eval_sources
    ref, est = torch.zeros(3, 100, device=DEV), torch.zeros(2, 3, 100, device=DEV)
    with pytest.raises(RuntimeError, match="ref must be Float"):
        op(ref.double(), est, [3], 8)
    with pytest.raises(RuntimeError, match="est must be Float"):
        op(ref, est.half(), [3], 8)
    with pytest.raises(RuntimeError, match="ref must have 2 dimensions"):
        op(ref[0], est, [3], 8)
    with pytest.raises(RuntimeError, match=r"est must be \[R, N, T\]"):
        op(ref, est[:, :2].contiguous(), [3], 8)
    with pytest.raises(RuntimeError, match=r"est must be \[R, N, T\]"):
        op(ref, torch.zeros(2, 3, 99, device=DEV), [3], 8)
    with pytest.raises(RuntimeError, match="at least one estimate set"):
        op(ref, est[:0], [3], 8)
    with pytest.raises(RuntimeError, match="counts sum to 2, ref has 3 rows"):
        op(ref, est, [1, 1], 8)
    with pytest.raises(RuntimeError, match="outside 0..16"):
        op(ref, est, [4, -1], 8)
    with pytest.raises(RuntimeError, match="est must be contiguous"):
        op(ref, torch.zeros(2, 3, 200, device=DEV)[:, :, ::2], [3], 8)
    with pytest.raises(RuntimeError, match="ref must be contiguous"):
        op(torch.zeros(100, 3, device=DEV).t(), est, [3], 8)
    with pytest.raises(RuntimeError):                                 # no CPU implementation: the op is HIP only
        op(ref.cpu(), est.cpu(), [3], 8)
    with pytest.raises(RuntimeError, match="HIP"):
        op(ref, est.cpu(), [3], 8)
    with pytest.raises(RuntimeError, match="flen = 0 outside"):       # the library's own refusals come through
        op(ref, est, [3], 0, True)
    with pytest.raises(RuntimeError, match="T = 100 outside flen = 101"):
        op(ref, est, [3], 101)
    for all_pairs in (False, True):                                    # nothing to do is not an error
        *vals, status = op(ref[:0], est[:, :0], [], 8, all_pairs)
        assert all(tuple(v.shape) == (2, 0) for v in vals) and tuple(status.shape) == (0,)
        *vals, status = op(ref[:0], est[:, :0], [0, 0], 8, all_pairs)
        assert all(tuple(v.shape) == (2, 0) for v in vals) and status.tolist() == [0, 0]
    *vals, status = op(ref, est, [2, 1], flen=8, all_pairs=True)       # shapes of the packed matrices
    assert all(tuple(v.shape) == (2, 5) and v.dtype == torch.float64 for v in vals) and tuple(status.shape) == (2,)


def test_compute_metrics_device_against_host():
    rng = np.random.default_rng(17)
    gt = sc.cases.references(rng, 2, 1500)
    inp, est = sc.cases.estimates(rng, gt, "mixture"), sc.cases.estimates(rng, gt, "noisy")
    host = evalkit.compute_metrics(inp, est, gt, bss="all")
    dev = evalkit.compute_metrics(inp, est, gt, metrics="device", bss="all")
    _check("compute_metrics", np.stack([np.stack([dev[0], dev[1]]), np.stack(dev[4][:2]), np.stack(dev[4][2:])]),
           np.stack([np.stack([host[0], host[1]]), np.stack(host[4][:2]), np.stack(host[4][2:])]))
    assert dev[2] == host[2] and dev[3] == host[3]


def test_record_device_against_host():
    """The scene and the model of test_evalkit.py::test_sample_directory_round_trip_and_record (surrogate scorer on the
    CPU; the ground truth there is one waveform per talker, repeated, so a sample with several matches takes the host
    route and is then equal exactly)."""
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
    orig_setup = jm.setup

    def setup(mic_positions, speaker_range, **kw):
        orig_setup(mic_positions, speaker_range, **kw)
        node = jm.Mic_processor.SRP_node
        node.SRP_Map_WINDOW_new = lambda signal, window=36000: node.set_map(g7["srp_map"])
    jm.setup = setup
    model = _Once(jm)
    gt = np.stack([mixr[0]] * spk.shape[0]).astype(np.float32)
    with redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        host = evalkit.evaluate_sample(model, meta, mixr, gt, bss="all")
        dev = evalkit.evaluate_sample(model, meta, mixr, gt, metrics="device", bss="all")
        plain = evalkit.evaluate_sample(model, meta, mixr, gt, metrics="device")
    assert host[1:] == dev[1:] and host[0].keys() == dev[0].keys() and len(host[0]["pred"]) >= 1
    for key in host[0]:
        if key != "pred":
            assert host[0][key] == dev[0][key], key
    bound = {"si_snr_in_mir": BOUND_DB["sdr"], "si_snri_mir": BOUND_DB["sdr"], "sir_in_mir": BOUND_DB["sir"],
             "sir_mir": BOUND_DB["sir"], "sar_in_mir": BOUND_DB["sar"], "sar_mir": BOUND_DB["sar"]}
    for ph, pd, pp in zip(host[0]["pred"], dev[0]["pred"], plain[0]["pred"]):
        assert ph.keys() == pd.keys() and set(pd) - set(pp) == {"sir_in_mir", "sir_mir", "sar_in_mir", "sar_mir"}
        for key in ph:
            if key in bound:
                print(f"record {key}: host {ph[key]!r} device {pd[key]!r}")
                assert ph[key] == pd[key] or abs(ph[key] - pd[key]) <= bound[key]
            else:
                assert ph[key] == pd[key], key
