"""BSS-eval SDR on the device (csrc/bss_kernels.hip) against ``evalkit.bss_eval_sdr`` on the same
float32-rounded inputs -- the repository's own float64 statement (mir_eval is absent: parity with it stays unpinned).

The bound.  MEASURED_DB is the largest |device - host| in dB over the cases of this file on an MI355X (perfect estimates
excluded); the tests assert ten times it, the slack being for the change of summation order with the grid.  The bound
may not exceed 1e-6 dB: the same algorithm in float64 on the CPU is eight orders below that.  Every test prints its
figure before it asserts."""
import ctypes
import functools
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import evalkit, native
from tests import bss_eval_cases as cases
from tests.bss_sources_cases import Once as _Once

pytestmark = pytest.mark.gpu

MEASURED_DB = 3.864e-14
BOUND_DB = 10 * MEASURED_DB
assert BOUND_DB <= 1e-6
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(seed, counts, T, flen, kinds=("mixture", "noisy")):
    """(refs, ests, host sdr [R, N]) of one generated batch: made once, shared, read-only."""
    refs, ests = cases.make_batch(seed, list(counts), T, kinds)
    want = cases.host_sdr(refs, ests, flen)
    for a in refs + ests + [want]:
        a.setflags(write=False)
    return refs, ests, want


def _op(refs, ests, flen):
    ref, est, counts = cases.pack(refs, ests)
    sdr, status = native.torch_ops().bss_eval_sdr(torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV), counts, flen)
    return sdr.cpu().numpy(), status.cpu().numpy()


def _check(tag, got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    err = float(np.max(np.abs(got - want))) if got.size else 0.0
    print(f"{tag}: max |device - host| = {err:.3e} dB over {got.size} values (bound {BOUND_DB:.1e})")
    assert np.all(np.isfinite(got)) and err <= BOUND_DB, (tag, err)


@pytest.mark.parametrize("counts", [(1,), (2,), (3, 1, 2), (0, 2, 0), (5,)])
def test_ragged_counts(counts):
    refs, ests, want = _case(11, counts, 1000, 16)
    got, status = _op(refs, ests, 16)
    assert status.tolist() == [0] * len(counts)
    _check(f"counts {counts}", got, want)


@pytest.mark.parametrize("S,flen", [(3, 21), (1, 64), (5, 13), (3, 43), (2, 64), (2, 1), (2, 2)])
def test_orders_around_a_tile_edge(S, flen):
    """Orders 63, 64, 65, 129 and 128 of the full system (tile 64), and one- and two-tap filters."""
    refs, ests, want = _case(12, (S,), 1000, flen)
    got, status = _op(refs, ests, flen)
    assert status.tolist() == [0]
    _check(f"S {S} flen {flen} order {S * flen}", got, want)


@pytest.mark.parametrize("T", ["flen", 257, 1000, 4099])
def test_sample_lengths(T):
    """One chunk, a chunk tail, several chunks with a tail; T == flen with one talker (two references of flen samples
    delayed by 0 .. flen - 1 span fewer than 2 flen dimensions: that Gram matrix has no factor)."""
    flen = 32
    counts = (1,) if T == "flen" else (2, 1)
    refs, ests, want = _case(13, counts, flen if T == "flen" else T, flen)
    got, status = _op(refs, ests, flen)
    assert status.tolist() == [0] * len(counts)
    _check(f"T {T}", got, want)


def test_three_kinds_of_estimate():
    refs, ests, want = _case(14, (3, 2), 2000, 24, cases.KINDS)
    got, status = _op(refs, ests, 24)
    assert got.shape == (3, 5) and status.tolist() == [0, 0]
    _check("kinds " + "/".join(cases.KINDS), got, want)


def test_working_size():
    refs, ests, want = _case(15, (3,), 16000, 512)
    got, status = _op(refs, ests, 512)
    assert status.tolist() == [0]
    _check("S 3 flen 512 T 16000", got, want)


def test_prefilled_outputs_and_workspace_give_equal_bytes():
    """The C entry point on buffers filled with 0xFF, then with 0x00: every output slot is written, nothing that is
    read was left from before."""
    refs, ests, want = _case(11, (3, 1, 2), 1000, 16)
    ref, est, counts = cases.pack(refs, ests)
    L, K, (R, N, T) = native.lib(), len(counts), est.shape
    c = (ctypes.c_int32 * K)(*counts)
    need = L.asw_bss_eval_sdr_workspace_bytes(c, K, R, T, 16)
    assert need == evalkit.bss_workspace_bytes(counts, R, T, 16)
    d_ref, d_est = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    outs = []
    for fill in (0xFF, 0x00, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        sdr = torch.full((R * N * 8,), fill, dtype=torch.uint8, device=DEV)
        status = torch.full((K * 4,), fill, dtype=torch.uint8, device=DEV)
        native.check(L.asw_bss_eval_sdr(native.ptr(d_ref), native.ptr(d_est), c, K, R, T, 16, native.ptr(sdr), native.ptr(status),
                                        native.ptr(ws), need, native.current_stream()))
        torch.cuda.synchronize()
        outs.append((sdr.cpu().numpy().tobytes(), status.cpu().numpy().tobytes()))
    assert outs[0] == outs[1] == outs[2]
    _check("prefilled", np.frombuffer(outs[0][0], dtype=np.float64).reshape(R, N), want)
    assert np.frombuffer(outs[0][1], dtype=np.int32).tolist() == [0, 0, 0]
    # the op gives the same bytes as the C call, call after call
    a, sa = _op(refs, ests, 16)
    b, sb = _op(refs, ests, 16)
    assert a.tobytes() == b.tobytes() == outs[0][0] and sa.tobytes() == sb.tobytes() == outs[0][1]


@functools.lru_cache(maxsize=None)
def _degenerate():
    refs, ests = cases.make_batch(16, [2, 3, 1, 2], 600)
    refs, ests = [r.copy() for r in refs], [e.copy() for e in ests]
    refs[1][2] = refs[1][0]                                            # a duplicated reference
    refs[3][1] = 0.0                                                   # an all-zero reference
    with np.errstate(all="ignore"):
        want = [np.stack([evalkit.bss_eval_sdr(r, e[s], 20) for s in range(2)]) for r, e in zip(refs, ests)]
    return refs, ests, want


def test_status_marks_degenerate_items_and_spares_their_neighbours():
    refs, ests, want = _degenerate()
    got, status = _op(refs, ests, 20)
    assert status.tolist() == [0, 1, 0, 1]
    _check("neighbours of degenerate items", np.concatenate([got[:, 0:2], got[:, 5:6]], axis=1),
           np.concatenate([want[0], want[2]], axis=1))


def test_batch_recomputes_degenerate_items_exactly():
    refs, ests, want = _degenerate()
    with np.errstate(divide="ignore"):                                 # the silent reference: log10(0) on the host route
        got, redone = evalkit.bss_eval_sdr_batch(refs, ests, flen=20, device=DEV)
    assert redone == [1, 3]
    for k in redone:
        assert got[k].tobytes() == want[k].tobytes()
    _check("batch, sound items", np.concatenate([got[0], got[2]], axis=1), np.concatenate([want[0], want[2]], axis=1))
    one = evalkit.bss_eval_sdr_device(refs[0], ests[0], flen=20, device=DEV)
    assert one.tobytes() == got[0].tobytes()


def test_perfect_estimate():
    refs, _ests, _want = _case(11, (2,), 1000, 16)
    host = evalkit.bss_eval_sdr(refs[0], refs[0], 16)
    got, status = _op(refs, [np.stack([refs[0]])], 16)
    print("perfect estimate: host", host, "device", got)
    assert status.tolist() == [0]
    assert np.all((host == np.inf) | (host > 200)) and np.all((got == np.inf) | (got > 200))


def test_adapter_refusals():
    op = native.torch_ops().bss_eval_sdr
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
        op(ref, est, [3], 0)
    with pytest.raises(RuntimeError, match="T = 100 outside flen = 101"):
        op(ref, est, [3], 101)
    sdr, status = op(ref[:0], est[:, :0], [], 8)                       # nothing to do is not an error
    assert tuple(sdr.shape) == (2, 0) and tuple(status.shape) == (0,)
    sdr, status = op(ref[:0], est[:, :0], [0, 0], 8)
    assert tuple(sdr.shape) == (2, 0) and status.tolist() == [0, 0]


def test_compute_metrics_device_against_host():
    rng = np.random.default_rng(17)
    gt = cases.references(rng, 2, 1500)
    inp, est = cases.estimates(rng, gt, "mixture"), cases.estimates(rng, gt, "noisy")
    host = evalkit.compute_metrics(inp, est, gt)
    dev = evalkit.compute_metrics(inp, est, gt, metrics="device")
    _check("compute_metrics", np.stack([dev[0], dev[1]]), np.stack([host[0], host[1]]))
    assert dev[2] == host[2] and dev[3] == host[3]                     # SI-SDR does not change


def test_record_device_against_host():
    """The scene and the model of test_evalkit.py::test_sample_directory_round_trip_and_record (surrogate scorer on the
    CPU; the ground truth there is one waveform per talker, repeated)."""
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
    with redirect_stdout(io.StringIO()):
        host = evalkit.evaluate_sample(model, meta, mixr, gt)
        dev = evalkit.evaluate_sample(model, meta, mixr, gt, metrics="device")
    assert host[1:] == dev[1:] and host[0].keys() == dev[0].keys() and len(host[0]["pred"]) >= 1
    for key in host[0]:
        if key != "pred":
            assert host[0][key] == dev[0][key], key
    for ph, pd in zip(host[0]["pred"], dev[0]["pred"]):
        assert ph.keys() == pd.keys()
        for key in ph:
            if key in ("si_snr_in_mir", "si_snri_mir"):
                err = abs(ph[key] - pd[key])
                print(f"record {key}: host {ph[key]!r} device {pd[key]!r} |d| {err:.3e}")
                assert err <= BOUND_DB
            else:
                assert ph[key] == pd[key], key
