"""GPU: the SRP-PHAT map kernels (csrc/srp_kernels.hip) stage by stage against the float64 reference of
tests/srp_restated.py -- the DFT + PHAT + cross-spectrum stage (ops.srp_cross_spectra), the steered-map stage
(ops.srp_map) and the whole op (torch.ops.asw.srp_phat_map) -- on shapes that reach every path of the kernels:
a second and third pass over the windows, more pairs than one block, ragged and empty bin slices, a single frame,
nb_pad of 64 and 128, grids of 1 / 255 / 256 / 257 points, the clamp at zero and the PHAT floor.

Every bar comes from the references alone: 4 x the distance of the float32 restatement from float64 (the factor
covers the different summation order of the MFMA K-loop and of the k-slices), with a floor of a few float32
roundings.  Each assertion logs the measured error, the yardstick and the bar.  Needs an MI355X."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests import srp_restated as sr

pytestmark = pytest.mark.gpu
CASES = sorted(sr.SHAPES)
RTOL, ATOL = 2e-4, 2e-5                     # the bar of test_gpu_srp_pipeline.py: every whole-op result stays inside it too


def _log(msg):
    """Print a diagnostic line; with ASW_DIAG_DIR set, also append it to diag_srp_kernels.txt there."""
    d = os.environ.get("ASW_DIAG_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "diag_srp_kernels.txt"), "a") as f:
            f.write(msg + "\n")
    print(msg)


def _ops():
    from acousticswarms_speech_amd import native
    return native.torch_ops()


_DEV = {}


def _dev(name):
    """Device copies of one case's operands (uploaded once)."""
    if name not in _DEV:
        from acousticswarms_speech_amd.srp import _twiddles
        c = sr.case(name)
        dev = torch.device("cuda", torch.cuda.current_device())
        nb_pad, tw = _twiddles(c.bins, c.shape.nfft, dev)
        assert nb_pad == (c.shape.nbins + 63) // 64 * 64
        up = lambda a: torch.from_numpy(np.array(a)).to(dev)            # noqa: E731  (np.array: a writable copy)
        _DEV[name] = dict(mix=up(c.mix), tw=tw, pi=up(c.pair_i), pj=up(c.pair_j), tau=up(c.tau), omega=up(c.omega))
    return _DEV[name]


def _cross_spectra(name, mix=None, n_windows=None):
    from acousticswarms_speech_amd import ops
    c, d = sr.case(name), _dev(name)
    s = c.shape
    cc = ops.srp_cross_spectra(d["mix"] if mix is None else mix, d["tw"], d["pi"], d["pj"], s.nbins, s.window, c.step,
                               s.n_windows if n_windows is None else n_windows, s.nfft, s.nfft // 4, sr.TOL)
    return cc


def _complex(cc):
    a = cc.cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _whole(name, mix=None, tau=None, n_windows=None, window=None, step=None):
    c, d = sr.case(name), _dev(name)
    s = c.shape
    out = _ops().srp_phat_map(d["mix"] if mix is None else mix, d["tw"], d["pi"], d["pj"], d["tau"] if tau is None else tau,
                              d["omega"], s.window if window is None else window, c.step if step is None else step,
                              s.n_windows if n_windows is None else n_windows, s.nfft, s.nfft // 4, sr.TOL)
    return out.cpu().numpy()


def _check_whole(tag, got, ref_map, ref_raw, yard):
    """The whole-op assertions: max-abs bar, the inherited rtol/atol bar, and the set of exact zeros."""
    bar = max(4 * yard, 2e-6)
    err = sr.max_abs(got.astype(np.float64), ref_map)
    zero = got == 0.0
    must, never = ref_raw < -bar, ref_raw > bar
    _log(f"{tag} whole op: max abs err {err:.3e}, yardstick {yard:.3e}, bar {bar:.3e}; exact zeros {int(zero.sum())} of "
         f"{zero.size} (reference below -bar: {int(must.sum())}, above +bar: {int(never.sum())}); map max {ref_map.max():.4f}")
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    assert err <= bar
    np.testing.assert_allclose(got, ref_map, rtol=RTOL, atol=ATOL)
    assert np.all(zero[must]), "a point with a negative reference response is not exactly 0.0f"
    assert not np.any(zero[never]), "a point with a positive reference response came out as 0.0f"


# ---- the three stages, case by case -------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_cross_spectra_stage(name):
    r = sr.refs(name)
    got = _complex(_cross_spectra(name))
    assert got.shape == r.cc64.shape and np.all(np.isfinite(got))
    err, bar = sr.rel_l2(got, r.cc64), max(4 * r.yard_cc, 1e-6)
    _log(f"case {name} cross-spectra: rel L2 err {err:.3e}, yardstick {r.yard_cc:.3e}, bar {bar:.3e}; "
         f"max abs err {sr.max_abs(got, r.cc64):.3e} (restatement {sr.max_abs(r.cc32, r.cc64):.3e})")
    assert err <= bar


def _map_stage(name, n_points=None):
    from acousticswarms_speech_amd import ops
    r, d = sr.refs(name), _dev(name)
    cc = np.ascontiguousarray(np.stack([r.cc64.real, r.cc64.imag], axis=-1).astype(np.float32))
    tau = d["tau"] if n_points is None else d["tau"][:n_points].contiguous()
    got = ops.srp_map(torch.from_numpy(cc).cuda(), tau, d["omega"], d["pi"], d["pj"]).cpu().numpy()
    sl = slice(None, n_points)
    yard = sr.max_abs(r.map32_stage[sl].astype(np.float64), r.map64[sl])
    return got, r.map64[sl], yard


@pytest.mark.parametrize("name,n_points", [(n, None) for n in CASES] + [("e", 1)])
def test_map_stage_alone(name, n_points):
    got, ref, yard = _map_stage(name, n_points)
    err, bar = sr.max_abs(got.astype(np.float64), ref), max(4 * yard, 1e-6)
    _log(f"case {name} (G = {ref.size}) map stage: max abs err {err:.3e}, yardstick {yard:.3e}, bar {bar:.3e}; "
         f"map {ref.min():.4f}..{ref.max():.4f}")
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert err <= bar


@pytest.mark.parametrize("name,n_points", [(n, None) for n in CASES] + [("e", 1)])
def test_whole_op(name, n_points):
    r, d = sr.refs(name), _dev(name)
    sl = slice(None, n_points)
    got = _whole(name, tau=None if n_points is None else d["tau"][:n_points].contiguous())
    yard = sr.max_abs(r.map32_whole[sl].astype(np.float64), r.map64[sl])
    _check_whole(f"case {name} (G = {got.size})", got, r.map64[sl], r.per64.max(axis=0)[sl], yard)


# ---- properties that need no oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("delays", ["roi", "one_second"])
def test_known_answer(delays):
    """Cross-spectra that are the conjugate steering vector of one grid point g0 give exactly 1 there and nothing
    above 1 anywhere.  With delays spread over a second the phases reach 2.5e4 rad: the range reduction has to be
    done in double, a float phase would be off by 1e-3 rad."""
    from acousticswarms_speech_amd import ops
    c, d = sr.case("b"), _dev("b")
    rng = np.random.default_rng(21)
    tau = np.array(c.tau) if delays == "roi" else rng.uniform(0.0, 1.0, c.tau.shape)
    g0 = 101
    dt = tau[g0, c.pair_i] - tau[g0, c.pair_j]
    z = np.exp(-1j * c.omega[:, None] * dt[None, :])                              # [nbins, P] float64
    cc = torch.from_numpy(np.stack([z.real, z.imag], axis=-1)[None].astype(np.float32)).cuda()
    got = ops.srp_map(cc, torch.from_numpy(tau).cuda(), d["omega"], d["pi"], d["pj"]).cpu().numpy().astype(np.float64)
    _log(f"known answer ({delays}): map[g0] - 1 = {got[g0] - 1:.3e}, max elsewhere {np.delete(got, g0).max():.6f}, "
         f"largest phase {np.abs(c.omega[-1] * dt).max():.3e} rad")
    assert abs(got[g0] - 1.0) <= 1e-6
    assert got.max() <= 1.0 + 1e-6


@pytest.mark.parametrize("name", ["c", "e"])
def test_windows_equal_single_window_calls(name):
    """The multi-window call (passes of 8 windows, running maximum through out[g]) against the element-wise maximum
    of n_windows single-window calls on contiguous copies of the window slices.  The DFT GEMM reads the same
    samples in the same K order whatever the base pointer and the row pitch, so the results are expected bit-equal."""
    c, d = sr.case(name), _dev(name)
    s = c.shape
    whole = _whole(name)
    best = np.zeros_like(whole)
    for w in range(s.n_windows):
        piece = d["mix"][:, w * c.step:w * c.step + s.window].contiguous()
        best = np.maximum(best, _whole(name, mix=piece, n_windows=1))
    diff = float(np.abs(whole - best).max())
    _log(f"case {name}: {s.n_windows}-window call vs maximum of single-window calls: max abs diff {diff:.3e}, "
         f"bit-equal {np.array_equal(whole, best)}")
    assert np.array_equal(whole, best)


def test_case_e_is_deterministic():
    a, b = _whole("e"), _whole("e")
    cc_a, cc_b = _cross_spectra("e").cpu().numpy(), _cross_spectra("e").cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(cc_a, cc_b)


def test_all_zero_mixture_gives_a_zero_map():
    d = _dev("b")
    got = _whole("b", mix=torch.zeros_like(d["mix"]))
    assert np.all(got == 0.0)
    assert np.all(_cross_spectra("b", mix=torch.zeros_like(d["mix"])).cpu().numpy() == 0.0)


def test_one_silent_channel_takes_the_phat_floor():
    """Channel 3 of case b zeroed: |X| = 0 there is floored at tol by the kernel and by the reference alike, so its
    pairs contribute exactly nothing and the map is that of the other six channels over all 21 pairs."""
    c, d = sr.case("b"), _dev("b")
    mix = np.array(c.mix)
    mix[3] = 0.0
    r = sr.refs("b", mix=mix, key="b_channel3_silent")
    dm = d["mix"].clone()
    dm[3] = 0.0
    touched = (c.pair_i == 3) | (c.pair_j == 3)
    assert np.all(r.cc64[:, :, touched] == 0) and np.all(_complex(_cross_spectra("b", mix=dm))[:, :, touched] == 0)
    _check_whole("case b, channel 3 silent", _whole("b", mix=dm), r.map64, r.per64.max(axis=0), r.yard_whole)


# ---- refusals: on the host, before any launch, with the constraint in the message ----------------------------------
def _still_works():
    """A refused call leaves nothing behind: the smallest case still meets its bar afterwards."""
    r = sr.refs("a")
    torch.cuda.synchronize()
    assert sr.max_abs(_whole("a").astype(np.float64), r.map64) <= max(4 * r.yard_whole, 2e-6)


def test_refuses_a_window_whose_half_is_no_multiple_of_four():
    from acousticswarms_speech_amd.mic_array import MicArray
    from tests.golden.make_golden_search import ROI, scene_in_roi
    mics, _, mix = scene_in_roi()
    with redirect_stdout(io.StringIO()):
        node = MicArray(mics, Spk_Range=ROI, device="cuda").SRP_node
    with pytest.raises(RuntimeError, match="multiples of 4"):
        node.SRP_Map_WINDOW_new(mix, window=24002)
    _still_works()


def test_refuses_a_window_shorter_than_a_frame():
    s = sr.case("b").shape
    with pytest.raises(RuntimeError, match="shorter than one 256-sample frame"):
        _whole("b", window=s.nfft // 2, step=s.nfft // 4, n_windows=1)
    with pytest.raises(RuntimeError, match="shorter than one 256-sample frame"):
        _whole("b", window=s.nfft - 4, step=s.nfft // 2, n_windows=1)
    from acousticswarms_speech_amd import ops
    d = _dev("b")
    for window in (s.nfft // 2, s.nfft - 4):                      # the stage entry point, with and without a whole hop missing
        with pytest.raises(RuntimeError, match="shorter than one 256-sample frame"):
            ops.srp_cross_spectra(d["mix"], d["tw"], d["pi"], d["pj"], s.nbins, window, s.nfft // 2, 1, s.nfft, s.nfft // 4)
    _still_works()


@pytest.mark.parametrize("M", [1, 33])
def test_refuses_an_unsupported_microphone_count(M):
    from acousticswarms_speech_amd import ops
    c, d = sr.case("b"), _dev("b")
    s = c.shape
    ii, jj = np.triu_indices(M, k=1)
    pi, pj = torch.from_numpy(ii.astype(np.int32)).cuda(), torch.from_numpy(jj.astype(np.int32)).cuda()
    mix = torch.zeros((M, c.T), dtype=torch.float32, device="cuda")
    tau = torch.zeros((s.G, M), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=f"{M} microphones"):
        _ops().srp_phat_map(mix, d["tw"], pi, pj, tau, d["omega"], s.window, c.step, s.n_windows, s.nfft, s.nfft // 4, sr.TOL)
    with pytest.raises(RuntimeError, match=f"{M} microphones"):
        ops.srp_cross_spectra(mix, d["tw"], pi, pj, s.nbins, s.window, c.step, s.n_windows, s.nfft, s.nfft // 4)
    cc = torch.zeros((1, s.nbins, len(ii), 2), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=f"{M} microphones"):
        ops.srp_map(cc, tau, d["omega"], pi, pj)
    _still_works()


def test_refuses_windows_past_the_end_of_the_mixture():
    s = sr.case("b").shape
    with pytest.raises(RuntimeError, match="past the end"):
        _whole("b", n_windows=s.n_windows + 1)
    with pytest.raises(RuntimeError, match="past the end"):       # the stage entry point judges all windows up front
        _cross_spectra("b", n_windows=s.n_windows + 1)
    _still_works()


# ---- through the product API: 16 microphones on the full region of interest ----------------------------------
@pytest.fixture(scope="module")
def sixteen():
    from acousticswarms_speech_amd.mic_array import MicArray
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 16, 144000)
    with redirect_stdout(io.StringIO()):
        node = MicArray(sc.mic_positions, Spk_Range=sr.FULL_ROI, device="cuda").SRP_node
    G = node.grids.shape[0]
    pick = np.sort(np.random.default_rng(5).choice(G, size=500, replace=False))
    return node, sc, pick


def _product(node, mix, pick, window, n_windows, tag):
    cc = sr.cc64(mix, window, node.n_fft, node.freq_bins)
    assert cc.shape[0] == n_windows
    tau = node.tau[pick]
    ref, per = sr.window_maps64(cc, tau, node.omega)
    yard = sr.max_abs(sr.window_maps32(sr.cc32(mix, window, node.n_fft, node.freq_bins), tau, node.omega)[0].astype(np.float64),
                      ref)
    node.reset()
    node.SRP_Map_WINDOW_new(mix, window=window)
    got = node.SRP_map
    _check_whole(f"16 mics, full ROI (G = {got.size}), {tag}", got[pick], ref, per.max(axis=0), yard)
    # MAX_POWER and the arg-max: the reference at the kernel's own strongest point and its nearest rivals
    bar = max(4 * yard, 2e-6)
    top = np.argsort(got)[-8:]
    ref_top = sr.window_maps64(cc, node.tau[top], node.omega)[0]
    _log(f"{tag}: MAX_POWER {node.MAX_POWER:.6f} vs reference {ref_top.max():.6f} at the kernel's top points "
         f"(arg-max {int(np.argmax(got))})")
    assert abs(node.MAX_POWER - float(ref_top.max())) <= bar
    assert int(np.argmax(got[pick])) == int(np.argmax(ref))
    assert int(top[-1]) == int(top[np.argmax(ref_top)]) == int(np.argmax(got))


def test_sixteen_mics_seven_windows(sixteen):
    node, sc, pick = sixteen
    _product(node, sc.mix, pick, 36000, 7, "window 36000, 7 windows")


def test_sixteen_mics_twelve_windows_second_pass(sixteen):
    """A 160 000-sample mixture at window 24 000: 12 windows, the product path's first run of the second pass."""
    from acousticswarms_speech_amd.scenes import make_scene
    node, sc, pick = sixteen
    mix = make_scene(1010, 5, 16, 160000, mic_positions=sc.mic_positions).mix
    _product(node, mix, pick, 24000, 12, "window 24000, 12 windows")
