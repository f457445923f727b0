"""GPU: the MUSIC / TOPS pruners (csrc/pruner_kernels.hip) -- the batched Hermitian eigensolver
against numpy.linalg.eigh, the covariance against the float64 restatement, the MUSIC / TOPS maps
against the reference's (fixtures g13 / g14), the whole search with Prone_method="MUSIC" against
the reference's stage trace (g15), a 16-mic full-ROI run, determinism.  Needs an MI355X."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests import pruners_restated as pr
from tests.golden.make_golden_pruners import ROI, checksum, scene
from tests.golden.surrogate import SurrogateSpot

pytestmark = pytest.mark.gpu
FULL_ROI = [-2.2, 2.25, 0.0, 6.2, 0.0, 0.9]


def _log(msg):
    """Print a diagnostic line; with ASW_DIAG_DIR set, also append it to diag_pruners.txt there."""
    d = os.environ.get("ASW_DIAG_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "diag_pruners.txt"), "a") as f:
            f.write(msg + "\n")
    print(msg)


def _ops():
    from acousticswarms_speech_amd import native
    return native.torch_ops()


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _node(mics, roi=ROI):
    from acousticswarms_speech_amd.mic_array import MicArray
    with redirect_stdout(io.StringIO()):
        return MicArray(mics, Spk_Range=roi, device="cuda").SRP_node


def _patches(node):
    with redirect_stdout(io.StringIO()):
        pk = node.find_valid_peak_new()
        ps = node.local_source_adaptive()
    return pk, ps


def _assert_same_patches(ps, g, pre=""):
    assert len(ps) == g[pre + "offsets"].shape[0]
    np.testing.assert_array_equal(np.stack([np.asarray(p.sample_offset, dtype=np.float64) for p in ps]), g[pre + "offsets"])
    np.testing.assert_array_equal(np.stack([np.asarray(p.width_list, dtype=np.float64) for p in ps]), g[pre + "widths"])
    np.testing.assert_array_equal(np.array([p.area_size() for p in ps]), g[pre + "npoints"])


def _spectrum(kind, M, rng):
    X = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
    U, _ = np.linalg.qr(X)
    if kind == "random":
        return X @ X.conj().T
    if kind == "rank3":
        lam = np.concatenate([1e-4 * (1 + rng.random(M - 3)), [3.0, 5.0, 9.0]])
    else:                                                  # near-degenerate pairs in the noise and the signal
        lam = np.concatenate([1e-3 * (1 + 1e-9 * np.arange(M - 3)), [2.0, 2.0 + 1e-9, 7.0]])
    return (U * lam) @ U.conj().T


@pytest.mark.parametrize("M", [4, 7, 16])
@pytest.mark.parametrize("kind", ["random", "rank3", "neardegenerate"])
def test_hermitian_eigh_against_numpy(M, kind):
    rng = np.random.default_rng(M * 10 + len(kind))
    A = np.stack([_spectrum(kind, M, rng) for _ in range(37)])
    A = 0.5 * (A + A.conj().transpose(0, 2, 1))
    w, V = _ops().hermitian_eigh(torch.from_numpy(A).cuda())
    w, V = w.cpu().numpy(), V.cpu().numpy()
    wr, Vr = np.linalg.eigh(A)
    scale = np.abs(wr).max(axis=1, keepdims=True)
    assert np.max(np.abs(w - wr) / np.abs(wr)) <= 1e-10
    P, Pr = V[..., -3:] @ V[..., -3:].conj().transpose(0, 2, 1), Vr[..., -3:] @ Vr[..., -3:].conj().transpose(0, 2, 1)
    sep = (wr[:, -3] - wr[:, -4]) / scale[:, 0] > 1e-3          # top-3 subspace well separated
    if sep.any():
        assert np.abs(P - Pr)[sep].max() <= 1e-9
    R = (V * w[:, None, :]) @ V.conj().transpose(0, 2, 1)
    assert np.abs(R - A).max() <= 1e-12 * scale.max()
    np.testing.assert_allclose(np.abs(V.conj().transpose(0, 2, 1) @ V), np.broadcast_to(np.eye(M), A.shape), atol=1e-12)


def test_covariance_matches_restatement():
    from acousticswarms_speech_amd.mic_array import FREQ_BINS, N_FFT
    _, _, mix = scene(48000)
    cov, mag = _ops().pruner_covariance(torch.from_numpy(mix).cuda(), int(FREQ_BINS[0]), len(FREQ_BINS), 24000, 24000, 2,
                                        N_FFT, N_FFT // 4)
    cov, mag = cov.cpu().numpy(), mag.cpu().numpy()
    for w in range(2):
        C, m = pr.covariance(pr.window_stft(mix, w * 24000, 24000, N_FFT), FREQ_BINS)
        err = np.abs(cov[w] - C).max(axis=(1, 2)) / np.abs(C).max(axis=(1, 2))
        _log(f"covariance window {w}: max rel err {err.max():.2e}")
        assert err.max() <= 1e-5
        np.testing.assert_allclose(mag[w], m, rtol=1e-5)


@pytest.mark.parametrize("T,tag", [(48000, "t48"), (144000, "t144")])
def test_music_map_matches_reference(golden, T, tag):
    g = golden("g13_music_map")
    mics, _, mix = scene(T)
    np.testing.assert_allclose(checksum(mix), g[f"{tag}_checksum"], rtol=1e-12)
    node = _node(mics)
    node.reset()
    node.MUSIC_Map_WINDOW(mix, window=int(g[f"{tag}_window"]))
    got, ref, spread = node.SRP_map.astype(np.float64), g[f"{tag}_map"], float(g[f"{tag}_spread"])
    err = _rel(got, ref)
    _log(f"MUSIC {tag}: max rel err vs reference {err:.3e} (stored spread {spread:.3e}), "
         f"vs restatement {_rel(got, pr.music_map(mix, int(g[f'{tag}_window']), node)):.3e}")
    assert err <= 2 * spread
    assert abs(node.MAX_POWER - float(g[f"{tag}_max_power"])) <= 2 * spread * abs(float(g[f"{tag}_max_power"]))
    assert abs(node.Min_POWER - float(g[f"{tag}_min_power"])) <= 2 * spread * abs(float(g[f"{tag}_min_power"]))
    pk, ps = _patches(node)
    assert pk == g[f"{tag}_peak_index"].tolist()
    _assert_same_patches(ps, g, f"{tag}_")
    if tag == "t48":                                       # window-0 eigenvalues of the device covariance
        from acousticswarms_speech_amd.mic_array import FREQ_BINS, N_FFT
        cov, _ = _ops().pruner_covariance(torch.from_numpy(mix).cuda(), int(FREQ_BINS[0]), len(FREQ_BINS), 24000, 24000, 1,
                                          N_FFT, N_FFT // 4)
        w, _ = _ops().hermitian_eigh(cov[0].contiguous())
        ev = g["t48_evals_w0"]
        assert np.max(np.abs(w.cpu().numpy() - ev) / np.abs(ev).max(axis=1, keepdims=True)) <= 1e-5


def test_tops_map_matches_reference(golden):
    g = golden("g14_tops_map")
    mics, _, mix = scene(int(g["T"]))
    np.testing.assert_allclose(checksum(mix), g["checksum"], rtol=1e-12)
    node = _node(mics)
    node.reset()
    node.TOPS_Map_WINDOW(mix, window=36000)
    got, ref, spread = node.SRP_map.astype(np.float64), g["map"], float(g["spread"])
    err = _rel(got, ref)
    _log(f"TOPS: max rel err vs reference {err:.3e} (stored spread {spread:.3e}), max_bin {node.tops_max_bin.tolist()}")
    assert node.tops_max_bin.tolist() == g["max_bin"].tolist()
    assert err <= 2 * spread
    assert abs(node.MAX_POWER - float(g["max_power"])) <= 2 * spread * abs(float(g["max_power"]))
    assert abs(node.Min_POWER - float(g["min_power"])) <= 2 * spread * abs(float(g["min_power"]))
    pk, ps = _patches(node)
    assert pk == g["peak_index"].tolist()
    _assert_same_patches(ps, g)


def test_tops_needs_a_whole_window():
    mics, _, mix = scene(48000)
    node = _node(mics)
    with pytest.raises(RuntimeError, match="72000"):
        node.TOPS_Map_WINDOW(mix, window=24000)


def test_maps_are_deterministic():
    mics, _, mix = scene(144000)
    node = _node(mics)
    for fn in (node.MUSIC_Map_WINDOW, node.TOPS_Map_WINDOW):
        fn(mix, window=36000)
        a = node.SRP_map.copy()
        fn(mix, window=36000)
        assert np.array_equal(a, node.SRP_map)


def test_pipeline_with_music_pruner_matches_reference_trace(golden):
    from acousticswarms_speech_amd.joint import JointModel
    g = golden("g15_music_stage_trace")
    mics, _, mix = scene(48000)
    np.testing.assert_allclose(checksum(mix), g["checksum"], rtol=1e-12)
    spot = SurrogateSpot()
    jm = JointModel(spot, None, device="cuda")
    with redirect_stdout(io.StringIO()):
        jm.setup(mics, ROI, prone_method="MUSIC")
        patches, _, _, _, _, spot_times = jm.forward(torch.from_numpy(mix))
    mp = jm.Mic_processor
    _log(f"pipeline(MUSIC): coarse kept {len(mp.trace['coarse_kept'])}, final {[p[3] for p in patches]}, "
         f"times {np.round(jm.times, 4)}")
    assert mp.Prone_method == "MUSIC"
    assert mp.trace["coarse_kept"] == g["kept"].tolist()
    assert spot.calls == [tuple(c) for c in g["calls"].tolist()]
    assert [p[3] for p in patches] == g["final_names"].tolist()
    np.testing.assert_allclose(np.stack([p[0].center_pos() for p in patches]), g["final_center"], atol=1e-6)
    assert spot_times == int(g["spot_times"])
    # the SRP configuration of the same geometry is a different cache entry
    with redirect_stdout(io.StringIO()):
        jm.setup(mics, ROI)
    assert jm.Mic_processor.Prone_method == "SRP"


def test_sixteen_mics_full_roi():
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(1010, 5, 16, 144000)
    node = _node(sc.mic_positions, FULL_ROI)
    G = node.grids.shape[0]
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(G, size=min(500, G), replace=False))
    node.MUSIC_Map_WINDOW(sc.mix, window=36000)
    mus = node.SRP_map.astype(np.float64)
    want = pr.music_map(sc.mix, 36000, node)
    e_m = _rel(mus[pick], want[pick])
    node.TOPS_Map_WINDOW(sc.mix, window=36000)
    tops = node.SRP_map.astype(np.float64)

    class Sub:                                             # TOPS restated at the sampled points only
        n_fft, freq_bins, tops_coef, tops_delta = node.n_fft, node.freq_bins, node.tops_coef, node.tops_delta[pick]
    want_t, bins = pr.tops_map(sc.mix, Sub)
    e_t = _rel(tops[pick], want_t)
    _log(f"16 mics, full ROI (G = {G}): MUSIC rel err {e_m:.2e}, TOPS rel err {e_t:.2e}, max_bin {bins.tolist()}")
    assert np.all(np.isfinite(mus)) and np.all(np.isfinite(tops))
    assert node.tops_max_bin.tolist() == bins.tolist()
    assert e_m <= 1e-5 and e_t <= 1e-5
