"""MUSIC / TOPS pruner fixtures (g13-g15): drive the REFERENCE's SRP_PHAT / Mic_Array with
Prone_method="MUSIC" / "TOPS" on the g7 scene recipe and record what they produce.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pruners.py [--only g13,g14,g15]

The GPU tests import ``scene`` from this module, so nothing here imports the reference at
module level.

Two adaptations of the reference are needed, both type conversions around the map and nothing
else (the map arithmetic and the peak picking are the reference's own):
* its ``reset()`` installs ``torch.zeros(G)`` as the map, and ``np.amax(tensor)`` in
  ``MUSIC_Map_WINDOW`` / ``TOPS_Map_WINDOW`` (SRP_Prunning.py:464,494) raises ``TypeError`` with
  the installed torch and numpy.  ``reset`` is wrapped so that it installs ``np.zeros(G)``;
* ``local_source_adaptive`` (:554) then calls ``SRP_map.numpy()``, which a numpy map lacks, so the
  two map methods are wrapped to hand the finished float64 map back as a torch tensor.

Besides the reference outputs each map fixture stores ``spread``: the largest relative difference
between the reference's (complex64) map and the float64 restatement in tests/pruners_restated.py.
Before saving, the generator checks that multiplying the reference map by (1 + u), |u| <= 3x that
spread, leaves the repo's patch list (SRPPhat.set_map + local_source_adaptive) unchanged.
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ROI = [-1.6, 1.6, 0.35, 2.75, 0.1, 0.7]          # the g7 region of interest
SCENE_SEED, N_SPK = 41, 3
NOISE_SEED = 7


def scene(T):
    """The g7 three-talker recipe (make_golden_search.scene_in_roi) at length T; at T = 48 000 it is
    that scene sample for sample."""
    from acousticswarms_speech_amd import scenes
    rng = np.random.default_rng(SCENE_SEED)
    mics, _ = scenes.desk_mics(rng, 7)
    spk = np.array([[-0.9, 1.4, 0.45], [0.7, 2.1, 0.30], [1.1, 0.9, 0.55]])
    mix = np.zeros((7, T))
    for s in range(N_SPK):
        x = scenes._speech_like(rng, T, 48000) * (0.5 - 0.1 * s)
        d = np.linalg.norm(spk[s] - mics, axis=1)
        for m in range(7):
            mix[m] += scenes._frac_delay(x, (d[m] - d[0]) / scenes.SPEED_OF_SOUND * 48000) * min(1.0, 1.0 / d[m])
    mix += 1e-3 * rng.standard_normal(mix.shape)
    return mics, spk, mix.astype(np.float32)


def checksum(mix):
    m = mix.astype(np.float64)
    return np.array([m.sum(), np.linalg.norm(m)])


def rel_spread(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def _ref_mic_array(mics, method):
    from sep.Mic_Array import Mic_Array
    with redirect_stdout(io.StringIO()):
        ma = Mic_Array(mics, Spk_Range=ROI, Prone_method=method)
    node = ma.SRP_node
    orig = node.reset

    def reset():                                   # adaptations (module docstring)
        orig()
        node.SRP_map = np.zeros(node.grids.shape[0])
    node.reset = reset
    import torch
    for name in ("MUSIC_Map_WINDOW", "TOPS_Map_WINDOW"):
        def wrapped(*a, _f=getattr(node, name), **k):
            _f(*a, **k)
            node.SRP_map = torch.from_numpy(np.asarray(node.SRP_map))
        setattr(node, name, wrapped)
    return ma


def _repo_node(mics):
    from acousticswarms_speech_amd.mic_array import MicArray
    with redirect_stdout(io.StringIO()):
        return MicArray(mics, Spk_Range=ROI).SRP_node


def _patches_of(node, m):
    from tests.golden.make_golden_search import _patch_arrays
    with redirect_stdout(io.StringIO()):
        node.set_map(m)
        return _patch_arrays(node.local_source_adaptive())


def _same_patches(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ("offsets", "widths", "npoints"))


def _check_margin(mics, ref_map, spread, ref_patches):
    node = _repo_node(mics)
    base = _patches_of(node, ref_map)
    assert _same_patches(base, ref_patches), "repo peak picking differs from the reference on the reference map"
    rng = np.random.default_rng(NOISE_SEED)
    for _ in range(4):
        u = rng.uniform(-3 * spread, 3 * spread, ref_map.shape)
        assert _same_patches(_patches_of(node, ref_map * (1 + u)), base), "patch list moves within 3x the spread"


def _map_outputs(ma, mix, name):
    import torch
    from tests.golden.make_golden_search import _patch_arrays
    node = ma.SRP_node
    with redirect_stdout(io.StringIO()):
        patches, _ = ma.Apply_SRP_PHAT(torch.from_numpy(mix))
        peak_index = node.find_valid_peak_new()
    ref = node.SRP_map.numpy().astype(np.float64)
    return ref, dict(map=ref, max_power=np.float64(node.MAX_POWER), min_power=np.float64(node.Min_POWER),
                     peak_index=np.array(peak_index), **_patch_arrays(patches))


def g13():
    """MUSIC at T = 48 000 (2 windows of 24 000) and T = 144 000 (4 windows of 36 000)."""
    from tests import pruners_restated as pr
    from sep.Traditional_SP.MUSIC_block import MUSIC
    from pyroomacoustics.transform.stft import analysis
    out = {}
    for T, tag in ((48000, "t48"), (144000, "t144")):
        mics, spk, mix = scene(T)
        ma = _ref_mic_array(mics, "MUSIC")
        ref, o = _map_outputs(ma, mix, tag)
        node = _repo_node(mics)
        win = 36000 if T >= 72000 else 24000
        rest = pr.music_map(mix, win, node)
        spread = rel_spread(ref, rest)
        _check_margin(mics, ref, spread, {k: o[k] for k in ("offsets", "widths", "npoints")})
        # the reference's window-0 eigenvalues (complex64 covariance, as MUSIC_process computes them)
        X = np.array([analysis(x, 2048, 512).T for x in mix[:, :win]])
        mu = MUSIC(ma.SRP_node.freq_bins, ma.SRP_node.mode_vec)
        mu.M = X.shape[0]
        evals = np.linalg.eigh(mu._compute_correlation_matricesvec(X))[0].astype(np.float64)
        o.update(checksum=checksum(mix), spread=np.float64(spread), evals_w0=evals, window=np.int64(win))
        out.update({f"{tag}_{k}": v for k, v in o.items()})
        print(f"g13 {tag}: spread {spread:.3e}, {len(o['peak_index'])} peaks, {o['offsets'].shape[0]} patches")
    _save("g13_music_map", scene_seed=np.int64(SCENE_SEED), roi=np.array(ROI), **out)


def g14():
    """TOPS at T = 144 000 (2 windows of 72 000)."""
    from tests import pruners_restated as pr
    T = 144000
    mics, spk, mix = scene(T)
    ma = _ref_mic_array(mics, "TOPS")
    ref, o = _map_outputs(ma, mix, "tops")
    node = _repo_node(mics)
    rest, bins = pr.tops_map(mix, node)
    spread = rel_spread(ref, rest)
    _check_margin(mics, ref, spread, {k: o[k] for k in ("offsets", "widths", "npoints")})
    # the reference's max_bin per window (TOPS_block.py:73-75, complex64 STFT)
    from pyroomacoustics.transform.stft import analysis
    fb = ma.SRP_node.freq_bins
    ref_bins = []
    for j in range(T // pr.TOPS_WINDOW):
        X = np.array([analysis(x, 2048, 512).T for x in mix[:, j * pr.TOPS_WINDOW:(j + 1) * pr.TOPS_WINDOW]])
        ref_bins.append(int(np.argmax(np.sum(np.sum(abs(X[:, fb, :]), axis=0), axis=1))))
    assert ref_bins == bins.tolist(), (ref_bins, bins)
    print(f"g14: spread {spread:.3e}, max_bin {ref_bins}, {len(o['peak_index'])} peaks, {o['offsets'].shape[0]} patches")
    _save("g14_tops_map", scene_seed=np.int64(SCENE_SEED), roi=np.array(ROI), T=np.int64(T), checksum=checksum(mix),
          spread=np.float64(spread), max_bin=np.array(ref_bins), **o)


def g15():
    """g10-style stage trace of the reference Mic_Array(Prone_method="MUSIC") with the surrogate scorer."""
    import torch
    from tests.golden.surrogate import SurrogateSpot
    mics, spk, mix = scene(48000)
    ma = _ref_mic_array(mics, "MUSIC")
    spot = SurrogateSpot()
    mix_t = torch.from_numpy(mix)
    with redirect_stdout(io.StringIO()):
        p1, _ = ma.Apply_SRP_PHAT(mix_t)
        srp_offsets = np.stack([np.asarray(p.sample_offset, dtype=np.float64) for p in p1])
        p2 = ma.Spotform_Big_Patch(mix_t, p1, spot)
        kept = [int(np.flatnonzero([q is p for q in p1])[0]) for p in p2]
        pairs = ma.Spotform_Small_Patch_Parallel(mix_t, p2, spot)
        audio, final, spot_times, _ = ma.Clustering_new(pairs)
    _save("g15_music_stage_trace", scene_seed=np.int64(SCENE_SEED), checksum=checksum(mix),
          n_srp=np.int64(len(p1)), srp_offsets=srp_offsets, kept=np.array(kept), calls=np.array(spot.calls),
          n_pairs=np.int64(len(pairs)), pair_names=np.array([p[3] for p in pairs]),
          final_names=np.array([p[3] for p in final]),
          final_center=np.stack([p[0].center_pos() for p in final]) if final else np.zeros((0, 3)),
          spot_times=np.int64(spot_times))
    print(f"g15: MUSIC {len(p1)} -> coarse {len(p2)} -> pairs {len(pairs)} -> final {len(final)}")


GENERATORS = {"g13": g13, "g14": g14, "g15": g15}


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from tests.golden import make_golden               # puts the reference on sys.path
    make_golden.install_stubs()
    import torch
    torch.set_num_threads(8)
    for k in [s for s in args.only.split(",") if s] or list(GENERATORS):
        print("==", k)
        GENERATORS[k]()


if __name__ == "__main__":
    main()
