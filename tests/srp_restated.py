"""References for the two stages of the SRP-PHAT map (csrc/srp_kernels.hip), CPU only.

``cc64`` / ``map64`` are the float64 reference: oracle/srp_ref.py stays in complex128 when it is given a
float64 signal, so they are that oracle plus a helper that goes from cross-spectra to the map and keeps the
per-window maps.  ``cc32`` / ``map32`` restate the same two stages in float32 with the precision plan of the
kernel header (float32 DFT as a matmul against the float32 twiddle table, float32 hypot and divide, complex64
frame mean; phase formed and range-reduced in float64, float32 cos / sin, float32 sequential accumulation over
(pair, bin)) and with no knowledge of tiles, slices or passes.  They are a yardstick only: the GPU tests take
their bars from the distance between the two, never from what the kernels return.

``case(name)`` builds the synthetic inputs of tests/test_gpu_srp_kernels.py (and the conditions that
tests/test_srp_restated_host.py checks on them) once per process; the arrays are read-only.
"""
from collections import namedtuple

import numpy as np

from oracle import srp_ref

FULL_ROI = [-2.2, 2.25, 0.0, 6.2, 0.0, 0.9]
SOUND = 343.0
FS = 16000                       # omega = 2 pi FS k / nfft, as mic_array.py builds it
TOL = 1e-8

Shape = namedtuple("Shape", "M nfft bin0 nbins window n_windows G seed")
# the smallest shapes that still reach each path of the kernels (hop = nfft / 4, step = window / 2 everywhere)
SHAPES = {
    "a": Shape(2, 256, 1, 5, 256, 1, 257, 11),        # one frame, nbins < 8 (empty k-slices), half the map clamped
    "b": Shape(7, 256, 2, 64, 1024, 8, 255, 12),      # exactly one full pass of 8 windows, nb_pad == nbins
    "c": Shape(7, 256, 2, 65, 1024, 9, 256, 13),      # second pass with one window, nb_pad = 128
    "d": Shape(16, 2048, 2, 198, 8192, 3, 300, 14),   # the product's bin range, P = 120
    "e": Shape(32, 256, 2, 40, 1024, 17, 300, 15),    # P = 496 > 256, 64 KiB of LDS, three passes
    "f": Shape(24, 256, 2, 11, 512, 2, 100, 16),      # P = 276 just over one block, ragged k-slices
}

Case = namedtuple("Case", "shape mics mix bins omega tau pair_i pair_j step T")
_CASES, _REFS = {}, {}


def _frozen(a):
    a.setflags(write=False)
    return a


def roi_delays(rng, G, mics):
    """[G, M] propagation delays (s) from G random points of the full region of interest."""
    r = FULL_ROI
    pts = np.stack([rng.uniform(r[0], r[1], G), rng.uniform(r[2], r[3], G), rng.uniform(r[4], r[5], G)], axis=1)
    return np.linalg.norm(pts[:, None, :] - mics[None], axis=2) / SOUND


def case(name):
    """Mixture of n_windows talkers from scenes.make_scene on one array.  Talker k is loud during the middle half of
    window k and faint elsewhere (seeded levels): window k hears it for half its length, the two neighbours for a
    quarter, so every window has a direction of its own and no window's response is a copy of another's."""
    if name in _CASES:
        return _CASES[name]
    from acousticswarms_speech_amd.scenes import make_scene
    s = SHAPES[name]
    step = s.window // 2
    T = step * (s.n_windows + 1)
    rng = np.random.default_rng(s.seed)
    T_gen = 24000
    mics = make_scene(s.seed, 1, s.M, 16).mic_positions
    mix = np.zeros((s.M, T))
    half = step // 2
    # an array tells talkers apart by direction far better than by range: from 8 seeded candidates per window keep
    # the ones evenly spread in azimuth, and hand them to the windows in a seeded order
    cand = [1000 * s.seed + i for i in range(8 * s.n_windows)]
    spk = np.stack([make_scene(q, 1, s.M, 16, mic_positions=mics).speaker_positions[0] for q in cand])
    by_azimuth = np.argsort(np.arctan2(spk[:, 0] - mics[:, 0].mean(), spk[:, 1] - mics[:, 1].mean()))
    keep = by_azimuth[np.round(np.linspace(0, len(cand) - 1, s.n_windows)).astype(int)]
    for k, q in enumerate(rng.permutation(keep)):
        one = make_scene(cand[q], 1, s.M, T_gen, fs=FS, noise_std=0.0, mic_positions=mics).mix.astype(np.float64)
        power = np.convolve(one[0] ** 2, np.ones(step), mode="valid")    # energy of every step-long span
        lo = k * step + half                                             # the loud span starts here in the mixture
        t0 = int(np.argmax(power[lo:T_gen - T + lo + 1]))                # the talker's loudest span is moved there
        level = np.full(T, 0.02 * rng.uniform(0.5, 1.0))
        level[lo:lo + step] = rng.uniform(0.5, 1.0)
        mix += one[:, t0:t0 + T] * level[None, :]
    mix += 1e-3 * rng.standard_normal(mix.shape)
    bins = np.arange(s.bin0, s.bin0 + s.nbins)
    ii, jj = np.triu_indices(s.M, k=1)
    c = Case(s, _frozen(mics), _frozen(mix.astype(np.float32)), _frozen(bins), _frozen(2 * np.pi * FS * bins / s.nfft),
             _frozen(roi_delays(rng, s.G, mics)), _frozen(ii.astype(np.int32)), _frozen(jj.astype(np.int32)), step, T)
    _CASES[name] = c
    return c


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(np.ravel(b)))


def max_abs(a, b):
    return float(np.max(np.abs(a - b)))


# ---- float64 reference ---------------------------------------------------------------------------------
def cc64(mix, window, nfft, bins, tol=TOL):
    """[n_windows, nbins, P] complex128 (oracle/srp_ref.cross_spectra on the signal cast to float64)."""
    return np.stack(srp_ref.cross_spectra(np.asarray(mix, dtype=np.float64), window, nfft, np.asarray(bins), tol))


def window_maps64(cc, tau, omega, chunk=256):
    """cc [W, nbins, P] -> (map [G]: running maximum from zeros, raw per-window responses [W, G]), float64.
    The steering block of one chunk is three chunk * nbins * P float64 arrays (146 MB at 16 microphones, 198 bins)."""
    W, nb, P = cc.shape
    M = tau.shape[1]
    ii, jj = np.triu_indices(M, k=1)
    assert len(ii) == P
    dt = tau[:, ii] - tau[:, jj]
    flat = np.asarray(cc, dtype=np.complex128).reshape(W, nb * P)
    fr, fi = np.ascontiguousarray(flat.real), np.ascontiguousarray(flat.imag)
    G = tau.shape[0]
    per = np.empty((W, G))
    for g0 in range(0, G, chunk):
        ph = (omega[None, :, None] * dt[g0:g0 + chunk, None, :]).reshape(-1, nb * P)
        per[:, g0:g0 + chunk] = (fr @ np.cos(ph).T - fi @ np.sin(ph).T) / (nb * P)   # Re(cc * exp(j ph)), summed
    return np.maximum(per.max(axis=0), 0.0), per


def map64(mix, window, nfft, bins, tau, omega, tol=TOL):
    return window_maps64(cc64(mix, window, nfft, bins, tol), tau, omega)[0]


def min_nonzero_magnitude(mix, window, nfft, bins):
    """(smallest non-zero |X|, number of exactly-zero values) over every used bin, frame, microphone and window."""
    x = np.asarray(mix, dtype=np.float64)
    step = window // 2
    lo, zeros = np.inf, 0
    for j in range(x.shape[1] // step - 1):
        if j * step + window > x.shape[1]:
            break
        for ch in x[:, j * step:j * step + window]:
            a = np.abs(srp_ref.stft_frames(ch, nfft, nfft // 4)[:, bins])
            zeros += int(np.count_nonzero(a == 0))
            if np.any(a > 0):
                lo = min(lo, float(a[a > 0].min()))
    return lo, zeros


# ---- float32 yardstick ---------------------------------------------------------------------------------
def twiddles32(bins, nfft):
    """(cos, -sin) [nbins, nfft] float32: the rows srp._twiddles uploads, without the padding."""
    ang = 2 * np.pi * np.asarray(bins, dtype=np.float64)[:, None] * np.arange(nfft, dtype=np.float64)[None, :] / nfft
    return np.cos(ang).astype(np.float32), (-np.sin(ang)).astype(np.float32)


def cc32(mix, window, nfft, bins, n_windows=None, tol=TOL):
    """[n_windows, nbins, P] complex64."""
    x = np.asarray(mix, dtype=np.float32)
    M, T = x.shape
    hop, step = nfft // 4, window // 2
    if n_windows is None:
        n_windows = sum(1 for j in range(T // step - 1) if j * step + window <= T)
    co, si = twiddles32(bins, nfft)
    F = (window - nfft) // hop + 1
    idx = np.arange(nfft)[None, :] + hop * np.arange(F)[:, None]
    ii, jj = np.triu_indices(M, k=1)
    out = []
    for w in range(n_windows):
        fr = x[:, w * step:w * step + window][:, idx].reshape(M * F, nfft)
        re, im = (fr @ co.T).reshape(M, F, -1), (fr @ si.T).reshape(M, F, -1)          # [M, F, nbins] float32
        a = np.maximum(np.hypot(re, im), np.float32(tol))
        p = (re / a + 1j * (im / a)).astype(np.complex64)
        assert re.dtype == np.float32 and a.dtype == np.float32
        cc = (p[ii] * np.conj(p[jj])).sum(axis=1, dtype=np.complex64) / np.float32(F)   # [P, nbins]
        out.append(cc.T.astype(np.complex64))
    return np.stack(out)


def window_maps32(cc, tau, omega, chunk=64):
    """cc [W, nbins, P] complex64 -> (map [G] float32, per-window [W, G] float32)."""
    cc = np.asarray(cc, dtype=np.complex64)
    W, nb, P = cc.shape
    ii, jj = np.triu_indices(tau.shape[1], k=1)
    assert len(ii) == P
    dt = tau[:, ii] - tau[:, jj]
    cr = np.ascontiguousarray(cc.real.transpose(0, 2, 1))                 # [W, P, nbins]: pair outer, bin inner
    ci = np.ascontiguousarray(cc.imag.transpose(0, 2, 1))
    scale = np.float32(1.0) / (np.float32(nb) * np.float32(P))
    G = tau.shape[0]
    per = np.empty((W, G), dtype=np.float32)
    for g0 in range(0, G, chunk):
        ph = dt[g0:g0 + chunk, :, None] * omega[None, None, :]            # float64 [g, P, nbins]
        r = (ph - 2 * np.pi * np.rint(ph / (2 * np.pi))).astype(np.float32)
        cs, sn = np.cos(r), np.sin(r)
        assert cs.dtype == np.float32
        for w in range(W):
            term = (cr[w][None] * cs - ci[w][None] * sn).reshape(cs.shape[0], -1)
            per[w, g0:g0 + chunk] = np.cumsum(term, axis=1, dtype=np.float32)[:, -1] * scale
    return np.maximum(per.max(axis=0), np.float32(0)), per


def map32(mix, window, nfft, bins, tau, omega, n_windows=None, tol=TOL):
    return window_maps32(cc32(mix, window, nfft, bins, n_windows, tol), tau, omega)[0]


# ---- per-case references, computed once ---------------------------------------------------------------------
Refs = namedtuple("Refs", "cc64 map64 per64 cc32 yard_cc map32_stage yard_map map32_whole yard_whole")


def refs(name, mix=None, key=None):
    """Everything the three stage assertions of one case need.  ``mix`` (with its own ``key``) replaces the case's
    mixture, for the variants that silence a channel."""
    key = key or name
    if key in _REFS:
        return _REFS[key]
    c = case(name)
    s = c.shape
    mix = c.mix if mix is None else mix
    c64 = cc64(mix, s.window, s.nfft, c.bins)
    m64, per = window_maps64(c64, c.tau, c.omega)
    c32 = cc32(mix, s.window, s.nfft, c.bins, s.n_windows)
    m32s = window_maps32(c64.astype(np.complex64), c.tau, c.omega)[0]     # the map stage alone, fed the cast reference
    m32w = window_maps32(c32, c.tau, c.omega)[0]
    r = Refs(_frozen(c64), _frozen(m64), _frozen(per), _frozen(c32), rel_l2(c32, c64), _frozen(m32s),
             max_abs(m32s, m64), _frozen(m32w), max_abs(m32w, m64))
    _REFS[key] = r
    return r
