"""Evaluation harness of the search: the reference's sample-directory format,
prediction <-> ground-truth matching, localisation / separation scores and the per-sample result
record of ``sep/eval/eval_model.py``.

Follows sep/eval/eval_model.py:18-91 (matching, metadata preprocessing), :129-249 (result
record) and sep/eval/get_items.py:10-46 (directory layout written by
datasets/generate_dataset.py:633-699: ``metadata.json`` + ``micNN_mixed.wav`` +
``mic00_voiceNN.wav``).  The two third-party metrics the reference calls are absent here: mir_eval's
BSS-eval SDR is restated below from the published BSS-eval v3 algorithm (fields ``si_snr_in_mir`` /
``si_snri_mir``), and asteroid's metric wrapper is not needed -- its SI-SDR is the plain scale-invariant
SDR of ``sep/helpers/eval_utils.py:11-39`` (``hostdsp.si_sdr``).  Both are "parity unpinned".
"""
import json
import os

import numpy as np

from .hostdsp import si_sdr
from .patch import FS, SPEED_OF_SOUND

NO_MATCH = 10000.0


def find_best_permutation(wav_gt, wav_pred, pos_gt, pos_pred, acceptable_range=1, accept_sisdr=-15, sisdr=None):
    """Pairs (prediction index, ground-truth index), in ground-truth order, that maximise the
    number of inliers (xy distance < acceptable_range AND SI-SDR > accept_sisdr) and, among
    those, minimise the mean of (distance - SI-SDR) over the inlier pairs
    (sep/eval/eval_model.py:18-59).

    The reference scores every permutation of max(n_gt, n_pred) items; the same optimum is the
    maximum-cardinality, minimum-cost matching of the inlier graph, found here with the
    Hungarian method (identical result up to exact ties, and usable beyond ~9 items).

    ``sisdr``: an [n_pred, n_gt] matrix of the SI-SDRs (``cross_sisdr_batch``), used in place of the ``si_sdr`` calls;
    the waveforms are then not looked at."""
    from scipy.optimize import linear_sum_assignment
    pos_gt, pos_pred = np.asarray(pos_gt, dtype=np.float64), np.asarray(pos_pred, dtype=np.float64)
    n_gt, n_pred = pos_gt.shape[0], pos_pred.shape[0]
    if n_gt == 0 or n_pred == 0:
        return []
    loss = np.full((n_gt, n_pred), NO_MATCH)
    inlier = np.zeros((n_gt, n_pred), dtype=bool)
    for i in range(n_gt):
        for j in range(n_pred):
            dis = np.linalg.norm(pos_gt[i][:2] - pos_pred[j][:2])
            neg = -si_sdr(np.asarray(wav_pred[j]), np.asarray(wav_gt[i])) if sisdr is None else -float(sisdr[j][i])
            loss[i, j] = neg + dis
            inlier[i, j] = dis < acceptable_range and neg < -accept_sisdr
    if not inlier.any():
        return []
    lmin = float(loss[inlier].min())
    span = float(loss[inlier].max()) - lmin + 1.0
    big = span * (min(n_gt, n_pred) + 1)                     # one more inlier always beats any cost change
    cost = np.where(inlier, (loss - lmin) - big, 0.0)
    rows, cols = linear_sum_assignment(cost)
    return [(int(j), int(i)) for i, j in zip(rows, cols) if inlier[i, j]]


def preprocess_metadata(metadata):
    """(mic names, mic_positions [M,3], voice names, voice_positions [S,3],
    sample_offsets_gt [M-1,S] rounded TDoA in samples, speaker range with +2 cm on z max)
    (sep/eval/eval_model.py:61-91)."""
    mics = sorted(k for k in metadata if k.startswith("mic"))
    mic_positions = np.array([metadata[k]["position"] for k in mics], dtype=np.float64)
    voices = sorted(k for k in metadata if k.startswith("voice"))
    voice_positions = np.array([metadata[k]["position"][:3] for k in voices], dtype=np.float64).reshape(-1, 3)
    gt = np.zeros((mic_positions.shape[0] - 1, len(voices)))
    for j in range(len(voices)):
        for i in range(1, mic_positions.shape[0]):
            d = np.linalg.norm(voice_positions[j] - mic_positions[i]) - np.linalg.norm(voice_positions[j] - mic_positions[0])
            gt[i - 1, j] = int(np.round(d / SPEED_OF_SOUND * FS))
    roi = list(metadata["ROI"])
    roi[-1] += 0.02
    return mics, mic_positions, voices, voice_positions, gt, roi


# ---- sample directories --------------------------------------------------------------------
def _read_wav(path):
    from scipy.io import wavfile
    _sr, x = wavfile.read(path)
    if x.dtype == np.int16:
        return x.astype(np.float32) / 32768.0
    if x.dtype == np.int32:
        return x.astype(np.float32) / 2147483648.0
    return x.astype(np.float32)


def write_scene_dir(scene, path):
    """Write a ``scenes.Scene`` in the reference's on-disk sample format (float32 wav)."""
    from scipy.io import wavfile
    os.makedirs(path, exist_ok=True)
    meta = {"ROI": [float(v) for v in scene.speaker_range], "real": False}
    for m in range(scene.mic_positions.shape[0]):
        meta[f"mic{m:02d}"] = {"position": [float(v) for v in scene.mic_positions[m]]}
        wavfile.write(os.path.join(path, f"mic{m:02d}_mixed.wav"), scene.fs, scene.mix[m].astype(np.float32))
    for s in range(scene.speaker_positions.shape[0]):
        meta[f"voice{s:02d}"] = {"position": [float(v) for v in scene.speaker_positions[s]]}
        wavfile.write(os.path.join(path, f"mic00_voice{s:02d}.wav"), scene.fs, scene.sources[s].astype(np.float32))
    with open(os.path.join(path, "metadata.json"), "w") as f:
        json.dump(meta, f, indent=1)


def get_items(path):
    """(metadata, mixture [M,T] float32, ground truth at mic 0 [S,T]) (sep/eval/get_items.py:10-46)."""
    with open(os.path.join(path, "metadata.json")) as f:
        metadata = json.load(f)
    mics = sorted(k for k in metadata if k.startswith("mic"))
    mix = np.stack([_read_wav(os.path.join(path, f"{m}_mixed.wav")) for m in mics])
    voices = sorted(k for k in metadata if k.startswith("voice"))
    gt = []
    for v in voices:
        den = os.path.join(path, f"{mics[0]}_{v}_denoised.wav")
        gt.append(_read_wav(den if os.path.exists(den) else os.path.join(path, f"{mics[0]}_{v}.wav")))
    return metadata, mix, np.stack(gt) if gt else np.zeros((0, mix.shape[1]), dtype=np.float32)


# ---- separation metrics ------------------------------------------------------------------------
def _project(reference_sources, estimated_source, flen):
    """Least-squares projection of ``estimated_source`` on the span of the references delayed by
    0..flen-1 samples (BSS-eval "mtifilt" decomposition, Vincent et al. 2006), solved through
    FFT-computed auto / cross-correlations and one (nsrc*flen)-square linear system."""
    from scipy.linalg import toeplitz
    from scipy.signal import fftconvolve
    nsrc, nsampl = reference_sources.shape
    ref = np.hstack((reference_sources, np.zeros((nsrc, flen - 1))))
    est = np.hstack((estimated_source, np.zeros(flen - 1)))
    n_fft = int(2 ** np.ceil(np.log2(nsampl + flen - 1.0)))
    sf = np.fft.fft(ref, n=n_fft, axis=1)
    sef = np.fft.fft(est, n=n_fft)
    G = np.zeros((nsrc * flen, nsrc * flen))
    for i in range(nsrc):
        for j in range(i, nsrc):
            ssf = np.real(np.fft.ifft(sf[i] * np.conj(sf[j])))
            ss = toeplitz(np.hstack((ssf[0], ssf[-1:-flen:-1])), r=ssf[:flen])
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = ss
            G[j * flen:(j + 1) * flen, i * flen:(i + 1) * flen] = ss.T
    D = np.zeros(nsrc * flen)
    for i in range(nsrc):
        ssef = np.real(np.fft.ifft(sf[i] * np.conj(sef)))
        D[i * flen:(i + 1) * flen] = np.hstack((ssef[0], ssef[-1:-flen:-1]))
    try:
        C = np.linalg.solve(G, D).reshape(flen, nsrc, order="F")
    except np.linalg.LinAlgError:
        C = np.linalg.lstsq(G, D, rcond=None)[0].reshape(flen, nsrc, order="F")
    sproj = np.zeros(nsampl + flen - 1)
    for i in range(nsrc):
        sproj += fftconvolve(C[:, i], ref[i])[:nsampl + flen - 1]
    return sproj


def bss_eval_sdr(reference_sources, estimated_sources, flen: int = 512):
    """Signal-to-distortion ratio of estimate j against reference j with a 512-tap
    time-invariant distortion filter allowed -- the quantity the reference takes from
    ``mir_eval.separation.bss_eval_sources(..., compute_permutation=False)``
    (sep/eval/get_items.py:50-52).  mir_eval is absent from the image and unpinned upstream; this
    is a restatement of the published BSS-eval v3 algorithm: "parity unpinned"."""
    return bss_eval_sources(reference_sources, estimated_sources, flen)[0]


def _bss_ratios(ref, est_row, j, flen, full_projection):
    """(sdr, sir, sar) of one estimate against reference ``j`` -- the one place the BSS-eval decomposition is written:
    s_true, e_spat, e_interf, e_artif, in that order; ``full_projection`` is ``_project(ref, est_row, flen)``."""
    nsampl = est_row.shape[0]
    s_true = np.hstack((ref[j], np.zeros(flen - 1)))
    e_spat = _project(ref[j:j + 1], est_row, flen) - s_true
    e_interf = full_projection - s_true - e_spat
    e_artif = -s_true - e_spat - e_interf
    e_artif[:nsampl] += est_row
    num, den = np.sum((s_true + e_spat) ** 2), np.sum((e_interf + e_artif) ** 2)
    den_i = np.sum(e_interf ** 2)
    num_a, den_a = np.sum((s_true + e_spat + e_interf) ** 2), np.sum(e_artif ** 2)
    return (np.inf if den == 0 else 10 * np.log10(num / den), np.inf if den_i == 0 else 10 * np.log10(num / den_i),
            np.inf if den_a == 0 else 10 * np.log10(num_a / den_a))


def _bss_inputs(reference_sources, estimated_sources):
    ref = np.atleast_2d(np.asarray(reference_sources, dtype=np.float64))
    est = np.atleast_2d(np.asarray(estimated_sources, dtype=np.float64))
    if ref.shape != est.shape:
        raise ValueError(f"reference {ref.shape} and estimate {est.shape} shapes differ")
    return ref, est


def bss_eval_matrices(reference_sources, estimated_sources, flen: int = 512):
    """(sdr, sir, sar), each [S_est, S_ref] float64: entry (e, j) scores estimate ``e`` against reference ``j`` with the
    decomposition of ``_bss_ratios`` -- s_true, e_spat, e_interf, e_artif, in that order and with those expressions --
    and sdr = 10 log10(sum (s_true + e_spat)^2 / sum (e_interf + e_artif)^2), sir = 10 log10(sum (s_true + e_spat)^2 /
    sum e_interf^2), sar = 10 log10(sum (s_true + e_spat + e_interf)^2 / sum e_artif^2); a ratio is +inf when its
    denominator is exactly 0 (one talker: e_interf is exactly 0 and sir is +inf)."""
    ref, est = _bss_inputs(reference_sources, estimated_sources)
    S = ref.shape[0]
    out = np.zeros((3, S, S))
    for e in range(S):
        full = _project(ref, est[e], flen)
        for j in range(S):
            out[:, e, j] = _bss_ratios(ref, est[e], j, flen, full)
    return out[0], out[1], out[2]


def best_permutation(sir_matrix):
    """``perm`` with ``perm[j]`` the estimate assigned to reference ``j``: the permutation that maximises the mean of
    ``sir_matrix[perm[j], j]`` ([S_est, S_ref]), the published rule.  Up to 6 talkers every permutation is scored in
    ``itertools.permutations`` order and the first maximum taken, as the published code does; above that the same optimum
    comes from ``scipy.optimize.linear_sum_assignment(maximize=True)``, for which +inf entries are replaced by a finite
    value larger than any sum of the others (so that an assignment through a +inf entry still beats every one without)."""
    import itertools
    sir = np.asarray(sir_matrix, dtype=np.float64)
    S = sir.shape[0]
    if sir.shape != (S, S):
        raise ValueError(f"sir matrix {sir.shape} is not square")
    if S <= 6:
        perms = list(itertools.permutations(range(S)))
        idx = np.arange(S)
        with np.errstate(invalid="ignore"):
            means = [np.mean(sir[list(p), idx]) if S else 0.0 for p in perms]
        return np.array(perms[int(np.argmax(means))], dtype=np.int64)
    from scipy.optimize import linear_sum_assignment
    finite = sir[np.isfinite(sir)]
    big = (S + 1) * (float(np.max(np.abs(finite))) + 1.0) if finite.size else 1.0
    est_of, ref_of = linear_sum_assignment(np.where(sir == np.inf, big, sir), maximize=True)
    perm = np.zeros(S, dtype=np.int64)
    perm[ref_of] = est_of
    return perm


def bss_eval_sources(reference_sources, estimated_sources, flen: int = 512, compute_permutation: bool = False):
    """(sdr, sir, sar, perm) as ``mir_eval.separation.bss_eval_sources(reference_sources, estimated_sources,
    compute_permutation)`` answers (sep/eval/get_items.py:50-52) -- like ``bss_eval_sdr`` a restatement of the published
    BSS-eval v3 algorithm, mir_eval being absent: "parity unpinned".  ``compute_permutation=False``: estimate j against
    reference j, ``perm = arange(S)``, and ``sdr`` is what ``bss_eval_sdr`` returns.  ``True``: ``bss_eval_matrices``,
    then ``perm = best_permutation(sir)`` and the three vectors ``m[perm[j], j]``."""
    ref, est = _bss_inputs(reference_sources, estimated_sources)
    S = ref.shape[0]
    if compute_permutation:
        sdr, sir, sar = bss_eval_matrices(ref, est, flen)
        perm = best_permutation(sir)
        idx = np.arange(S)
        return sdr[perm, idx], sir[perm, idx], sar[perm, idx], perm
    out = np.zeros((3, S))
    for j in range(S):
        out[:, j] = _bss_ratios(ref, est[j], j, flen, _project(ref, est[j], flen))
    return out[0], out[1], out[2], np.arange(S)


# ---- BSS-eval SDR on the device (csrc/bss_kernels.hip: asw_bss_eval_sdr) -------------------------
METRICS = ("host", "device")
BSS_WORKSPACE_BUDGET = 1 << 30          # bytes of device workspace one call may ask for (G at 5 talkers is 52 MB)
BSS_MAX_TALKERS, BSS_MAX_FLEN, BSS_MAX_ORDER = 16, 1024, 8192          # the library's limits (include/asw_hip.h)
_BSS_TILE, _BSS_CHUNK, _BSS_SPLIT = 64, 1024, 8


def check_metrics(metrics):
    if metrics not in METRICS:
        raise ValueError(f"metrics must be one of {METRICS}, got {metrics!r}")


BSS_FIELDS = ("sdr", "all")             # what the record takes from BSS-eval: the SDR alone, or SIR and SAR too


def check_bss(bss):
    if bss not in BSS_FIELDS:
        raise ValueError(f"bss must be one of {BSS_FIELDS}, got {bss!r}")


def bss_sources_workspace_bytes(counts, R: int, T: int, flen: int, all_pairs: bool = False, sdr_only: bool = False) -> int:
    """What ``asw_bss_eval_sources_workspace_bytes`` answers for one call, restated so that the packing rule below is a
    pure function (tests/test_bss_sources_host.py holds the two equal): the lists, the correlations and their partial
    sums, the dense systems, the solutions and the energy partials.  ``all_pairs``: R S^2 single-reference solves and
    projection rows per item instead of R S.  ``sdr_only``: what a call with neither ``sir`` nor ``sar`` needs -- two
    energy partials per row and chunk instead of five."""
    counts = [int(c) for c in counts]
    rows = sum(R * S * (S if all_pairs else 1) for S in counts)
    P = sum((R + 1) * S * S for S in counts)
    nsys = sum(S + 1 if S > 1 else S for S in counts)
    nsolve = rows + sum(R * S for S in counts if S > 1)
    nchunk = -(-T // _BSS_CHUNK)
    cps = -(-nchunk // min(nchunk, _BSS_SPLIT))
    nsplit = -(-nchunk // cps)
    nchunk_p = -(-(T + flen - 1) // _BSS_CHUNK)
    gram = sum(S * flen * flen + ((S * flen) ** 2 if S > 1 else 0) for S in counts)
    x = rows * flen + sum(R * S * S * flen for S in counts if S > 1)
    tables = 32 * len(counts) + 24 * nsys + 16 * P + 24 * nsolve + 8 * rows
    return tables + 8 * (P * nsplit * flen + P * flen + gram + x + (2 if sdr_only else 5) * rows * nchunk_p)


def bss_workspace_bytes(counts, R: int, T: int, flen: int) -> int:
    """What ``asw_bss_eval_sdr_workspace_bytes`` answers for one call (tests/test_bss_eval_host.py holds the two equal):
    the formula above for matched pairs and the SDR alone."""
    return bss_sources_workspace_bytes(counts, R, T, flen, all_pairs=False, sdr_only=True)


def pack_bss_items(counts, lengths, R: int, flen: int = 512, budget: int = BSS_WORKSPACE_BUDGET, all_pairs: bool = False,
                   sdr_only: bool = True):
    """The device calls of a batch: items stay whole and in order, a call holds items of one length only and takes as
    many as its workspace (``bss_sources_workspace_bytes``) fits into ``budget``.  -> list of (first, last) item ranges,
    ``last`` exclusive, covering every item once.  ``ValueError`` for an item the library refuses (talkers outside
    0..16, talkers * flen > 8192, T < flen), ``RuntimeError`` for one whose workspace alone exceeds the budget.
    ``all_pairs`` and ``sdr_only`` say which call is sized; the defaults are the calls of ``bss_eval_sdr``."""
    def call_bytes(c, T):
        return bss_sources_workspace_bytes(c, R, T, flen, all_pairs, sdr_only)
    if R < 1 or not 1 <= flen <= BSS_MAX_FLEN:
        raise ValueError(f"R = {R} < 1 or flen = {flen} outside 1..{BSS_MAX_FLEN}")
    if len(counts) != len(lengths):
        raise ValueError(f"{len(lengths)} lengths for {len(counts)} items")
    calls, first = [], 0
    for k, (S, T) in enumerate(zip(counts, lengths)):
        S, T = int(S), int(T)
        if not 0 <= S <= BSS_MAX_TALKERS or S * flen > BSS_MAX_ORDER:
            raise ValueError(f"item {k}: {S} talkers of {flen} taps (at most {BSS_MAX_TALKERS} and {BSS_MAX_ORDER} in all)")
        if T < flen:
            raise ValueError(f"item {k}: {T} samples are fewer than flen = {flen}")
        if call_bytes([S], T) > budget:
            raise RuntimeError(f"item {k} alone needs {call_bytes([S], T)} bytes of workspace, budget {budget}")
        if k > first and (T != int(lengths[first]) or call_bytes(counts[first:k + 1], T) > budget):
            calls.append((first, k))
            first = k
    if first < len(counts):
        calls.append((first, len(counts)))
    return calls


def _device_op(name, device, op=None):
    """(op, device) of a batch route: ``torch.ops.asw.<name>`` on a GPU, or the stand-in ``op`` on CPU tensors (host
    tests).  Without a stand-in a missing library or GPU is a ``RuntimeError``: there is no quiet fall-back to the host
    metric."""
    import torch
    if op is not None:
        return op, torch.device("cpu" if device is None else device)
    from . import native
    op = getattr(native.torch_ops(), name)                 # RuntimeError when the library has not been built
    if not torch.cuda.is_available():
        raise RuntimeError('metrics="device" needs a GPU: none is visible to torch')
    return op, torch.device("cuda:0" if device is None else device)


def _bss_batch(name, all_pairs, unpack, on_host, refs, est_sets, flen, device, op, budget):
    """The batch route of both BSS ops: checks, float32 rounding, op and device, packing, one upload and one
    ``torch.ops.asw.<name>`` call per range of ``pack_bss_items``, then item after item ``on_host(ref, est)`` where the
    device reports status 1 and else ``unpack(rows, S)`` of the item's float64 [R, width] slices, one per value the op
    returns.  ``all_pairs`` None: the op takes no such argument and gives the SDR alone (``bss_eval_sdr``); else width is
    S^2 when it is true."""
    import torch
    if len(refs) != len(est_sets):
        raise ValueError(f"{len(est_sets)} estimate sets for {len(refs)} samples")
    if not refs:
        return [], []
    refs = [np.ascontiguousarray(np.atleast_2d(r), dtype=np.float32) for r in refs]
    ests = [np.ascontiguousarray(e, dtype=np.float32) for e in est_sets]
    R = ests[0].shape[0] if ests[0].ndim == 3 else -1
    for k, (r, e) in enumerate(zip(refs, ests)):
        if e.ndim != 3 or e.shape[0] != R or e.shape[1:] != r.shape:
            raise ValueError(f"sample {k}: estimates {e.shape} do not go with references {r.shape} as [R = {R}, S, T]")
    op, dev = _device_op(name, device, op)
    mode = () if all_pairs is None else (all_pairs,)
    counts, lengths = [r.shape[0] for r in refs], [r.shape[1] for r in refs]
    calls = pack_bss_items(counts, lengths, R, flen, budget, all_pairs=bool(all_pairs), sdr_only=all_pairs is None)
    out, recomputed = [None] * len(refs), []
    for first, last in calls:
        ref = torch.from_numpy(np.concatenate(refs[first:last], axis=0)).to(dev)
        est = torch.from_numpy(np.concatenate(ests[first:last], axis=1)).to(dev)
        *vals, status = op(ref, est, counts[first:last], int(flen), *mode)
        vals, status = [v.cpu().numpy() for v in vals], status.cpu().numpy()
        c0 = 0
        for k in range(first, last):
            S = counts[k]
            width = S * S if all_pairs else S
            if status[k - first] != 0:
                recomputed.append(k)
                out[k] = on_host(refs[k], ests[k])
            else:
                out[k] = unpack([np.array(v[:, c0:c0 + width], dtype=np.float64) for v in vals], S)
            c0 += width
    return out, recomputed


def bss_eval_sdr_batch(refs, est_sets, flen: int = 512, device=None, op=None, budget: int = BSS_WORKSPACE_BUDGET):
    """``bss_eval_sdr`` of many samples on the device.  ``refs[k]`` is [S_k, T_k], ``est_sets[k]`` is [R, S_k, T_k] (R
    estimate sets of the same references, one R for the batch); talker counts and lengths may differ from sample to
    sample.  The samples are rounded to float32 (exact for wav and network output) and packed into as few
    ``torch.ops.asw.bss_eval_sdr`` calls as ``pack_bss_items`` allows.  -> (list of [R, S_k] float64 arrays, sorted list
    of the items that were recomputed on the host).  An item is recomputed with ``bss_eval_sdr`` when the device
    reports status 1 for it -- silent or duplicated references, where the Gram matrix has no Cholesky factor and the
    host statement itself leaves ``solve`` for ``lstsq`` -- so its values are exactly the host result.
    ``op`` replaces the device op (a stand-in on CPU tensors in the host tests); without it a missing library or GPU
    is a ``RuntimeError``."""
    def on_host(ref, est):
        return np.stack([bss_eval_sdr(ref, e, flen) for e in est])
    return _bss_batch("bss_eval_sdr", None, lambda rows, S: rows[0], on_host, refs, est_sets, flen, device, op, budget)


def bss_eval_sdr_device(reference_sources, estimated_sets, flen: int = 512, device=None, op=None):
    """[R, S] float64: ``bss_eval_sdr(reference_sources, estimated_sets[r], flen)`` for every set r, on the device
    (one ``bss_eval_sdr_batch`` call of one sample)."""
    out, _ = bss_eval_sdr_batch([reference_sources], [estimated_sets], flen, device, op)
    return out[0]


# ---- SDR, SIR, SAR and the best permutation on the device (asw_bss_eval_sources) -----------------
def bss_eval_sources_batch(refs, est_sets, flen: int = 512, compute_permutation: bool = False, device=None, op=None,
                           budget: int = BSS_WORKSPACE_BUDGET):
    """``bss_eval_sources`` of many samples on the device: inputs, float32 rounding and packing as ``bss_eval_sdr_batch``
    (``pack_bss_items`` sized for ``torch.ops.asw.bss_eval_sources`` in the mode asked for).  -> (list of (sdr, sir, sar,
    perm) per sample, the first three [R, S_k] float64 and ``perm`` [R, S_k] int64, sorted list of the items that were
    recomputed on the host).  ``compute_permutation=True`` takes the all-pairs form of the op, reads the [S, S]
    matrices back and lets ``best_permutation`` decide on the host, per estimate set.  An item the device marks
    ``status = 1`` is recomputed with ``bss_eval_sources``, so its values are exactly the host's.  ``op`` replaces the
    device op (a stand-in on CPU tensors in the host tests); without it a missing library or GPU is a ``RuntimeError``."""
    all_pairs = bool(compute_permutation)

    def on_host(ref, est):
        sets = [bss_eval_sources(ref, e, flen, compute_permutation) for e in est]
        return tuple(np.stack([s[q] for s in sets]) for q in range(4))

    def unpack(rows, S):
        R, idx = rows[0].shape[0], np.arange(S)
        if not all_pairs:
            return (*rows, np.tile(idx, (R, 1)))
        mats = [m.reshape(R, S, S) for m in rows]
        perm = np.stack([best_permutation(mats[1][r]) for r in range(R)]).reshape(R, S)
        return tuple(np.stack([m[r][perm[r], idx] for r in range(R)]).reshape(R, S) for m in mats) + (perm,)
    return _bss_batch("bss_eval_sources", all_pairs, unpack, on_host, refs, est_sets, flen, device, op, budget)


def bss_eval_sources_device(reference_sources, estimated_sets, flen: int = 512, compute_permutation: bool = False,
                            device=None, op=None):
    """(sdr, sir, sar, perm), each [R, S]: ``bss_eval_sources(reference_sources, estimated_sets[r], flen,
    compute_permutation)`` for every set r, on the device (one ``bss_eval_sources_batch`` call of one sample)."""
    out, _ = bss_eval_sources_batch([reference_sources], [estimated_sets], flen, compute_permutation, device, op)
    return out[0]


# ---- SI-SDR matrices on the device (csrc/eval_kernels.hip: asw_cross_sisdr) ----------------------
XS_MAX_ITEMS, XS_MAX_EST, XS_MAX_REF = 65535, 4096, 64          # the library's limits (include/asw_hip.h)


def cross_sisdr_f64(est, ref):
    """[P, S] float64: ``hostdsp.si_sdr(est_p, ref_s)`` of every pair, on the float32 values of ``est`` [P, T] and
    ``ref`` [S, T] widened exactly -- the statement ``asw_cross_sisdr`` is pinned to.  What ``si_sdr`` does with a
    silent reference (a division by zero) or an all-zero estimate (``ValueError`` from ``log10``) happens here too."""
    est = np.atleast_2d(np.asarray(est, dtype=np.float32)).astype(np.float64)
    ref = np.atleast_2d(np.asarray(ref, dtype=np.float32)).astype(np.float64)
    out = np.zeros((est.shape[0], ref.shape[0]))
    for p in range(est.shape[0]):
        for s in range(ref.shape[0]):
            out[p, s] = si_sdr(est[p], ref[s])
    return out


def cross_sisdr_batch(est_list, ref_list, device=None, op=None):
    """``cross_sisdr_f64`` of many items on the device.  ``est_list[k]`` is [P_k, T_k], ``ref_list[k]`` is [S_k, T_k];
    the counts and lengths may differ from item to item (P_k or S_k may be 0).  The rows are rounded to float32 (exact
    for wav and network output) and the items of one length go out in ONE ``torch.ops.asw.cross_sisdr`` call (at most
    65535 items each).  -> (list of [P_k, S_k] float64 arrays, sorted list of the items that were recomputed on the
    host).  An item is recomputed with ``cross_sisdr_f64`` when the device reports status 1 for it -- a silent
    reference, an all-zero estimate, a value that is not finite -- so it behaves exactly as the host statement does,
    the exception included.  ``op`` replaces the device op (a stand-in on CPU tensors in the host tests); without it a
    missing library or GPU is a ``RuntimeError``."""
    import torch
    if len(est_list) != len(ref_list):
        raise ValueError(f"{len(est_list)} estimate sets for {len(ref_list)} reference sets")
    if not est_list:
        return [], []
    ests = [np.ascontiguousarray(e, dtype=np.float32) for e in est_list]
    refs = [np.ascontiguousarray(r, dtype=np.float32) for r in ref_list]
    by_length = {}
    for k, (e, r) in enumerate(zip(ests, refs)):
        if e.ndim != 2 or r.ndim != 2 or e.shape[1] != r.shape[1]:
            raise ValueError(f"item {k}: estimates {e.shape} and references {r.shape} are not [P, T] and [S, T]")
        if e.shape[0] > XS_MAX_EST or r.shape[0] > XS_MAX_REF:
            raise ValueError(f"item {k}: {e.shape[0]} estimates (at most {XS_MAX_EST}) or {r.shape[0]} references "
                             f"(at most {XS_MAX_REF})")
        by_length.setdefault(e.shape[1], []).append(k)
    op, dev = _device_op("cross_sisdr", device, op)
    out, recomputed = [None] * len(ests), []
    for T, members in by_length.items():
        for first in range(0, len(members), XS_MAX_ITEMS):
            ks = members[first:first + XS_MAX_ITEMS]
            est = torch.from_numpy(np.concatenate([ests[k] for k in ks], axis=0)).to(dev)
            ref = torch.from_numpy(np.concatenate([refs[k] for k in ks], axis=0)).to(dev)
            vals, status = op(est, ref, [ests[k].shape[0] for k in ks], [refs[k].shape[0] for k in ks])
            vals, status = vals.cpu().numpy(), status.cpu().numpy()
            pos = 0
            for q, k in enumerate(ks):
                P, S = ests[k].shape[0], refs[k].shape[0]
                if status[q] != 0:
                    recomputed.append(k)
                    out[k] = cross_sisdr_f64(ests[k], refs[k])
                else:
                    out[k] = np.array(vals[pos:pos + P * S], dtype=np.float64).reshape(P, S)
                pos += P * S
    return out, sorted(recomputed)


# ---- oracle mask baselines on the device (csrc/stft_kernels.hip: asw_oracle_masks) ---------------
ORACLES = ("irm", "ibm")                # the reference's two baselines (sep/helpers/irm.py, ibm.py)


def check_oracle(oracle):
    """``oracle`` as a tuple of baseline names without repeats, in the order given; an unknown name raises."""
    names = (oracle,) if isinstance(oracle, str) else tuple(oracle)
    for name in names:
        if name not in ORACLES:
            raise ValueError(f"oracle baselines must be among {ORACLES}, got {name!r}")
    return tuple(dict.fromkeys(names))


def oracle_masks_batch(refs, mixes, kind, alpha: float = 1.0, theta: float = 0.5, device=None, op=None):
    """``oracle_masks.irm_f64`` / ``ibm_f64`` (``kind`` "irm" / "ibm") of many items on the device.  ``refs[k]`` is
    [S_k, N_k], ``mixes[k]`` is [N_k]; counts and lengths may differ from item to item.  The rows are rounded to
    float32 (exact for wav and network output) and the items of one length go out in ONE ``torch.ops.asw.oracle_masks``
    call (at most 65535 items each), as ``cross_sisdr_batch`` groups.  -> list of [S_k, N_k] float64 arrays in item
    order; an item without references gives a [0, N_k] array and is not sent.  ``theta`` counts for "ibm" only.  ``op``
    replaces the device op (a stand-in on CPU tensors in the host tests); without it a missing library or GPU is a
    ``RuntimeError``."""
    import torch
    from .oracle_masks import NFFT, check_kind
    check_kind(kind)
    if len(refs) != len(mixes):
        raise ValueError(f"{len(mixes)} mixtures for {len(refs)} reference sets")
    if not refs:
        return []
    refs = [np.ascontiguousarray(r, dtype=np.float32) for r in refs]
    mixes = [np.ascontiguousarray(m, dtype=np.float32) for m in mixes]
    by_length = {}
    for k, (r, m) in enumerate(zip(refs, mixes)):
        if r.ndim != 2 or m.ndim != 1 or r.shape[1] != m.shape[0]:
            raise ValueError(f"item {k}: references {r.shape} and mixture {m.shape} are not [S, N] and [N]")
        if r.shape[0] > XS_MAX_REF:
            raise ValueError(f"item {k}: {r.shape[0]} references (at most {XS_MAX_REF})")
        if m.shape[0] < NFFT:
            raise ValueError(f"item {k}: {m.shape[0]} samples are fewer than the window of {NFFT}")
        if r.shape[0] > 0:
            by_length.setdefault(m.shape[0], []).append(k)
    out = [np.zeros(r.shape) for r in refs]
    if not by_length:
        return out
    op, dev = _device_op("oracle_masks", device, op)
    for N, members in by_length.items():
        for first in range(0, len(members), XS_MAX_ITEMS):
            ks = members[first:first + XS_MAX_ITEMS]
            mix = torch.from_numpy(np.stack([mixes[k] for k in ks])).to(dev)
            ref = torch.from_numpy(np.concatenate([refs[k] for k in ks], axis=0)).to(dev)
            rows = op(mix, ref, [refs[k].shape[0] for k in ks], [N] * len(ks), kind, float(alpha), float(theta)).cpu().numpy()
            pos = 0
            for k in ks:
                S = refs[k].shape[0]
                out[k] = np.array(rows[pos:pos + S], dtype=np.float64)
                pos += S
    return out


def oracle_estimates(gt, mix_row, oracle, metrics="host", op=None):
    """{name: [S, N] float32} for the baselines of ``oracle``: the mask estimates of every ground truth of one sample
    (references ``gt`` [S, N] in ground-truth order, mixture ``mix_row`` [N]) from the statements (``metrics="host"``) or
    from one ``oracle_masks_batch`` call per baseline, rounded to float32 -- what every scoring op here reads."""
    from .oracle_masks import masks_f64
    if metrics == "host":
        return {name: masks_f64(gt, mix_row, name).astype(np.float32) for name in oracle}
    return {name: oracle_masks_batch([gt], [mix_row], name, op=op)[0].astype(np.float32) for name in oracle}


def compute_metrics(input_signal, est_signal, gt, metrics="host", bss="sdr", oracle=(), oracle_est=None):
    """(input_sdr, output_sdr, input_sisdr, output_sisdr) per matched talker, as
    sep/eval/get_items.py:46-70 with permute=False: BSS-eval SDR and SI-SDR of the unprocessed
    reference-microphone signal and of the separated output against the ground truth.
    ``metrics="device"`` takes the two BSS-eval SDRs from one ``bss_eval_sdr_device`` call (R = 2: the
    unprocessed set and the separated set); the signals are read as float32 there.  ``bss="all"`` appends a fifth
    entry, ``(input_sir, output_sir, input_sar, output_sar)``, from ``bss_eval_sources`` (host) or one
    ``bss_eval_sources_device`` call (device), which then gives the two SDRs as well.
    ``oracle``: baseline names (``ORACLES``); a last entry is then appended, {name: (sdr, sisdr)} -- the BSS-eval SDR and
    the SI-SDR of the baseline's estimates against ``gt``, row for row.  ``oracle_est`` holds the estimates {name: [n, T]},
    one row per row of ``gt`` (``record_from_result`` picks them from the masks of the sample's whole ground truth);
    without it they are ``oracle_estimates(gt, input_signal[0], ...)``.  On the device the baselines' rows join the same
    BSS call as further estimate sets."""
    check_metrics(metrics)
    check_bss(bss)
    oracle = check_oracle(oracle)
    gt = np.asarray(gt, dtype=np.float64)
    inp = np.asarray(input_signal, dtype=np.float64)
    est = np.asarray(est_signal, dtype=np.float64)
    if oracle and oracle_est is None:
        oracle_est = oracle_estimates(gt, inp[0], oracle, metrics)
    extra = [np.asarray(oracle_est[name], dtype=np.float64) for name in oracle]
    input_sisdr = [si_sdr(inp[i], gt[i]) for i in range(gt.shape[0])]
    output_sisdr = [si_sdr(est[i], gt[i]) for i in range(gt.shape[0])]
    if metrics == "host":
        sdr, sir, sar = (np.stack(v) for v in zip(*(bss_eval_sources(gt, rows)[:3] for rows in (inp, est, *extra))))
    elif bss == "all":
        sdr, sir, sar, _perm = bss_eval_sources_device(gt, np.stack([inp, est, *extra]))
    else:
        sdr = bss_eval_sdr_device(gt, np.stack([inp, est, *extra]))
    out = (sdr[0], sdr[1], input_sisdr, output_sisdr)
    if bss == "all":
        out += ((sir[0], sir[1], sar[0], sar[1]),)
    if oracle:
        out += ({name: (sdr[2 + q], [si_sdr(rows[i], gt[i]) for i in range(gt.shape[0])])
                 for q, (name, rows) in enumerate(zip(oracle, extra))},)
    return out


# ---- one sample --------------------------------------------------------------------------------
def evaluate_sample(model, metadata, mix, gt, metrics="host", bss="sdr", oracle=()):
    """Run ``model`` (a ``JointModel``) on one sample and build the reference's result record
    (sep/eval/eval_model.py:129-236).  Returns (record, tp, fp, fn).  ``metrics``: "host" or "device", where the
    record's two BSS-eval SDR fields come from (``compute_metrics``).  ``bss``: "sdr" (the record as it was) or "all"
    (``sir_in_mir``, ``sir_mir``, ``sar_in_mir``, ``sar_mir`` added to every matched talker's entry).  ``oracle``: the
    oracle mask baselines to score next to the output, as in ``record_from_result``; () leaves the record as it was."""
    check_metrics(metrics)
    check_bss(bss)
    oracle = check_oracle(oracle)
    return record_from_result(metadata, mix, gt, search_result(model, metadata, mix), metrics, bss=bss, oracle=oracle)


def search_result(model, metadata, mix):
    """The first step of ``evaluate_sample``: ``model`` set up for the sample's array and run on ``mix``.  -> what the
    record is built from, under the keys of ``shard.localize_batch(..., separate=, details=True)``: ``centres`` [K, 3],
    ``offsets`` (the ``localization_offset`` of every talker), ``audio_offsets``, ``audio_loc`` [K, T] (the
    localisation-stage audio) and ``audio`` (the separated audio, None without a separation model)."""
    import torch
    _mics, mic_positions, _voices, _gt_pos, _offsets_gt, roi = preprocess_metadata(metadata)
    model.setup(mic_positions=mic_positions, speaker_range=roi)
    patches, audio_loc, audio, _, _, _ = model(torch.from_numpy(np.ascontiguousarray(mix, dtype=np.float32)))
    n_out = len(patches)
    return {"centres": np.array([p[0].center_pos() for p in patches]).reshape(-1, 3),
            "offsets": [np.asarray(p[4]["localization_offset"]) for p in patches],
            "audio_offsets": [np.asarray(p[4]["audio_offset"]) for p in patches],
            "audio_loc": np.asarray(audio_loc).reshape(n_out, -1) if n_out else np.zeros((0, mix.shape[1])),
            "audio": audio}


def _separated(result):
    """The audio the record scores: the joint decoder's output when there is one, else the localisation stage's."""
    audio = result.get("audio")
    return result["audio_loc"] if audio is None else np.asarray(audio)


def record_from_result(metadata, mix, gt, result, metrics="host", scores=None, bss="sdr", oracle=()):
    """The second step of ``evaluate_sample``: the reference's result record (sep/eval/eval_model.py:129-236) from what
    the search returned (``search_result``, or a dict of ``shard.localize_batch(..., details=True)``).  Returns
    (record, tp, fp, fn).  Without ``scores`` every SI-SDR is ``hostdsp.si_sdr`` on the host and ``metrics`` says where
    the two BSS-eval SDR fields come from (``compute_metrics``).  ``scores`` (``records_from_results``) holds them
    ready-made: ``"sisdr"``, the [1 + K (+ K), n_gt] matrix of ``cross_sisdr_batch`` over the rows [mix[0]; separated;
    localisation stage] (the third block only with a separation model), ``"perm"``, the matching found from it, and
    ``"bss"``, the BSS-eval SDRs of the unprocessed and of the separated set, one row of ``matched`` values each.
    ``bss="all"`` adds four fields to every matched talker's entry: ``sir_in_mir`` / ``sar_in_mir`` of the unprocessed
    set and ``sir_mir`` / ``sar_mir`` of the separated set, the raw values and no differences (one talker has SIR +inf on
    both sides); ``scores["bss"]`` then holds their four rows too, after the two SDR rows and in the fields' order.
    ``oracle``: names among ``ORACLES``.  For "irm" every matched talker's entry gains ``si_snri_irm`` -- the SI-SDR of the
    ideal ratio mask's estimate for that ground truth, minus ``si_snr_in`` -- and ``si_snri_mir_irm`` -- its BSS-eval SDR
    minus ``si_snr_in_mir``; "ibm" likewise.  The masks are those of ``mix[0]`` with the sample's whole ground truth as
    references, in ground-truth order (``oracle_estimates``: the statements for ``metrics="host"``, the device
    otherwise), rounded to float32 and scored as the separated output is; ``scores["oracle"]`` holds them ready-made as
    {name: (sdr row, sisdr row)} of ``matched`` values.  With () the record is what it was."""
    check_metrics(metrics)
    check_bss(bss)
    oracle = check_oracle(oracle)
    _mics, mic_positions, _voices, gt_pos, offsets_gt, roi = preprocess_metadata(metadata)
    est_pos, audio_loc, sep_audio = result["centres"], result["audio_loc"], _separated(result)
    n_out = len(est_pos)
    est_off = [np.asarray(o) for o in result["offsets"]]
    if scores is not None:
        perm = scores["perm"]
    else:
        perm = find_best_permutation(gt, sep_audio, gt_pos, est_pos, acceptable_range=1) if n_out else []
    rec = {"mic_pos": mic_positions.tolist(), "speaker_pos": gt_pos.tolist(), "gt": [], "pred": [],
           "false_positive": [], "est_offsets": np.array(est_off).tolist(), "perm": perm}
    tp, fn, fp = len(perm), gt.shape[0] - len(perm), n_out - len(perm)
    for s in range(gt_pos.shape[0]):
        rec["gt"].append({"sample": offsets_gt[:, s].tolist(), "pos": gt_pos[s].tolist()})
    unmatched = list(range(n_out))
    # cols: per matched pair the SDR of the unprocessed and of the separated set, their SI-SDRs, the SI-SDR of the
    # localisation stage and, with bss="all", the four SIR / SAR values in the order of the fields below
    cols, oracle_cols = [], {}
    if perm and scores is not None:
        oracle_cols = scores.get("oracle") or {}
        M, loc0 = scores["sisdr"], 1 + (n_out if result.get("audio") is not None else 0)
        cols = [*scores["bss"][:2], [float(M[0, s]) for _o, s in perm], [float(M[1 + o, s]) for o, s in perm],
                [float(M[loc0 + o, s]) for o, s in perm], *scores["bss"][2:]]
    elif perm:
        # matched pairs in the reference's order (eval_model.py:162-187): separated output (joint
        # decoder when attached), localisation-stage output, ground truth, unprocessed mic 0
        pa = np.array(perm)
        ref_sig = np.repeat(mix[0:1].astype(np.float64), len(perm), axis=0)
        picked = {name: rows[pa[:, 1]] for name, rows in oracle_estimates(gt, mix[0], oracle, metrics).items()}
        m = compute_metrics(ref_sig, sep_audio[pa[:, 0]], gt[pa[:, 1]], metrics, bss, oracle, picked)
        loc_sisdr = [si_sdr(audio_loc[o].astype(np.float64), gt[s].astype(np.float64)) for o, s in perm]
        cols = [*m[:4], loc_sisdr, *(m[4] if bss == "all" else ())]
        oracle_cols = m[-1] if oracle else {}
    for i, (out_id, s) in enumerate(perm):
        unmatched.remove(out_id)
        in_sdr, out_sdr, in_sisdr, out_sisdr, loc_sisdr, *extra = (c[i] for c in cols)
        rec["pred"].append({
            "voice_id": s, "shifts": est_off[out_id].tolist(), "pos": est_pos[out_id].tolist(),
            "sample_err": float(np.mean(np.abs(est_off[out_id] - offsets_gt[:, s]))),
            "dis_err": float(np.linalg.norm(est_pos[out_id][:2] - gt_pos[s][:2])),
            "si_snr_in_mir": float(in_sdr), "si_snri_mir": float(out_sdr - in_sdr),   # BSS-eval SDR (restated)
            "si_snr_in": in_sisdr,
            "si_snri": out_sisdr - in_sisdr,
            "si_snr_in_old": in_sisdr,
            "si_snri_old": loc_sisdr - in_sisdr,
            **{k: float(v) for k, v in zip(("sir_in_mir", "sir_mir", "sar_in_mir", "sar_mir"), extra)},
            **{f"si_snri{kind}_{name}": float(oracle_cols[name][q][i] - base)
               for name in oracle for q, kind, base in ((1, "", in_sisdr), (0, "_mir", in_sdr))}})
    for rid in unmatched:
        rec["false_positive"].append({"pos": est_pos[rid].tolist(),
                                      "sample": np.asarray(result["audio_offsets"][rid]).tolist()})
    return rec, tp, fp, fn


def records_from_results(samples, results, metrics="host", ops=None, stats=None, bss="sdr", oracle=()):
    """The records of a batch: ``samples[k]`` = (metadata, mix, gt) as ``get_items`` reads them, ``results[k]`` what the
    search returned for it (``search_result`` / ``shard.localize_batch(..., details=True)``).  -> [(record, tp, fp, fn)]
    in sample order.  ``metrics="host"``: ``record_from_result`` per sample, the host statements throughout.
    ``metrics="device"``, three steps:
      1. ONE ``cross_sisdr_batch`` call: the estimate rows of a sample are [mix[0]; separated_0..K-1;
         localisation-stage_0..K-1] (the third block only with a separation model), the references its ground truth;
         the matcher's matrix and the record's four SI-SDR fields are entries of that one matrix;
      2. the matching of every sample on the host (``find_best_permutation(sisdr=...)``);
      3. ONE ``bss_eval_sdr_batch`` call over the matched rows of all samples (R = 2: unprocessed and separated);
         with ``bss="all"`` ONE ``bss_eval_sources_batch`` call in its place (the BSS stand-in of ``ops`` then has that
         op's signature).
    ``ops``: stand-ins (cross op, BSS op) for the two device ops (host tests).  ``stats``: a dict that receives the
    seconds of the steps (``"sisdr_s"``, ``"match_s"``, ``"bss_s"``).
    ``oracle``: baseline names as in ``record_from_result``.  On the device ONE ``oracle_masks_batch`` call per baseline
    comes first and covers every sample; its rows, rounded to float32, are appended to the estimate rows of step 1 (one
    per ground truth) and, picked by the matching, to the estimate sets of step 3 (R = 2 + the baselines): the number of
    device calls grows by the oracle calls only.  ``ops`` may then carry a third stand-in, for the oracle op, and
    ``stats`` receives ``"oracle_s"`` too."""
    import time
    check_metrics(metrics)
    check_bss(bss)
    oracle = check_oracle(oracle)
    if len(samples) != len(results):
        raise ValueError(f"{len(results)} results for {len(samples)} samples")
    if metrics == "host":
        return [record_from_result(meta, mix, gt, res, "host", bss=bss, oracle=oracle)
                for (meta, mix, gt), res in zip(samples, results)]
    cross_op, bss_op, *more_ops = ops if ops is not None else (None, None)
    t_start = time.perf_counter()
    masks = {name: [rows.astype(np.float32) for rows in
                    oracle_masks_batch([gt for _meta, _mix, gt in samples], [mix[0] for _meta, mix, _gt in samples], name,
                                       op=more_ops[0] if more_ops else None)] for name in oracle}
    t0 = time.perf_counter()
    est_rows, oracle_row0 = [], []
    for k, ((_meta, mix, _gt), res) in enumerate(zip(samples, results)):
        rows = [np.asarray(mix[0:1], dtype=np.float32), np.asarray(_separated(res), dtype=np.float32)]
        if res.get("audio") is not None:
            rows.append(np.asarray(res["audio_loc"], dtype=np.float32))
        oracle_row0.append(sum(r.reshape(-1, mix.shape[1]).shape[0] for r in rows))
        rows += [masks[name][k] for name in oracle]
        est_rows.append(np.concatenate([r.reshape(-1, mix.shape[1]) for r in rows], axis=0))
    mats, _ = cross_sisdr_batch(est_rows, [gt for _meta, _mix, gt in samples], op=cross_op)
    t1 = time.perf_counter()
    perms = []
    for (meta, _mix, gt), res, M in zip(samples, results, mats):
        K = len(res["centres"])
        gt_pos = preprocess_metadata(meta)[3]
        perms.append(find_best_permutation(gt, None, gt_pos, res["centres"], acceptable_range=1, sisdr=M[1:1 + K])
                     if K else [])
    t2 = time.perf_counter()
    matched = [k for k, perm in enumerate(perms) if perm]
    refs, sets = [], []
    for k in matched:
        (_meta, mix, gt), pa = samples[k], np.array(perms[k])
        ref_sig = np.repeat(np.asarray(mix[0:1], dtype=np.float32), len(pa), axis=0)
        refs.append(np.asarray(gt)[pa[:, 1]])
        sets.append(np.stack([ref_sig, np.asarray(_separated(results[k]), dtype=np.float32)[pa[:, 0]],
                              *(masks[name][k][pa[:, 1]] for name in oracle)]))
    if bss == "all":
        vals, _ = bss_eval_sources_batch(refs, sets, op=bss_op)
        scored = {k: (*sdr[:2], *sir[:2], *sar[:2]) for k, (sdr, sir, sar, _perm) in zip(matched, vals)}
        sdrs = {k: sdr for k, (sdr, _sir, _sar, _perm) in zip(matched, vals)}
    else:
        vals, _ = bss_eval_sdr_batch(refs, sets, op=bss_op)
        scored = {k: tuple(sdr[:2]) for k, sdr in zip(matched, vals)}
        sdrs = dict(zip(matched, vals))
    # per baseline the SDR row of its estimate set and the diagonal entries of its block of the SI-SDR matrix
    oracle_scores = {k: {name: (sdrs[k][2 + q], [float(mats[k][oracle_row0[k] + q * len(samples[k][2]) + s, s])
                                                 for _o, s in perms[k]]) for q, name in enumerate(oracle)} for k in matched}
    if stats is not None:
        stats.update(sisdr_s=t1 - t0, match_s=t2 - t1, bss_s=time.perf_counter() - t2)
        if oracle:
            stats.update(oracle_s=t0 - t_start)
    return [record_from_result(meta, mix, gt, res, "device",
                               {"sisdr": mats[k], "perm": perms[k], "bss": scored.get(k), "oracle": oracle_scores.get(k)},
                               bss=bss, oracle=oracle)
            for k, ((meta, mix, gt), res) in enumerate(zip(samples, results))]


def group_samples(shapes, batch):
    """The calls of ``evaluate_dataset(batch=)``: ``shapes[k]`` = (M, T) of sample k in sorted order; consecutive
    samples of equal shape go together, at most ``batch`` to a call.  -> list of (first, last) ranges, ``last``
    exclusive, covering every sample once and in order."""
    if batch < 1:
        raise ValueError(f"batch = {batch} < 1")
    groups, first = [], 0
    for k in range(1, len(shapes) + 1):
        if k == len(shapes) or tuple(shapes[k]) != tuple(shapes[first]) or k - first == batch:
            groups.append((first, k))
            first = k
    return groups


def evaluate_dataset(model, dataset_dir, results_folder=None, metrics="host", batch=1, concurrent=2, stats=None,
                     bss="sdr", oracle=()):
    """Every sample directory of ``dataset_dir``; writes ``result_<sample>.json`` like the
    reference and returns overall (tp, fp, fn, precision, recall).  ``metrics``, ``bss`` and ``oracle`` as in
    ``evaluate_sample``.

    ``batch=1``: one ``evaluate_sample`` per directory.  ``batch=N``: the directories in sorted order, consecutive
    samples of equal (M, T) in calls of at most N (``group_samples``); a call is ONE
    ``shard.localize_batch(..., geometries=, separate=, details=True, concurrent=concurrent)`` -- every sample on its
    own array -- followed by ONE ``records_from_results``.  Same files, same totals.  ``stats``: a dict that receives
    the summed seconds of reading, searching, the metrics steps and writing (tests/perf_eval_dataset.py)."""
    import time
    check_metrics(metrics)
    check_bss(bss)
    oracle = check_oracle(oracle)
    if batch < 1:
        raise ValueError(f"batch = {batch} < 1")
    tot = np.zeros(3, dtype=np.int64)
    spent = {"read_s": 0.0, "search_s": 0.0, "sisdr_s": 0.0, "match_s": 0.0, "bss_s": 0.0, "record_s": 0.0, "write_s": 0.0}
    if oracle:
        spent["oracle_s"] = 0.0

    def write(name, rec, tp, fp, fn):
        tot[:] += (tp, fp, fn)
        if results_folder is not None:
            t0 = time.perf_counter()
            os.makedirs(results_folder, exist_ok=True)
            with open(os.path.join(results_folder, f"result_{name}.json"), "w") as f:
                json.dump(rec, f, indent=4)
            spent["write_s"] += time.perf_counter() - t0

    def flush(group):
        from .shard import localize_batch
        samples = [item for _name, item in group]
        geometries = []
        for meta, _mix, _gt in samples:
            _mics, mic_positions, _voices, _gt_pos, _offsets_gt, roi = preprocess_metadata(meta)
            geometries.append((mic_positions, roi))
        import torch
        mixes = [torch.from_numpy(np.ascontiguousarray(mix, dtype=np.float32)) for _meta, mix, _gt in samples]
        t0 = time.perf_counter()
        results = localize_batch(model, mixes, geometries=geometries,
                                 separate=model.sep_model is not None, details=True, concurrent=concurrent)
        t1 = time.perf_counter()
        step = {}
        records = records_from_results(samples, results, metrics, stats=step, bss=bss, oracle=oracle)
        spent["search_s"] += t1 - t0
        spent["record_s"] += time.perf_counter() - t1
        for key, value in step.items():
            spent[key] += value
        for (name, _item), out in zip(group, records):
            write(name, *out)

    group = []
    for name in sorted(d for d in os.listdir(dataset_dir) if os.path.isdir(os.path.join(dataset_dir, d))):
        t0 = time.perf_counter()
        metadata, mix, gt = get_items(os.path.join(dataset_dir, name))
        spent["read_s"] += time.perf_counter() - t0
        if batch == 1:
            t0 = time.perf_counter()                         # evaluate_sample, its two steps timed apart
            result = search_result(model, metadata, mix)
            t1 = time.perf_counter()
            rec, tp, fp, fn = record_from_result(metadata, mix, gt, result, metrics, bss=bss, oracle=oracle)
            spent["search_s"] += t1 - t0
            spent["record_s"] += time.perf_counter() - t1
            write(name, rec, tp, fp, fn)
            continue
        # the grouping rule applied as the samples arrive: a second group means this sample opens a new call
        if len(group_samples([item[1].shape for _n, item in group] + [mix.shape], batch)) > 1:
            flush(group)
            group = []
        group.append((name, (metadata, mix, gt)))
    if group:
        flush(group)
    if stats is not None:
        stats.update(spent)
    tp, fp, fn = (int(v) for v in tot)
    return {"tp": tp, "fp": fp, "fn": fn, "precision": tp / max(tp + fp, 1), "recall": tp / max(tp + fn, 1)}
