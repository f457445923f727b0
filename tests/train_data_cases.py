"""Cases shared by tests/test_train_data_host.py and tests/test_gpu_train_data.py: the noise sizes,
the roll shifts, the train_batch items, the loss rows, and a float32 torch restatement of asteroid's SingleSrcNegSDR that
the float64 loss statements are compared with.  Every statement is computed once and cached."""
import functools
import os

import numpy as np
import torch

from acousticswarms_speech_amd import train_data as td

# (T, rows, max_rows_per_pass): below one 1024-point transform; odd with L = 2048; even; odd with L = 16384; the two
# lengths of the training sets; a seam plus a remainder (passes of 2, 2 and 1 rows).  Then the sizes at which the code
# takes another path: the shortest row, the last T of L = 1024 and the first of L = 2048 (a single row: a pair without
# its second member), and the longest row (column transforms of 1024 points, two columns per workgroup).
NOISE_CASES = ((7, 3, 0), (1023, 3, 0), (2050, 3, 0), (4801, 3, 0), (48000, 2, 0), (144000, 2, 0), (4801, 5, 2),
               (2, 1, 0), (512, 1, 0), (513, 1, 0), (524288, 1, 0))
NOISE_KEY = 0x9E3779B97F4A7C15          # beyond 2^63: both key words in use, the sign bit too


@functools.lru_cache(maxsize=None)
def noise_statement(T, rows):
    out = td.colored_noise_f64(NOISE_KEY, rows, T)
    out.setflags(write=False)
    return out


def row_errors(got, want):
    """max |got - want| over the last axis, relative to the row's max |want| (absolute for a row of zeros)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    peak = np.max(np.abs(want), axis=-1)
    return np.max(np.abs(got - want), axis=-1) / np.where(peak > 0, peak, 1.0)


# ---- roll and train_batch: K = 2, M = 7, T = 2050 -----------------------------------------------------------------------
K, M, T = 2, 7, 2050
ROLL_SHIFTS = ([0, 1, -1, T - 1, -(T - 1), T, -T], [0, T + 1, -(T + 1), 5, -7, 2 * T, -3 * T])     # the second: beyond T


@functools.lru_cache(maxsize=None)
def batch_mix():
    rng = np.random.default_rng(18)
    mix = (0.1 * rng.standard_normal((K, M, T))).astype(np.float32)
    mix.setflags(write=False)
    return mix


def batch_items(s_max, noisy):
    """The item tables of one train_batch call: four items with counts 0..s_max (cycled), both mixtures, the two roll shift
    vectors alternating over the talker blocks; ``noisy`` picks non-zero levels (one item keeps a zero white level, one a
    zero pink level)."""
    n = 4
    shifts = np.zeros((n, s_max, M), dtype=np.int32)
    for i in range(n):
        for s in range(s_max):
            shifts[i, s] = ROLL_SHIFTS[(i // 2 + s) % 2]
    items = dict(item_mix=[i % K for i in range(n)], shifts=shifts, counts=[i % (s_max + 1) for i in range(n)],
                 pink_level=[0.0] * n, white_level=[0.0] * n, pink_key=[1000 + i for i in range(n)],
                 white_key=[(0xD1B54A32D192ED03 * (i + 1)) % 2 ** 64 for i in range(n)])
    if noisy:
        items["pink_level"] = [5e-3 * (i + 1) / n for i in range(n)]
        items["white_level"] = [1e-3 * (n - i) / n for i in range(n)]
        items["pink_level"][1] = 0.0
        items["white_level"][n - 1] = 0.0
    return items


@functools.lru_cache(maxsize=None)
def batch_statement(s_max, noisy, rounded):
    it = batch_items(s_max, noisy)
    out = td.train_batch_f64(batch_mix(), it["item_mix"], it["shifts"], it["counts"], it["pink_level"], it["white_level"],
                             it["pink_key"], it["white_key"], rounded=rounded)
    out.setflags(write=False)
    return out


# ---- losses: N = 5, T = 4801 --------------------------------------------------------------------------------------------
LOSS_NAMES = ("l1", "snr", "snr_w_scaled_neg", "fused", "sisdr")


@functools.lru_cache(maxsize=None)
def loss_rows():
    """(est, gt) float32 [5][4801]: an all-zero gt (a negative sample), est == gt (only the EPS terms are left), a DC
    offset of 1 under a signal of 1e-3 (raw moments would lose ten digits), and two ordinary rows."""
    rng = np.random.default_rng(4801)
    n, t = 5, 4801
    gt = (0.1 * rng.standard_normal((n, t))).astype(np.float32)
    est = (gt + 0.03 * rng.standard_normal((n, t))).astype(np.float32)
    gt[0] = 0.0
    est[1] = gt[1]
    sig = rng.standard_normal(t)
    gt[2] = (1.0 + 1e-3 * sig).astype(np.float32)
    est[2] = (1.0 + 1e-3 * (sig + 0.1 * rng.standard_normal(t))).astype(np.float32)
    est.setflags(write=False)
    gt.setflags(write=False)
    return est, gt


def neg_sdr_f32(est, gt, kind):
    """asteroid.losses.sdr.SingleSrcNegSDR(kind) (zero_mean=True, take_log=True, reduction='none', EPS=1e-8) restated in
    float32 torch from its published source; est, gt [N][T] tensors -> [N]."""
    eps = 1e-8
    gt = gt - torch.mean(gt, dim=1, keepdim=True)
    est = est - torch.mean(est, dim=1, keepdim=True)
    if kind == "sisdr":
        dot = torch.sum(est * gt, dim=1, keepdim=True)
        energy = torch.sum(gt ** 2, dim=1, keepdim=True) + eps
        target = dot * gt / energy
    else:
        target = gt
    noise = est - target
    losses = torch.sum(target ** 2, dim=1) / (torch.sum(noise ** 2, dim=1) + eps)
    return -10 * torch.log10(losses + eps)


def loss_f32(est, gt, name):
    """The reference's loss modules in float32 torch over ``neg_sdr_f32``; est, gt [N][1][t] tensors."""
    if name == "l1":
        return float(torch.mean(torch.abs(est - gt)))
    e, g = est[:, 0], gt[:, 0]
    mask = torch.absolute(g).max(dim=1)[0] == 0
    if name == "sisdr":
        return float(torch.mean(neg_sdr_f32(e[~mask], g[~mask], "sisdr")))
    r, n = td.LOSS_PARAMS[name]
    l1 = torch.abs(e - g)
    snr = neg_sdr_f32(e, g, "snr")
    loss = 0.0
    if mask.any():
        loss += float(torch.mean(l1[mask])) * n
    if (~mask).any():
        loss += float(torch.mean(l1[~mask])) * r + float(torch.mean(snr[~mask])) * (1 - r)
    return loss


# ---- the tiny dataset of tests/golden/g18_training_batches.npz ------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_training_batches.npz")


def rebuild_dataset(root):
    """Write the fixture's sample directories under ``root``, byte for byte."""
    golden = np.load(GOLDEN)
    for name in golden["file_names"]:
        path = os.path.join(root, str(name))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(golden["file_" + str(name)].tobytes())
    return str(root)


def make_sets(root):
    """The four datasets of the fixture over ``root``, with the fixture's parameters."""
    from tests.golden import make_golden_training as mg
    return {"loc_train": td.LocalizationDataset(root, "train", **mg.LOC_TRAIN), "loc_test": td.LocalizationDataset(root, "test", **mg.LOC_TEST),
            "sep_train": td.SeparationDataset(root, "train", **mg.SEP_TRAIN), "sep_test": td.SeparationDataset(root, "test", **mg.SEP_TEST)}
