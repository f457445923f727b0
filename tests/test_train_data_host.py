"""Host: the float64 statements and the host backend of acousticswarms_speech_amd/train_data.py
against what the reference returned (tests/golden/g18_training_batches.npz, written by make_golden_training.py), the
published Philox4x32-10 vectors, and properties.  No GPU."""
import json
import os
import random

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import train_data as td
from tests import train_data_cases as cases
from tests.golden import make_golden_training as mg


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    """The tiny dataset, rebuilt from the fixture's bytes."""
    return cases.rebuild_dataset(tmp_path_factory.mktemp("g18"))


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


# ---- 1. the reference's recorded outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("loc_train", "loc_test", "sep_train", "sep_test"))
def test_host_backend_returns_what_the_reference_returned(golden, dataset_dir, name):
    ds = cases.make_sets(dataset_dir)[name]
    probes = golden["probes"]
    for seed in mg.SEEDS:
        seed_all(seed)
        for j, idx in enumerate(mg.ITEMS):
            data, gt, extra = ds[idx]
            key = f"{name}_s{seed}_{j}"
            data, gt = data.numpy(), gt.numpy()
            assert data.dtype == np.float32 and gt.dtype == np.float32
            assert data.shape == (golden[key + "_data_sum"].shape[0], mg.T) and gt.shape == (golden[key + "_gt_sum"].shape[0], mg.T)
            assert np.array_equal(np.asarray(extra, dtype=np.float64), golden[key + "_extra"]), key
            assert np.array_equal(gt[:, probes], golden[key + "_gt_probe"]), key
            assert np.array_equal(gt.astype(np.float64).sum(-1), golden[key + "_gt_sum"]), key
            assert np.array_equal(data[:, probes], golden[key + "_data_probe"]), key
            assert np.array_equal(data.astype(np.float64).sum(-1), golden[key + "_data_sum"]), key
            assert np.array_equal((data.astype(np.float64) ** 2).sum(-1), golden[key + "_data_sq"]), key


@pytest.mark.parametrize("seed,rows,T", mg.PINK_CASES)
def test_pink_from_normals_is_powerlaw_psd_gaussian(golden, seed, rows, T):
    want = golden[f"pink_s{seed}_{rows}x{T}"]
    rng = np.random.default_rng(seed)
    sr = rng.normal(size=(rows, T // 2 + 1))
    si = rng.normal(size=(rows, T // 2 + 1))
    got = td.pink_from_normals(sr, si, T)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"pink_from_normals T={T}: {err:.3e} of the peak")
    assert err <= 1e-13


def loss_tolerance(name):
    """float32 sums of T = 4801 terms carry at most T 2^-24 relative error; on a logarithmic term that is 10 / ln 10 times
    as many dB; snr_w_scaled_neg weighs the L1 of the negative rows by 500."""
    est, gt = cases.loss_rows()
    rel = est.shape[1] * 2.0 ** -24
    l1 = float(np.max(td.row_losses_f64(est, gt)[:, 0]))
    weight = 500.0 if name == "snr_w_scaled_neg" else 1.0
    return weight * l1 * rel + (0.0 if name == "l1" else 10.0 / np.log(10.0) * rel)


@pytest.mark.parametrize("name", cases.LOSS_NAMES)
def test_loss_statements(golden, name):
    est, gt = cases.loss_rows()
    got = td.loss_f64(est[:, None, :], gt[:, None, :], name)
    recorded = float(golden["loss_" + name])                     # the reference's modules over the restated SingleSrcNegSDR
    restated = cases.loss_f32(torch.from_numpy(np.array(est))[:, None, :], torch.from_numpy(np.array(gt))[:, None, :], name)
    print(f"loss {name}: statement {got!r}, reference modules {recorded!r}, float32 restatement {restated!r}")
    assert abs(got - recorded) <= loss_tolerance(name) and abs(got - restated) <= loss_tolerance(name)
    # the named entry points are the same statement
    e3, g3 = est[:, None, :], gt[:, None, :]
    if name == "l1":
        assert td.l1_loss(e3, g3) == got
    elif name == "sisdr":
        assert td.sisdr_loss(e3, g3) == got
    else:
        assert td.composite_loss(e3, g3, *td.LOSS_PARAMS[name]) == got


def test_separation_loss_reshapes_to_rows():
    est, gt = cases.loss_rows()
    e, g = est[:4].reshape(2, 2, -1), gt[:4].reshape(2, 2, -1)
    assert td.loss_f64(e, g, "snr") == td.loss_f64(est[:4, None, :], gt[:4, None, :], "snr")
    with pytest.raises(ValueError):
        td.loss_f64(e, g, "mse")


# ---- 2. Philox4x32-10: the known-answer vectors of the Random123 distribution ---------------------------------------------
@pytest.mark.parametrize("counter,key,want", (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))))
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w[0]) for w in td.philox4x32(counter, key)) == want


def test_philox_normals_counter_layout():
    """(index, row, stream, 0) under the key's low and high word: a block of philox_normals is the plain generator's."""
    key, row = 0x299F31D0A4093822, 7
    w = td.philox4x32((np.array([3]), row, td.STREAM_WHITE, 0), (0xA4093822, 0x299F31D0))
    u1, u2 = td.words_to_uniform(w[0], w[1]), td.words_to_uniform(w[2], w[3])
    z0, z1 = td.philox_normals(key, row, 4, td.STREAM_WHITE)
    assert z0[3] == (np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2))[0] and z1[3] == (np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2))[0]
    assert not np.array_equal(z0, td.philox_normals(key, row, 4, td.STREAM_PINK)[0])
    assert not np.array_equal(z0, td.philox_normals(key, row + 1, 4, td.STREAM_WHITE)[0])
    assert np.array_equal(z0, td.philox_normals(key - 2 ** 64, row, 4, td.STREAM_WHITE)[0])      # keys are 64-bit words


# ---- 3. the noise statement ---------------------------------------------------------------------------------------------
def test_uniforms_lie_strictly_inside_the_unit_interval():
    lo, hi = td.words_to_uniform(0, 0), td.words_to_uniform(0xFFFFFFFF, 0xFFFFFFFF)
    assert lo == 2.0 ** -53 and hi == 1.0 - 2.0 ** -53 and 0.0 < lo < hi < 1.0
    u = td.words_to_uniform(np.array([0, 1, 0x80000000]), np.array([0xFFF, 0x1000, 0]))
    assert np.array_equal(u * 2.0 ** 53, [1.0, 2.0 ** 21 + 3.0, 2.0 ** 52 + 1.0])                  # exact odd numerators


NOISE_ROWS, NOISE_T = 256, 4096


def test_noise_has_unit_variance_and_a_pink_slope():
    """256 rows of 4096 samples.  The variance of a row of 1/f noise scatters by sqrt(sum 1/k^2) / sum 1/k = 16 % (few low
    bins carry most of the power), so the mean over 256 rows scatters by 1 %: the bar of 5 % is five of those.  The slope
    of the row-averaged periodogram over bins 4..1024, fitted in log-log, has a standard error of about
    sqrt(12 / (256 n)) / span with n = 1021 bins over a span of ln(256): 0.001; the bar of 0.02 is far outside it.  The
    statement alone measures 1.006 and -1.0025 here."""
    y = td.colored_noise_f64(2024, NOISE_ROWS, NOISE_T)
    var = float(np.mean(np.var(y, axis=1)))
    p = np.mean(np.abs(np.fft.rfft(y, axis=1)) ** 2, axis=0)
    k = np.arange(4, 1025)
    slope = float(np.polyfit(np.log(k), np.log(p[k]), 1)[0])
    w = np.stack([td.philox_normals(2024, r, NOISE_T, td.STREAM_WHITE)[0] for r in range(8)])
    print(f"pink: variance {var:.4f}, slope {slope:.4f}; white: mean {w.mean():.4f}, variance {w.var():.4f}")
    assert abs(var - 1.0) <= 0.05 and abs(slope + 1.0) <= 0.02
    # the white stream: 32768 unit normals, mean within 4 / sqrt(n) and variance within 4 sqrt(2 / n)
    assert abs(w.mean()) <= 4 / np.sqrt(w.size) and abs(w.var() - 1.0) <= 4 * np.sqrt(2.0 / w.size)


def test_perturb_is_the_sum_rounded_once():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 257)).astype(np.float32)
    full = td.perturb_f64(x, 5e-3, 1e-3, 11, 12, rounded=False)
    w = np.stack([td.philox_normals(12, c, 257, td.STREAM_WHITE)[0] for c in range(3)])
    assert np.array_equal(full, x.astype(np.float64) + 1e-3 * w + 5e-3 * td.colored_noise_f64(11, 3, 257))
    assert np.array_equal(td.perturb_f64(x, 5e-3, 1e-3, 11, 12), full.astype(np.float32))
    assert td.perturb_f64(x, 0.0, 0.0, 11, 12).tobytes() == x.tobytes()


# ---- 4. roll_rows ---------------------------------------------------------------------------------------------------------
def test_roll_rows():
    mix = cases.batch_mix()[0]
    T = cases.T
    for shifts in cases.ROLL_SHIFTS:
        out = td.roll_rows(mix, shifts)
        for c, s in enumerate(shifts):
            if abs(s) > T:
                assert not out[c].any()
            else:
                t = np.arange(T)
                assert np.array_equal(out[c], mix[c][(t - s) % T])
    assert np.array_equal(td.roll_rows(mix, [T] * 7), mix) and np.array_equal(td.roll_rows(mix, [-T] * 7), mix)
    assert np.array_equal(td.roll_rows(mix, [1] * 7)[:, 1:], mix[:, :-1])
    # the reference's function on the same rows (torch.roll per channel, zero beyond T)
    for shifts in cases.ROLL_SHIFTS:
        ref = torch.zeros(7, T)
        for c, s in enumerate(shifts):
            if abs(s) <= T:
                ref[c] = torch.roll(torch.from_numpy(np.array(mix[c])), s)
        assert np.array_equal(td.roll_rows(mix, shifts), ref.numpy())


# ---- 5. decisions -------------------------------------------------------------------------------------------------------------
def test_negative_regions_keep_out_and_positive_regions_are_audible(dataset_dir):
    ds = td.LocalizationDataset(dataset_dir, "train", **dict(mg.LOC_TRAIN, negatives=0.6))
    seed_all(5)
    seen = {"neg": 0, "pos": 0}
    for idx in range(40):
        dec = ds.decide(idx)
        _d, metadata = ds._metadata(idx)
        offsets, _ = td.voice_offsets(metadata, ds.sr)
        w = dec.extra
        linf = np.max(np.abs(offsets - dec.shifts[0]), axis=1)
        if not dec.gt.any():
            seen["neg"] += 1
            assert np.min(linf) > td.MAX_SHIFTS[w] + 1                       # outside every talker's patch, with the margin
        else:
            seen["pos"] += 1
            assert np.min(linf) <= td.MAX_SHIFTS[w] and (dec.gt > 0).any()
    assert seen["neg"] >= 10 and seen["pos"] >= 10
    with open(os.path.join(dataset_dir, "00000", "metadata.json")) as f:
        metadata = json.load(f)
    for w in (0, 1):
        for _ in range(10):
            s, point = td.negative_region(metadata, w, 48000)
            assert np.min(np.max(np.abs(td.voice_offsets(metadata, 48000)[0] - s), axis=1)) > td.MAX_SHIFTS[w] + 1
            assert 0.0 <= point[2] <= td.MAX_SPEAKER_RELATIVE_HEIGHT and s[0] == 0
    assert td.neg_prob(30, 3, 0.3, True) == pytest.approx(0.4) and td.neg_prob(3, 3, 0.3, True) == 0.2
    assert td.neg_prob(300, 3, 0.3, True) == 0.5 and td.neg_prob(300, 3, 0.3, False) == 0.3


def test_real_samples_take_their_shifts_from_the_metadata(dataset_dir, tmp_path):
    """The ``real`` branch: M shifts per talker in the metadata, used as they are (no [0] prefix, no perturbation)."""
    import shutil
    root = tmp_path / "real"
    shutil.copytree(os.path.join(dataset_dir, "00000"), root / "00000")
    with open(root / "00000" / "metadata.json") as f:
        metadata = json.load(f)
    metadata["real"] = True
    for k in metadata:
        if k.startswith("voice"):
            metadata[k]["shifts"] = [5] + [5 + v for v in metadata[k]["shifts"]]
    with open(root / "00000" / "metadata.json", "w") as f:
        json.dump(metadata, f)
    ds = td.LocalizationDataset(str(root), "train", **dict(mg.LOC_TRAIN, negatives=0.0))
    seed_all(1)
    dec = ds.decide(0)
    offsets, _ = td.voice_offsets(metadata, 48000)
    assert any(np.array_equal(dec.shifts[0], o) for o in offsets) and dec.gt.any()
    sep = td.SeparationDataset(str(root), "test", **mg.SEP_TEST)
    assert np.array_equal(sep.decide(0).shifts[:3], offsets)


def test_batches_host_backend_and_dataloader(dataset_dir):
    sets = cases.make_sets(dataset_dir)
    for name, ds in sets.items():
        a = list(ds.batches(3, seed=4, backend="host"))
        b = list(ds.batches(2, seed=4, backend="host"))
        assert [x[0].shape[0] for x in a] == [2] and [x[0].shape[0] for x in b] == [2]      # two samples in the directory
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y)                                                       # seeded per item, not per batch
        rows = (4 if name.startswith("sep") else 1) * 7
        assert a[0][0].shape == (2, rows, mg.T) and a[0][0].dtype == torch.float32
        assert a[0][1].shape == (2, 4 if name.startswith("sep") else 1, mg.T)
        assert a[0][2].shape == ((2,) if name.startswith("sep") else (2, 2))
    loader = torch.utils.data.DataLoader(sets["sep_test"], batch_size=2)
    data, gt, n = next(iter(loader))
    assert data.shape == (2, 28, mg.T) and gt.shape == (2, 4, mg.T) and n.tolist() == [3, 3]
    with pytest.raises(ValueError):
        next(sets["loc_test"].batches(2, backend="cpu"))


# ---- 6. mine_negatives ----------------------------------------------------------------------------------------------------
def test_mine_negatives_with_a_stub_pruner(dataset_dir, tmp_path):
    import shutil
    import types
    root = tmp_path / "mine"
    shutil.copytree(dataset_dir, root)
    os.remove(root / "00001" / "metadata.json")
    with open(root / "00000" / "metadata.json") as f:
        metadata = json.load(f)
    gt = np.array([metadata[k]["shifts"] for k in metadata if k.startswith("voice")])         # [S][M-1]
    offsets = [gt[0] + 4, gt[1] + np.array([5, 0, 0, 0, 0, 0]), gt[2] - 4, np.array([60, -60, 60, -60, 60, -60])]
    calls = []

    class StubArray:
        def __init__(self, mic_positions, Spk_Range=None, Prone_method=None, grid_size=None):
            calls.append((mic_positions.shape, list(Spk_Range), Prone_method, grid_size))

        def Apply_SRP_PHAT(self, mix):
            calls.append(tuple(mix.shape))
            return [types.SimpleNamespace(sample_offset=o) for o in offsets], None

    with pytest.warns(UserWarning, match="no metadata.json"):
        done = td.mine_negatives(str(root), sample_number=3, start=0, mic_array=StubArray)
    assert list(done) == [str(root / "00000")]
    assert calls == [((7, 3), list(metadata["ROI"]), "SRP", 0.065), (7, mg.T)]
    with open(root / "00000" / "challeng_sample.json") as f:
        written = json.load(f)
    # within 4.9 samples on every channel of some talker: positive
    assert written == {"negative_sample": [offsets[1].tolist(), offsets[3].tolist()], "positive_sample": [offsets[0].tolist(), offsets[2].tolist()]}
    assert not os.path.exists(root / "00002")


# ---- 7. codec -------------------------------------------------------------------------------------------------------------------
def test_a_compression_prob_that_would_apply_the_codec_raises(dataset_dir):
    for cls in (td.LocalizationDataset, td.SeparationDataset):
        with pytest.raises(NotImplementedError, match="Opus"):
            cls(dataset_dir, "train")                                     # the reference's default of 0.7
        with pytest.raises(NotImplementedError, match="Opus"):
            cls(dataset_dir, "test", compression_prob=-0.5)               # validation: abs(compression_prob) > 1e-6
        with pytest.raises(NotImplementedError, match="Opus"):
            cls(dataset_dir, "val", compression_prob=1e-3)
        cls(dataset_dir, "train", compression_prob=0)
        cls(dataset_dir, "train", compression_prob=-0.5)                  # never below a uniform draw: the codec is never applied
        cls(dataset_dir, "test", compression_prob=1e-7)
