"""Training-batch fixture (g18): run the REFERENCE's own ``powerlaw_psd_gaussian`` (sep/helpers/pink_noise.py), both
``Dataset.__getitem__`` (sep/training/SpeakerLocalization/dataset.py, SpeakerSeparation/dataset.py) and ``CompositeLoss``
/ ``SISDRLoss`` / ``nn.L1Loss`` (sep/training/losses.py, base_network.py) on a tiny sample directory and record what
they return, together with the directory's contents.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_training.py

The reference's modules import packages that are absent here (torchaudio, soundfile, opuslib, asteroid, ...): they are
replaced by the inert stubs of ``make_golden.install_stubs`` so that the ``import`` lines succeed.  Two stand-ins supply
behaviour, both stated here: ``utils.read_audio_file_torch`` is replaced by the project's wav reader (``torchaudio`` is
absent; the wavs are float32, read back bit for bit), and ``asteroid.losses.sdr.SingleSrcNegSDR`` by the float32 torch
restatement of its published formula in tests/train_data_cases.py -- so the loss values pin the reference's masks, means
and weights, and parity with an installed asteroid stays unpinned.

The directory: two samples of 7 microphones, 3 talkers and T = 2400 written by ``evalkit.write_scene_dir``, with each
talker's ``shifts`` (the rounded TDoA of the synthetic convention), the ROI and a ``challeng_sample.json`` added.
Recorded per item (dataset, seed, place in the sequence drawn after one ``seed_all``): the data and the ground truth at
PROBES, every row's float64 sum and sum of squares, and the third member of the tuple -- a wrong draw anywhere moves all
of them.  Full arrays would not fit the size limit of a committed file (a separation item is 28 x 2400 floats of noise).
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

T = 2400
PROBES = np.array([0, 1, 2, 3, 4, 5, 17, 255, 256, 1023, 1199, 1200, 1201, 2047, 2393, 2394, 2395, 2396, 2397, 2398, 2399])
N_SAMPLES, N_TALKERS, N_MICS = 2, 3, 7
SEEDS = (0, 1, 2)
ITEMS = (0, 1, 2, 3, 4, 5)                 # indices drawn one after the other under one seed (idx % 2 picks the sample)
LOC_TRAIN = dict(n_mics=N_MICS, sr=48000, negatives=0.5, compression_prob=0, fixed_window_condition=-1, challenge_ratio=0.5)
LOC_TEST = dict(n_mics=N_MICS, sr=48000, negatives=0.5, compression_prob=0, fixed_window_condition=1, challenge_ratio=0.5,
                scale_neg_prob=True)
SEP_TRAIN = dict(n_mics=N_MICS, n_speakers=4, sr=48000, compression_prob=0, speaker_drop_prob=0.3, speaker_add_prob=0.5)
SEP_TEST = dict(n_mics=N_MICS, n_speakers=4, sr=48000, compression_prob=0)
PINK_CASES = ((5, 2, 2400), (6, 2, 801))   # (seed, rows, T): even and odd


def false_positives(scene_tdoa):
    """A challeng_sample.json for a sample: two points well away from every talker, one next to talker 0 (so that the
    retry of get_negative_region_SRP is taken)."""
    near = (scene_tdoa[0] + np.array([1, -1, 0, 1, 0, -1])).astype(int).tolist()
    return {"negative_sample": [[40, -35, 30, -32, 28, -40], near, [-25, 31, -37, 22, -29, 33]], "positive_sample": []}


def write_dataset(root, n_samples=N_SAMPLES, T=T):
    """The tiny dataset (the fixture holds its bytes; the GPU validation test writes a longer one): -> {relative path: bytes}."""
    from acousticswarms_speech_amd import evalkit
    from acousticswarms_speech_amd.scenes import make_scene
    files = {}
    seed = 180
    for k in range(n_samples):
        d = os.path.join(root, f"{k:05d}")
        while True:                            # 50 ms can fall into a pause of a talker: the reference asserts an audible target
            scene = make_scene(seed, N_TALKERS, N_MICS, T)
            seed += 1
            if all((src > 0).any() for src in scene.sources):
                break
        evalkit.write_scene_dir(scene, d)
        with open(os.path.join(d, "metadata.json")) as f:
            meta = json.load(f)
        tdoa = np.asarray(scene.tdoa_samples())
        tdoa = tdoa if tdoa.shape[0] == N_TALKERS else tdoa.T                  # [talkers][M - 1]
        for s in range(N_TALKERS):
            meta[f"voice{s:02d}"]["shifts"] = [int(np.round(v)) for v in tdoa[s]]
        with open(os.path.join(d, "metadata.json"), "w") as f:
            json.dump(meta, f, indent=1)
        with open(os.path.join(d, "challeng_sample.json"), "w") as f:
            json.dump(false_positives(np.round(tdoa)), f, indent=1)
        for name in sorted(os.listdir(d)):
            with open(os.path.join(d, name), "rb") as f:
                files[f"{k:05d}/{name}"] = f.read()
    return files


def item_record(out, key, data, gt, extra):
    data, gt = np.asarray(data), np.asarray(gt)
    assert data.dtype == np.float32 and gt.dtype == np.float32
    out[key + "_data_probe"] = data[:, PROBES]
    out[key + "_data_sum"] = data.astype(np.float64).sum(-1)
    out[key + "_data_sq"] = (data.astype(np.float64) ** 2).sum(-1)
    out[key + "_gt_probe"] = gt[:, PROBES]
    out[key + "_gt_sum"] = gt.astype(np.float64).sum(-1)
    out[key + "_extra"] = np.asarray(extra, dtype=np.float64)


def main():
    sys.path.insert(0, ROOT)
    import torch
    from tests.golden import make_golden
    from tests import train_data_cases as cases
    make_golden.install_stubs()

    class SingleSrcNegSDR:                                      # the restated formula, see the module docstring
        def __init__(self, sdr_type):
            self.kind = sdr_type

        def __call__(self, est, gt):
            return cases.neg_sdr_f32(est, gt, self.kind)
    sys.modules["asteroid.losses.sdr"].SingleSrcNegSDR = SingleSrcNegSDR
    from acousticswarms_speech_amd import evalkit
    import sep.helpers.utils as utils
    from sep.helpers.pink_noise import powerlaw_psd_gaussian
    utils.read_audio_file_torch = lambda path: torch.from_numpy(evalkit._read_wav(path))[None, :]
    from sep.training.SpeakerLocalization.dataset import Dataset as LocDataset
    from sep.training.SpeakerSeparation.dataset import Dataset as SepDataset
    from sep.training.losses import CompositeLoss, SISDRLoss

    out = {"probes": PROBES}
    seen = {"pos": 0, "neg_random": 0, "neg_srp": 0, "w0": 0, "w1": 0, "fake": 0, "dropped": 0}
    with tempfile.TemporaryDirectory() as root:
        files = write_dataset(root)
        out["file_names"] = np.array(sorted(files))
        for name in sorted(files):
            out["file_" + name] = np.frombuffer(files[name], dtype=np.uint8)
        for base, meth, tag in ((LocDataset, "get_positive_region", "pos"), (LocDataset, "get_negative_region", "neg_random"),
                                (LocDataset, "get_negative_region_SRP", "neg_srp"), (SepDataset, "get_negative_region", "fake")):
            def wrap(fn, tag=tag):
                def counted(self, *a, **k):
                    seen[tag] += 1
                    return fn(self, *a, **k)
                return counted
            setattr(base, meth, wrap(getattr(base, meth)))
        sets = {"loc_train": LocDataset("train", root, **LOC_TRAIN), "loc_test": LocDataset("test", root, **LOC_TEST),
                "sep_train": SepDataset(root, "train", **SEP_TRAIN), "sep_test": SepDataset(root, "test", **SEP_TEST)}
        for name, ds in sets.items():
            for seed in SEEDS:
                utils.seed_all(seed)
                for j, idx in enumerate(ITEMS):
                    data, gt, extra = ds[idx]
                    if name.startswith("loc"):
                        seen["w%d" % int(np.argmax(extra.numpy()))] += 1
                    elif int(extra) < N_TALKERS:
                        seen["dropped"] += 1
                    item_record(out, f"{name}_s{seed}_{j}", data.numpy(), gt.numpy(), extra)
    print("occurrences:", seen)
    assert all(v > 0 for v in seen.values()), seen

    for seed, rows, t in PINK_CASES:
        out[f"pink_s{seed}_{rows}x{t}"] = powerlaw_psd_gaussian(1, (rows, t), random_state=seed)

    est, gt = cases.loss_rows()
    e, g = torch.from_numpy(np.array(est))[:, None, :], torch.from_numpy(np.array(gt))[:, None, :]
    out["loss_l1"] = np.float64(torch.nn.L1Loss()(e, g))
    out["loss_snr"] = np.float64(CompositeLoss()(e, g))
    out["loss_snr_w_scaled_neg"] = np.float64(CompositeLoss(r=0, n=500)(e, g))
    out["loss_fused"] = np.float64(CompositeLoss(r=0.05)(e, g))
    out["loss_sisdr"] = np.float64(SISDRLoss()(e, g))

    path = os.path.join(HERE, "g18_training_batches.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
