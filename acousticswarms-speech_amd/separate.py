"""Separate one recording of any length into its talkers:

    python -m acousticswarms_speech_amd.separate RECORDING_DIR --spot_experiment_dir D --sep_experiment_dir D --out DIR
        [--block 48000] [--hop N] [--localize every|first] [--link_radius 0.25] [--sr 48000]
        [--precision f16x3|f16x3_safe|f32] [--spot_batch_size 128] [--geometry host|device]

RECORDING_DIR is a sample directory as ``evalkit.get_items`` reads it (``metadata.json`` with the microphone positions
and the region of interest, ``micNN_mixed.wav``); ground-truth files are not needed.  Loads both networks like
``evaluate``, sets the array up once, runs ``JointModel.forward_long`` and writes ``trackNN.wav`` (float32) per track
and ``tracks.json`` into DIR.  No counterpart in the reference.  Nothing runs at import."""
import argparse
import json
import os

import numpy as np

from .evaluate import PRECISIONS


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acousticswarms_speech_amd.separate",
                                description="Localise and separate the talkers of one recording of any length.")
    p.add_argument("recording", type=str, help="Path to the recording's directory (metadata.json, micNN_mixed.wav)")
    p.add_argument("--spot_experiment_dir", type=str, help="Experiment directory for spotforming submodel")
    p.add_argument("--sep_experiment_dir", type=str, help="Experiment directory for separation submodel")
    p.add_argument("--out", type=str, help="Directory for trackNN.wav and tracks.json")
    p.add_argument("--block", type=int, default=48000, help="Samples per block: the clip length the networks run at")
    p.add_argument("--hop", type=int, default=None, help="Samples between block starts (default block - block // 8)")
    p.add_argument("--localize", choices=("every", "first"), default="every",
                   help="Search every block and link the talkers, or search block 0 and keep its talkers throughout")
    p.add_argument("--link_radius", type=float, default=0.25, help="Metres within which a detection continues a track")
    p.add_argument("--sr", type=int, default=48000, help="Sampling rate written into the wav files")
    p.add_argument("--spot_batch_size", dest="spot_batch_size", type=int, default=128,
                   help="Batch size for spotforming submodel")
    p.add_argument("--precision", choices=PRECISIONS, default="f32", help="Arithmetic of both networks")
    p.add_argument("--geometry", choices=("host", "device"), default="host", help="Where the array geometry is built")
    return p


def write_tracks(result, out_dir, sr=48000, settings=None):
    """``JointModel.forward_long``'s result -> ``trackNN.wav`` per track (float32, the writer ``evalkit`` uses) and
    ``tracks.json``: the settings given, the block starts, and per track its file, its mean position, the blocks it is
    present in and its position in each of them (null where absent).  -> the dict written as ``tracks.json``."""
    from scipy.io import wavfile
    os.makedirs(out_dir, exist_ok=True)
    tracks = []
    for s, audio in enumerate(result["audio"]):
        name = f"track{s:02d}.wav"
        wavfile.write(os.path.join(out_dir, name), int(sr), np.ascontiguousarray(audio, dtype=np.float32))
        present = [bool(v) for v in result["present"][s]]
        tracks.append({"file": name, "position": [float(v) for v in result["positions"]["mean"][s]], "present": present,
                       "positions": [[float(v) for v in c] if here else None
                                     for c, here in zip(result["positions"]["per_block"][s], present)]})
    doc = dict(settings or {}, sr=int(sr), starts=[int(a) for a in result["starts"]], tracks=tracks)
    with open(os.path.join(out_dir, "tracks.json"), "w") as f:
        json.dump(doc, f, indent=1)
    return doc


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.spot_experiment_dir or not args.sep_experiment_dir or not args.out:
        raise SystemExit("--spot_experiment_dir, --sep_experiment_dir and --out are all needed")
    from . import evalkit
    from .experiment import load_model_from_exp
    from .joint import JointModel
    metadata, mix, _gt = evalkit.get_items(args.recording)
    _mics, mic_positions, _voices, _gt_pos, _offsets_gt, roi = evalkit.preprocess_metadata(metadata)
    device = "cuda:0"
    spot = load_model_from_exp(args.spot_experiment_dir, precision=args.precision, batch_size=args.spot_batch_size)
    sep = load_model_from_exp(args.sep_experiment_dir, precision=args.precision)
    model = JointModel(spot, sep, device=device, geometry=args.geometry).to(device)
    model.setup(mic_positions=mic_positions, speaker_range=roi)
    hop = args.block - args.block // 8 if args.hop is None else args.hop
    result = model.forward_long(mix, block=args.block, hop=hop, localize=args.localize, link_radius=args.link_radius)
    doc = write_tracks(result, args.out, args.sr, {"block": args.block, "hop": hop, "localize": args.localize,
                                                   "link_radius": args.link_radius})
    print("{} tracks over {} blocks written to {}".format(len(doc["tracks"]), len(doc["starts"]), args.out))
    return doc


if __name__ == "__main__":
    main()
