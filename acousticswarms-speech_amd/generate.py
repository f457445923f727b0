"""The dataset generator, the counterpart of the reference's ``python datasets/generate_dataset.py``:

    python -m acousticswarms_speech_amd.generate OUT --n_outputs N [--voices DIR] [--n_voices_min 3] [--n_voices_max 5]
        [--max_order 15 | --sample_rt60 | --generate_rt60] [--duration 3.0] [--n_mics 7] [--sr 48000] [--seed 0]
        [--backend device|host] [--batch 16]

Writes the sample directories ``OUT/NNNNN/`` that ``evalkit.get_items`` and ``python -m acousticswarms_speech_amd.evaluate``
read -- with ``--generate_rt60`` the sweep ``OUT/rt_60_i/NNNNN/`` of one geometry under four reverberation times -- and
``OUT/args.json``.  Scenes follow ``room_scenes`` (the reference's recipe over one ``numpy.random.RandomState(seed)``) and
are simulated ``--batch`` at a time, on the device by default.  Voices are ``scenes._speech_like`` unless ``--voices``
names a directory of wav files at ``--sr`` (no resampling, no trimming).  Nothing runs at import."""
import argparse
import json
import os


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acousticswarms_speech_amd.generate",
                                description="Generate a reverberant dataset of sample directories.")
    p.add_argument("output_path", type=str, help="Output directory to write the synthetic dataset")
    p.add_argument("--n_outputs", type=int, required=True, help="Number of samples")
    p.add_argument("--voices", type=str, default=None, help="Directory with voice wav files at --sr (default: synthetic voices)")
    p.add_argument("--n_mics", type=int, default=7)
    p.add_argument("--n_voices_min", type=int, default=3)
    p.add_argument("--n_voices_max", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--sr", type=int, default=48000)
    p.add_argument("--start_index", type=int, default=0)
    p.add_argument("--duration", type=float, default=3.0)
    p.add_argument("--max_order", type=int, default=15, help="Order of reflections to consider during simulation")
    mode = p.add_mutually_exclusive_group()
    mode.add_argument("--sample_rt60", action="store_true", help="Draw a reverberation time per sample instead of a fixed order")
    mode.add_argument("--generate_rt60", action="store_true", help="Write every scenario under four reverberation times")
    p.add_argument("--backend", choices=("device", "host"), default="device", help="Where the rooms are simulated")
    p.add_argument("--batch", type=int, default=16, help="Scenes per simulation call")
    return p


def main(argv=None):
    import numpy as np

    from . import room_scenes as rs
    args = build_parser().parse_args(argv)
    if not 1 <= args.n_voices_min <= args.n_voices_max:
        raise SystemExit("--n_voices_min and --n_voices_max must satisfy 1 <= min <= max")
    if args.batch < 1 or args.n_outputs < 0:
        raise SystemExit("--batch must be at least 1 and --n_outputs at least 0")
    rng = np.random.RandomState(args.seed)
    T = int(round(args.duration * args.sr))
    voices = rs.list_voices(args.voices) if args.voices else None
    os.makedirs(args.output_path, exist_ok=True)

    pending = []                                            # (spec, directory)

    def flush():
        if pending:
            scenes = rs.simulate_rooms([sp for sp, _d in pending], backend=args.backend)
            for scene, (sp, d) in zip(scenes, pending):
                rs.write_room_scene_dir(scene, sp, d)
            pending.clear()

    for i in range(args.start_index, args.start_index + args.n_outputs):
        n_voices = rng.randint(args.n_voices_min, args.n_voices_max + 1)
        name = f"{i:05d}"
        if args.generate_rt60:
            # one geometry and one set of voices under a reverberation time from each band (generate_sample_rt60)
            base = rs.make_room_spec(rng, n_voices, args.n_mics, T, fs=args.sr, voices=voices, rt60_room=True)
            for b, band in enumerate(rs.RT60_BANDS):
                pending.append((rs.with_rt60(base, rng.uniform(*band)), os.path.join(args.output_path, f"rt_60_{b}", name)))
        else:
            spec = rs.make_room_spec(rng, n_voices, args.n_mics, T, args.max_order, None, args.sr, voices)
            if args.sample_rt60:
                spec = rs.with_rt60(spec, rng.uniform(*rs.RT60_SAMPLED))
            pending.append((spec, os.path.join(args.output_path, name)))
        if len(pending) >= args.batch:
            flush()
    flush()
    with open(os.path.join(args.output_path, "args.json"), "w") as f:
        json.dump(vars(args), f, indent=4)
    return 0


if __name__ == "__main__":
    main()
