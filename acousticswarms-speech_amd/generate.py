"""The dataset generator, the counterpart of the reference's ``python datasets/generate_dataset.py``:

    python -m acousticswarms_speech_amd.generate OUT --n_outputs N [--voices DIR] [--n_voices_min 3] [--n_voices_max 5]
        [--max_order 15 | --sample_rt60 | --generate_rt60] [--duration 3.0] [--n_mics 7] [--sr 48000] [--seed 0]
        [--backend device|host] [--batch 16] [--voice_prep none|reference] [--voice_index PATH]
        [--generate_dereverb] [--generate_colocated | --generate_size]

Writes the sample directories ``OUT/NNNNN/`` that ``evalkit.get_items`` and ``python -m acousticswarms_speech_amd.evaluate``
read -- with ``--generate_rt60`` the sweep ``OUT/rt_60_i/NNNNN/`` of one geometry under four reverberation times -- and
``OUT/args.json``.  Scenes follow ``room_scenes`` (the reference's recipe over one ``numpy.random.RandomState(seed)``) and
are simulated ``--batch`` at a time, on the device by default.  Voices are ``scenes._speech_like`` unless ``--voices``
names a directory of wav files: at ``--sr`` and taken as they are by default, or with ``--voice_prep reference`` a corpus
of speaker directories at any rate, prepared as the reference's ``get_voices`` does (``voiceprep``: resampled, trimmed,
checked for activity; the audio of a whole batch comes from one resample call per source rate).
``--generate_dereverb`` adds the order-0 ground truth ``mic00_voiceNN_dereverb.wav`` to every sample,
``--generate_colocated`` writes every scene a second time on a 10 cm circular array to ``OUT_colocated/``, and
``--generate_size`` writes every scenario on three desks of falling size to ``OUT/large|middle|small/NNNNN``.  Nothing
runs at import."""
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
    p.add_argument("--voice_prep", choices=("none", "reference"), default="none",
                   help="reference: resample, trim and select the voice files as the reference's get_voices does")
    p.add_argument("--voice_index", type=str, default=None, help="JSON file that keeps the per-file index of --voice_prep reference")
    p.add_argument("--generate_dereverb", action="store_true", help="Also write the dereverberated (order 0) ground truth")
    p.add_argument("--generate_colocated", action="store_true", help="Also write every scenario on a colocated circular array")
    p.add_argument("--generate_size", action="store_true", help="Write every scenario on three desks of different sizes")
    return p


def main(argv=None):
    import numpy as np

    from . import room_scenes as rs
    from .voiceprep import VoiceIndex, colocated_array
    args = build_parser().parse_args(argv)
    if not 1 <= args.n_voices_min <= args.n_voices_max:
        raise SystemExit("--n_voices_min and --n_voices_max must satisfy 1 <= min <= max")
    if args.batch < 1 or args.n_outputs < 0:
        raise SystemExit("--batch must be at least 1 and --n_outputs at least 0")
    # what the reference's main cannot reach: its rt60 sweep and its size sweep each ignore the other modes
    if args.generate_size and (args.generate_rt60 or args.sample_rt60 or args.generate_colocated):
        raise SystemExit("--generate_size goes with neither --generate_rt60, --sample_rt60 nor --generate_colocated")
    if args.generate_colocated and args.generate_rt60:
        raise SystemExit("--generate_colocated does not go with --generate_rt60")
    if args.voice_prep == "reference" and not args.voices:
        raise SystemExit("--voice_prep reference prepares voice files: it needs --voices")
    if args.voice_index and args.voice_prep != "reference":
        raise SystemExit("--voice_index belongs to --voice_prep reference")
    rng = np.random.RandomState(args.seed)
    T = int(round(args.duration * args.sr))
    voices = rs.list_voices(args.voices) if args.voices else None
    index = VoiceIndex(args.sr, args.backend, path=args.voice_index) if args.voice_prep == "reference" else None
    os.makedirs(args.output_path, exist_ok=True)

    pending = []                                            # (spec, directory)

    def flush():
        if pending:
            specs = [sp for sp, _d in pending]
            rs.fetch_voices(specs, backend=args.backend)
            if args.generate_dereverb:                      # the same scenes at order 0, in the same calls
                specs = specs + [rs.with_order(sp, 0) for sp in specs]
            # prepared voices are held to equal bytes on both backends: the samples no sound reaches are written as zeros,
            # not as the transforms' rounding noise; the default path keeps the bytes it always wrote
            scenes = rs.simulate_rooms(specs, backend=args.backend, exact_silence=args.voice_prep == "reference")
            for k, (sp, d) in enumerate(pending):
                rs.write_room_scene_dir(scenes[k], sp, d)
                if args.generate_dereverb:
                    rs.write_dereverb(scenes[len(pending) + k], d)
            pending.clear()

    for i in range(args.start_index, args.start_index + args.n_outputs):
        n_voices = rng.randint(args.n_voices_min, args.n_voices_max + 1)
        name = f"{i:05d}"
        if args.generate_rt60:
            # one geometry and one set of voices under a reverberation time from each band (generate_sample_rt60)
            base = rs.make_room_spec(rng, n_voices, args.n_mics, T, fs=args.sr, voices=voices, rt60_room=True,
                                     prep=args.voice_prep, index=index)
            for b, band in enumerate(rs.RT60_BANDS):
                pending.append((rs.with_rt60(base, rng.uniform(*band)), os.path.join(args.output_path, f"rt_60_{b}", name)))
        elif args.generate_size:
            # one room, one set of talkers and voices on three desks in one place (generate_sample_size)
            base = rs.make_room_spec(rng, n_voices, args.n_mics, T, args.max_order, None, args.sr, voices, prep=args.voice_prep,
                                     index=index, geometry=rs.draw_geometry_three_desks)
            for size, mics, desk in zip(("large", "middle", "small"), base.meta["desks_mics"], base.meta["desks"]):
                pending.append((rs.with_mics(base, mics, desk), os.path.join(args.output_path, size, name)))
        else:
            spec = rs.make_room_spec(rng, n_voices, args.n_mics, T, args.max_order, None, args.sr, voices, prep=args.voice_prep,
                                     index=index)
            if args.sample_rt60:
                spec = rs.with_rt60(spec, rng.uniform(*rs.RT60_SAMPLED))
            pending.append((spec, os.path.join(args.output_path, name)))
            if args.generate_colocated:
                mics = colocated_array(rng, np.mean(spec.mics, axis=0), args.n_mics)
                pending.append((rs.with_mics(spec, mics), os.path.join(args.output_path.rstrip("/") + "_colocated", name)))
        if len(pending) >= args.batch:
            flush()
    flush()
    if index is not None:
        index.save()
    with open(os.path.join(args.output_path, "args.json"), "w") as f:
        json.dump(vars(args), f, indent=4)
    return 0


if __name__ == "__main__":
    main()
