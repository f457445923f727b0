"""Room recipe fixture (g17): run the REFERENCE's own ``get_random_mic_positions_desk``, ``get_random_speaker_positions``
and ``calculate_sample_offset`` (datasets/generate_dataset.py) under ``np.random.seed`` and record the positions they
return.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_room.py

The reference's module imports packages that are absent here and unused by these three functions (librosa,
pyroomacoustics, soundfile, tqdm): they are replaced by the inert stubs of ``make_golden.install_stubs`` so that the
``import`` lines succeed; no stub supplies arithmetic.  Before the three functions this script draws the room, ceiling
and absorption with ``np.random.uniform`` in the order and ranges of ``generate_sample`` (or, for the RT60 room, the
room and ceiling of ``generate_sample_rt60``, which draws no absorption and sets the short pick-up range): those four
lines are this script's own, the ranges are read from the reference's module.

Recorded per case (seed, talkers, rt60 room): room, absorption, microphones, desk, wall, talkers, offsets as
``calculate_sample_offset`` returns them, and the ROI.  Positions only, a few KB.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

CASES = [(seed, n, rt) for seed in (0, 1, 6) for n in (3, 5) for rt in (False,)] + [(3, 3, True), (4, 5, True)]
N_MICS = 7


def key(seed, n, rt):
    return f"s{seed}_n{n}_{'rt60' if rt else 'room'}"


def main():
    sys.path.insert(0, ROOT)
    from tests.golden import make_golden
    make_golden.install_stubs()
    for name in ("tqdm",):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    import importlib.util
    # by file: the reference's datasets/ is no package, and an installed package of that name would shadow it
    spec = importlib.util.spec_from_file_location("reference_generate_dataset",
                                                  os.path.join(make_golden.REF, "datasets", "generate_dataset.py"))
    gd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gd)

    args = argparse.Namespace(dimensions=3, sr=48000, n_mics=N_MICS)
    out = {}
    for seed, n, rt in CASES:
        np.random.seed(seed)
        if rt:
            gd.SPK_RANGE_W, gd.SPK_RANGE_H = 1.6, 2.4                       # what generate_sample_rt60 sets
            length, width = np.random.uniform(low=4, high=4.2), np.random.uniform(low=4, high=4.2)
            ceiling = np.random.uniform(low=1.6, high=1.7)
            absorption = np.nan
        else:
            gd.SPK_RANGE_W, gd.SPK_RANGE_H = 3, 4.5
            length = np.random.uniform(low=gd.ROOM_LENGTH_MIN, high=gd.ROOM_LENGTH_MAX)
            width = np.random.uniform(low=gd.ROOM_WIDTH_MIN, high=gd.ROOM_WIDTH_MAX)
            ceiling = np.random.uniform(low=gd.CEIL_MIN, high=gd.CEIL_MAX)
            absorption = np.random.uniform(low=gd.MIN_ABSORPTION, high=gd.MAX_ABSORPTION)
        mics, desk, wall = gd.get_random_mic_positions_desk(n_mics=N_MICS, left=0, right=length, bottom=0, top=width, args=args)
        voices, offsets, roi = gd.get_random_speaker_positions(n, mics, wall, left=0, right=length, up=width, down=0, args=args)
        k = key(seed, n, rt)
        out[k + "_room"] = np.array([length, width, ceiling], dtype=np.float64)
        out[k + "_absorption"] = np.float64(absorption)
        out[k + "_mics"] = np.asarray(mics, dtype=np.float64)
        out[k + "_desk"] = np.asarray(desk, dtype=np.float64)
        out[k + "_wall"] = np.int64(wall)
        out[k + "_voices"] = np.asarray(voices, dtype=np.float64)
        out[k + "_offsets"] = np.asarray(offsets, dtype=np.float64)
        out[k + "_roi"] = np.asarray(roi, dtype=np.float64)
    path = os.path.join(HERE, "g17_room_recipe.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB), walls {[int(out[key(*c) + '_wall']) for c in CASES]}")


if __name__ == "__main__":
    main()
