"""Voice recipe fixture (g19): run the REFERENCE's own ``get_voices`` and ``get_random_mic_positions_three_desks``
(datasets/generate_dataset.py) under ``np.random.seed`` and record what they choose.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_voices.py

The reference's module imports packages that are absent here (librosa, pyroomacoustics, soundfile, tqdm): they are
replaced by the inert stubs of ``make_golden.install_stubs``, as in ``make_golden_room.py``.  ``get_voices`` calls three
things outside numpy, and this script answers each from a table it builds itself -- data, not arithmetic:

* ``glob.glob(dir/*.wav)``: the sorted file names of that speaker directory;
* ``librosa.core.load(file)``: a ramp ``file_id * 1e7 + 1 + arange(n)`` of the file's length n at the scene rate, from
  which the returned clip tells which file it came from, where it begins and how many samples it kept before the zeros;
* ``librosa.effects.trim(voice)``: the file's (begin, end) and an alternating +-std array of that length, so that
  ``voice_trimmed.std()`` is the table's std.

So the fixture pins the sequence of draws, the retry on rejected files, the activity pad and the crop or zero-padding
of ``get_voices``; it pins nothing of librosa.  After every case one more ``np.random.uniform()`` is recorded: it tells
whether the same number of draws was made.  The table holds rejected files (silent ones and short ones) and clips that
come out shorter than, as long as and longer than the scene.

For the three desks this script draws the room, ceiling and absorption with ``np.random.uniform`` in the order and
ranges of ``generate_sample_size`` (its own four lines, the ranges read from the reference's module) and records what
``get_random_mic_positions_three_desks`` returns, over seeds of which at least one makes it draw again (its message
on the standard output is counted).  Arrays and names only, a few KB.
"""
import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SR = 48000
N_MICS = 7
# per speaker directory: (n, begin, end, std) of its files u0.wav, u1.wav, ... at SR
TABLE = {
    "corpus/p225": [(200000, 9000, 150000, 0.05), (30000, 2000, 29000, 0.04), (60000, 100, 300, 0.05)],
    "corpus/p226": [(48000, 100, 47000, 0.03), (90000, 0, 90000, 1e-5)],
    "corpus/p227": [(40000, 12000, 33000, 0.02), (150000, 30000, 120000, 0.06), (100000, 0, 24000, 0.05),
                    (70000, 5000, 64000, 0.01)],
    "corpus/p228": [(96000, 20000, 70000, 0.08)],
    "corpus/p229": [(52000, 9700, 48200, 1e-6), (52000, 9700, 48200, 0.02), (300000, 0, 300000, 0.1)],
    "corpus/p230": [(57600, 9600, 38400, 0.03), (20000, 0, 20000, 0.03), (120000, 60000, 119000, 0.04)],
}
VOICE_CASES = [(seed, n, duration) for seed in (0, 1, 2, 3, 4, 5) for n, duration in ((3, 1.0), (5, 0.6), (6, 3.0))]
DESK_SEEDS_PLAIN = (0, 1, 2)


def main():
    sys.path.insert(0, ROOT)
    from tests.golden import make_golden
    make_golden.install_stubs()
    if "tqdm" not in sys.modules:
        try:
            __import__("tqdm")
        except ImportError:
            sys.modules["tqdm"] = types.ModuleType("tqdm")
    dirs = sorted(TABLE)
    files, entry = [], []
    for d in dirs:
        for k, e in enumerate(TABLE[d]):
            files.append(f"{d}/u{k}.wav")
            entry.append(e)
    fid = {f: i for i, f in enumerate(files)}

    def load(path, sr=None, mono=True):
        assert sr == SR and mono
        i = fid[path]
        return i * 1e7 + 1 + np.arange(entry[i][0], dtype=np.float64), sr

    def trim(voice, top_db=None):
        assert top_db == 18
        _n, begin, end, std = entry[int(voice[0] // 1e7)]
        return std * (1.0 - 2.0 * (np.arange(end - begin) % 2)), (begin, end)

    lib = sys.modules["librosa"]
    lib.core = types.SimpleNamespace(load=load)
    lib.effects.trim = trim

    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_generate_dataset",
                                                  os.path.join(make_golden.REF, "datasets", "generate_dataset.py"))
    gd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gd)
    gd.glob = types.SimpleNamespace(glob=lambda pattern: [f for f in files if os.path.dirname(f) == os.path.dirname(pattern)])

    out = {"dirs": np.array(dirs), "files": np.array(files), "entries": np.array(entry, dtype=np.float64), "sr": np.int64(SR),
           "voice_cases": np.array(VOICE_CASES, dtype=np.float64)}
    seen = set()
    for c, (seed, n, duration) in enumerate(VOICE_CASES):
        args = argparse.Namespace(sr=SR, duration=duration)
        T = int(round(duration * SR))
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()) as log:
            got = gd.get_voices(dirs, n, args)
        after = np.random.uniform()
        picks = []
        for voice, _identity in got:
            assert voice.shape == (T,)
            i = int(voice[0] // 1e7)
            kept = int(np.count_nonzero(voice))
            picks.append((i, int(voice[0] - i * 1e7) - 1, kept))
            L = min(entry[i][2] + 9600, entry[i][0]) - max(entry[i][1] - 9600, 0)
            seen.add("short" if L < T else "equal" if L == T else "long")
        if log.getvalue():
            seen.add("retry")
        out[f"v{c}_picks"] = np.array(picks, dtype=np.int64)
        out[f"v{c}_ids"] = np.array([identity for _v, identity in got])
        out[f"v{c}_after"] = np.float64(after)
    assert seen == {"short", "equal", "long", "retry"}, seen

    args = argparse.Namespace(dimensions=3, sr=SR, n_mics=N_MICS)

    def desks(seed):
        np.random.seed(seed)
        length = np.random.uniform(low=gd.ROOM_LENGTH_MIN, high=gd.ROOM_LENGTH_MAX)
        width = np.random.uniform(low=gd.ROOM_WIDTH_MIN, high=gd.ROOM_WIDTH_MAX)
        ceiling = np.random.uniform(low=gd.CEIL_MIN, high=gd.CEIL_MAX)
        absorption = np.random.uniform(low=0.1, high=0.99)
        with contextlib.redirect_stdout(io.StringIO()) as log:
            large, middle, small, sizes, wall = gd.get_random_mic_positions_three_desks(n_mics=N_MICS, left=0, right=length, bottom=0,
                                                                                       top=width, args=args)
        return (np.array([length, width, ceiling]), absorption, np.stack([large, middle, small]), np.array(sizes), int(wall),
                log.getvalue().count("Re-generating"), np.random.uniform())

    again = next(s for s in range(3, 1000) if desks(s)[5] > 0)
    seeds = list(DESK_SEEDS_PLAIN) + [again]
    out["desk_seeds"] = np.array(seeds, dtype=np.int64)
    for s in seeds:
        room, absorption, mics, sizes, wall, redraws, after = desks(s)
        out[f"d{s}_room"], out[f"d{s}_absorption"], out[f"d{s}_mics"] = room, np.float64(absorption), mics
        out[f"d{s}_sizes"], out[f"d{s}_wall"], out[f"d{s}_redraws"], out[f"d{s}_after"] = sizes, np.int64(wall), np.int64(redraws), np.float64(after)
    path = os.path.join(HERE, "g19_voice_recipe.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB), desk seeds {seeds}, redraws {[int(out[f'd{s}_redraws']) for s in seeds]}")


if __name__ == "__main__":
    main()
