"""Pruning-map stage times on one MI355X: SRP-PHAT / MUSIC / TOPS maps on the full ROI
(make_scene(1010, 5, 7, T): G = 11 995 clusters), 7 mics, T = 48 000 and 144 000.  Device time from HIP events
around the map call, wall time around call + synchronise; median of 5 after one warm-up call.
TOPS needs T >= 72 000, so it has no T = 48 000 row.  Prints one JSON line per (method, T).

    python tests/perf_pruners.py
"""
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acousticswarms_speech_amd.mic_array import MicArray  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402

FULL_ROI = [-2.2, 2.25, 0.0, 6.2, 0.0, 0.9]
REPS = 5


def main():
    for T in (48000, 144000):
        sc = make_scene(1010, 5, 7, T)
        with redirect_stdout(io.StringIO()):
            node = MicArray(sc.mic_positions, Spk_Range=FULL_ROI, device="cuda").SRP_node
        win = 36000 if T >= 72000 else 24000
        for name, fn in (("SRP", node.SRP_Map_WINDOW_new), ("MUSIC", node.MUSIC_Map_WINDOW),
                         ("TOPS", node.TOPS_Map_WINDOW)):
            if name == "TOPS" and T < 72000:
                continue
            fn(sc.mix, window=win)
            torch.cuda.synchronize()
            dev, wall = [], []
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                fn(sc.mix, window=win)
                b.record()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(a.elapsed_time(b))
            print(json.dumps({"method": name, "T": T, "G": int(node.grids.shape[0]), "window": win,
                              "device_ms": round(float(np.median(dev)), 3), "wall_ms": round(float(np.median(wall)), 3),
                              "device_ms_all": [round(x, 3) for x in dev]}), flush=True)


if __name__ == "__main__":
    main()
