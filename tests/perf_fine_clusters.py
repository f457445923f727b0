"""The fine stage's clustering on the host against ``clustering="device"`` on one MI355X.  A script, not a test.

clustering  per ``JointModel.forward`` on the bench scene (make_scene(1010, 5, 7, 48000, reverb=True); FULL spot
            network, f16x3, random weights): the wall time the searching thread spends inside the per-coarse-patch
            ``MicArray._resident_group`` calls (host mode) or the per-chunk ``MicArray._device_groups`` calls (device
            mode), waits for the device included, and how many such calls a search makes.
search      the same forwards: the fine and the clustering stage and the whole search.  In a single forward all but the
            last chunk's clustering hides behind the GPU, so the fine stage shows it only in part.
batch       ``shard.localize_batch`` on 16 five-speaker mixtures (seeds 2000-2015, one array) with ``concurrent`` = 2, 3
            and 4, per mode.
Everything alternates between the two modes within one run and is the median of ``--reps`` (5) after one warm-up;
``clustering="host"`` in the same run is the yardstick.  Appends one JSON line per record to
profiles/clusters/perf_clusters.jsonl (``--out``).  Nothing is asserted about the times.

    python tests/perf_fine_clusters.py [--reps N] [--skip-batch] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd.config import FULL  # noqa: E402
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.mic_array import MicArray  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.shard import localize_batch  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_spot_state_dict  # noqa: E402

MODES = ("host", "device")


def med(v):
    return round(float(np.median(v)), 6)


def models(spot, sc):
    out = {}
    for mode in MODES:
        jm = JointModel(spot, None, device="cuda", clustering=mode)
        with redirect_stdout(io.StringIO()):
            jm.setup(sc.mic_positions, sc.speaker_range)
        out[mode] = jm
    return out


def timed(cls, name, acc):
    """Wrap ``cls.name`` so that ``acc`` = [seconds, calls] grows with every call; returns the undo."""
    inner = getattr(cls, name)

    def wrapper(self, *a, **kw):
        t0 = time.perf_counter()
        try:
            return inner(self, *a, **kw)
        finally:
            acc[0] += time.perf_counter() - t0
            acc[1] += 1
    setattr(cls, name, wrapper)
    return lambda: setattr(cls, name, inner)


def search_records(emit, spot, reps):
    sc = make_scene(1010, 5, 7, 48000, reverb=True)
    mix = torch.from_numpy(sc.mix)
    jms = models(spot, sc)
    acc = {"host": [0.0, 0], "device": [0.0, 0]}
    undo = [timed(MicArray, "_resident_group", acc["host"]), timed(MicArray, "_device_groups", acc["device"])]
    times = {m: [] for m in MODES}
    clus = {m: [] for m in MODES}
    calls, talkers, traces = {}, {}, {}
    try:
        with redirect_stdout(io.StringIO()):
            for m in MODES:
                jms[m].forward(mix)                                     # warm-up
            for _ in range(reps):
                for m in MODES:
                    acc[m][0], acc[m][1] = 0.0, 0
                    patches = jms[m].forward(mix)[0]
                    torch.cuda.synchronize()
                    talkers[m] = [p[3] for p in patches]
                    traces[m] = dict(jms[m].Mic_processor.trace["fine_clusters"])
                    times[m].append(list(jms[m].times[:4]))
                    clus[m].append(acc[m][0])
                    calls[m] = acc[m][1]
    finally:
        for u in undo:
            u()
    scene = "make_scene(1010, 5, 7, 48000, reverb=True)"
    emit({"record": "clustering", "scene": scene, "reps": reps,
          "candidates": int(jms["host"].Mic_processor.spotforming_times),
          "open_coarse_patches": len(traces["host"]), "cluster_heads": sum(len(c) for c in traces["host"].values()),
          "same_fine_clusters": traces["host"] == traces["device"],
          "host": {"clustering_calls": calls["host"], "in_clustering_s": med(clus["host"]),
                   "in_clustering_s_all": [round(t, 5) for t in clus["host"]]},
          "device": {"clustering_calls": calls["device"], "in_clustering_s": med(clus["device"]),
                     "in_clustering_s_all": [round(t, 5) for t in clus["device"]]}})
    rec = {"record": "search", "scene": scene, "reps": reps, "same_talkers": talkers["host"] == talkers["device"],
           "talkers": len(talkers["host"])}
    for m in MODES:
        t = np.array(times[m])
        rec[m] = {"fine_s": med(t[:, 2]), "clustering_s": med(t[:, 3]), "search_s": med(t.sum(axis=1)),
                  "fine_s_all": [round(float(v), 5) for v in t[:, 2]]}
    emit(rec)


def batch_records(emit, spot, reps, n_mix=16):
    sc0 = make_scene(2000, 5, 7, 48000)
    mixes = [torch.from_numpy(make_scene(2000 + i, 5, 7, 48000, mic_positions=sc0.mic_positions).mix) for i in range(n_mix)]
    jms = models(spot, sc0)
    with redirect_stdout(io.StringIO()):
        for m in MODES:
            localize_batch(jms[m], mixes[:4], concurrent=2)         # warm-up
    for concurrent in (2, 3, 4):
        times = {m: [] for m in MODES}
        names = {}
        for _ in range(reps):
            for m in MODES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with redirect_stdout(io.StringIO()):
                    out = localize_batch(jms[m], mixes, concurrent=concurrent)
                torch.cuda.synchronize()
                times[m].append(time.perf_counter() - t0)
                names[m] = [list(r["names"]) for r in out]
        emit({"record": "batch", "mixtures": n_mix, "T": 48000, "concurrent": concurrent, "reps": reps,
              "mixtures_with_the_same_talkers": sum(a == b for a, b in zip(names["host"], names["device"])),
              "host_mixtures_per_s": round(n_mix / med(times["host"]), 3),
              "device_mixtures_per_s": round(n_mix / med(times["device"]), 3),
              "host_s_all": [round(t, 3) for t in times["host"]], "device_s_all": [round(t, 3) for t in times["device"]]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clusters", "perf_clusters.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-batch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, gpu=torch.cuda.get_device_name(0))      # ("device" is a mode's record)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=256, precision="f16x3").to("cuda")
    search_records(emit, spot, args.reps)
    if not args.skip_batch:
        batch_records(emit, spot, args.reps)


if __name__ == "__main__":
    main()
