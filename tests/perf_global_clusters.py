"""The global clustering's decisions on the host against ``global_clustering="device"`` on one MI355X.  A script, not a
test.

search  per ``JointModel.forward`` on the bench scene (make_scene(1010, 5, 7, 48000, reverb=True); FULL spot network,
        f16x3, random weights): ``times[3]``, the global clustering stage, and the whole forward's wall time, with how
        many cluster heads the fine stage hands over.
batch   ``shard.localize_batch`` on 16 five-speaker mixtures (seeds 2000-2015, one array) with ``concurrent`` = 2 and 4,
        per mode.
Both modes run with ``segments="device"``; ``global_clustering="host"`` in the same run is the yardstick.  Everything
alternates between the two modes within one run and is the median of ``--reps`` (5) after one warm-up.  Appends one
JSON line per record to profiles/clusters/perf_global_clusters.jsonl (``--out``).  Nothing is asserted about the times.

    python tests/perf_global_clusters.py [--reps N] [--skip-batch] [--out FILE]
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
        jm = JointModel(spot, None, device="cuda", segments="device", global_clustering=mode)
        with redirect_stdout(io.StringIO()):
            jm.setup(sc.mic_positions, sc.speaker_range)
        out[mode] = jm
    return out


def search_records(emit, spot, reps):
    sc = make_scene(1010, 5, 7, 48000, reverb=True)
    mix = torch.from_numpy(sc.mix)
    jms = models(spot, sc)
    heads = [0]
    stage = MicArray.Clustering_new

    def counted(self, output_pair, *a, **kw):
        heads[0] = len(output_pair)
        return stage(self, output_pair, *a, **kw)
    MicArray.Clustering_new = counted
    times = {m: [] for m in MODES}
    wall = {m: [] for m in MODES}
    talkers, traces = {}, {}
    try:
        with redirect_stdout(io.StringIO()):
            for m in MODES:
                jms[m].forward(mix)                                     # warm-up
            for _ in range(reps):
                for m in MODES:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    patches = jms[m].forward(mix)[0]
                    torch.cuda.synchronize()
                    wall[m].append(time.perf_counter() - t0)
                    talkers[m] = [p[3] for p in patches]
                    traces[m] = [list(c) for c in jms[m].Mic_processor.trace["final_clusters"]]
                    times[m].append(list(jms[m].times[:4]))
    finally:
        MicArray.Clustering_new = stage
    rec = {"record": "search", "scene": "make_scene(1010, 5, 7, 48000, reverb=True)", "reps": reps,
           "cluster_heads": heads[0], "talkers": len(talkers["host"]), "same_talkers": talkers["host"] == talkers["device"],
           "same_final_clusters": traces["host"] == traces["device"]}
    for m in MODES:
        t = np.array(times[m])
        rec[m] = {"clustering_s": med(t[:, 3]), "search_s": med(t.sum(axis=1)), "forward_s": med(wall[m]),
                  "clustering_s_all": [round(float(v), 5) for v in t[:, 3]]}
    emit(rec)


def batch_records(emit, spot, reps, n_mix=16):
    sc0 = make_scene(2000, 5, 7, 48000)
    mixes = [torch.from_numpy(make_scene(2000 + i, 5, 7, 48000, mic_positions=sc0.mic_positions).mix) for i in range(n_mix)]
    jms = models(spot, sc0)
    with redirect_stdout(io.StringIO()):
        for m in MODES:
            localize_batch(jms[m], mixes[:4], concurrent=2)         # warm-up
    for concurrent in (2, 4):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clusters", "perf_global_clusters.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-batch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, gpu=torch.cuda.get_device_name(0))     # ("device" is a mode's key in the records)
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
