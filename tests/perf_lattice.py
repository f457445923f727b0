"""The coarse TDoA lattice (``Prone_method="DENSE"``) on one MI355X: what it costs to build and what a search over it
costs.  A script, not a test.

lattice   ``dense_grid.coarse_lattice`` in numpy on a host-built node against ``SRPPhat.coarse_lattice`` of a
          device-built node (csrc/geometry_kernels.hip: kernels, the read-back of the four tables and the
          synchronise), width 8, alternating in one run, median of 5 after one warm-up each; on the bench region of
          interest (1 302 400 lookup points) with 7 and with 16 microphones.
search    one ``JointModel.forward`` in DENSE mode (device-built array, FULL spot network, f16x3, no separation
          network) on the configs[2] scene after one warm-up forward: stage times and candidate counts.

Appends one JSON line per record to profiles/lattice/perf_lattice.jsonl (``--out``).  Nothing is asserted about the
times: the records say which way the comparison came out.

    python tests/perf_lattice.py [--skip-search] [--out FILE]
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
from acousticswarms_speech_amd.dense_grid import coarse_lattice  # noqa: E402
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.mic_array import MicArray  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.search import INIT_WIDTH  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_spot_state_dict  # noqa: E402

REPS = 5


def lattice_records(emit):
    for n_mics in (7, 16):
        sc = make_scene(1010, 5, n_mics, 4000)
        with redirect_stdout(io.StringIO()):
            host = MicArray(sc.mic_positions, Spk_Range=sc.speaker_range, device="cuda").SRP_node
            dev = MicArray(sc.mic_positions, Spk_Range=sc.speaker_range, device="cuda", geometry="device",
                           Prone_method="DENSE").SRP_node
        times = {"host": [], "device": []}
        for rep in range(REPS + 1):                            # rep 0 warms both forms up
            for mode in ("host", "device"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lat = coarse_lattice(host, INIT_WIDTH) if mode == "host" else dev.coarse_lattice(INIT_WIDTH)
                torch.cuda.synchronize()
                if rep:
                    times[mode].append(time.perf_counter() - t0)
        h, d = float(np.median(times["host"])), float(np.median(times["device"]))
        emit({"record": "lattice", "mics": n_mics, "roi": list(sc.speaker_range), "width": INIT_WIDTH,
              "lookup_points": int(host._planes_1[0].size), "kept_points": int(lat.members.shape[0]),
              "cubes": lat.n_cubes, "largest_cube": int(np.diff(lat.bounds).max()), "reps": REPS,
              "host_s": round(h, 4), "device_s": round(d, 4), "host_over_device": round(h / d, 2),
              "host_s_all": [round(t, 4) for t in times["host"]], "device_s_all": [round(t, 4) for t in times["device"]],
              "device_build_split_ms": {k: round(1e3 * v, 3) for k, v in dev.build_times.items()}})


def search_record(emit):
    sc = make_scene(1010, 5, 7, 48000, reverb=True)            # the configs[2] scene
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=256, precision="f16x3").to("cuda")
    jm = JointModel(spot, None, device="cuda", geometry="device")
    mix = torch.from_numpy(sc.mix)
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, sc.speaker_range, prone_method="DENSE")
        jm.forward(mix)                                        # warm-up
        patches, _al, _a, _d0, _d1, spot_times = jm.forward(mix)
    mp = jm.Mic_processor
    emit({"record": "search", "scene": "configs[2]: make_scene(1010, 5, 7, 48000, reverb=True)", "prone_method": "DENSE",
          "spot_network": "FULL, f16x3, batch 256", "lattice_cubes": mp.SRP_node.lattice.n_cubes,
          "coarse_candidates": int(mp.big_spotforming_times), "coarse_kept": len(mp.trace["coarse_kept"]),
          "fine_candidates": int(mp.spotforming_times), "spot_evaluations": int(spot_times), "talkers": len(patches),
          "stage_s": {k: round(float(t), 4) for k, t in zip(("stage1", "coarse", "fine", "clustering", "separation"), jm.times)},
          "search_s": round(float(sum(jm.times[:4])), 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice", "perf_lattice.jsonl"))
    ap.add_argument("--skip-search", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    lattice_records(emit)
    if not args.skip_search:
        search_record(emit)


if __name__ == "__main__":
    main()
