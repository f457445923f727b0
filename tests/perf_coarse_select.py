"""The coarse stage of a lattice search decided on the host against ``coarse="device"`` on one MI355X.  A script, not a
test.

search  per ``JointModel.forward`` in DENSE and in DENSE_NMS mode on the configs[2] scene (make_scene(1010, 5, 7, 48000,
        reverb=True); device-built array, FULL spot network, f16x3, random weights, no separation network):
        ``times[0] + times[1]`` -- stage 1, which builds the patch list in host mode, plus the coarse stage -- and the
        whole forward's wall time, with how many patches stage 1 and the coarse stage built.
``coarse="host"`` in the same run is the yardstick: the two modes alternate within one run and every figure is the
median of ``--reps`` (5) after one warm-up each.  Appends one JSON line per record to
profiles/lattice/perf_coarse.jsonl (``--out``).  Nothing is asserted about the times.

    python tests/perf_coarse_select.py [--reps N] [--out FILE]
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
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_spot_state_dict  # noqa: E402

MODES = ("host", "device")


def med(v):
    return round(float(np.median(v)), 6)


def search_records(emit, spot, reps):
    sc = make_scene(1010, 5, 7, 48000, reverb=True)            # the configs[2] scene
    mix = torch.from_numpy(sc.mix)
    for method in ("DENSE", "DENSE_NMS"):
        jms = {}
        for m in MODES:
            jms[m] = JointModel(spot, None, device="cuda", geometry="device", coarse=m)
            with redirect_stdout(io.StringIO()):
                jms[m].setup(sc.mic_positions, sc.speaker_range, prone_method=method)
        times = {m: [] for m in MODES}
        wall = {m: [] for m in MODES}
        talkers, kept, built = {}, {}, {}
        with redirect_stdout(io.StringIO()):
            for m in MODES:
                jms[m].forward(mix)                             # warm-up
            for _ in range(reps):
                for m in MODES:
                    mp = jms[m].Mic_processor
                    stage1 = mp.Apply_SRP_PHAT
                    lists = []
                    mp.Apply_SRP_PHAT = lambda x, stage1=stage1, lists=lists: (lists.append(stage1(x)), lists[-1])[1]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    patches = jms[m].forward(mix)[0]
                    torch.cuda.synchronize()
                    wall[m].append(time.perf_counter() - t0)
                    del mp.Apply_SRP_PHAT
                    times[m].append(list(jms[m].times[:4]))
                    talkers[m] = [p[3] for p in patches]
                    kept[m] = list(mp.trace["coarse_kept"])
                    built[m] = getattr(lists[0][0], "built", len(lists[0][0]))
        mp = jms["host"].Mic_processor
        rec = {"record": "search", "scene": "configs[2]: make_scene(1010, 5, 7, 48000, reverb=True)", "prone_method": method,
               "spot_network": "FULL, f16x3, batch 256, random weights", "reps": reps,
               "lattice_cubes": mp.SRP_node.lattice.n_cubes, "coarse_kept": len(kept["host"]),
               "same_coarse_kept": kept["host"] == kept["device"], "same_talkers": talkers["host"] == talkers["device"],
               "talkers": len(talkers["host"])}
        for m in MODES:
            t = np.array(times[m])
            rec[m] = {"stage1_plus_coarse_s": med(t[:, 0] + t[:, 1]), "stage1_s": med(t[:, 0]), "coarse_s": med(t[:, 1]),
                      "search_s": med(t.sum(axis=1)), "forward_s": med(wall[m]), "patches_built": int(built[m]),
                      "stage1_plus_coarse_s_all": [round(float(v), 5) for v in t[:, 0] + t[:, 1]],
                      "forward_s_all": [round(float(v), 5) for v in wall[m]]}
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice", "perf_coarse.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
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


if __name__ == "__main__":
    main()
