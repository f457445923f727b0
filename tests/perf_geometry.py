"""Geometry build on the device against the host build, on one MI355X.  A script, not a test.

setup     JointModel.setup() wall time (build + what setup() does around it, ending in a device synchronise),
          geometry="host" (the numpy build) and geometry="device" (csrc/geometry_kernels.hip), median of 5 after one
          warm-up build each, alternating, on the bench geometry (make_scene(1010, 5, 7, ...), its own speaker range)
          and on the full region of interest; plus the split of the device build (kernels, device-to-host copies,
          host remainder: SRPPhat.build_times).
batch     mixtures/s of shard.localize_batch for 64 five-speaker mixtures (seeds 2000-2063, T = 48 000), each recorded
          with its own array: geometries= with geometry="device", the same with geometry="host", and today's
          shared-array run (all 64 generated on the first array, one setup()).

Appends one JSON line per record to profiles/geometry/perf_setup.jsonl (``--out``) and exits non-zero if the device
form does not beat the host form on a setup time or on the batch rate.

    python tests/perf_geometry.py [--mixtures 64] [--out FILE]
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
from acousticswarms_speech_amd.shard import localize_batch  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_spot_state_dict  # noqa: E402

FULL_ROI = [-2.2, 2.25, 0.0, 6.2, 0.0, 0.9]
REPS = 5


def timed_setup(jm, mics, roi, mode):
    jm.previous_config = None                                  # setup() would reuse an unchanged configuration
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with redirect_stdout(io.StringIO()):
        jm.setup(mics, roi, geometry=mode)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def setup_records(emit):
    sc = make_scene(1010, 5, 7, 4000, reverb=True)
    jm = JointModel(None, None, device="cuda")
    ok = True
    for name, roi in (("bench geometry", list(sc.speaker_range)), ("full ROI", FULL_ROI)):
        times = {"host": [], "device": []}
        split = []
        for rep in range(REPS + 1):                            # rep 0 warms both paths up (code objects, pinned buffers)
            for mode in ("host", "device"):
                dt = timed_setup(jm, sc.mic_positions, roi, mode)
                if rep:
                    times[mode].append(dt)
                    if mode == "device":
                        split.append(dict(jm.Mic_processor.SRP_node.build_times))
        G = int(jm.Mic_processor.SRP_node.grids.shape[0])
        host, dev = float(np.median(times["host"])), float(np.median(times["device"]))
        emit({"record": "setup", "geometry": name, "roi": roi, "G": G, "reps": REPS,
              "setup_host_s": round(host, 4), "setup_device_s": round(dev, 4), "host_over_device": round(host / dev, 2),
              "setup_host_s_all": [round(t, 4) for t in times["host"]], "setup_device_s_all": [round(t, 4) for t in times["device"]],
              "device_build_split_ms": {k: round(1e3 * float(np.median([s[k] for s in split])), 3) for k in split[0]},
              "label_sweeps": int(jm.Mic_processor.SRP_node.label_sweeps)})
        ok = ok and dev < host
    return ok


def batch_records(emit, n):
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=256, precision="f16x3").to("cuda")
    own = [make_scene(2000 + k, 5, 7, 48000) for k in range(n)]
    shared = [own[0]] + [make_scene(2000 + k, 5, 7, 48000, mic_positions=own[0].mic_positions) for k in range(1, n)]
    geometries = [(s.mic_positions, s.speaker_range) for s in own]
    assert len({s.mic_positions.tobytes() for s in own}) == n
    rate, talkers = {}, {}
    for form in ("shared array", "device", "host"):
        scenes = shared if form == "shared array" else own
        mixes = [torch.from_numpy(s.mix) for s in scenes]
        jm = JointModel(spot, None, device="cuda", geometry="host" if form == "shared array" else form)
        with redirect_stdout(io.StringIO()):
            if form == "shared array":
                jm.setup(own[0].mic_positions, own[0].speaker_range)
                jm.forward(mixes[0])                           # warm-up
                geo = None
            else:
                localize_batch(jm, mixes[:2], geometries=geometries[:2])      # warm-up (code objects, pinned buffers)
                jm._geometry_cache.clear()                                    # the timed run starts with an empty LRU
                geo = geometries
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = localize_batch(jm, mixes, geometries=geo)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        rate[form] = n / dt
        talkers[form] = [len(r["names"]) for r in out]
        stats = dict(jm.geometry_stats)
        emit({"record": "batch", "form": form, "mixtures": n, "T": 48000, "concurrent": 2, "seconds": round(dt, 3),
              "mixtures_per_s": round(rate[form], 3), "talkers_found_mean": round(float(np.mean(talkers[form])), 2),
              "geometry_builds_incl_warmup": stats["builds"]})
    assert talkers["device"] == talkers["host"], "device-built and host-built arrays found different talkers"
    emit({"record": "batch ratios", "mixtures": n, "device_over_host": round(rate["device"] / rate["host"], 3),
          "device_over_shared_array": round(rate["device"] / rate["shared array"], 3),
          "host_over_shared_array": round(rate["host"] / rate["shared array"], 3)})
    return rate["device"] > rate["host"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixtures", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry", "perf_setup.jsonl"))
    ap.add_argument("--skip-batch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ok = setup_records(emit)
    if not args.skip_batch:
        ok = batch_records(emit, args.mixtures) and ok
    if not ok:
        sys.exit("the device-built geometry did not beat the host build on every figure")


if __name__ == "__main__":
    main()
