"""``evalkit.evaluate_dataset`` end to end on one MI355X: the per-sample loop with host metrics (the behaviour before
``batch=`` existed, the baseline), the loop with device metrics, and ``batch=N`` with device metrics.  A script, not a
test.

Generates ``--samples`` (16) sample directories -- make_scene(2000 + k, 5 talkers, 7 mics, T = 48 000), each with its
own array -- and evaluates them with the FULL spot and separation networks (random weights, f16x3, spot batch 64),
writing the result files.  The three legs alternate in one process; ``--warmups`` (3) rounds are discarded and every
figure is the median of ``--reps`` (5); each leg ends in a device synchronise; the host side runs on the machine's
threads as given (16 on the GPU machines).  One JSON line goes to profiles/eval/perf_eval_dataset.jsonl (``--out``):
seconds per sample of each leg, its split among search + separation, the SI-SDR pass, the matching, BSS-eval SDR, the
rest of the record, reading the wav files and writing the JSON files (``evaluate_dataset(stats=)``; in the per-sample
legs the whole metrics pass is "record_s"), and the launch-rule histogram of ``localize_batch.last_stats`` for the
batched leg.  Nothing is asserted about the times.

    python tests/perf_eval_dataset.py [--samples N] [--batch N] [--warmups N] [--reps N] [--out FILE]
"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd import evalkit  # noqa: E402
from acousticswarms_speech_amd.config import FULL, SEP_FULL  # noqa: E402
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.sep import SepModel  # noqa: E402
from acousticswarms_speech_amd.shard import localize_batch  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict  # noqa: E402

T = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "perf_eval_dataset.jsonl"))
    args = ap.parse_args()
    root = tempfile.mkdtemp(prefix="perf_eval_dataset_")
    try:
        for k in range(args.samples):
            evalkit.write_scene_dir(make_scene(2000 + k, 5, 7, T), os.path.join(root, "ds", f"{k:05d}"))
        spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")
        sep = SepModel(SEP_FULL, make_sep_state_dict(SEP_FULL, 9), precision="f16x3").to("cuda")
        jm = JointModel(spot, sep, device="cuda")
        legs = {"loop_host": dict(batch=1, metrics="host"), "loop_device": dict(batch=1, metrics="device"),
                "batched_device": dict(batch=args.batch, metrics="device")}
        times, splits, totals, rules = {k: [] for k in legs}, {k: [] for k in legs}, {}, []
        for rnd in range(args.warmups + args.reps):
            for name, kw in legs.items():
                stats = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with redirect_stdout(io.StringIO()):
                    tot = evalkit.evaluate_dataset(jm, os.path.join(root, "ds"), os.path.join(root, "res_" + name),
                                                   stats=stats, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(f"round {rnd} {name}: {dt / args.samples:.3f} s per sample", file=sys.stderr, flush=True)
                if rnd < args.warmups:
                    continue
                times[name].append(dt)
                splits[name].append(stats)
                totals[name] = tot
                if name == "batched_device":
                    rules.append(dict(getattr(localize_batch, "last_stats", {}).get("launch_rule", {})))
        rec = {"what": "evaluate_dataset", "samples": args.samples, "talkers": 5, "mics": 7, "T": T, "precision": "f16x3",
               "batch": args.batch, "warmups": args.warmups, "reps": args.reps, "threads": torch.get_num_threads(),
               "device": torch.cuda.get_device_name(0), "totals": totals, "launch_rule": rules[-1] if rules else {}}
        for name in legs:
            rec[name] = {"s_per_sample": round(float(np.median(times[name])) / args.samples, 6),
                         "split_s_per_sample": {key: round(float(np.median([s[key] for s in splits[name]])) / args.samples, 6)
                                                for key in sorted(splits[name][0])}}
        line = json.dumps(rec)
        print(line)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
