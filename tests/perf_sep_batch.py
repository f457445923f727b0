"""The joint separation of a batch of mixtures in packed calls (``SepModel.infer_batch``) against the per-mixture
``infer_sample`` loop on one MI355X.  A script, not a test.

separate  FULL separation network, f16x3, random weights, T = 48 000, 7 microphones: 16 mixtures of 5 talkers, and 16
          mixtures of 2-6 talkers (make_scene(3000 + k, S_k, ...), the talkers' true sample offsets).  Wall time of one
          ``infer_batch`` call and of the loop ``[infer_sample(m, s) for m, s in ...]``, both from host arrays to host
          arrays.  The loop is the code as it was before ``infer_batch`` existed.
localize  16 five-talker mixtures (seeds 2000-2015, one array, T = 48 000; FULL spot network, f16x3, batch 64)
          through ``shard.localize_batch(..., concurrent=2)`` without and with ``separate=True``.
The two sides of a record alternate within one run and every figure is the median of ``--reps`` (5) after one warm-up
each.  Appends one JSON line per record to profiles/sep/perf_sep_batch.jsonl (``--out``).  Nothing is asserted about
the times.

    python tests/perf_sep_batch.py [--reps N] [--out FILE] [--no-localize]
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
from acousticswarms_speech_amd.config import FULL, SEP_FULL  # noqa: E402
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.sep import SepModel, pack_items  # noqa: E402
from acousticswarms_speech_amd.shard import localize_batch  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict  # noqa: E402

T = 48000


def med(v):
    return round(float(np.median(v)), 6)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def separate_records(emit, sep, reps):
    for name, counts in (("16 x 5 talkers", [5] * 16), ("16 x 2-6 talkers", [2 + (3 * k) % 5 for k in range(16)])):
        scenes = [make_scene(3000 + k, c, 7, T) for k, c in enumerate(counts)]
        mixes = [sc.mix for sc in scenes]
        samples = [list(sc.tdoa_samples()) for sc in scenes]
        sides = {"infer_batch": lambda: sep.infer_batch(mixes, samples),
                 "infer_sample_loop": lambda: [sep.infer_sample(m, s) for m, s in zip(mixes, samples)]}
        out = {k: fn() for k, fn in sides.items()}                 # warm-up (workspace, code objects)
        worst = max(float(np.abs(a - b).max()) for a, b in zip(out["infer_batch"], out["infer_sample_loop"]))
        times = {k: [] for k in sides}
        for _ in range(reps):
            for k, fn in sides.items():
                times[k].append(timed(fn)[0])
        rec = {"record": "separate", "workload": name, "counts": counts, "sequences": sum(counts),
               "device_calls": len(pack_items(counts)), "network": "SEP_FULL, f16x3, random weights", "T": T, "reps": reps,
               "max_abs_difference": worst}
        for k in sides:
            rec[k] = {"s": med(times[k]), "s_all": [round(v, 5) for v in times[k]]}
        emit(rec)


def localize_records(emit, sep, reps):
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")
    first = make_scene(2000, 5, 7, T)
    scenes = [make_scene(2000 + k, 5, 7, T, mic_positions=first.mic_positions) for k in range(16)]
    mixes = [torch.from_numpy(s.mix) for s in scenes]
    jm = JointModel(spot, sep, device="cuda")
    times = {False: [], True: []}
    with redirect_stdout(io.StringIO()):
        jm.setup(first.mic_positions, first.speaker_range)
        for separate in (False, True):
            localize_batch(jm, mixes[:4], concurrent=2, separate=separate)       # warm-up
        for _ in range(reps):
            for separate in (False, True):
                dt, out = timed(lambda: localize_batch(jm, mixes, concurrent=2, separate=separate))
                times[separate].append(dt)
                if separate:
                    talkers = [int(r["audio"].shape[0]) for r in out]
    emit({"record": "localize", "workload": "16 x 5 talkers, seeds 2000-2015, concurrent=2", "T": T, "reps": reps,
          "spot_network": "FULL, f16x3, batch 64, random weights", "sep_network": "SEP_FULL, f16x3, random weights",
          "talkers_found": talkers, "device_calls": len(pack_items(talkers)),
          "localize_s": med(times[False]), "localize_and_separate_s": med(times[True]),
          "localize_s_all": [round(v, 5) for v in times[False]],
          "localize_and_separate_s_all": [round(v, 5) for v in times[True]]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sep", "perf_sep_batch.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-localize", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, gpu=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    sep = SepModel(SEP_FULL, make_sep_state_dict(SEP_FULL, 9), precision="f16x3").to("cuda")
    separate_records(emit, sep, args.reps)
    if not args.no_localize:
        localize_records(emit, sep, args.reps)


if __name__ == "__main__":
    main()
