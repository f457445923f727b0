"""Diagnostic (not a pytest module): the three fp32-class arithmetic modes -- f16x3, f16x3_safe, f32 -- side by side.

Spot network: FULL net on the bench scene (configs[2]: 7 mics, 5 talkers, reverberant, T = 48 000), internal batch 256,
256 candidates per step, the modes alternated in ONE process (mode A step, mode B step, mode C step, again), three
warm-up steps per mode, then `--steps` timed steps each (host clock around a step that ends in a device synchronise);
median and range.  Then, untimed, one step per mode under the launch profiler for the per-launch table.
Separation network: FULL net at 5 and 27 speakers, T = 48 000, the same protocol.

Appends one JSON line per (network, size) to profiles/safe_mode/perf_modes.jsonl (or --out).  There is no pass mark:
the yardsticks are the two existing modes of the same run.  Needs an MI355X; without one it fails."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd import native, ops  # noqa: E402
from acousticswarms_speech_amd.config import FULL, SEP_FULL  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene, random_offsets  # noqa: E402
from acousticswarms_speech_amd.sep import SepModel  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict  # noqa: E402

MODES = ("f16x3", "f16x3_safe", "f32")


def _profile(step):
    L = native.lib()
    L.asw_profile_enable(1)
    step()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 18)
    native.check(L.asw_profile_report(buf, len(buf)))
    L.asw_profile_enable(0)
    rep = json.loads(buf.value.decode())
    return {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}


def measure(model, step, steps, warmup=3):
    """step(): one call on `model`, any precision.  -> {mode: {...}}"""
    for mode in MODES:
        model.set_precision(mode)
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(steps):
        for mode in MODES:                       # alternated: drift of the shared host hits every mode alike
            model.set_precision(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for mode in MODES:
        model.set_precision(mode)
        ops.f16x3_overflow_count(reset=True)
        table = _profile(step)
        t = times[mode]
        out[mode] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                     "steps": len(t), "guard": ops.f16x3_overflow_count(reset=True), "launch_table_ms": table}
    for mode in MODES:
        out[mode]["ratio_to_f16x3"] = round(out[mode]["median_ms"] / out["f16x3"]["median_ms"], 4)
        out[mode]["ratio_to_f32"] = round(out[mode]["median_ms"] / out["f32"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--T", type=int, default=48000)
    ap.add_argument("--speakers", type=int, nargs="*", default=[5, 27])
    ap.add_argument("--skip-spot", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "safe_mode", "perf_modes.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_precision_modes: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    scene = make_scene(1010, n_speakers=5, n_mics=7, T=args.T, reverb=True)
    mix = torch.from_numpy(scene.mix).to(dev)

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        brief = {m: {k: v for k, v in rec["modes"][m].items() if k != "launch_table_ms"} for m in MODES}
        print(json.dumps({**{k: v for k, v in rec.items() if k != "modes"}, "modes": brief}), flush=True)
        for m in MODES:
            top = list(rec["modes"][m]["launch_table_ms"].items())[:12]
            print(f"  {m}: " + ", ".join(f"{k} {v['ms']:.2f} ms x{v['launches']}" for k, v in top), flush=True)

    if not args.skip_spot:
        model = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=args.batch, precision="f16x3").to(dev)
        off = torch.from_numpy(random_offsets(7, args.candidates, 6, 140)).to(dev)
        step = lambda: model.shift_and_sep_device(mix, off, strict=1, want_wave=False, want_energy=True, window=12000)
        res = measure(model, step, args.steps)
        for m in MODES:
            res[m]["candidates_per_s"] = round(args.candidates / res[m]["median_ms"] * 1e3, 1)
        emit({"what": "spot FULL shift_and_sep", "T": args.T, "candidates": args.candidates, "batch": args.batch, "modes": res})
        del model
        torch.cuda.empty_cache()
    if args.speakers:
        sep = SepModel(SEP_FULL, make_sep_state_dict(SEP_FULL, 9), precision="f16x3").to(dev)
        for S in args.speakers:
            offs = torch.from_numpy(random_offsets(7, S, 6, 140)).to(dev)
            res = measure(sep, lambda: sep.infer_device(mix, offs), args.steps)
            emit({"what": "sep FULL infer", "T": args.T, "speakers": S, "modes": res})


if __name__ == "__main__":
    main()
