"""The room simulator on one MI355X.  A script, not a test; nothing is asserted about the times.

One record, printed as one JSON line and appended to profiles/roomsim/perf_roomsim.jsonl (``--out``):

``rir``       ``room_rir`` for one scene of 5 talkers and 7 microphones (35 pairs) of the recipe at order 15 and order 50,
              the length that of ``roomsim.rir_length`` at T = 48 000: ``kernel_ms`` by device events around ``--reps``
              back-to-back calls after one warm-up, ``host_s`` the statement ``roomsim.rir_f64`` on the same inputs on this
              machine's CPUs, ``max_rel_err`` the largest per-response difference over the response's peak.  Order 150
              is run once on the device alone (``order150_ms``).
``convolve``  ``room_convolve`` of those 5 dry voices through the order-50 responses at T = 48 000 and 144 000, the same
              way, with the launch profile of one further call.
``scenes``    16 scenes x 5 talkers of the recipe (order 15, T = 48 000) through ``room_scenes.simulate_rooms``:
              ``device_s`` with the upload of the voices and the read-back of the float32 scenes, ``kernels_ms`` the two
              ops alone by device events, ``host_s`` the statements scene after scene.

    python tests/perf_roomsim.py [--out FILE] [--reps N] [--skip-host]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd import native, room_scenes, roomsim  # noqa: E402
from tests.roomsim_cases import row_errors  # noqa: E402

FS, S, M = 48000, 5, 7


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def launches(fn):
    L = native.lib()
    L.asw_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    native.check(L.asw_profile_report(buf, len(buf)))
    L.asw_profile_enable(0)
    return {n: [v["launches"], round(v["ms"], 3)] for n, v in json.loads(buf.value.decode()).items()}


def host_tensors(spec_list, orders):
    rooms = torch.from_numpy(np.array([sp.room for sp in spec_list], dtype=np.float64))
    absorption = torch.from_numpy(np.array([sp.absorption for sp in spec_list], dtype=np.float64))
    src = torch.from_numpy(np.concatenate([sp.sources for sp in spec_list]).astype(np.float64))
    mics = torch.from_numpy(np.stack([sp.mics for sp in spec_list]).astype(np.float64))
    return rooms, absorption, list(orders), src, mics, [sp.dry.shape[0] for sp in spec_list]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roomsim", "perf_roomsim.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    t = native.torch_ops()
    rec = {"record": "roomsim", "talkers": S, "mics": M, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": torch.get_num_threads(), "rir": {}, "convolve": {}, "scenes": {}}

    spec = room_scenes.make_room_spec(np.random.RandomState(100), S, M, 48000, 15)
    rec["room"], rec["absorption"] = spec.room, spec.absorption
    responses = {}
    for order in (15, 50):
        length = roomsim.rir_length(spec.room, order, FS, 48000)
        rooms, absorption, orders, src, mics, counts = host_tensors([spec], [order])
        run = lambda: t.room_rir(rooms, absorption, orders, src, mics, counts, float(FS), length)  # noqa: E731
        r = {"images": roomsim.image_count(order), "length": length, "kernel_ms": round(events_ms(run, args.reps), 4)}
        responses[order] = run()
        if not args.skip_host:
            t0 = time.perf_counter()
            want = roomsim.rir_f64(rooms.numpy(), absorption.numpy(), orders, src.numpy(), mics.numpy(), counts, FS, length)
            r["host_s"] = round(time.perf_counter() - t0, 4)
            r["max_rel_err"] = float(np.max(row_errors(responses[order].cpu().numpy(), want, 2)))
        rec["rir"][f"order{order}"] = r
    rooms, absorption, orders, src, mics, counts = host_tensors([spec], [150])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h150 = t.room_rir(rooms, absorption, orders, src, mics, counts, float(FS), 48000)
    torch.cuda.synchronize()
    rec["rir"]["order150_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    rec["rir"]["order150_images"] = roomsim.image_count(150)
    rec["rir"]["order150_finite"] = bool(torch.isfinite(h150).all())
    del h150

    for T in (48000, 144000):
        sp = room_scenes.make_room_spec(np.random.RandomState(100), S, M, T, 15)
        length = roomsim.rir_length(sp.room, 50, FS, T)
        rooms, absorption, orders, src, mics, counts = host_tensors([sp], [50])
        rir = t.room_rir(rooms, absorption, orders, src, mics, counts, float(FS), length)
        dry = torch.from_numpy(sp.dry).cuda()
        run = lambda: t.room_convolve(dry, rir, counts)  # noqa: E731
        r = {"length": length, "kernel_ms": round(events_ms(run, args.reps), 4), "launch_ms": launches(run),
             "workspace_bytes": int(native.lib().asw_room_convolve_workspace_bytes((ctypes.c_int32 * 1)(S), 1, M, length, T))}
        if not args.skip_host:
            premix, mix = run()
            t0 = time.perf_counter()
            want_premix, want_mix = roomsim.convolve_f64(sp.dry, rir.cpu().numpy(), counts)
            r["host_s"] = round(time.perf_counter() - t0, 4)
            r["max_rel_err"] = max(float(np.max(row_errors(premix.cpu().numpy(), want_premix, 2))),
                                   float(np.max(row_errors(mix.cpu().numpy(), want_mix, 2))))
            del premix, mix, want_premix, want_mix
        rec["convolve"][f"T{T}"] = r
        del rir, dry

    rng = np.random.RandomState(200)
    specs = [room_scenes.make_room_spec(rng, S, M, 48000, 15) for _ in range(16)]
    room_scenes.simulate_rooms(specs, backend="device")                        # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = room_scenes.simulate_rooms(specs, backend="device")
        times.append(time.perf_counter() - t0)
    rooms, absorption, orders, src, mics, counts = host_tensors(specs, [15] * 16)
    length = max(roomsim.rir_length(sp.room, 15, FS, 48000) for sp in specs)
    dry = torch.from_numpy(np.concatenate([sp.dry for sp in specs])).cuda()

    def both():
        return t.room_convolve(dry, t.room_rir(rooms, absorption, orders, src, mics, counts, float(FS), length), counts)
    rec["scenes"] = {"scenes": 16, "T": 48000, "order": 15, "length": length, "device_s": round(float(np.median(times)), 5),
                     "device_s_all": [round(v, 5) for v in times], "kernels_ms": round(events_ms(both, args.reps), 4),
                     "launch_ms": launches(both)}
    if not args.skip_host:
        t0 = time.perf_counter()
        host = room_scenes.simulate_rooms(specs, backend="host")
        rec["scenes"]["host_s"] = round(time.perf_counter() - t0, 3)
        rec["scenes"]["max_float32_ulps"] = max(
            float(np.max(np.abs(h.mix.astype(np.float64) - d.mix)) / np.spacing(np.float32(np.max(np.abs(h.mix))))) for h, d in zip(host, dev))
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
