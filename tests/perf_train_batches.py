"""Training batches on one MI355X.  A script, not a test; nothing is asserted about the times.

One record, printed as one JSON line and appended to profiles/train_batches/perf_train_batches.jsonl (``--out``).  Per
case -- 8 localization items (7 rows each) at T = 48 000 and 144 000, 8 separation items of 5 talkers (35 rows each) at
T = 48 000, all perturbed:

``statement_s``   the numpy statement ``train_data.train_batch_f64`` (Philox in numpy, ``irfft``), one thread;
``host_loop_s``   a reference-style loop: per item ``default_rng(seed).normal`` twice, ``pink_from_normals``,
                  ``numpy.random``-style white noise and the float64 sum, the items spread over this machine's 16 threads
                  (what the reference's loader workers do);
``device_ms``     ``ops.colored_noise`` + ``ops.train_batch`` with the mixtures already on the device, by device events
                  around ``--reps`` back-to-back calls after one warm-up;
``device_upload_ms``  the same with the upload of the float32 mixtures from pageable host memory, by the wall clock;
``launch_ms``     the launch profile of one further call: ``noise_chirp`` (the chirp's spectrum, once per call),
                  ``noise_spectrum_cols`` (Philox spectrum, chirp product on the way in, column transforms),
                  ``noise_rows_product`` (row transforms both ways and the product with the chirp's spectrum),
                  ``noise_cols_inv`` (inverse column transforms, final chirp product, the write), ``train_batch``;
``train_batch_hbm_share``  the bytes ``train_batch`` must move (float32 mixture and float64 pink row in, float32 out) over
                  its time, as a share of ``--hbm-tbs`` (8 TB/s).

    python tests/perf_train_batches.py [--out FILE] [--reps N] [--skip-host]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd import native, ops  # noqa: E402
from acousticswarms_speech_amd import train_data as td  # noqa: E402

M, ITEMS = 7, 8
CASES = (("localization_T48000", 1, 48000), ("localization_T144000", 1, 144000), ("separation_T48000", 5, 48000))


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


def host_item(args):
    """One item the way the reference's ``perturb_audio`` makes it."""
    x, seed, pink_level, white_level = args
    rng = np.random.default_rng(seed)
    size = (x.shape[0], x.shape[1] // 2 + 1)
    pink = td.pink_from_normals(rng.normal(size=size), rng.normal(size=size), x.shape[1])
    white = np.random.RandomState(seed).normal(0, 1, size=x.shape)
    return ((x.astype(np.float64) + white_level * white) + pink_level * pink).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_batches", "perf_train_batches.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = {"record": "train_batches", "items": ITEMS, "mics": M, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "host_threads": 16, "cases": {}}
    for name, S, T in CASES:
        rng = np.random.default_rng(S * T)
        mix = (0.1 * rng.standard_normal((ITEMS, M, T))).astype(np.float32)
        shifts = rng.integers(-140, 141, size=(ITEMS, S, M)).astype(np.int32)
        shifts[:, :, 0] = 0
        counts, item_mix = [S] * ITEMS, list(range(ITEMS))
        pink_level, white_level = [5e-3 * (i + 1) / ITEMS for i in range(ITEMS)], [1e-3 * (i + 1) / ITEMS for i in range(ITEMS)]
        pink_key, white_key = [100 + i for i in range(ITEMS)], [200 + i for i in range(ITEMS)]
        rows = S * M
        keys, ids = [k for k in pink_key for _ in range(rows)], list(range(rows)) * ITEMS

        def device(mix_dev):
            pink = ops.colored_noise(keys, ids, T, device="cuda:0").reshape(ITEMS, rows, T)
            return ops.train_batch(mix_dev, item_mix, shifts, counts, pink_level, white_level, white_key, pink=pink)
        mix_dev = torch.from_numpy(mix).cuda()
        r = {"rows": ITEMS * rows, "T": T, "device_ms": round(events_ms(lambda: device(mix_dev), args.reps), 4)}
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device(torch.from_numpy(mix).cuda())
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        r["device_upload_ms"] = round(float(np.median(times)), 4)
        r["launch_ms"] = launches(lambda: device(mix_dev))
        tb_ms = r["launch_ms"]["train_batch"][1]
        r["train_batch_hbm_share"] = round(ITEMS * rows * T * 16.0 / (tb_ms * 1e-3) / (args.hbm_tbs * 1e12), 4) if tb_ms > 0 else None
        r["noise_workspace_bytes"] = int(native.lib().asw_colored_noise_workspace_bytes(ITEMS * rows, T, 0))
        if not args.skip_host:
            got = device(mix_dev).cpu().numpy()
            t0 = time.perf_counter()
            want = td.train_batch_f64(mix, item_mix, shifts, counts, pink_level, white_level, pink_key, white_key)
            r["statement_s"] = round(time.perf_counter() - t0, 4)
            r["float32_samples_that_differ"] = int(np.sum(got != want))
            rolled = [np.concatenate([td.roll_rows(mix[i], shifts[i, s]) for s in range(S)]) for i in range(ITEMS)]
            jobs = [(rolled[i], 300 + i, pink_level[i], white_level[i]) for i in range(ITEMS)]
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=16) as ex:
                list(ex.map(host_item, jobs))
            r["host_loop_s"] = round(time.perf_counter() - t0, 4)
        rec["cases"][name] = r
        del mix_dev
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
