"""Voice preparation on one MI355X.  A script, not a test; nothing is asserted about the times.

One record, printed as one JSON line and appended to profiles/voice_prep/perf_voice_prep.jsonl (``--out``):

``index``   the index pass of one speaker directory, 400 clips of 4 s at 44.1 kHz to 48 kHz (160/147, 21 or 22 taps per
            output): ``ops.voice_resample`` of the whole rows to float32 and ``ops.voice_trim`` on the result, the clips
            already on the device, by device events around ``--reps`` back-to-back calls after one warm-up
            (``device_ms``), the same with the upload of the clips from pageable host memory by the wall clock
            (``device_upload_ms``), and the launch profile of one further call (``launch_ms``);
``fetch``   the fetch pass of 16 scenes x 5 talkers x 48 000 samples cut out of such clips: one ``ops.voice_resample``
            call with windows, without and with the upload;
``host``    the same work through ``scipy.signal.resample_poly`` and the numpy trim (``voiceprep.trim_f64``) spread over
            16 threads, by the wall clock; the fetch pass resamples the whole clip and cuts, as the reference does.

Per kernel the bytes it must move (float32 in and out; the trim reads its rows twice more for the variance) over its
time as a share of ``--hbm-tbs`` (8 TB/s), and for the resampler the float64 multiply-add pairs per second it achieved:
with 21-61 taps per output it is bound by those, not by memory, when the first share is small.

    python tests/perf_voice_prep.py [--out FILE] [--reps N] [--skip-host]
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
from acousticswarms_speech_amd import voiceprep as vp  # noqa: E402

SR_IN, SR_OUT, CLIPS, SECONDS = 44100, 48000, 400, 4.0
SCENES, TALKERS, T = 16, 5, 48000


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


def wall_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def launches(fn):
    L = native.lib()
    L.asw_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    native.check(L.asw_profile_report(buf, len(buf)))
    L.asw_profile_enable(0)
    return {n: [v["launches"], round(v["ms"], 4)] for n, v in json.loads(buf.value.decode()).items()}


def clip(k, n):
    rng = np.random.RandomState(k)
    t = np.arange(n) / SR_IN
    x = 1e-4 * rng.standard_normal(n)
    a, b = int(0.15 * n), int(0.85 * n)
    x[a:b] += 0.3 * np.sin(2 * np.pi * (120 + k % 80) * t[a:b]) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t[a:b]))
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_prep", "perf_voice_prep.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda:0")
    n_in = int(SR_IN * SECONDS)
    clips = [clip(k, n_in) for k in range(CLIPS)]
    x_host = np.concatenate(clips)
    offs, lens = [k * n_in for k in range(CLIPS)], [n_in] * CLIPS
    n_out = vp.resampled_length(n_in, SR_OUT, SR_IN)
    up, down = vp.reduced(SR_OUT, SR_IN)
    taps = (vp.resample_filter(up, down).shape[0] - 1) / up
    rec = {"record": "voice_prep", "device": torch.cuda.get_device_name(0), "reps": args.reps, "host_threads": 16,
           "ratio": [up, down], "taps_per_output": round(taps, 2)}

    def index_pass(x):
        y = ops.voice_resample(x, offs, lens, SR_OUT, SR_IN, [0] * CLIPS, [n_out] * CLIPS, n_out)
        return ops.voice_trim(y.reshape(-1), [r * n_out for r in range(CLIPS)], [n_out] * CLIPS)
    x_dev = torch.from_numpy(x_host).to(dev)
    r = {"clips": CLIPS, "samples_in": n_in, "samples_out": n_out, "device_ms": round(events_ms(lambda: index_pass(x_dev), args.reps), 4),
         "device_upload_ms": round(wall_ms(lambda: index_pass(torch.from_numpy(x_host).to(dev)), args.reps), 4),
         "launch_ms": launches(lambda: index_pass(x_dev))}
    ms = {k: v[1] for k, v in r["launch_ms"].items()}
    out_samples = CLIPS * n_out
    r["resample_hbm_share"] = round((CLIPS * n_in + out_samples) * 4.0 / (ms["voice_resample"] * 1e-3) / (args.hbm_tbs * 1e12), 4)
    r["resample_f64_fma_per_s"] = round(out_samples * taps / (ms["voice_resample"] * 1e-3), 0)
    trim_ms = ms["voice_block_sums"] + ms["voice_trim"]
    r["trim_hbm_share"] = round(out_samples * 4.0 * 3 / (trim_ms * 1e-3) / (args.hbm_tbs * 1e12), 4)
    bounds, stats = (t.cpu().numpy() for t in index_pass(x_dev))
    rec["index"] = r

    rng = np.random.RandomState(0)
    rows = SCENES * TALKERS
    pick = rng.randint(0, CLIPS, rows)
    begin = [int(rng.randint(0, n_out - T)) for _ in range(rows)]

    def fetch_pass(x):
        return ops.voice_resample(x, [offs[k] for k in pick], [n_in] * rows, SR_OUT, SR_IN, begin, [T] * rows, T)
    sub_host = np.concatenate([clips[k] for k in pick])
    sub_offs = [r_ * n_in for r_ in range(rows)]

    def fetch_upload():
        return ops.voice_resample(torch.from_numpy(sub_host).to(dev), sub_offs, [n_in] * rows, SR_OUT, SR_IN, begin, [T] * rows, T)
    f = {"rows": rows, "T": T, "device_ms": round(events_ms(lambda: fetch_pass(x_dev), args.reps), 4),
         "device_upload_ms": round(wall_ms(fetch_upload, args.reps), 4), "launch_ms": launches(lambda: fetch_pass(x_dev))}
    fms = f["launch_ms"]["voice_resample"][1]
    f["resample_hbm_share"] = round(rows * T * (down / up + 1.0) * 4.0 / (fms * 1e-3) / (args.hbm_tbs * 1e12), 4)
    f["resample_f64_fma_per_s"] = round(rows * T * taps / (fms * 1e-3), 0)
    rec["fetch"] = f

    if not args.skip_host:
        from scipy.signal import resample_poly

        def host_index(x):
            y = resample_poly(x.astype(np.float64), up, down).astype(np.float32)
            return vp.trim_f64(y)

        def host_fetch(job):
            k, b = job
            return resample_poly(clips[k].astype(np.float64), up, down).astype(np.float32)[b:b + T]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as ex:
            host = list(ex.map(host_index, clips))
        h = {"index_s": round(time.perf_counter() - t0, 4)}
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as ex:
            list(ex.map(host_fetch, zip(pick, begin)))
        h["fetch_s"] = round(time.perf_counter() - t0, 4)
        # scipy's resampler adds in another order than the statement: the bounds agree unless a frame sits on the threshold
        h["index_bounds_that_differ_from_scipy_path"] = int(sum((int(bounds[k, 0]), int(bounds[k, 1])) != host[k][:2] for k in range(CLIPS)))
        rec["host"] = h
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
