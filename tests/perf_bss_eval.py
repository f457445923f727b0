"""BSS-eval SDR of one sample: the host statement (``evalkit.bss_eval_sdr``, once per estimate set) against the device
op (``evalkit.bss_eval_sdr_device``: upload, ``torch.ops.asw.bss_eval_sdr``, read-back) on one MI355X.  A script, not a
test.

Sizes: S = 5 and S = 2 talkers, flen = 512, T = 48 000, R = 2 estimate sets (the unprocessed microphone and a noisy
separation), as ``evalkit.compute_metrics`` sends them.  The two sides alternate in one run, median of 5 after one
warm-up of the device side; the host side runs on this machine's CPUs with the thread count numpy finds.  ``device_s``
is the whole Python call, ``kernels_s`` the op alone between two stream synchronisations with the inputs already on
the device, ``launch_ms`` one further call under the library's launch profiler (HIP events around every launch: the sum
per kernel, with the number of launches).

Appends one JSON line per size to profiles/eval/perf_bss_eval.jsonl (``--out``).  Nothing is asserted about the times.

    python tests/perf_bss_eval.py [--out FILE] [--reps N]
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
from acousticswarms_speech_amd import evalkit, native  # noqa: E402
from tests import bss_eval_cases as cases  # noqa: E402

FLEN, T, R = 512, 48000, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "perf_bss_eval.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    op = native.torch_ops().bss_eval_sdr
    for S in (5, 2):
        refs, ests = cases.make_batch(48, [S], T)
        ref, est = refs[0], ests[0]
        d_ref, d_est = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
        evalkit.bss_eval_sdr_device(ref, est, FLEN)                          # warm-up
        host_t, dev_t, ker_t = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            want = np.stack([evalkit.bss_eval_sdr(ref, est[r], FLEN) for r in range(R)])
            host_t.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = evalkit.bss_eval_sdr_device(ref, est, FLEN)
            dev_t.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _sdr, status = op(d_ref, d_est, [S], FLEN)
            torch.cuda.synchronize()
            ker_t.append(time.perf_counter() - t0)
        h, d, k = (float(np.median(t)) for t in (host_t, dev_t, ker_t))
        L = native.lib()
        L.asw_profile_enable(1)
        op(d_ref, d_est, [S], FLEN)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        native.check(L.asw_profile_report(buf, len(buf)))
        L.asw_profile_enable(0)
        launches = {n: [v["launches"], round(v["ms"], 3)] for n, v in json.loads(buf.value.decode()).items()}
        rec = {"record": "bss_eval_sdr", "talkers": S, "flen": FLEN, "T": T, "estimate_sets": R, "reps": args.reps,
               "order": S * FLEN, "workspace_bytes": evalkit.bss_workspace_bytes([S], R, T, FLEN), "status": status.cpu().tolist(),
               "max_abs_diff_db": float(np.max(np.abs(got - want))), "host_s": round(h, 4), "device_s": round(d, 5),
               "kernels_s": round(k, 5), "host_over_device": round(h / d, 1), "launch_ms": launches,
               "host_s_all": [round(t, 4) for t in host_t], "device_s_all": [round(t, 5) for t in dev_t],
               "kernels_s_all": [round(t, 5) for t in ker_t], "host_threads": torch.get_num_threads(),
               "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
