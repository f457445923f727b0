"""The oracle mask baselines of a batch on one MI355X.  A script, not a test; nothing is asserted about the times.

Sizes: 16 samples x 5 talkers x N = 48 000 (48 frames each), the ideal ratio mask and the ideal binary mask, each ONE
device call.  One record, printed as one JSON line and appended to profiles/eval/perf_oracle_masks.jsonl (``--out``).
Per mask: ``device_s`` is ``evalkit.oracle_masks_batch`` (upload, op, read-back of 31 MB of float64), ``kernels_s`` the
op alone with the inputs on the device, between two synchronisations, ``launch_ms`` one further call under the
library's launch profiler, ``host_s`` the float64 statements (``oracle_masks.irm_f64`` / ``ibm_f64``, numpy.fft) sample
after sample on this machine's CPUs and, where scipy is importable, ``scipy_s`` the same arithmetic through
``scipy.signal.stft`` / ``istft`` as the reference calls them; medians of ``--reps`` after one warm-up, the sides
alternating.  ``max_rel_err`` is the largest per-row max abs difference over max abs value, device against statement.

    python tests/perf_oracle_masks.py [--out FILE] [--reps N]
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd import evalkit, native  # noqa: E402
from acousticswarms_speech_amd import oracle_masks as om  # noqa: E402
from tests.oracle_masks_cases import sources  # noqa: E402

K, S, N = 16, 5, 48000


def scipy_masks(gt, mix, kind):
    import scipy.signal
    X = scipy.signal.stft(mix.astype(np.float64), nperseg=2048)[2]
    P = np.abs(scipy.signal.stft(gt.astype(np.float64), nperseg=2048)[2])
    if kind == "irm":
        model = om.EPS
        for j in range(gt.shape[0]):
            model = model + P[j]
        mask = P / model
    else:
        mask = np.where(P / (om.EPS + np.abs(X)) >= 0.5, 1.0, 0.0)
    return scipy.signal.istft(X[None] * mask)[1][..., :mix.shape[0]]


def launches(op, *args):
    L = native.lib()
    L.asw_profile_enable(1)
    op(*args)
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    native.check(L.asw_profile_report(buf, len(buf)))
    L.asw_profile_enable(0)
    return {n: [v["launches"], round(v["ms"], 3)] for n, v in json.loads(buf.value.decode()).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "perf_oracle_masks.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    have_scipy = importlib.util.find_spec("scipy") is not None
    data = [sources(160 + k, S, N) for k in range(K)]
    refs, mixes = [g for g, _m in data], [m for _g, m in data]
    d_mix = torch.from_numpy(np.stack(mixes)).cuda()
    d_ref = torch.from_numpy(np.concatenate(refs)).cuda()
    op = native.torch_ops().oracle_masks
    rec = {"record": "oracle_masks", "samples": K, "talkers": S, "N": N, "frames": om.frame_count(N), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "scipy": have_scipy,
           "workspace_bytes": int(native.lib().asw_oracle_masks_workspace_bytes((ctypes.c_int32 * K)(*[S] * K),
                                                                                (ctypes.c_int32 * K)(*[N] * K), K))}
    for kind in om.KINDS:
        evalkit.oracle_masks_batch(refs, mixes, kind)                          # warm-up
        times = {"host": [], "scipy": [], "device": [], "kernels": []}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            want = [om.masks_f64(g, m, kind) for g, m in data]
            times["host"].append(time.perf_counter() - t0)
            if have_scipy:
                t0 = time.perf_counter()
                for g, m in data:
                    scipy_masks(g, m, kind)
                times["scipy"].append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = evalkit.oracle_masks_batch(refs, mixes, kind)
            times["device"].append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            op(d_mix, d_ref, [S] * K, [N] * K, kind)
            torch.cuda.synchronize()
            times["kernels"].append(time.perf_counter() - t0)
        err = max(float(np.max(np.max(np.abs(g - w), axis=1) / np.max(np.abs(w), axis=1))) for g, w in zip(got, want))
        med = {k: float(np.median(v)) for k, v in times.items() if v}
        rec[kind] = {"max_rel_err": err, **{f"{k}_s": round(v, 6) for k, v in med.items()},
                     "host_over_device": round(med["host"] / med["device"], 1),
                     "host_over_kernels": round(med["host"] / med["kernels"], 1),
                     **({"scipy_over_device": round(med["scipy"] / med["device"], 1)} if have_scipy else {}),
                     "launch_ms": launches(op, d_mix, d_ref, [S] * K, [N] * K, kind),
                     **{f"{k}_s_all": [round(t, 6) for t in v] for k, v in times.items() if v}}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
