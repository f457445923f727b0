"""Full BSS-eval of one sample on one MI355X.  A script, not a test; nothing is asserted about the times.

Sizes: S = 5 and S = 2 talkers, flen = 512, T = 48 000, R = 2 estimate sets ("mixture" and "noisy"), as
``tests/perf_bss_eval.py``.  Two records per size, appended to profiles/eval/perf_bss_sources.jsonl (``--out``):

``bss_eval_sdr_entry``: the old C entry point ``asw_bss_eval_sdr`` of this build (inputs on the device, the call between
two stream synchronisations), and with ``--parent-lib PATH`` the same call into another build of the library (the parent
commit's ``libasw_hip.so``) in the same process, the two alternating, median of 5 after one warm-up each; also whether
the two builds wrote the same sdr bytes.

``bss_eval_sources``: the new entry through ``evalkit.bss_eval_sources_device`` (upload, op, read-back, and with
``compute_permutation=True`` the choice on the host), matched and all pairs, each alternating with the host statement
(``evalkit.bss_eval_sources`` per estimate set, on this machine's CPUs with the thread count numpy finds), median of 5;
``kernels_s`` the op alone with the inputs on the device, ``launch_ms`` one further call under the library's launch
profiler, and the largest |device - statement| per ratio.

    python tests/perf_bss_sources.py [--out FILE] [--reps N] [--parent-lib PATH]
"""
import argparse
import ctypes
import hashlib
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


def sdr_entry(L):
    """``asw_bss_eval_sdr`` of library ``L`` as a function (d_ref, d_est, counts) -> (sdr bytes, seconds)."""
    L.asw_bss_eval_sdr_workspace_bytes.restype = ctypes.c_size_t
    L.asw_bss_eval_sdr_workspace_bytes.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4
    L.asw_bss_eval_sdr.restype = ctypes.c_int
    L.asw_bss_eval_sdr.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]

    def call(d_ref, d_est, counts, flen=FLEN):
        K, (sets, N, length) = len(counts), d_est.shape
        c = (ctypes.c_int32 * K)(*counts)
        need = L.asw_bss_eval_sdr_workspace_bytes(c, K, sets, length, flen)
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=d_ref.device)
        sdr = torch.empty((sets, N), dtype=torch.float64, device=d_ref.device)
        status = torch.empty(K, dtype=torch.int32, device=d_ref.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.asw_bss_eval_sdr(native.ptr(d_ref), native.ptr(d_est), c, K, sets, length, flen, native.ptr(sdr), native.ptr(status),
                                native.ptr(ws), need, native.current_stream())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return sdr.cpu().numpy().tobytes(), dt
    return call


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "perf_bss_sources.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    this = sdr_entry(native.lib())
    parent = sdr_entry(ctypes.CDLL(args.parent_lib)) if args.parent_lib else None
    op = native.torch_ops().bss_eval_sources
    common = {"flen": FLEN, "T": T, "estimate_sets": R, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for S in (5, 2):
        refs, ests = cases.make_batch(48, [S], T)
        ref, est = refs[0], ests[0]
        d_ref, d_est = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
        # 1. the old entry, this build against the parent's
        sides = {"this": this, **({"parent": parent} if parent else {})}
        times, digest = {k: [] for k in sides}, {}
        for fn in sides.values():
            fn(d_ref, d_est, [S])                                            # warm-up
        for _ in range(args.reps):
            for name, fn in sides.items():
                raw, dt = fn(d_ref, d_est, [S])
                times[name].append(dt)
                digest[name] = hashlib.sha256(raw).hexdigest()
        rec = {"record": "bss_eval_sdr_entry", "talkers": S, **common,
               **{f"{k}_s": round(float(np.median(v)), 6) for k, v in times.items()},
               **{f"{k}_s_all": [round(t, 6) for t in v] for k, v in times.items()}, "sdr_sha256": digest}
        if parent:
            rec["this_over_parent"] = round(float(np.median(times["this"]) / np.median(times["parent"])), 4)
            rec["same_bytes"] = digest["this"] == digest["parent"]
        emit(rec)
        # 2. the new entry, matched and all pairs, against the host statement
        for permute in (False, True):
            evalkit.bss_eval_sources_device(ref, est, FLEN, permute)         # warm-up
            host_t, dev_t, ker_t = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                want = [evalkit.bss_eval_sources(ref, est[r], FLEN, permute) for r in range(R)]
                host_t.append(time.perf_counter() - t0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = evalkit.bss_eval_sources_device(ref, est, FLEN, permute)
                dev_t.append(time.perf_counter() - t0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = op(d_ref, d_est, [S], FLEN, permute)
                torch.cuda.synchronize()
                ker_t.append(time.perf_counter() - t0)
            h, d, k = (float(np.median(t)) for t in (host_t, dev_t, ker_t))
            diff = {}
            for q, name in enumerate(("sdr", "sir", "sar")):
                w = np.stack([s[q] for s in want])
                fin = np.isfinite(w)
                diff[name] = float(np.max(np.abs(got[q][fin] - w[fin]))) if fin.any() else 0.0
            emit({"record": "bss_eval_sources", "talkers": S, "all_pairs": permute, **common, "order": S * FLEN,
                  "workspace_bytes": evalkit.bss_sources_workspace_bytes([S], R, T, FLEN, permute),
                  "status": out[3].cpu().tolist(), "same_perm": bool(np.array_equal(got[3], np.stack([s[3] for s in want]))),
                  "max_abs_diff_db": diff, "host_s": round(h, 4), "device_s": round(d, 5), "kernels_s": round(k, 5),
                  "host_over_device": round(h / d, 1), "launch_ms": launches(op, d_ref, d_est, [S], FLEN, permute),
                  "host_s_all": [round(t, 4) for t in host_t], "device_s_all": [round(t, 5) for t in dev_t],
                  "kernels_s_all": [round(t, 5) for t in ker_t], "host_threads": torch.get_num_threads()})


if __name__ == "__main__":
    main()
