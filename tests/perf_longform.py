"""A 60 s recording through the long-form path against the loop a user would write without it, on one MI355X.
A script, not a test.

The recording: make_scene(2000, 5 talkers, 7 microphones, Ttot = 2 880 000 samples at 48 kHz); blocks of 48 000 at the
default hop of 42 000 (69 blocks).  FULL spot network (batch 64) and FULL separation network, f16x3, random weights.

kernels   ``frame_blocks`` (the 12 blocks of one packed separation call, and all 69 in one call) and ``stitch_blocks``
          (345 rows into 5 tracks): device events around ``--kernel-iters`` back-to-back calls that rotate over enough
          buffer sets to exceed the 256 MiB Infinity Cache, so the bytes come from HBM; time per call, achieved bytes per
          second over the bytes the statement needs, and its share of the 8 TB/s peak.
separate  ``SepModel.infer_long`` with the talkers' true sample offsets, against per-block ``infer_sample`` (a host
          read-back per block) and the overlap-add in numpy float64.
first     ``JointModel.forward_long(localize="first")`` against ``forward`` on block 0, ``infer_sample`` on the others
          and the same overlap-add.
every     ``JointModel.forward_long(localize="every")`` against ``forward`` per block, ``longform.link_tracks`` and the
          same overlap-add.  Both sides link with ``--link-radius`` 10 m, not the default 0.25 m: random weights find
          some 17 "talkers" per block at unrelated places, which at 0.25 m would open a new track for nearly every one
          (over a thousand tracks of 60 s each); a trained model finds the same few talkers again, and 10 m keeps the
          number of tracks near the number of talkers per block, which is that case's amount of work.
Both sides of a record go from host arrays to host arrays and alternate within one run; every figure is the median of
the repetitions after one warm-up of each side (``every``: warmed on the first four blocks).  Reported per record:
seconds per minute of audio and the real-time factor (processing time / audio time).  Appends one JSON line per record
to profiles/longform/perf_longform.jsonl (``--out``).  Nothing is asserted about the times.

    python tests/perf_longform.py [--reps N] [--every-reps N] [--kernel-iters N] [--out FILE] [--link-radius M]
        [--only kernels,separate,first,every]
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
from acousticswarms_speech_amd import longform, native  # noqa: E402
from acousticswarms_speech_amd.config import FULL, SEP_FULL  # noqa: E402
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.sep import SepModel  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict  # noqa: E402

FS, T, TTOT, M, S = 48000, 48000, 60 * 48000, 7, 5
HOP = T - T // 8
HBM_PEAK = 8.0e12          # bytes per second, the MI355X's specification
L3_BYTES = 256 << 20


def med(v):
    return round(float(np.median(v)), 6)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stitch_numpy(rows, starts, det_of, Ttot):
    """The overlap-add of ``longform.stitch_f64``, a block at a time: rows[k] [n_k, T], det_of [K, S] -> float32 [S, Ttot]"""
    w = longform.taper(T, T - HOP)
    num, den = np.zeros((det_of.shape[1], Ttot)), np.zeros(Ttot)
    for k, a in enumerate(starts):
        den[a:a + T] += w
        here = det_of[k] >= 0
        num[here, a:a + T] += w * rows[k][det_of[k][here]]
    return (num / den).astype(np.float32)


def pair_record(emit, name, sides, reps, warm, extra):
    """``sides``: {label: fn}; warm-up through ``warm`` ({label: fn}), then ``reps`` alternating timed calls"""
    for fn in warm.values():
        fn()
    times, out = {k: [] for k in sides}, {}
    for _ in range(reps):
        for k, fn in sides.items():
            dt, out[k] = timed(fn)
            times[k].append(dt)
            print(f"# {name} {k}: {dt:.3f} s", file=sys.__stdout__, flush=True)      # a long record shows that it is alive
    rec = {"record": name, "Ttot": TTOT, "block": T, "hop": HOP, "blocks": len(longform.block_starts(TTOT, T, HOP)), "reps": reps}
    for k in sides:
        s = med(times[k])
        rec[k] = {"s": s, "s_per_minute_of_audio": round(s * 60.0 * FS / TTOT, 6), "real_time_factor": round(s * FS / TTOT, 6),
                  "s_all": [round(v, 5) for v in times[k]]}
    rec.update(extra(out))
    emit(rec)


def kernel_records(emit, iters):
    ops, dev = native.torch_ops(), "cuda"
    starts = [int(a) for a in longform.block_starts(TTOT, T, HOP)]
    K = len(starts)
    taper = torch.from_numpy(longform.taper(T, T - HOP)).to(dev)

    def measure(name, call, sets, nbytes, shape):
        n_sets = len(sets)
        outs = [call(x) for x in sets]                                  # warm-up; the results rotate too, each in its own buffer
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for i in range(iters):
            outs[i % n_sets] = call(sets[i % n_sets])
        b.record()
        b.synchronize()
        s = a.elapsed_time(b) * 1e-3 / iters
        emit({"record": "kernel", "kernel": name, "shape": shape, "iters": iters, "buffer_sets": n_sets, "bytes": nbytes,
              "s_per_call": round(s, 9), "bytes_per_s": round(nbytes / s, 1), "share_of_hbm_peak": round(nbytes / s / HBM_PEAK, 4),
              "method": "device events around back-to-back calls, launch gaps included"})

    def sets_for(nbytes, make):
        return [make() for _ in range(L3_BYTES // nbytes + 2)]
    for nb in (12, K):
        nbytes = 2 * nb * M * T * 4                                     # every sample of the blocks read once, written once
        sets = sets_for(nbytes, lambda: torch.randn(M, TTOT, device=dev))
        measure("frame_blocks", lambda mix: ops.frame_blocks(mix, starts[:nb], T), sets, nbytes,
                {"M": M, "Ttot": TTOT, "T": T, "blocks": nb})
        del sets
    row_of = list(range(K * S))
    # rows read once, the result written once, the taper once (it stays in the caches)
    nbytes = K * S * T * 4 + S * TTOT * 4 + T * 8
    sets = sets_for(nbytes, lambda: torch.randn(K * S, T, device=dev))
    measure("stitch_blocks", lambda rows: ops.stitch_blocks(rows, taper, starts, row_of, TTOT), sets, nbytes,
            {"rows": K * S, "T": T, "tracks": S, "Ttot": TTOT, "blocks": K})


def separate_record(emit, sep, scene, reps):
    mix, samples = scene.mix, list(scene.tdoa_samples())
    starts = longform.block_starts(TTOT, T, HOP)
    det_of = np.tile(np.arange(S), (len(starts), 1))

    def loop():
        return stitch_numpy([sep.infer_sample(mix[:, a:a + T], samples) for a in starts], starts, det_of, TTOT)
    sides = {"infer_long": lambda: sep.infer_long(mix, samples), "infer_sample_loop": loop}
    pair_record(emit, "separate", sides, reps, sides, lambda out: {
        "talkers": S, "network": "SEP_FULL, f16x3, random weights",
        "max_abs_difference": float(np.abs(out["infer_long"] - out["infer_sample_loop"]).max())})


def joint_records(emit, jm, scene, reps, every_reps, only, radius):
    mix = scene.mix
    starts = longform.block_starts(TTOT, T, HOP)
    nets = {"spot_network": "FULL, f16x3, batch 64, random weights", "sep_network": "SEP_FULL, f16x3, random weights"}

    def block(a, m=mix):
        return torch.from_numpy(m[:, a:a + T])

    def loop_first():
        patches, _al, audio, _d0, _d1, _st = jm.forward(block(0))
        if not patches:
            return np.empty((0, TTOT), dtype=np.float32)
        samples = [p[0].sample_offset for p in patches]
        rows = [np.asarray(audio)] + [jm.sep_model.infer_sample(block(a), samples) for a in starts[1:]]
        return stitch_numpy(rows, starts, np.tile(np.arange(len(patches)), (len(starts), 1)), TTOT)

    def loop_every(m=mix, st=starts):
        rows, centres = [], []
        for a in st:
            patches, _al, audio, _d0, _d1, _st = jm.forward(block(a, m))
            rows.append(np.empty((0, T), dtype=np.float32) if audio is None else np.asarray(audio))
            centres.append(np.array([p[0].center_pos() for p in patches]).reshape(-1, 3))
        det_of, _pos = longform.link_tracks(centres, radius)
        return stitch_numpy(rows, st, det_of, int(st[-1]) + T)
    short = np.ascontiguousarray(mix[:, :int(starts[3]) + T])            # the first four blocks
    with redirect_stdout(io.StringIO()):
        if "first" in only:
            sides = {"forward_long": lambda: jm.forward_long(mix, localize="first")["audio"], "forward_loop": loop_first}
            pair_record(emit, "first", sides, reps, sides, lambda out: dict(nets, tracks={k: int(v.shape[0]) for k, v in out.items()}))
        if "every" in only:
            sides = {"forward_long": lambda: jm.forward_long(mix, localize="every", link_radius=radius)["audio"], "forward_loop": loop_every}
            warm = {"forward_long": lambda: jm.forward_long(short, localize="every", link_radius=radius),
                    "forward_loop": lambda: loop_every(short, starts[:4])}
            pair_record(emit, "every", sides, every_reps, warm,
                        lambda out: dict(nets, link_radius=radius, tracks={k: int(v.shape[0]) for k, v in out.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longform", "perf_longform.jsonl"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every-reps", type=int, default=2)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--link-radius", type=float, default=10.0)
    ap.add_argument("--only", default="kernels,separate,first,every")
    args = ap.parse_args()
    only = set(args.only.split(","))
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, gpu=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
        line = json.dumps(rec)
        print(line, file=sys.__stdout__, flush=True)           # the searches' own lines are swallowed, these are not
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if "kernels" in only:
        kernel_records(emit, args.kernel_iters)
    if only & {"separate", "first", "every"}:
        scene = make_scene(2000, S, M, TTOT)
        sep = SepModel(SEP_FULL, make_sep_state_dict(SEP_FULL, 9), precision="f16x3").to("cuda")
        if "separate" in only:
            separate_record(emit, sep, scene, args.reps)
        if only & {"first", "every"}:
            spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")
            jm = JointModel(spot, sep, device="cuda")
            with redirect_stdout(io.StringIO()):
                jm.setup(scene.mic_positions, scene.speaker_range)
            joint_records(emit, jm, scene, args.reps, args.every_reps, only, args.link_radius)


if __name__ == "__main__":
    main()
