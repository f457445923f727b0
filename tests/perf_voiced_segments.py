"""Voiced segments on the host against ``segments="device"`` on one MI355X.  A script, not a test.

heads     ``hostdsp.split_wav`` over the cluster heads of the bench scene (every waveform the global clustering of
          make_scene(1010, 5, 7, 48000, reverb=True) compares; FULL spot network, f16x3, random weights) against ONE
          ``torch.ops.asw.voiced_segments`` call on the same rows where the fine stage left them: device events
          around the op (``op_gpu_s``) and the wall time of the op plus the read-back of both tables (``op_s``).
search    one ``JointModel.forward`` per mode on that scene: the fine and the clustering stage.  In a single forward
          the host's ``split_wav`` calls hide behind the GPU, so the fine stage shows them only in part.
batch     ``shard.localize_batch`` on 16 five-speaker mixtures (seeds 2000-2015, one array) with ``concurrent`` = 2, 3
          and 4, per mode.
Everything alternates between the two modes within one run and is the median of ``--reps`` (5) after one warm-up;
``segments="host"`` in the same run is the yardstick.  Appends one JSON line per record to
profiles/segments/perf_segments.jsonl (``--out``).  Nothing is asserted about the times.

    python tests/perf_voiced_segments.py [--reps N] [--skip-batch] [--out FILE]
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
from acousticswarms_speech_amd import native  # noqa: E402
from acousticswarms_speech_amd.config import FULL  # noqa: E402
from acousticswarms_speech_amd.hostdsp import split_wav, voiced_margin_db  # noqa: E402
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.mic_array import MicArray  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.shard import localize_batch  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_spot_state_dict  # noqa: E402

MODES = ("host", "device")


def med(v):
    return round(float(np.median(v)), 6)


def models(spot, sc):
    out = {}
    for mode in MODES:
        jm = JointModel(spot, None, device="cuda", segments=mode)
        with redirect_stdout(io.StringIO()):
            jm.setup(sc.mic_positions, sc.speaker_range)
        out[mode] = jm
    return out


def search_and_heads(emit, spot, reps):
    sc = make_scene(1010, 5, 7, 48000, reverb=True)
    mix = torch.from_numpy(sc.mix)
    jms = models(spot, sc)
    heads = {}
    inner = MicArray.Clustering_new

    def recording(self, output_pair, *a, **kw):
        heads["host"] = [np.asarray(p[1]) for p in output_pair]
        heads["rows"] = [self._dev_cache[id(p[1])][1] for p in output_pair]
        return inner(self, output_pair, *a, **kw)
    MicArray.Clustering_new = recording
    try:
        with redirect_stdout(io.StringIO()):
            jms["host"].forward(mix)
    finally:
        MicArray.Clustering_new = inner
    waves_h, waves_d = heads["host"], torch.stack(heads["rows"])
    ops = native.torch_ops()
    ops.voiced_segments(waves_d)                                    # warm-up
    t_host, t_op, t_gpu = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        segs_h = [split_wav(w) for w in waves_h]
        t_host.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        seg, cnt, _ms = ops.voiced_segments(waves_d)
        e1.record()
        seg, cnt = seg.cpu().numpy(), cnt.cpu().numpy()
        t_op.append(time.perf_counter() - t0)
        t_gpu.append(e0.elapsed_time(e1) * 1e-3)
    same = sum([[int(a), int(b)] for a, b in s] == seg[i, :cnt[i]].tolist() for i, s in enumerate(segs_h))
    close = sum(voiced_margin_db(w) < 1e-3 for w in waves_h)
    emit({"record": "heads", "scene": "make_scene(1010, 5, 7, 48000, reverb=True)", "heads": len(waves_h), "T": 48000,
          "reps": reps, "split_wav_s": med(t_host), "op_s": med(t_op), "op_gpu_s": med(t_gpu),
          "split_wav_over_op": round(med(t_host) / med(t_op), 1), "heads_with_equal_segments": int(same),
          "heads_within_1e-3_dB_of_a_decision": int(close), "segments": int(cnt.sum()),
          "split_wav_s_all": [round(t, 5) for t in t_host], "op_s_all": [round(t, 6) for t in t_op]})

    times = {m: [] for m in MODES}
    talkers = {}
    with redirect_stdout(io.StringIO()):
        for m in MODES:
            jms[m].forward(mix)                                     # warm-up
        for _ in range(reps):
            for m in MODES:
                patches = jms[m].forward(mix)[0]
                talkers[m] = [p[3] for p in patches]
                times[m].append(list(jms[m].times[:4]))
    rec = {"record": "search", "scene": "make_scene(1010, 5, 7, 48000, reverb=True)", "reps": reps,
           "same_talkers": talkers["host"] == talkers["device"], "talkers": len(talkers["host"])}
    for m in MODES:
        t = np.array(times[m])
        rec[m] = {"fine_s": med(t[:, 2]), "clustering_s": med(t[:, 3]), "search_s": med(t.sum(axis=1)),
                  "clustering_s_all": [round(float(v), 5) for v in t[:, 3]]}
    emit(rec)


def batch_records(emit, spot, reps, n_mix=16):
    sc0 = make_scene(2000, 5, 7, 48000)
    mixes = [torch.from_numpy(make_scene(2000 + i, 5, 7, 48000, mic_positions=sc0.mic_positions).mix) for i in range(n_mix)]
    jms = models(spot, sc0)
    with redirect_stdout(io.StringIO()):
        for m in MODES:
            localize_batch(jms[m], mixes[:4], concurrent=2)         # warm-up
    for concurrent in (2, 3, 4):
        times = {m: [] for m in MODES}
        names = {}
        for _ in range(reps):
            for m in MODES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with redirect_stdout(io.StringIO()):
                    out = localize_batch(jms[m], mixes, concurrent=concurrent)
                torch.cuda.synchronize()
                times[m].append(time.perf_counter() - t0)
                names[m] = [list(r["names"]) for r in out]
        emit({"record": "batch", "mixtures": n_mix, "T": 48000, "concurrent": concurrent, "reps": reps,
              "mixtures_with_the_same_talkers": sum(a == b for a, b in zip(names["host"], names["device"])),
              "host_mixtures_per_s": round(n_mix / med(times["host"]), 3),
              "device_mixtures_per_s": round(n_mix / med(times["device"]), 3),
              "host_s_all": [round(t, 3) for t in times["host"]], "device_s_all": [round(t, 3) for t in times["device"]]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments", "perf_segments.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-batch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=256, precision="f16x3").to("cuda")
    search_and_heads(emit, spot, args.reps)
    if not args.skip_batch:
        batch_records(emit, spot, args.reps)


if __name__ == "__main__":
    main()
