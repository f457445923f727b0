"""Non-maximum suppression over the lattice (``Prone_method="DENSE_NMS"``) on one MI355X: the numpy statement against
the kernel, and what the mode does to a search.  A script, not a test.

nms       ``dense_grid.lattice_local_maxima`` in numpy against ``dense_grid.lattice_local_maxima_device``
          (csrc/geometry_kernels.hip: the column-0 check, the upload of the scores, both kernels, the read-back of
          best and degree), radius 1, alternating in one run, median of 5 after one warm-up each, on three tables: the
          g7 lattice at width 8 (3 364 cubes of 6 pairs) and at width 4 (15 970), and the 16-microphone width-2 table
          of ``dense_tdoa_candidates`` (36 199 cubes of 15 pairs; the statement takes about a minute there and is
          timed once).  ``device_all_pairs_s`` is the same call at radius 2^30, where the range found in column 0 is
          the whole table: what the restriction to that range saves.
search    one ``JointModel.forward`` in DENSE_NMS mode next to one in DENSE mode (device-built array, FULL spot
          network, f16x3, no separation network) on the configs[2] scene, each after one warm-up forward: kept cubes,
          spot evaluations, talkers, stage times.

Appends one JSON line per record to profiles/lattice/perf_nms.jsonl (``--out``).  Nothing is asserted about the times.

    python tests/perf_lattice_nms.py [--skip-search] [--skip-large] [--out FILE]
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
from acousticswarms_speech_amd.config import FULL  # noqa: E402
from acousticswarms_speech_amd.dense_grid import (coarse_lattice, dense_tdoa_candidates, lattice_local_maxima,  # noqa: E402
                                                  lattice_local_maxima_device)
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.mic_array import MicArray  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.search import LATTICE_NMS_RADIUS  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_spot_state_dict  # noqa: E402

REPS = 5


def tables(large):
    g7 = np.load(os.path.join(ROOT, "tests", "golden", "g7_srp_map.npz"))
    with redirect_stdout(io.StringIO()):
        node = MicArray(g7["mics"], Spk_Range=list(g7["roi"])).SRP_node
    yield "g7 lattice, width 8", coarse_lattice(node, 8).cells, REPS
    yield "g7 lattice, width 4", coarse_lattice(node, 4).cells, REPS
    if large:
        sc = make_scene(1010, 5, 16, 4000)
        offs, _counts, _ = dense_tdoa_candidates(sc.mic_positions, sc.speaker_range, width=2, step=0.05, with_points=False)
        yield "16 microphones, dense_tdoa_candidates width 2", (offs // 2).astype(np.int32), 1


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def nms_records(emit, large):
    for name, cells, host_reps in tables(large):
        N, P = cells.shape
        scores = np.random.default_rng(N).standard_normal(N)
        cells_d = torch.from_numpy(np.ascontiguousarray(cells)).cuda()
        times = {"host": [], "device": [], "all_pairs": []}
        lattice_local_maxima_device(cells_d, scores, 1)                        # warm-up
        lattice_local_maxima_device(cells_d, scores, 1 << 30)
        for rep in range(REPS):
            if rep < host_reps:
                want, t = timed(lambda: lattice_local_maxima(cells, scores, 1))
                times["host"].append(t)
            got, t = timed(lambda: lattice_local_maxima_device(cells_d, scores, 1))
            times["device"].append(t)
            _, t = timed(lambda: lattice_local_maxima_device(cells_d, scores, 1 << 30))
            times["all_pairs"].append(t)
        same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
        h, d, a = (float(np.median(times[k])) for k in ("host", "device", "all_pairs"))
        emit({"record": "nms", "table": name, "cubes": int(N), "pairs": int(P), "radius": 1, "reps": REPS,
              "host_reps": host_reps, "maxima": int(np.sum(want[0] == np.arange(N))),
              "degree_min_median_max": [int(want[1].min()), float(np.median(want[1])), int(want[1].max())],
              "device_equals_host": same, "host_s": round(h, 4), "device_s": round(d, 6), "device_all_pairs_s": round(a, 6),
              "host_over_device": round(h / d, 1), "all_pairs_over_restricted": round(a / d, 2),
              "host_s_all": [round(t, 4) for t in times["host"]], "device_s_all": [round(t, 6) for t in times["device"]],
              "device_all_pairs_s_all": [round(t, 6) for t in times["all_pairs"]]})


def search_records(emit):
    sc = make_scene(1010, 5, 7, 48000, reverb=True)            # the configs[2] scene
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=256, precision="f16x3").to("cuda")
    mix = torch.from_numpy(sc.mix)
    for method in ("DENSE", "DENSE_NMS"):
        jm = JointModel(spot, None, device="cuda", geometry="device")
        with redirect_stdout(io.StringIO()):
            jm.setup(sc.mic_positions, sc.speaker_range, prone_method=method)
            jm.forward(mix)                                    # warm-up
            patches, _al, _a, _d0, _d1, spot_times = jm.forward(mix)
        mp = jm.Mic_processor
        rec = {"record": "search", "scene": "configs[2]: make_scene(1010, 5, 7, 48000, reverb=True)", "prone_method": method,
               "spot_network": "FULL, f16x3, batch 256, random weights", "lattice_cubes": mp.SRP_node.lattice.n_cubes,
               "coarse_candidates": int(mp.big_spotforming_times), "coarse_kept": len(mp.trace["coarse_kept"]),
               "fine_candidates": int(mp.spotforming_times), "spot_evaluations": int(spot_times), "talkers": len(patches),
               "stage_s": {k: round(float(t), 4) for k, t in zip(("stage1", "coarse", "fine", "clustering", "separation"),
                                                                 jm.times)},
               "search_s": round(float(sum(jm.times[:4])), 4)}
        if method == "DENSE_NMS":
            nms = mp.lattice_nms
            rec.update(radius=int(LATTICE_NMS_RADIUS), local_maxima=int(np.sum(nms["best"] == np.arange(len(nms["best"])))))
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice", "perf_nms.jsonl"))
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--skip-large", action="store_true", help="leave out the 36 199-cube table (a minute of numpy)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    nms_records(emit, not args.skip_large)
    if not args.skip_search:
        search_records(emit)


if __name__ == "__main__":
    main()
