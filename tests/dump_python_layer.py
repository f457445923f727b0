"""Results of the Python layer above the C ABI -- the two models, the search under ``JointModel.forward`` and
``localize_batch``, the device helpers -- for a byte-for-byte comparison between two states of that layer (a refactor
against its parent commit, on one build of the library).  A script, not a test, in the manner of
``dump_small_kernels.py``: fixed seeds, one ``.npz``, compares against nothing.  Run it once in each checkout, each in a
fresh process, and compare the two files array by array.  The arrays named ``batched2_*`` come from
``localize_batch(concurrent=2)``, which is not bit-reproducible from run to run (two runs share their launches
differently): names and ``spot_times`` equal, centres within 1e-6.

    python tests/dump_python_layer.py OUT.npz
"""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd.config import FULL, SEP_SMALL  # noqa: E402
from acousticswarms_speech_amd.joint import JointModel  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.sep import SepModel  # noqa: E402
from acousticswarms_speech_amd.shard import localize_batch  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict  # noqa: E402

T = 24000
TAP_FLOATS = 1 << 16      # of a tap, which is as large as the last internal batch, the first 256 KB are kept
DEVICE_MODES = dict(geometry="device", segments="device", clustering="device", global_clustering="device", coarse="device")


def text(obj):
    return np.array(json.dumps(obj, sort_keys=True, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o)))


def forward(out, tag, jm, mix):
    patches, audio_loc, audio, _d0, _d1, spot_times = jm.forward(mix)
    out[f"{tag}_names"] = text([p[3] for p in patches])
    out[f"{tag}_centres"] = np.array([p[0].center_pos() for p in patches]).reshape(-1, 3)
    out[f"{tag}_powers"] = np.array([p[2] for p in patches])
    out[f"{tag}_spot_times"] = np.array(spot_times)
    out[f"{tag}_head_audio"] = np.asarray(audio_loc)
    out[f"{tag}_separated"] = np.zeros((0, T), dtype=np.float32) if audio is None else np.asarray(audio)
    out[f"{tag}_trace"] = text(jm.Mic_processor.trace)


def batch(out, tag, results):
    for k, r in enumerate(results):
        out[f"{tag}_{k}_names"] = text(list(r["names"]))
        out[f"{tag}_{k}_spot_times"] = np.array(r["spot_times"])
        out[f"{tag}_{k}_centres"], out[f"{tag}_{k}_powers"] = r["centres"], r["powers"]
        if "audio" in r:
            out[f"{tag}_{k}_audio"] = r["audio"]


def helpers(out, spot, jm, mix):
    """the nine device helpers on the head rows the fine stage returns for mixture 0"""
    mp = jm.Mic_processor
    mix_dev = mix.cuda()
    p1, _ = mp.Apply_SRP_PHAT(mix)
    pairs = mp.Spotform_Small_Patch_Parallel(mix_dev, mp.Spotform_Big_Patch(mix_dev, p1, spot), spot)
    rows = np.stack([np.asarray(p[1].cpu() if torch.is_tensor(p[1]) else p[1], dtype=np.float32) for p in pairs])[:12]
    n = rows.shape[0]
    waves = torch.from_numpy(rows).cuda()
    seg_tab, cnt = spot.voiced_segments(waves)
    lists = [[tuple(int(v) for v in ab) for ab in row[:c]] for row, c in zip(seg_tab.cpu().numpy(), cnt.cpu().numpy())]
    full = spot.pair_sisdr_device(waves)
    seg_res = spot.segment_sisdr_resident(waves, seg_tab, cnt)
    w64 = waves.double()
    en = torch.stack([(w64 * w64).sum(dim=1), (w64 * w64).mean(dim=1).sqrt()], dim=1).contiguous()
    gate = np.full(n, 0.25 * float(en[:, 0].max()))
    dis1 = torch.linspace(1.0, 2.0, n, dtype=torch.float64).cuda()
    got = {"head_rows": rows, "voiced_segments": spot.voiced_segments(waves), "pair_sisdr": spot.pair_sisdr(waves),
           "pair_sisdr_device": full, "segment_sisdr": spot.segment_sisdr(waves, lists),
           "segment_sisdr_device": spot.segment_sisdr_device(waves, seg_tab, cnt), "segment_sisdr_resident": seg_res,
           "fine_clusters": spot.fine_clusters(waves, [0, n // 2, n], en, gate, [gate[0], gate[0]], 0.5),
           "global_clusters": spot.global_clusters(full, seg_res, cnt, np.eye(n, dtype=np.uint8)),
           "coarse_select": spot.coarse_select(en, dis1, cap=8)}
    for name, value in got.items():
        for i, v in enumerate(value if isinstance(value, tuple) else (value,)):
            out[f"helper_{name}_{i}"] = v


def sep_calls(out, sep, mixes):
    offs = [np.array([3, -5, 8, -13, 21, -34]), np.array([-40, 30, -20, 10, -5, 2])]
    out["sep_infer_sample"] = sep.infer_sample(mixes[0], offs)
    for k, rows in enumerate(sep.infer_batch([mixes[0], mixes[1]], [offs, offs[:1]])):
        out[f"sep_infer_batch_{k}"] = rows
    x = torch.from_numpy(np.random.default_rng(77).standard_normal((2, 14, 2100)).astype(np.float32))
    out["sep_forward_counts_2_1"] = sep(x, torch.tensor([2, 1]).view(-1, 1))
    out["sep_tap_enc0"] = sep.get_tap("enc0")[:TAP_FLOATS]


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out = {}
    first = make_scene(2000, 5, 7, T)
    scenes = [make_scene(2000 + k, 5, 7, T, mic_positions=first.mic_positions) for k in range(4)]
    mixes = [torch.from_numpy(s.mix) for s in scenes]
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")
    sep = SepModel(SEP_SMALL, make_sep_state_dict(SEP_SMALL, 31), precision="f16x3").to("cuda")
    with redirect_stdout(io.StringIO()):
        jm = JointModel(spot, sep, device="cuda")
        jm.setup(first.mic_positions, first.speaker_range)
        forward(out, "host", jm, mixes[0])
        out["spot_tap_enc0"] = spot.get_tap("enc0")[:TAP_FLOATS]
        batch(out, "loop1", localize_batch(jm, mixes, concurrent=1, separate=True))
        batch(out, "batched2", localize_batch(jm, mixes, concurrent=2))
        helpers(out, spot, jm, mixes[0])
        jd = JointModel(spot, sep, device="cuda", **DEVICE_MODES)
        jd.setup(first.mic_positions, first.speaker_range, prone_method="DENSE_NMS")
        forward(out, "device", jd, mixes[0])
    sep_calls(out, sep, mixes)
    torch.cuda.synchronize()
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez(sys.argv[1], **arrays)
    print(f"{len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
