"""Outputs of the small kernels and of the entry points built on them, for a byte-for-byte comparison between two
builds of the library (a refactor against its parent commit).  A script, not a test: with fixed seeds it calls through
``ops.py`` and the two models on one MI355X and writes every result into one ``.npz``; it compares against nothing.
Run it once in each checkout, each in a fresh process, and compare the two files array by array.

    python tests/dump_small_kernels.py OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acousticswarms_speech_amd import native, ops  # noqa: E402
from acousticswarms_speech_amd.config import SEP_SMALL, SMALL  # noqa: E402
from acousticswarms_speech_amd.scenes import make_scene  # noqa: E402
from acousticswarms_speech_amd.sep import SepModel  # noqa: E402
from acousticswarms_speech_amd.spot import SpotModel  # noqa: E402
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
_seed = [100]


def rand(*shape, scale=1.0):
    _seed[0] += 1
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(_seed[0])) * scale).cuda()


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def kernels(out):
    for rows, N in ((5, 256), (7, 1024)):
        x, r, g, b = rand(rows, N, scale=2.0), rand(rows, N), 1 + 0.2 * rand(N), 0.1 * rand(N)
        out[f"add_layernorm_{rows}x{N}"] = ops.add_layernorm(x, r, g, b)
    for N in (100, 512):
        x, y, g, b = rand(37, N), rand(37, N), 1 + 0.1 * rand(N), 0.1 * rand(N)
        s, o = ops.add_layernorm2(x, y, 0.5, g, b, want_sum=True)
        out[f"add_layernorm2_sum_N{N}"], out[f"add_layernorm2_ln_N{N}"] = s, o
        out[f"add_layernorm2_alpha1_N{N}"] = ops.add_layernorm2(x, y, 1.0, g, b)[1]
        out[f"add_layernorm2_no_y_swish_N{N}"] = ops.add_layernorm2(x, None, 0.0, g, b, eps=1e-6, act=2)[1]
        out[f"add_layernorm2_sum_only_N{N}"] = ops.add_layernorm2(x, y, 0.25, want_sum=True, want_ln=False)[0]
    for NB, S, L, d, H in ((2, 3, 5, 128, 8), (1, 27, 2, 512, 8), (70, 2, 1, 128, 8)):
        out[f"inter_attention_{NB}x{S}x{L}x{d}"] = ops.inter_attention(rand(NB, S, L, 3 * d, scale=0.7), H)
    for counts in ([1, 3, 2], [40, 24]):                                 # [40, 24]: two LDS regions per workgroup
        qkv = rand(sum(counts), 2, 3 * 512, scale=0.7)
        out["inter_attention_groups_" + "_".join(map(str, counts))] = ops.inter_attention_groups(qkv, counts, 8)
    mix = torch.from_numpy(make_scene(4, 3, 7, 4000).mix).cuda()
    mix2 = torch.from_numpy(make_scene(5, 2, 7, 4000).mix).cuda()
    offs = np.array([[0, 0, 0, 0, 0, 0], [131, -131, 7, -7, 64, -64], [2500, -2500, 3999, -3999, 4000, -4100],
                     [17, -3, 8, 0, -12, 40]], dtype=np.int32)
    for S in (1, 4):
        out[f"joint_shift_stats_S{S}_mean"], out[f"joint_shift_stats_S{S}_std"] = ops.joint_shift_stats(mix, i32(offs[:S]))
    m, s = ops.joint_shift_stats_groups(torch.stack([mix, mix2]).contiguous(), i32(np.concatenate([offs[:3], offs[1:]])), [3, 3])
    out["joint_shift_stats_groups_mean"], out["joint_shift_stats_groups_std"] = m, s
    qkv = rand(2, 70, 3 * 256, scale=0.7)
    for precision in ("f32", "f16x3", "f16"):
        out[f"attention_{precision}_L70_hd128"] = ops.attention(qkv, 2, precision=precision)
    L, d, H = 70, 128, 2
    out["relpos_attention_L70_hd64"] = ops.relpos_attention(rand(2, L, 3 * d, scale=0.7), rand(2 * L - 1, d, scale=0.7),
                                                            rand(d, scale=0.3), rand(d, scale=0.3), H, 1.0 / d ** 0.5)
    # attention over time, every kernel of csrc/attention.hip: the short MFMA kernels at 1, 3 and 5 key tiles and their
    # last length (320), the flash kernel from its first length (321); the VALU kernel at head_dim 16, 32, 48, 64 and
    # 1, 2, 3 key tiles of 128; rel-pos on VALU (head_dim 16, 32) and MFMA (64): one tile, exactly one, a ragged tail, four
    for L in (5, 64, 188, 320, 321, 563):
        qkv = rand(2, L, 3 * 256, scale=0.7)
        for precision in ("f32", "f16x3", "f16"):
            out[f"attention_{precision}_L{L}_hd128"] = ops.attention(qkv, 2, precision=precision)
    for d in (128, 256, 96, 512):
        for L in (5, 130, 300):
            out[f"attention_f32_L{L}_hd{d // (2 if d == 96 else 8)}"] = ops.attention(rand(2, L, 3 * d, scale=0.7), 2 if d == 96 else 8)
    for d in (128, 256, 512):
        for L in (5, 64, 70, 200):
            out[f"relpos_attention_L{L}_hd{d // 8}"] = ops.relpos_attention(
                rand(2, L, 3 * d, scale=0.7), rand(2 * L - 1, d, scale=0.7), rand(d, scale=0.3), rand(d, scale=0.3), 8, 1.0 / d ** 0.5)
    for T in (4000, 4001):
        y = rand(5, T) + 0.1
        out[f"energies_T{T}_w1000"] = ops.energies(y, 1000)
        out[f"energies_T{T}_w333"] = ops.energies(y, 333)
        out[f"center_rows_T{T}"] = native.torch_ops().center_rows_(y.clone())
        mixT = rand(7, T, scale=0.1)
        for circular in (True, False):
            mu, sg = ops.shift_stats(mixT, i32(offs), circular=circular)
            out[f"shift_stats_T{T}_circular{int(circular)}_mean"], out[f"shift_stats_T{T}_circular{int(circular)}_std"] = mu, sg


def models(out):
    g = np.load(os.path.join(GOLDEN, "g11b_sep_infer_small.npz"))
    gd = np.load(os.path.join(GOLDEN, "g11d_sep_forward_ragged.npz"))
    mix = make_scene(4, 3, 7, 4000).mix
    mix2 = make_scene(5, 2, 7, 4000).mix
    samples = [list(g[f"samples{i}"]) for i in range(3)]
    spot_offs = [np.array([0, 0, 0, 0, 0, 0]), np.array([3, -5, 8, -13, 21, -34]), np.array([-40, 30, -20, 10, -5, 2])]
    for precision in ("f32", "f16x3"):
        sep = SepModel(SEP_SMALL, make_sep_state_dict(SEP_SMALL, 31), precision=precision).to("cuda")
        for i, s in enumerate(samples):
            out[f"sep_infer_sample_{precision}_{i}"] = sep.infer_sample(torch.from_numpy(mix), s)
        rows = sep.infer_batch([mix, mix2, mix], [samples[2], [], samples[0]])
        for k, r in enumerate(rows):
            out[f"sep_infer_batch_{precision}_{k}"] = r
        out[f"sep_infer_batch_one_item_{precision}"] = sep.infer_batch([mix], [samples[1]])[0]
        counts = [int(c) for c in gd["counts_a"]]
        x = torch.from_numpy(np.random.default_rng(900 + 2100).standard_normal((len(counts), 21, 2100)).astype(np.float32))
        out[f"sep_forward_counts_{precision}"] = sep(x, torch.tensor(counts).view(-1, 1))
        spot = SpotModel(SMALL, make_spot_state_dict(SMALL, 3), batch_size=2, precision=precision).to("cuda:0")
        for strict in (0, 1):
            out[f"spot_shift_and_sep_{precision}_strict{strict}"] = spot.shift_and_sep(torch.from_numpy(mix), spot_offs, Strict=strict)
        out[f"spot_shift_and_score_{precision}"] = spot.shift_and_score(torch.from_numpy(mix), spot_offs, Strict=1, window=1000)


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out = {}
    kernels(out)
    models(out)
    torch.cuda.synchronize()
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez(sys.argv[1], **arrays)
    print(f"{len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
