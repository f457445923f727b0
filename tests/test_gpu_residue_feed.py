"""The A feed of the pipelined f16x3 tiles (ResidueA, csrc/f16x3_tile.h; pipe_mainloop, csrc/pipegemm.hip: one stage
loop, two walks).  On the residue walk, strided convolutions with taps > stride deposit every input row once per tile and
run all the taps that read it from one LDS image; every other shape, and every shape under ASW_NO_RESIDUE_FEED, takes
the chunk walk of the same loop, one tap per image -- with the skip operand, the gate tensor or a dilation, which the
residue walk never sees.  Mask path and convolutions against torch float64 on the CPU of the same fp32
inputs, at the bar tests/test_gpu_kernels.py holds these kernels to (relative l2 error < 3e-6; single-pass f16 mode:
2e-3, its bar in tests/test_gpu_f16x3.py), full and ragged tiles, both feeds (ASW_NO_RESIDUE_FEED=1 in a child process).

The dispatcher sends a convolution to the pipelined tiles only when batch x tiles >= 512 and a 256-row tile wastes
less than 10 % more rows than a 192-row one, so the shapes with B = 2 and M_out around 300 check whatever kernel that
shape reaches (the 128 x 128 two-barrier tile today) and run none of the residue feed's code: they are kept as the
shapes the feed was specified with, not as coverage of it.  The B = 256, M_out = 500 shapes are the ones that reach
convgemm16p and its residue feed, and the two mask-path shapes reach the mask path's: the launch name in the detailed
profile confirms the kernel and, by its " res" tag, the feed, in the default process and in the child without it.  Their batch repeats four distinct items, so the
float64 reference is four items' worth of work and every one of the 256 outputs is still compared."""
import ctypes
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

BAR = {"f16x3": 3e-6, "f16": 2e-3}


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _relerr(a, b):                       # the definition of tests/test_gpu_kernels.py
    a = a.double().flatten()
    b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _launch_names(fn):
    """fn() under the detailed launch profile -> (its result, the launch names)"""
    from acousticswarms_speech_amd import native
    L = native.lib()
    L.asw_profile_enable(2)
    try:
        out = fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        native.check(L.asw_profile_report(buf, len(buf)))
    finally:
        L.asw_profile_enable(0)
    return out, list(json.loads(buf.value.decode()))


def _assert_feed(names, prefix, applies=True):
    """The detailed launch name says which feed ran: "... s<stride> res]" on the residue-image feed, "... s<stride>]"
    on the chunk-per-tap one.  Where the residue feed applies to the shape it must have run unless the process was
    started with ASW_NO_RESIDUE_FEED, and then it must not have; where it does not apply it must not have run."""
    mine = [n for n in names if n.startswith(prefix)]
    assert mine, names
    want_res = applies and "ASW_NO_RESIDUE_FEED" not in os.environ
    for n in mine:
        assert n.endswith(" res]") == want_res, (n, want_res)


# ---------------------------------------------------------------- mask path
MASK = {"full_tile": dict(B=2, E=256, Tp=4096),            # 256 frames: exactly one full tile, zero left padding
        "ragged_two_columns": dict(B=1, E=512, Tp=4800)}   # 300 frames: phantom frames of tile 1 read real rows
_mask_ref = {}


def _mask_reference(name):
    """inputs and the float64 reference of one mask-path case, computed once"""
    if name not in _mask_ref:
        c = MASK[name]
        B, E, Tp, C, EK, ES = c["B"], c["E"], c["Tp"], 64, 33, 16
        x, ref = _rand(B, C, Tp, seed=40), _rand(B, 1, Tp, seed=41)
        wb, bb = _rand(E, 1, EK, seed=42, scale=0.2), _rand(E, seed=43, scale=0.1)
        wm, bm = _rand(E, C, EK, seed=44, scale=1 / math.sqrt(C * EK)), _rand(E, seed=45, scale=0.1)
        wd, bd = _rand(E, 1, EK, seed=46, scale=1 / math.sqrt(E)), 0.05
        d = torch.float64
        y = F.relu(F.conv1d(ref.to(d), wb.to(d), bb.to(d), stride=ES, padding=EK // 2))
        mask = F.relu(F.conv1d(x.to(d), wm.to(d), bm.to(d), stride=ES, padding=EK // 2))
        lat = y * mask
        t = Tp - 100
        full = F.conv_transpose1d(lat, wd.to(d), torch.tensor([bd], dtype=d), stride=EK // 2)
        _mask_ref[name] = dict(c, x=x, ref=ref, wb=wb, bb=bb, wm=wm, bm=bm, wd=wd, bd=bd, frames=lat.shape[-1], t=t,
                               taps_want=torch.einsum("bef,ej->bfj", lat, wd[:, 0].to(d)),
                               want=full[..., 9:-8][..., -t:][:, 0])
    return _mask_ref[name]


def _run_mask(name, precision):
    from acousticswarms_speech_amd import ops
    r = _mask_reference(name)
    B, Tp, E, EK, ES, Fr = r["B"], r["Tp"], r["E"], 33, 16, r["frames"]
    assert Fr == {"full_tile": 256, "ragged_two_columns": 300}[name]
    RL = EK // 2 + Tp + 64 + 64
    refx = torch.zeros(B, RL)
    refx[:, EK // 2:EK // 2 + Tp] = r["ref"][:, 0]
    xc = r["x"].transpose(1, 2).contiguous().cuda()
    ops.f16x3_overflow_count(reset=True)
    parts, names = _launch_names(lambda: ops.mask_path(xc, refx.cuda(), ES, r["wm"], r["bm"].cuda(), r["wb"], r["bb"].cuda(),
                                                        r["wd"], Fr, ES, EK // 2, precision=precision))
    _assert_feed(names, "maskpath16p<256,256,32>")
    assert parts.shape == (E // 256, B, Fr, 64)
    out = ops.overlap_add_parts(parts, EK, EK // 2, r["t"], 9, 8, r["bd"])
    return {"taps": _relerr(parts.sum(0)[..., :EK].cpu(), r["taps_want"]), "decode": _relerr(out.cpu(), r["want"]),
            "overflow": ops.f16x3_overflow_count(reset=True)}


# ---------------------------------------------------------------- convolutions
# C, N, taps, stride, M_out, B, distinct items, stats, expected launch-name prefix (None: whatever the shape reaches)
# and what the shapes of the chunk walk alone add ({}: nothing): dil, skip (a second input added on load), gate (a tensor
# the output is multiplied by)
CONV = {
    "k7s4_M296_B2": (128, 256, 7, 4, 296, 2, 2, True, None, {}),
    "k5s4_M270_B2": (128, 256, 5, 4, 270, 2, 2, True, None, {}),
    "k5s2_M300_B2": (128, 256, 5, 2, 300, 2, 2, True, None, {}),
    # the shapes that reach the pipelined tiles: two row tiles per item, the second ragged (244 frames of 256)
    "k7s4_M500_B256": (128, 256, 7, 4, 500, 256, 4, True, "convgemm16p<256,256,32,stats>", {}),
    "k7s4_M500_B256_plain": (128, 256, 7, 4, 500, 256, 4, False, "convgemm16p<256,256,32,plain>", {}),   # range guard live
    "k5s4_M500_B256": (128, 256, 5, 4, 500, 256, 4, True, "convgemm16p<256,256,32,stats>", {}),
    "k5s2_M500_B256": (128, 256, 5, 2, 500, 256, 4, True, "convgemm16p<256,256,32,stats>", {}),         # three taps on one image
    "k7s4_C64_M500_B256": (64, 256, 7, 4, 500, 256, 4, True, "convgemm16p<128,256,32,stats>", {}),      # K <= 512: 4-wave tile
    # the chunk walk where the residue walk never applies (the last 128- or 256-row tile ragged as above): the decoder's
    # transposed convolution (one tap, skip operand, statistics), the gated linear, a dilated stride-1 convolution
    "k1_skip_C256_M500_B256": (256, 256, 1, 1, 500, 256, 4, True, "convgemm16p<128,256,32,stats>", dict(skip=True)),
    "k1_gate_C1024_M500_B256": (1024, 256, 1, 1, 500, 256, 4, False, "convgemm16pm<256,256,32,plain>", dict(gate=True)),
    "k3d2_M500_B256": (128, 256, 3, 1, 500, 256, 4, True, "convgemm16p<128,256,32,stats>", dict(dil=2)),
}


def _conv_row(name):
    *row, extra = CONV[name]
    return (*row, dict(dict(dil=1, skip=False, gate=False), **extra))


_conv_ref = {}


def _conv_reference(name):
    if name not in _conv_ref:
        C, N, K, s, M, B, nd, stats, _, o = _conv_row(name)
        pad = o["dil"] * (K // 2)
        T = (M - 1) * s + 1 + o["dil"] * (K - 1) - 2 * pad  # the shortest input with M output frames
        T += s - 1                                          # ... and the longest: rows past the last tap exist
        x = _rand(nd, C, T, seed=60)
        w = _rand(N, C, K, seed=61, scale=1 / math.sqrt(C * K))
        b = _rand(N, seed=62, scale=0.1)
        x2 = _rand(nd, C, T, seed=63) if o["skip"] else None
        gate = _rand(nd, M, N, seed=64) if o["gate"] else None
        xin = x.double() + x2.double() if o["skip"] else x.double()
        want = F.conv1d(xin, w.double(), b.double(), stride=s, padding=pad, dilation=o["dil"]).transpose(1, 2).contiguous()
        assert want.shape == (nd, M, N)
        if o["gate"]:
            want = want * gate.double()
        _conv_ref[name] = dict(x=x, w=w, b=b, x2=x2, gate=gate, pad=pad, want=want)
    return _conv_ref[name]


def _run_conv(name, precision):
    from acousticswarms_speech_amd import ops
    C, N, K, s, M, B, nd, stats, prefix, o = _conv_row(name)
    r = _conv_reference(name)

    def items(t):                                           # item b = distinct item b % nd
        return None if t is None else t.cuda().repeat(B // nd, 1, 1)
    xc = items(r["x"].transpose(1, 2).contiguous())
    x2c = items(None if r["x2"] is None else r["x2"].transpose(1, 2).contiguous())
    gc = items(r["gate"])
    wt = ops.pack_conv_weight(r["w"]).cuda()
    ops.f16x3_overflow_count(reset=True)
    (out, st), names = _launch_names(lambda: ops.convgemm(xc, wt, M, N, C, taps=K, stride=s, dil=o["dil"], pad=r["pad"],
                                                           bias=r["b"].cuda(), A2=x2c, mul=gc,
                                                           stats_chan_mod=N if stats else 0, precision=precision))
    if prefix is not None:
        assert any(n.startswith(prefix) for n in names), names
        _assert_feed(names, prefix, applies=K > s >= 2)
    want = r["want"].cuda()
    diff = out.view(B // nd, nd, M, N).double() - want
    fig = {"rel": float(diff.norm() / (want.norm() * math.sqrt(B // nd))), "overflow": ops.f16x3_overflow_count(reset=True)}
    if stats:
        # partial sums (sum | sum of squares) x (first | second half of the channels), over the valid frames only
        got = st.double().sum(1).view(B // nd, nd, 4)
        h = N // 2
        ref = torch.stack([want[..., :h].sum((1, 2)), (want[..., :h] ** 2).sum((1, 2)),
                           want[..., h:].sum((1, 2)), (want[..., h:] ** 2).sum((1, 2))], dim=1)
        fig["stats_sq"] = float(((got[..., 1::2] - ref[:, 1::2]).abs() / ref[:, 1::2]).max())
        fig["stats_sum"] = float(((got[..., 0::2] - ref[:, 0::2]).abs() / (1e-2 + 1e-5 * ref[:, 0::2].abs())).max())
    return fig


def _check(fig, precision, what):
    print(f"residue feed {what} {precision}: {fig}")
    for k in ("taps", "decode", "rel"):
        if k in fig:
            assert fig[k] < BAR[precision], (what, k, fig)
    if precision == "f16x3":
        assert fig["overflow"] == 0, (what, fig)
        # Statistics are fp32 sums of M * N / 2 outputs whose own error is the bar above: squares to 1e-5 relative,
        # the plain sum (it cancels: a bias-sized mean) to 1e-2 + 1e-5 |sum| -- the bounds test_pipelined_wide_tiles_f16x3
        # sets for the same epilogue; stats_sum is the error as a fraction of that.  A phantom frame counted in
        # would add about 1 / M_out, 2e-3 and more.
        if "stats_sq" in fig:
            assert fig["stats_sq"] < 1e-5 and fig["stats_sum"] < 1.0, (what, fig)


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("name", list(MASK))
def test_mask_path_residue_feed(name, precision):
    _check(_run_mask(name, precision), precision, "mask " + name)


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("name", list(CONV))
def test_strided_conv_residue_feed(name, precision):
    _check(_run_conv(name, precision), precision, "conv " + name)


def _all_f16x3():
    out = {"mask " + n: _run_mask(n, "f16x3") for n in MASK}
    out.update({"conv " + n: _run_conv(n, "f16x3") for n in CONV})
    return out


def test_both_feeds_inside_the_bar():
    """Every shape once more on the chunk-per-tap feed (ASW_NO_RESIDUE_FEED=1 is read once per process: a fresh child;
    it takes under 3 s on an MI355X with the float64 references of all eleven rows, the limit of 300 s is for a cold start).
    The two feeds add the K terms in different orders, so they are not compared bit for bit; each is held to the bar."""
    env = dict(os.environ, ASW_NO_RESIDUE_FEED="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    figs = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(figs) == {"mask " + n for n in MASK} | {"conv " + n for n in CONV}
    for what, fig in figs.items():
        _check(fig, "f16x3", what + " [chunk-per-tap feed]")


if __name__ == "__main__":
    assert os.environ.get("ASW_NO_RESIDUE_FEED") == "1"
    print(json.dumps(_all_f16x3()))
