"""The full-rate decoder upsampling fused into the residual stack that feeds it (csrc/resstack.hip, UP): the last layer
of a 64-channel stack adds the skip rows to its LayerNorm rows in registers, applies the next decoder block's 64 -> 64
channel stride-2 transposed convolution and writes the raw rows and their GroupNorm partial sums; its own output is
never written.

Kernel level: the fused launch against the two separate launches (asw_resstack64_f16x3, then asw_convgemm_f32 with the
skip added on load) on the same inputs, both measured against the same chain in torch float64 on the CPU.  The bar is
relative: the fused relative L2 error may exceed the separate path's own by at most 1.5 x (the order of the sum over K
changes, so no bit identity), and the four finalised GroupNorm statistics agree with the separate path's to 1e-6
relative.  Network level: SMALL, 8 candidates, energies with the fusion on against off below 1e-5 relative.
Needs an MI355X."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
C, K, B = 64, 7, 2


def _log(msg):
    print(msg)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


# name -> (T, dilations, GroupNorm + GLU on load)
CASES = {
    # 96 rows per phase: the polyphase single layer (two phases per tile); T is no multiple of 49, 32 or the tile:
    # partly empty fragments, a short last phase, rows past the end
    "poly": (4737, (49,), False),
    "contiguous": (300, (1,), False),
    "pair": (500, (1, 7), False),
    "pair-glu": (500, (1, 7), True),
    # the other two polyphase widths (the row bookkeeping of all three goes through one row map, csrc/resstack.hip):
    # 48 rows per phase, the smallest length that still takes the polyphase form: four phases per tile, a short last
    # phase, rows past the end
    "poly4": (2357, (49,), False),
    # 224 rows per phase, the smallest length with one phase per tile
    "poly1": (10987, (49,), False),
}
_CACHE = {}


def _case(name):
    """inputs, the float64 reference and the separate path's result of a case, made once"""
    if name in _CACHE:
        return _CACHE[name]
    from acousticswarms_speech_amd import ops
    T, dils, glu = CASES[name]
    seed = 100 * (1 + list(CASES).index(name))
    layers = [(_rand(C, C, K, seed=seed + 10 * i, scale=1.0 / math.sqrt(C * K)), _rand(C, seed=seed + 10 * i + 1, scale=0.1),
               1 + _rand(C, seed=seed + 10 * i + 2, scale=0.1), _rand(C, seed=seed + 10 * i + 3, scale=0.1), d)
              for i, d in enumerate(dils)]
    skip = _rand(B, T, C, seed=seed + 50)
    up_w = _rand(C, 2 * C, 2, seed=seed + 51, scale=1.0 / math.sqrt(C))        # ConvTranspose1d weight [Cin][2 Cout][stride]
    # The bias has a mean well away from zero, as the raw rows in front of a GroupNorm have.  A bound RELATIVE to a group
    # mean says something about the code only where that mean is resolved: with zero-mean biases the gate half of the
    # contiguous case came out at a mean of 5e-4 (rms 1), and the 9e-10 by which the two paths' fp32 partial sums then
    # differ -- rounding, the separate path's as much as the fused one's -- read as 1.8e-6 "relative".  The difference
    # is also bounded in units of the group's rms below, where no mean can be small.
    up_b = 0.5 + _rand(2 * C, seed=seed + 52, scale=0.1)
    wt = up_w.permute(2, 1, 0).reshape(4 * C, C).contiguous()                   # Wt[r * 128 + n][c]
    bb = up_b.repeat(2).contiguous()
    if glu:
        raw_in = _rand(B, T, 2 * C, seed=seed + 53)
        mr = torch.tensor([[0.05, 0.9, -0.1, 1.2], [-0.02, 1.1, 0.07, 0.8]])
        gg, gb = 1 + _rand(2 * C, seed=seed + 54, scale=0.1), _rand(2 * C, seed=seed + 55, scale=0.1)
        r64 = raw_in.double()
        a = (r64[..., :C] - mr[:, 0, None, None].double()) * mr[:, 1, None, None].double() * gg[:C].double() + gb[:C].double()
        g = (r64[..., C:] - mr[:, 2, None, None].double()) * mr[:, 3, None, None].double() * gg[C:].double() + gb[C:].double()
        x64 = (a * torch.sigmoid(g)).transpose(1, 2)
        x_dev, glu_dev = None, (raw_in.cuda(), mr.cuda(), gg.cuda(), gb.cuda())
    else:
        x = _rand(B, T, C, seed=seed + 53)
        x64 = x.double().transpose(1, 2)
        x_dev, glu_dev = x.cuda(), None
    # float64: LayerNorm layers, + skip, transposed convolution; raw row t = output frames 2 t, 2 t + 1
    for w, b, g, be, d in layers:
        y = F.relu(F.conv1d(x64, w.double(), b.double(), dilation=d, padding=d * (K - 1) // 2)) + x64
        x64 = F.layer_norm(y.transpose(1, 2), (C,), g.double(), be.double(), 1e-5).transpose(1, 2)
    up = F.conv_transpose1d(x64 + skip.double().transpose(1, 2), up_w.double(), up_b.double(), stride=2)
    want = up.transpose(1, 2).reshape(B, T, 4 * C).contiguous()
    dev_layers = [(ops.pack_conv_weight(w).cuda(), b.cuda(), g.cuda(), be.cuda(), d) for w, b, g, be, d in layers]
    args = dict(layers=dev_layers, wt=wt.cuda(), bb=bb.cuda(), skip=skip.cuda(), x=x_dev, glu=glu_dev, T=T)
    # the separate path: the stack, then the one-tap GEMM with the skip added on load and the partial sums
    xs = ops.resstack(x_dev, dev_layers, taps=K, glu=glu_dev)
    raw_sep, st_sep = ops.convgemm(xs, args["wt"], T, 4 * C, C, bias=args["bb"], A2=args["skip"], stats_chan_mod=2 * C,
                                   precision="f16x3")
    mr_sep = ops.gn_finalize(st_sep, 2 * T, C)
    torch.cuda.synchronize()
    _CACHE[name] = (args, want, raw_sep.cpu(), mr_sep.cpu())
    return _CACHE[name]


def _fused(args):
    from acousticswarms_speech_amd import ops
    raw, st = ops.resstack_up(args["x"], args["layers"], args["wt"], args["bb"], args["skip"], taps=K, glu=args["glu"])
    mr = ops.gn_finalize(st, 2 * args["T"], C)
    torch.cuda.synchronize()
    return raw, st, mr


@pytest.mark.parametrize("name", list(CASES))
def test_fused_launch_vs_separate_launches_and_float64(name):
    """Relative L2 against float64 measured on the MI355X, fused / separate: poly 2.113e-07 / 2.113e-07, contiguous
    2.134e-07 / 2.141e-07, pair 2.472e-07 / 2.471e-07, pair-glu 2.526e-07 / 2.522e-07, poly4 2.105e-07 / 2.105e-07,
    poly1 2.124e-07 / 2.123e-07; the finalised statistics differ
    from the separate path's by at most 1.2e-07 relative."""
    args, want, raw_sep, mr_sep = _case(name)
    raw, st, mr = _fused(args)
    assert torch.isfinite(raw).all() and torch.isfinite(st).all()       # every row and every slot written
    e_fused, e_sep = _rel(raw.cpu(), want), _rel(raw_sep, want)
    rel_mr = ((mr.cpu().double() - mr_sep.double()).abs() / mr_sep.double().abs()).max(0).values.tolist()
    msg = (f"up fusion {name}: rel L2 vs float64 fused {e_fused:.3e}, separate {e_sep:.3e} (ratio {e_fused / e_sep:.3f}); "
           f"statistics (mean0, rstd0, mean1, rstd1) rel vs separate {['%.2e' % v for v in rel_mr]}")
    _log(msg)
    assert e_fused <= 1.5 * e_sep, msg
    assert max(rel_mr) <= 1e-6, msg
    # the means again, in units of the group's rms (1 / rstd): no less strict, whatever the mean is
    for m, r in ((0, 1), (2, 3)):
        dm = (mr.cpu().double()[:, m] - mr_sep.double()[:, m]).abs() * mr_sep.double()[:, r]
        assert float(dm.max()) <= 1e-6, (msg, m, float(dm.max()))
    # the edges, where a misplaced row would vanish in a whole-tensor norm: no row differs from the separate path's by
    # more than a few units of the arithmetic's error
    worst = float((raw.cpu().double() - raw_sep.double()).abs().amax(dim=(0, 2)).max())
    assert worst <= 1e-4 * float(want.abs().max()), (msg, worst)


@pytest.mark.parametrize("name", ["poly", "pair"])
def test_fused_launch_is_deterministic(name):
    args, *_ = _case(name)
    raw1, st1, _ = _fused(args)
    raw2, st2, _ = _fused(args)
    assert torch.equal(raw1, raw2) and torch.equal(st1, st2)


# ---- the network -----------------------------------------------------------------------------------------------------
def _names(fn):
    """launch names of the detailed profile while fn() runs"""
    from acousticswarms_speech_amd import native
    L = native.lib()
    L.asw_profile_enable(2)
    out = fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    native.check(L.asw_profile_report(buf, len(buf)))
    L.asw_profile_enable(0)
    return out, list(json.loads(buf.value.decode()))


@pytest.fixture(scope="module")
def small_scene():
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    model = SpotModel(SMALL, make_spot_state_dict(SMALL, seed=17), batch_size=8, precision="f16x3").to("cuda")
    mix = torch.from_numpy(make_scene(19, 3, 7, 9600 + 17).mix)
    rng = np.random.default_rng(23)
    offs = [np.zeros(6, dtype=np.int64)] + [rng.integers(-40, 41, size=6) for _ in range(7)]
    return model, mix, offs


def _up_launches(names):
    return [n for n in names if n.startswith("resstack64<") and ",up>" in n]


def _separate_up(names):
    """the 64 -> 64 block's own GEMM launch: N = 256 from K = 64"""
    return [n for n in names if n.startswith("convgemm") and " N256 K64 " in n]


def test_network_energies_fusion_on_vs_off(small_scene):
    model, mix, offs = small_scene
    model.set_precision("f16x3")
    model.set_up_fusion(True)
    en_on, names_on = _names(lambda: model.shift_and_score(mix, offs, Strict=1, window=1000))
    model.set_up_fusion(False)
    en_off, names_off = _names(lambda: model.shift_and_score(mix, offs, Strict=1, window=1000))
    model.set_up_fusion(True)
    rel = np.abs(en_on - en_off) / np.abs(en_off)
    _log(f"up fusion, SMALL, 8 candidates: energies on vs off, largest relative difference {rel.max():.3e}")
    _log(f"  launches on: {sorted(names_on)}")
    _log(f"  launches off: {sorted(names_off)}")
    assert np.all(en_off > 0) and rel.max() < 1e-5
    assert len(_up_launches(names_on)) == 1 and not _separate_up(names_on)
    assert not _up_launches(names_off) and len(_separate_up(names_off)) == 1


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_unsupported_modes_keep_the_separate_launch(small_scene, precision):
    """f32 and the single-pass mode.  f16x3_safe is not among them (test_safe_mode_fuses_as_f16x3_does)."""
    model, mix, offs = small_scene
    model.set_up_fusion(True)
    model.set_precision(precision)
    try:
        _, names = _names(lambda: model.shift_and_score(mix, offs[:2], Strict=1, window=1000))
    finally:
        model.set_precision("f16x3")
    _log(f"up fusion, {precision}: {sorted(n for n in names if 'N256 K64' in n or ',up>' in n)}")
    assert not _up_launches(names)
    assert len([n for n in names if " N256 K64 " in n]) == 1


def test_safe_mode_fuses_as_f16x3_does(small_scene):
    """f16x3_safe runs this site -- a LayerNorm output plus a skip tensor, "Normed" -- on the kernels f16x3 runs it on, so
    it takes the fused launch too: tests/test_gpu_safe_precision.py pins that the two modes' launch plans differ in the
    exact-f32 sites and in nothing else, launch for launch.  Energies against its own separate launch below 1e-5."""
    model, mix, offs = small_scene
    model.set_precision("f16x3_safe")
    try:
        model.set_up_fusion(True)
        en_on, names_on = _names(lambda: model.shift_and_score(mix, offs[:2], Strict=1, window=1000))
        model.set_up_fusion(False)
        en_off, names_off = _names(lambda: model.shift_and_score(mix, offs[:2], Strict=1, window=1000))
    finally:
        model.set_up_fusion(True)
        model.set_precision("f16x3")
    rel = np.abs(en_on - en_off) / np.abs(en_off)
    _log(f"up fusion, f16x3_safe: energies on vs off, largest relative difference {rel.max():.3e}")
    assert rel.max() < 1e-5
    assert len(_up_launches(names_on)) == 1 and not _separate_up(names_on)
    assert not _up_launches(names_off) and len(_separate_up(names_off)) == 1


def test_forward_keeps_the_separate_launch_and_the_tap(small_scene):
    model, mix, offs = small_scene
    model.set_precision("f16x3")
    model.set_up_fusion(True)
    model.shift_and_score(mix, offs[:2], Strict=1, window=1000)
    with pytest.raises(RuntimeError, match="no activation named dec0"):
        model.get_tap("dec0")
    assert model.get_tap("dec1").numel() > 0
    model.set_up_fusion(False)
    model.shift_and_score(mix, offs[:2], Strict=1, window=1000)
    assert model.get_tap("dec0").numel() > 0
    model.set_up_fusion(True)
    x = _rand(2, 7, 1000, seed=5)
    _, names = _names(lambda: model.forward(x, torch.tensor([[0.0, 1.0]] * 2)))
    assert not _up_launches(names) and model.get_tap("dec0").numel() > 0
