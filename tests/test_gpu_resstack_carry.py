"""The carried-halo form of the fused 64-channel pair (csrc/resstack.hip, CARRY): a workgroup walks a run of consecutive
row tiles of one item and hands the 2 x 21 layer-0 rows two neighbouring tiles share from tile to tile, instead of
computing them in both.  A row's arithmetic does not depend on the tile that computes it, so the acceptance bar is bit
identity with the recomputed-halo tiling (runs_per_item = -1), for the output and for the GLU side output; next to it
the bars of tests/test_gpu_resstack.py (relative L2 <= 2e-5 against torch fp32, <= 3e-6 against the per-layer HIP
kernels, <= 2e-3 in the single-pass mode) and of tests/test_gpu_srcstack.py (<= 3e-6 against the staged pair).
Lengths: 470 = head tile + one steady tile, 471 one row more, 982 = 214 + 3 x 256, 1000; 726 with two runs (each a head
and a steady tile); 3010 with 1, 2, 5 runs and the library's own choice.  Needs an MI355X."""
import re

import pytest
import torch

from tests.test_gpu_resstack import C, _dev_layers, _hip_layers, _layers, _profiled, _rand, _rel, _torch_stack

pytestmark = pytest.mark.gpu
K, B = 7, 3
CASES = [(470, 0), (471, 0), (982, 0), (1000, 0), (726, 2), (3010, 1), (3010, 2), (3010, 5), (3010, 0)]


_REF = {}


def _plain_reference(T):
    """input, layers, torch fp32 and per-layer HIP results for length T: made once, shared by the run counts"""
    if ("plain", T) not in _REF:
        from acousticswarms_speech_amd import ops
        x = _rand(B, C, T, seed=3)
        layers = _layers((1, 7), K)
        xc = x.transpose(1, 2).contiguous().cuda()
        _REF["plain", T] = (xc, _dev_layers(ops, layers), _torch_stack(x, layers, K), _hip_layers(ops, xc, layers, K).cpu())
    return _REF["plain", T]


def _glu_reference(T):
    if ("glu", T) not in _REF:
        from acousticswarms_speech_amd import ops
        raw = _rand(B, T, 2 * C, seed=7).cuda()
        gg, gb = (1 + _rand(2 * C, seed=8, scale=0.1)).cuda(), _rand(2 * C, seed=9, scale=0.1).cuda()
        st = torch.zeros(B, 1, 4, device="cuda")
        st[:, 0, 0] = raw[:, :, :C].sum((1, 2)); st[:, 0, 1] = (raw[:, :, :C] ** 2).sum((1, 2))
        st[:, 0, 2] = raw[:, :, C:].sum((1, 2)); st[:, 0, 3] = (raw[:, :, C:] ** 2).sum((1, 2))
        x, mr = ops.gn_glu(raw, st, gg, gb), ops.gn_finalize(st, T, C)          # the separate GroupNorm + GLU pass
        layers = _layers((1, 7), K, seed=70)
        want = _torch_stack(x.cpu().transpose(1, 2).contiguous(), layers, K)
        _REF["glu", T] = ((raw, mr, gg, gb), x, _dev_layers(ops, layers), want, _hip_layers(ops, x, layers, K).cpu())
    return _REF["glu", T]


@pytest.mark.parametrize("T,runs", CASES)
def test_carried_pair_plain(T, runs):
    from acousticswarms_speech_amd import ops
    xc, dl, want, per_layer = _plain_reference(T)
    got, names = _profiled(lambda: ops.resstack(xc, dl, taps=K, runs_per_item=runs))
    off, names_off = _profiled(lambda: ops.resstack(xc, dl, taps=K, runs_per_item=-1))
    assert any(n.startswith("resstack64<2,4x2,carry>") for n in names), names
    assert any(n.startswith("resstack64<2,4x2>") for n in names_off), names_off
    r, r2 = _rel(got.cpu(), want), _rel(got.cpu(), per_layer)
    print(f"carried pair T={T} runs={runs}: rel vs torch {r:.3e}, vs per-layer HIP {r2:.3e}, bit-equal to the "
          f"recomputed-halo tiling {torch.equal(got, off)}")
    assert torch.isfinite(got).all()
    assert r < 2e-5 and r2 < 3e-6
    assert torch.equal(got, off)


@pytest.mark.parametrize("T,runs", CASES)
def test_carried_pair_glu_on_load(T, runs):
    from acousticswarms_speech_amd import ops
    glu, x, dl, want, per_layer = _glu_reference(T)
    side = torch.full((B, T, C), float("nan"), device="cuda")
    side_off = torch.full((B, T, C), float("nan"), device="cuda")
    got, names = _profiled(lambda: ops.resstack(None, dl, taps=K, glu=glu, glu_out=side, runs_per_item=runs))
    off = ops.resstack(None, dl, taps=K, glu=glu, glu_out=side_off, runs_per_item=-1)
    assert any(n.startswith("resstack64<2,4x2,carry,glu>") for n in names), names
    r, r2 = _rel(got.cpu(), want), _rel(got.cpu(), per_layer)
    print(f"carried glu pair T={T} runs={runs}: rel vs torch {r:.3e}, vs per-layer HIP {r2:.3e}, bit-equal to the "
          f"recomputed-halo tiling {torch.equal(got, off)}; side output: max abs diff to asw_gn_glu "
          f"{float((side - x).abs().max()):.3e}, bit-equal {torch.equal(side, x)}, to the other tiling's {torch.equal(side, side_off)}")
    assert torch.isfinite(got).all() and torch.isfinite(side).all()       # every side row written
    assert r < 2e-5 and r2 < 3e-6
    assert torch.equal(got, off) and torch.equal(side, side_off)
    assert torch.equal(side, x)                                           # the separate GroupNorm + GLU pass, bit for bit
    assert torch.equal(got, ops.resstack(x, dl, taps=K, runs_per_item=runs))


def test_carried_pair_source_fed():
    """the source-fed pair at T = 1000 with two runs per item against the staged pair (separate preproc pass)"""
    from acousticswarms_speech_amd import ops
    from tests.test_gpu_srcstack import M, OFFSETS, _weights
    pre_w, pre_b, layers = _weights()
    Tp = 1000
    mix_d, off_d = _rand(M, Tp, seed=1007, scale=0.3).cuda(), torch.from_numpy(OFFSETS).cuda()
    mean, std = ops.shift_stats(mix_d, off_d, True)
    hi, lo, _ = ops.shift_norm_src(mix_d, off_d, mean, std, Tp, True)
    fed = [(w, b.cuda(), g.cuda(), be.cuda(), d) for w, b, g, be, d in layers]
    got, names = _profiled(lambda: ops.resstack_src(hi, lo, pre_w, pre_b, fed, taps=K, runs_per_item=2))
    off = ops.resstack_src(hi, lo, pre_w, pre_b, fed, taps=K, runs_per_item=-1)
    assert any(re.match(r"resstack64<2,4x2,carry,src>\[B3 M1000 d1 r2\]", n) for n in names), names
    x0, _ = ops.shift_norm_preproc(mix_d, off_d, mean, std, pre_w.cuda(), pre_b.cuda(), Tp, True)
    want = ops.resstack(x0, [(ops.pack_conv_weight(w).cuda(), b.cuda(), g.cuda(), be.cuda(), d) for w, b, g, be, d in layers], taps=K)
    for name, (r0, r1) in {"all": (0, Tp), "head": (0, 8), "tail": (Tp - 8, Tp), "run boundary": (466, 474)}.items():
        ra = _rel(got[:, r0:r1].cpu(), want[:, r0:r1].cpu())
        print(f"carried src pair rows {name}: rel vs preproc + pair {ra:.3e}")
        assert ra <= 3e-6, (name, ra)
    assert torch.isfinite(got).all() and torch.equal(got, off)


@pytest.mark.parametrize("T", [5, 214])
def test_single_tile_keeps_the_recomputed_halo_form(T):
    from acousticswarms_speech_amd import ops
    xc, dl, want, per_layer = _plain_reference(T)
    got, names = _profiled(lambda: ops.resstack(xc, dl, taps=K))
    assert any(n.startswith("resstack64<2,4x2>") for n in names) and not any("carry" in n for n in names), names
    assert _rel(got.cpu(), want) < 2e-5 and _rel(got.cpu(), per_layer) < 3e-6


def test_single_item_is_cut_into_several_runs():
    from acousticswarms_speech_amd import ops
    xc, dl, want, per_layer = _plain_reference(3010)
    got, names = _profiled(lambda: ops.resstack(xc[:1].contiguous(), dl, taps=K))
    m = [re.match(r"resstack64<2,4x2,carry>\[B1 M3010 d1 r(\d+)\]", n) for n in names]
    assert any(m), names
    assert int(next(x for x in m if x).group(1)) > 1
    assert torch.equal(got, ops.resstack(xc[:1].contiguous(), dl, taps=K, runs_per_item=-1))
    assert _rel(got.cpu(), want[:1]) < 2e-5 and _rel(got.cpu(), per_layer[:1]) < 3e-6


def test_carried_pair_single_pass_f16_mode():
    from acousticswarms_speech_amd import ops
    xc, dl, want, _ = _plain_reference(1000)
    got, names = _profiled(lambda: ops.resstack(xc, dl, taps=K, precision="f16"))
    assert any(n.startswith("resstack64<2,4x2,carry>") for n in names), names
    r = _rel(got.cpu(), want)
    print(f"carried pair single-pass f16: rel {r:.3e}")
    assert r < 2e-3
    assert torch.equal(got, ops.resstack(xc, dl, taps=K, precision="f16", runs_per_item=-1))
