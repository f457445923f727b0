"""The split-fp16 kernels (convgemm16*, convgemm16p*, resconv16, downconv64, resstack64 in all its forms) in both of
their arithmetic modes -- "f16x3" (three MFMAs on fp16 hi / lo halves) and single-pass "f16" (one MFMA on
round-to-nearest hi halves) -- against the CPU model of their own arithmetic, tests/f16_model.py: split the operands
as the kernel does, take the exact products, sum in float64.  A correct kernel differs from that model only by its
fp32 accumulation and epilogue, so either mode is held near 1e-7 -- the one-term mode about a thousand times tighter
than its 2e-3 bar against float64 of the inputs, which cannot see anything smaller than the mode's own rounding (a
wrong row, a stale lo half in the residual, a tap read one row off at a tile edge).

Measures, per case: relative L2 over the tensor, and the worst row (the row's error norm over that row's model norm,
rows of all batch items pooled); the four GroupNorm partial sums where the kernel writes them.  The launch name is
read from the detailed profile.  Every case prints launch, model vs truth, kernel vs model and the bar (pytest -s).

Bars.  None is set by hand and none comes from the kernel under test: per case, 4 x the distance between the float64
model and its float32 stand-in (the same exact products added to a float32 accumulator 16 k at a time, k ascending and
descending, the larger of the two), per measure.  The factor covers the MFMA's unspecified order over its 16 k and
the fp32 epilogue.  Fused chains of two or three layers in the ONE-TERM mode are the exception: a 1-ulp fp32
difference in a layer's output flips a round-to-nearest hi half (2^-11) for a few elements in ten thousand and no lo
term catches it, so their bar is 4 x the distance by which the case's own model moves when every hand-over is nudged
by up to +-2 fp32 ulps (about 3e-5 on the whole tensor); their worst row is logged, not asserted.  Single layers in
"f16" get the tight bar.  tests/test_f16_model_host.py reproduces the sizing without a GPU.

Bars and measured distances by family (stand-in sized; ranges over a family's cases; the per-case table is DESIGN.md 7s):

    family                               mode    bar L2            bar row           kernel L2 / row (MI355X)
    -----------------------------------  ------  ----------------  ----------------  ------------------------
    convgemm16 LayerNorm tiles           f16x3   1.8e-07..6.1e-07  2.9e-07..7.0e-07  8.6e-08..2.2e-07 / 1.5e-07..2.6e-07
    convgemm16 LayerNorm tiles           f16     1.4e-07..3.7e-07  1.9e-07..4.3e-07  7.6e-08..1.4e-07 / 1.3e-07..1.7e-07
    resconv16                            f16x3   1.6e-07..1.1e-06  3.0e-07..1.5e-06  8.1e-08..4.0e-07 / 1.4e-07..5.4e-07
    resconv16                            f16     1.3e-07..6.6e-07  2.1e-07..8.4e-07  7.1e-08..2.4e-07 / 1.3e-07..3.0e-07
    downconv64                           f16x3   6.6e-07           8.6e-07           2.3e-07 / 3.0e-07
    downconv64                           f16     4.0e-07           5.6e-07           1.4e-07 / 1.8e-07
    convgemm16p / 16pm GEMM tiles        f16x3   5.0e-07..9.9e-07  6.5e-07..1.6e-06  1.8e-07..3.5e-07 / 2.2e-07..6.4e-07
    convgemm16p / 16pm GEMM tiles        f16     3.1e-07..5.9e-07  4.0e-07..9.9e-07  1.1e-07..2.1e-07 / 1.4e-07..3.4e-07
    convgemm16 / 16m GEMM tiles          f16x3   3.5e-07..9.9e-07  4.5e-07..1.6e-06  1.2e-07..3.5e-07 / 1.5e-07..6.4e-07
    convgemm16 / 16m GEMM tiles          f16     2.4e-07..5.9e-07  3.0e-07..9.9e-07  7.9e-08..2.1e-07 / 9.9e-08..3.4e-07
    resstack64, one layer                f16x3   1.6e-07..4.0e-07  3.1e-07..1.0e-06  8.6e-08..1.6e-07 / 1.6e-07..3.4e-07
    resstack64, one layer                f16     1.3e-07..2.5e-07  2.2e-07..5.7e-07  8.1e-08..1.1e-07 / 1.7e-07..2.4e-07
    resstack64, 2-3 fused layers         f16x3   4.0e-07..7.9e-07  5.9e-07..1.2e-06  1.4e-07..2.9e-07 / 1.7e-07..4.3e-07
    resstack64, 2-3 fused layers         f16     5.2e-07..3.1e-05  reported only     1.2e-07..1.4e-05 / 1.7e-07..1.3e-04
    resstack64 UpFeed                    f16x3   4.5e-07..6.1e-07  8.3e-07..1.1e-06  1.6e-07..2.1e-07 / 2.6e-07..3.5e-07
    resstack64 source-fed pair           f16x3   5.3e-07           8.6e-07           2.0e-07 / 3.7e-07
    range rows, convgemm16               f16x3   1.0e-07..3.6e-07  1.2e-07..4.7e-07  2.6e-08..1.2e-07 / 3.0e-08..1.6e-07
    range rows, convgemm16               f16     1.0e-07..3.3e-07  1.2e-07..3.3e-07  2.6e-08..1.1e-07 / 3.0e-08..1.1e-07
    range rows, resstack64               f16x3   4.1e-07..1.3e-06  7.5e-07..2.2e-06  2.0e-07..4.7e-07 / 2.9e-07..7.9e-07
    range rows, resstack64               f16     3.1e-05..7.4e-05  reported only     1.1e-06..2.0e-05 / 9.3e-06..1.4e-04
    range rows, resconv16                f16x3   4.0e-07..7.7e-07  7.8e-07..1.3e-06  1.5e-07..2.8e-07 / 2.7e-07..5.1e-07
    range rows, resconv16                f16     2.5e-07..4.6e-07  4.4e-07..7.7e-07  1.1e-07..1.8e-07 / 1.8e-07..3.0e-07

Range: activations x 2^-10 and 2^6, weights x 1e-3 and 30 stay within the bars recomputed at that scale, and one
activation of 1e6 leaves every output finite and equal to the model's, whose split clamps at +-65504 in both modes.
Needs an MI355X."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import f16_model as fm
from tests import f16_model_cases as mc

pytestmark = pytest.mark.gpu


def _log(msg):
    print(msg)


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


def _distinct(case, t):
    """device tensor of the whole batch -> numpy of the items the model has; the copies must equal them bit for bit"""
    if case.rep > 1:
        v = t.view(case.rep, t.shape[0] // case.rep, *t.shape[1:])
        assert torch.equal(v, v[:1].expand_as(v)), "repeated batch items differ"
        t = v[0]
    elif getattr(case, "B", 0) == 3:
        assert torch.equal(t[0], t[1]), "item 1 is a copy of item 0: bit-equal outputs expected"
        t = t[[0, 2]]
    return t.cpu().numpy()


@pytest.mark.parametrize("name,mode", mc.case_ids(), ids=[f"{n}-{m}" for n, m in mc.case_ids()])
def test_kernel_vs_model_of_its_arithmetic(name, mode):
    from acousticswarms_speech_amd import ops
    case = mc.all_cases()[name]
    res, names = _launch_names(lambda: case.device(ops, mode))
    out, stats = res if isinstance(res, tuple) else (res, None)
    finite = bool(torch.isfinite(out).all())
    got = _distinct(case, out)
    s = mc.sizing(case, mode)                          # (after the launch: a GLU case's model splits the side output)
    model = s["model"]
    l2, row = fm.measures(got, model) if finite else (float("inf"), float("inf"))
    bar_row = "reported only" if s["bar_row"] is None else f"{s['bar_row']:.3e}"
    _log(f"{name} {mode}: {case.expected if case.expected in names else names}  model vs truth {s['truth'][0]:.3e} / {s['truth'][1]:.3e}  kernel vs model "
         f"{l2:.3e} / {row:.3e}  bar {s['bar_l2']:.3e} / {bar_row}" + (f" (nudged model's worst row {s['chain_row']:.3e})"
                                                                      if s["chain_row"] is not None else ""))
    # (a GLU form with UpFeed comes with the launch that wrote the side output)
    assert case.expected in names and len(names) <= 2, names
    assert finite, "non-finite output"
    assert l2 < s["bar_l2"], (l2, s["bar_l2"])
    if s["bar_row"] is not None:
        assert row < s["bar_row"], (row, s["bar_row"])
    if getattr(case, "side", None) is not None:
        # the staged fp32 tensor itself: asw::gn_glu_value's expression in float64 (hardware exp2 / rcp: about 3e-7)
        want = fm.gn_glu(case.inp["raw"], case.glu_mr(), case.inp["gg"], case.inp["gb"])
        d = fm.measures(case.side, want)
        _log(f"{name} {mode}: GroupNorm + GLU side output vs float64 {d[0]:.3e} / {d[1]:.3e}")
        assert d[0] < 3e-7 and d[1] < 1e-6, d
    if case.stats:
        assert stats is not None and bool(torch.isfinite(stats).all())
        st = stats.double().sum(1)
        st = _distinct(case, st) if case.rep > 1 else st.cpu().numpy()
        want, bound = fm.stats4(model, case.stats), fm.stats_bounds(model, case.stats, s["bar_l2"])
        frac = np.abs(st - want) / bound
        _log(f"{name} {mode}: partial sums, error as a fraction of its bound (sum0, sq0, sum1, sq1) {np.round(frac.max(0), 3)}")
        assert frac.max() < 1.0, (st, want, bound)


def test_device_activation_split_matches_the_model_bit_for_bit():
    """The only place the device split is visible from outside: asw_shift_norm_src writes the fp16 hi / lo planes of
    its sources with split4t<3> (csrc/prep_kernels.hip, src_planes_kernel).  The kernel normalises inside, (q - mean)
    / std, so the sources are multiples of 2^-15 (their own int16 quantisation is exact) with mean 0 and std 1, 2^10
    and 2^-4 (exact too): the planes must equal the model's split of the same fp32 values bit for bit -- truncation on
    both signs, zeros, and at std = 2^10 remainders below the smallest fp16 normal.  With an arbitrary mean and std
    the fp32 value of channel 0 is read back from refn instead, all 24 bits of it in use."""
    from acousticswarms_speech_amd import ops
    M, T, pad = 7, 1000, 24
    rng = np.random.default_rng(5)
    mix = (rng.integers(-32767, 32768, size=(M, T)) / 32768.0).astype(np.float32)
    mix[:, :4] = 0.0
    off = torch.zeros(3, M - 1, dtype=torch.int32).cuda()
    stds = np.array([1.0, 1024.0, 1.0 / 16], dtype=np.float32)
    hi, lo, refn = ops.shift_norm_src(torch.from_numpy(mix).cuda(), off, torch.zeros(3).cuda(), torch.from_numpy(stds).cuda(),
                                      T + pad, True)
    u = np.zeros((3, T + pad, 8), dtype=np.float32)
    u[:, pad:, :M] = mix.T[None] / stds[:, None, None]
    u[..., 7] = 1.0
    wh, wl = fm.split_act(u, 3)
    assert np.array_equal(refn.cpu().numpy(), u[..., 0])
    assert np.array_equal(hi.cpu().numpy().view(np.uint16), wh.view(np.uint16))
    assert np.array_equal(lo.cpu().numpy().view(np.uint16), wl.view(np.uint16))
    sub = (wl != 0) & (np.abs(wl.astype(np.float32)) < 2.0 ** -14)
    assert sub.sum() > 100 and (wl.astype(np.float32) < 0).sum() > 100          # the edges were in the data
    # arbitrary statistics: channel 0's fp32 value is refn
    hi, lo, refn = ops.shift_norm_src(torch.from_numpy(mix).cuda(), off, torch.full((3,), 0.123).cuda(),
                                      torch.full((3,), 3.0).cuda(), T + pad, True)
    wh, wl = fm.split_act(refn.cpu().numpy(), 3)
    assert np.array_equal(hi.cpu().numpy()[..., 0].view(np.uint16), wh.view(np.uint16))
    assert np.array_equal(lo.cpu().numpy()[..., 0].view(np.uint16), wl.view(np.uint16))
