"""CPU only: the model of the split-fp16 kernels' arithmetic (tests/f16_model.py) is itself checked here -- its weight
split against the library's host functions bit for bit, the properties of its activation split, its distance from
float64 truth (so that a later edit of the model cannot drift unnoticed) and the sizing of the bars that
tests/test_gpu_f16_model.py applies, recorded so that they can be reproduced without a GPU."""
import numpy as np
import pytest

from tests import f16_model as fm
from tests import f16_model_cases as mc
from tests.test_weight_pack_host import _weights, pack_lib, split_lib


def _within_2x(value, figure):
    return figure / 2 < value < figure * 2


# ---------------------------------------------------------------------------------------------- the weight split
@pytest.mark.parametrize("N,K,seed,scale", [(32, 16, 21, 1.0), (64, 448, 22, 1.0), (64, 64, 23, 1e-30), (32, 48, 24, 1e30)])
def test_weight_split_equals_the_library_bit_for_bit(N, K, seed, scale):
    """split_np / split_w against asw_split_weights_f16, and asw_pack_fragments_f16 holds the same halves (a
    permutation: tests/test_weight_pack_host.py pins which)"""
    w = (_weights(N, K, seed) * np.float32(scale)).astype(np.float32)
    rc, hi, lo, sh = split_lib(w)
    mh, ml, msh = fm.split_np(w)
    assert rc == 0 and sh == msh
    assert hi.tobytes() == mh.tobytes() and lo.tobytes() == ml.tobytes()
    wh, wl, wsh = fm.split_w(w)
    assert wsh == sh and wh.shape == w.shape
    assert np.array_equal(wh.ravel(), hi.view(np.float16).astype(np.float64))
    assert np.array_equal(wl.ravel(), lo.view(np.float16).astype(np.float64))
    rc, fh, fl, fsh = pack_lib(w, N, K)
    assert rc == 0 and fsh == sh
    assert sorted(fh.tolist()) == sorted(mh.tolist()) and sorted(fl.tolist()) == sorted(ml.tolist())


# ---------------------------------------------------------------------------------------------- the activation split
def test_activation_split_residual_below_2_to_minus_20():
    """|x - hi - lo| < 2^-20 |x| wherever the remainder's own last bit is an fp16 normal's or the subnormal step
    2^-24 is below the bound: 2^-4 <= |x| < 65504"""
    rng = np.random.default_rng(1)
    x = (rng.choice([-1.0, 1.0], 200000) * rng.uniform(1, 2, 200000) * np.exp2(rng.integers(-4, 15, 200000))).astype(np.float32)
    for nterm in (3, 1):
        hi, lo = fm.split_act(x, nterm)
        r = np.abs(x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
        assert np.all(r < 2.0 ** -20 * np.abs(x)), nterm
        assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo))


def test_activation_split_truncates_toward_zero_on_both_signs():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(100000).astype(np.float32)
    x = np.concatenate([x, -x])
    hi, lo = fm.split_act(x, 3)
    h, l = hi.astype(np.float64), lo.astype(np.float64)
    assert np.all(np.abs(h) <= np.abs(x)) and np.all(np.abs(h + l) <= np.abs(x))          # never away from zero
    assert np.all((np.sign(h) == np.sign(x)) | (h == 0)) and np.all((np.sign(l) == np.sign(x)) | (l == 0))
    assert np.array_equal(hi[:100000], -hi[100000:]) and np.array_equal(lo[:100000], -lo[100000:])      # odd symmetry
    normal = np.abs(x) >= 2.0 ** -14
    assert np.all(np.abs(x - h)[normal] < 2.0 ** -10 * np.abs(x)[normal])                 # 11 bits in hi
    # one term: hi is the nearest fp16, the remainder changes sign with it
    hi1, lo1 = fm.split_act(x, 1)
    assert np.array_equal(hi1, x.astype(np.float16))
    assert np.all(np.abs(x - hi1.astype(np.float64))[normal] <= 2.0 ** -11 * np.abs(x)[normal])
    assert (lo1.astype(np.float64) * x < 0).sum() > 10000


def test_activation_split_clamps_and_edge_values():
    big = np.array([1e6, -1e6, 65504.0, 65519.0, 65520.0, 3e38], dtype=np.float32)
    for nterm in (3, 1):
        hi, lo = fm.split_act(big, nterm)
        assert np.array_equal(np.abs(hi.astype(np.float32)), np.full(6, 65504.0, np.float32)), nterm
        assert np.array_equal(lo.astype(np.float32), np.array([65504.0, -65504.0, 0.0, 15.0, 16.0, 65504.0], np.float32)), nterm
    z = np.array([0.0, -0.0], dtype=np.float32)
    hi, lo = fm.split_act(z, 3)
    assert np.array_equal(hi.view(np.uint16), np.array([0, 0x8000], np.uint16)) and not lo.astype(np.float32).any()
    # remainders below the smallest fp16 normal (2^-14) are subnormal and truncated; below 2^-24 they vanish
    x = np.array([2.0 ** -11 + 2.0 ** -23 + 2.0 ** -25, -(2.0 ** -11 + 2.0 ** -25), 2.0 ** -25, -2.0 ** -25], dtype=np.float32)
    hi, lo = fm.split_act(x, 3)
    assert np.array_equal(hi.astype(np.float64), np.array([2.0 ** -11, -2.0 ** -11, 0.0, 0.0]))
    assert np.array_equal(lo.astype(np.float64), np.array([2.0 ** -23, 0.0, 0.0, 0.0]))
    assert np.array_equal(np.signbit(lo), np.array([False, True, False, True]))


# ---------------------------------------------------------------------------------------------- model against truth
def _unit_layer():
    """dilation 1, C = 64, 7 taps, T = 700, unit-scale data: convolution + bias"""
    rng = np.random.default_rng(0)
    C, K, T = 64, 7, 700
    x = rng.standard_normal((1, T, C)).astype(np.float32)
    w = (rng.standard_normal((C, K * C)) / np.sqrt(C * K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    return lambda nterm, acc="f64", korder=1: fm.conv_layer(x, w, nterm, taps=K, pad=3, bias=b, acc=acc, korder=korder)


def test_model_against_float64_truth_at_unit_scale():
    """three-term model 1.55e-7 (worst row 2.3e-7) from float64 truth, one-term 2.9e-4; the float32 stand-in 1.0e-7
    to 1.7e-7 (worst row 2.5e-7) from the model in either mode; bars about 7e-7 / 1e-6.  Each within 2 x."""
    f = _unit_layer()
    truth = f(0)
    m3, bar3 = fm.bars(lambda acc, k: f(3, acc, k))
    m1, bar1 = fm.bars(lambda acc, k: f(1, acc, k))
    t3, t1 = fm.measures(m3, truth), fm.measures(m1, truth)
    print(f"unit layer: three-term vs truth {t3}, one-term {t1}, bars {bar3} / {bar1}")
    assert _within_2x(t3[0], 1.55e-7) and _within_2x(t3[1], 2.3e-7)
    assert _within_2x(t1[0], 2.9e-4)
    for bar in (bar3, bar1):
        assert 1.0e-7 / 2 < bar[0] / fm.BAR_FACTOR < 1.7e-7 * 2 and _within_2x(bar[1] / fm.BAR_FACTOR, 2.5e-7)
    assert _within_2x(bar3[0], 7e-7) and _within_2x(bar3[1], 1e-6)


def test_one_term_chains_move_by_their_flipped_halves():
    """the two-layer (1, 7) model with its hand-over nudged by up to +-2 fp32 ulps: 7.7e-6 whole-tensor / 6.9e-5 worst
    row in the one-term mode, 1.7e-7 / 3.0e-7 in f16x3 (each within 2 x) -- why fused one-term chains get a bar of their own"""
    c = mc.all_cases()["stack-d1.7-T500"]
    x, layers = c.inp["x"], c.inp["layers"]
    d1 = fm.nudged_distance(x, layers, 7, 1, c.model(1))
    d3 = fm.nudged_distance(x, layers, 7, 3, c.model(3))
    print(f"nudged (1, 7) pair: one-term {d1}, three-term {d3}")
    assert _within_2x(d1[0], 7.7e-6) and _within_2x(d1[1], 6.9e-5)
    assert _within_2x(d3[0], 1.7e-7) and _within_2x(d3[1], 3.0e-7)


# ---------------------------------------------------------------------------------------------- the bars, recorded
# (bar L2, bar worst row) as `python -m tests.f16_model_cases` prints them; None: reported, not asserted
RECORDED = {
    ("ln-N64-precf16x3", "f16x3"): (1.75e-07, 2.92e-07), ("ln-N64-precf16x3", "f16"): (1.39e-07, 1.89e-07),
    ("res-C64-T300-dil1", "f16x3"): (3.99e-07, 7.73e-07), ("res-C64-T300-dil1", "f16"): (2.48e-07, 4.32e-07),
    ("res-C128-T520-dil7", "f16x3"): (5.64e-07, 9.85e-07), ("res-C128-T520-dil7", "f16"): (3.36e-07, 5.74e-07),
    ("down-N128-T258", "f16x3"): (6.56e-07, 8.63e-07), ("down-N128-T258", "f16"): (3.96e-07, 5.62e-07),
    ("gemm-B2-M300-N256-K128-precf16x3-formstats+A2", "f16x3"): (3.59e-07, 4.66e-07),
    ("gemm-B2-M300-N256-K128-precf16x3-formstats+A2", "f16"): (2.38e-07, 3.14e-07),
    ("stack-d1-T37", "f16x3"): (4.01e-07, 5.97e-07), ("stack-d1-T37", "f16"): (2.53e-07, 4.34e-07),
    ("stack-d1.7-T215", "f16x3"): (6.51e-07, 1.07e-06), ("stack-d1.7-T215", "f16"): (2.96e-05, None),
    ("stack-d1.2.4-K5-T233", "f16x3"): (7.90e-07, 1.22e-06), ("stack-d1.2.4-K5-T233", "f16"): (3.12e-05, None),
    ("up-contiguous", "f16x3"): (4.56e-07, 8.32e-07),
    ("src-pair-T470", "f16x3"): (5.27e-07, 8.65e-07),
    ("range-gemm-sat", "f16x3"): (3.29e-07, 4.53e-07), ("range-gemm-sat", "f16"): (3.29e-07, 3.29e-07),
    ("range-stack-w30", "f16x3"): (1.29e-06, 2.23e-06),
}


@pytest.mark.parametrize("name,mode", list(RECORDED), ids=[f"{n}-{m}" for n, m in RECORDED])
def test_bar_sizing_reproduces(name, mode):
    """the bars the GPU test applies to a case, computed here as it computes them (the table rounds to three digits)"""
    s = mc.sizing(mc.all_cases()[name], mode)
    want = RECORDED[(name, mode)]
    print(f"{name} {mode}: model vs truth {s['truth']}, bar {s['bar_l2']:.3e} / {s['bar_row']}")
    assert s["bar_l2"] == pytest.approx(want[0], rel=0.02)
    if want[1] is None:
        assert s["bar_row"] is None and s["chain_row"] > 0
    else:
        assert s["bar_row"] == pytest.approx(want[1], rel=0.02)


def test_every_one_term_branch_is_a_case():
    """every f16x3 row of the dispatch table is run in the one-term mode as well, and the UpFeed and source-fed forms
    (which have no one-term instantiation) in f16x3 only"""
    from tests.test_gpu_f16x3 import _DISPATCH
    ids = set(mc.case_ids())
    for p in _DISPATCH:
        if p.values[1].get("prec", "f16x3") == "f16x3":
            assert (p.id, "f16x3") in ids and (p.id, "f16") in ids, p.id
    for name, c in mc.all_cases().items():
        if name.startswith(("up-", "src-")):
            assert c.modes == ("f16x3",)
