"""tests/attention_cases.py without a GPU: the float64 statements equal torch's float64 of the expressions the existing
attention tests use (the pad-and-reshape rel_shift among them), split_attn equals a bit-level restatement, and every
GPU case's inputs are what their family claims -- asserted from the float64 scores.  Prints, per case, the score
range, the condition values and both bars (pytest -s)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_cases as ac
from tests import f16_model as fm


def _rand(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).double()


def _close(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


# ------------------------------------------------------------------------------------------------ statement parity
@pytest.mark.parametrize("L,d,H", [(19, 128, 8), (70, 96, 2), (130, 256, 2)])
def test_attention_statement_is_the_expression_of_test_attention(L, d, H):
    B, hd = 2, d // H
    qkv = _rand(B, L, 3 * d, seed=28)
    q, k, v = [t.view(B, L, H, hd).transpose(1, 2) for t in qkv.split(d, dim=-1)]
    want = (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1) @ v).transpose(1, 2).reshape(B, L, d)
    assert _close(ac.attention_f64(qkv.numpy(), H), want.numpy()) < 1e-12


@pytest.mark.parametrize("L,d,H", [(5, 128, 8), (64, 256, 8), (75, 128, 2), (130, 64, 2)])
def test_relpos_statement_is_the_pad_and_reshape_rel_shift(L, d, H):
    B, hd = 2, d // H
    qkv = _rand(B, L, 3 * d, seed=11, scale=0.7)
    P = _rand(2 * L - 1, d, seed=12, scale=0.7)
    bu, bv = _rand(d, seed=13, scale=0.3), _rand(d, seed=14, scale=0.3)
    scale = 1.0 / math.sqrt(d)
    q, k, v = [t.view(B, L, H, hd) for t in qkv.split(d, dim=-1)]
    qu = (q + bu.view(1, 1, H, hd)).transpose(1, 2)
    qv = (q + bv.view(1, 1, H, hd)).transpose(1, 2)
    a = torch.matmul(qu * scale, k.permute(0, 2, 3, 1))
    bd = torch.matmul(qv * scale, P.view(1, -1, H, hd).permute(0, 2, 3, 1))
    bd = F.pad(bd, (1, 0)).view(B, H, -1, L)[:, :, 1:].view(B, H, L, 2 * L - 1)[..., :L]      # rel_shift
    want = torch.matmul(torch.softmax(a + bd, dim=-1), v.transpose(1, 2)).transpose(1, 2).reshape(B, L, d)
    got = ac.relpos_attention_f64(qkv.numpy(), P.numpy(), bu.numpy(), bv.numpy(), H, scale)
    assert _close(got, want.numpy()) < 1e-12
    _ac, bd64 = ac.relpos_scores(qkv.numpy(), P.numpy(), bu.numpy(), bv.numpy(), H, scale)
    assert _close(bd64, bd.numpy()) < 1e-12


def _inter_torch(qkv, H):
    NB, S, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    q, k, v = [t.permute(0, 2, 1, 3).reshape(NB * L, S, H, hd).transpose(1, 2) for t in qkv.split(d, dim=-1)]
    att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    return (att @ v).transpose(1, 2).reshape(NB, L, S, d).permute(0, 2, 1, 3)


def test_inter_statement_is_the_expression_of_test_inter_attention():
    H, d, L = 8, 128, 5
    qkv = _rand(2, 6, L, 3 * d, seed=15, scale=0.7)
    assert _close(ac.inter_attention_f64(qkv.numpy(), H), _inter_torch(qkv, H).numpy()) < 1e-12
    counts = [3, 0, 1, 6, 2]
    x = _rand(sum(counts), L, 3 * d, seed=16, scale=0.7)
    got = ac.inter_attention_f64(x.numpy(), H, counts)
    n0 = 0
    for S in counts:                                                    # the statement of test_inter_attention, per group
        if S:
            want = _inter_torch(x[n0:n0 + S].unsqueeze(0), H)[0]
            assert _close(got[n0:n0 + S], want.numpy()) < 1e-12
            n0 += S


def test_the_float32_stand_ins_hold_float32():
    for cid in ("valu-hd16-L17-ramp", "relpos_valu-hd16-L17-rel_ramp+", "inter_groups-hd16-S3_0_1_6_2-ramp"):
        c = ac.all_cases()[cid]
        out = ac.statement(c, np.float32)
        assert out.dtype == np.float32 and out.shape == ac.statement(c, np.float64).shape


# ------------------------------------------------------------------------------------------------------ split_attn
def _rtz16_bits(x):
    """float32 -> the float64 value of its fp16 truncation, from the bit pattern; finite overflow saturates"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    sign = np.where(b >> 31, -1.0, 1.0)
    e = ((b >> 23) & 0xFF) - 127
    mant = (b & 0x7FFFFF) | np.where(((b >> 23) & 0xFF) > 0, 1 << 23, 0)          # 24 bits, value mant * 2^(e - 23)
    e = np.where(((b >> 23) & 0xFF) > 0, e, -126)
    # fp16 keeps 11 bits above 2^-14 and whole multiples of 2^-24 below it
    drop = np.where(e >= -14, 13, np.minimum(13 + (-14 - e), 40))
    kept = (mant >> drop) << drop
    val = sign * kept.astype(np.float64) * np.exp2((e - 23).astype(np.float64))
    return np.clip(val, -65504.0, 65504.0)


def _rn16_value(r):
    """float64 r -> nearest fp16 value (ties to even), by counting in fp16 quanta"""
    r = np.asarray(r, np.float64)
    ex = np.floor(np.log2(np.maximum(np.abs(r), 2.0 ** -40)))
    q = np.exp2(np.maximum(ex, -14.0) - 10.0)
    return np.rint(r / q) * q


def test_split_attn_equals_a_bit_level_restatement():
    rng = np.random.default_rng(5)
    x = np.concatenate([
        rng.standard_normal(5000) * np.exp2(rng.integers(-20, 14, 5000)),         # both signs, every binade in range
        rng.standard_normal(2000) * 2.0 ** -13,                                    # remainders below the smallest fp16 normal
        rng.standard_normal(1990) * 2.0 ** -22,                                    # hi itself subnormal
        rng.uniform(65000, 65504, 1000) * rng.choice([-1.0, 1.0], 1000),
        [0.0, -0.0, 65504.0, -65504.0, 65503.99, -65503.99, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 1.0]]).astype(np.float32)
    assert x.size == 10000 and np.all(np.abs(x) <= 65504)
    hi = _rtz16_bits(x)
    assert np.all(np.abs(hi) <= np.abs(x.astype(np.float64)))                       # truncation, on both signs
    want = hi + _rn16_value(x.astype(np.float64) - hi)
    got = fm.split_attn(x)
    assert np.array_equal(got, want)
    nz = x != 0
    assert np.max(np.abs(got[nz] - x[nz]) / np.maximum(np.abs(x[nz]), 2.0 ** -3)) <= 2.0 ** -22


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("cid", list(ac.all_cases()))
def test_inputs_are_what_the_family_claims(cid):
    c = ac.all_cases()[cid]
    v = ac.conditions(c)
    s = ac.sizing(cid)
    print(f"{cid}: scores {v['lo']:.1f} .. {v['hi']:.1f}  " + "  ".join(f"{k} {x:.2f}" for k, x in v.items() if k not in ("lo", "hi"))
          + f"  bar {s['bar_l2']:.3e} / {s['bar_row']:.3e}  model vs truth {s['model_vs_truth'][0]:.3e} / {s['model_vs_truth'][1]:.3e}")
    assert np.all(np.isfinite(s["truth"])) and np.all(np.isfinite(s["model"]))
    # (one key, or two keys 50 apart in score: the float32 stand-in is exact and the bar is 0 -- so must the kernel be)
    assert 0 <= s["bar_l2"] < 1e-2 and 0 <= s["bar_row"] < 1e-2
    assert s["bar_l2"] > 0 or c.L == 1 or (c.counts is not None and min(x for x in c.counts if x) <= 2)
    tiles = c.kind != "inter" and c.L > ac.TILE
    if c.family == "ramp" and tiles:
        assert v["even_up"] >= 0.9 and v["odd_down"] >= 0.9, v
        assert v["hi"] > (88.8 if c.hd == 128 else 40.0), v
    if c.family == "neg_offset":
        assert v["hi"] < -100.0, v
    if c.family == "pos_offset":
        assert v["lo"] > 100.0, v
    if c.family == "peaked":
        assert v["part"] < 4.0, v
    if c.family == "rel_ramp+" and tiles:
        assert v["bd_up"] >= 0.9 and v["all_up"] >= 0.9, v
    if c.family == "rel_ramp-" and tiles:
        assert v["bd_down"] >= 0.9 and v["all_down"] >= 0.9, v


def test_the_case_table_is_the_one_the_kernels_need():
    cases = ac.all_cases().values()
    routes = {c.route for c in cases}
    assert routes == {"mfma16", "mfma64", "flash", "valu", "relpos_mfma", "relpos_valu", "relpos_valu64", "inter", "inter_groups"}
    for c in cases:
        assert (c.family in ac.REL_FAMILIES) if c.kind == "relpos" else (c.family in ac.FAMILIES)
    assert {c.L for c in cases if c.route == "flash"} == {321, 385}
    assert {c.id for c in cases if c.child} == set(ac.case_ids(child=True)) and all(c.route == "relpos_valu64" for c in cases if c.child)
