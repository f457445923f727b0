"""The attention kernels on softmax rows that are not flat (tests/attention_cases.py: families flat, peaked, ramp,
neg_offset, pos_offset, rel_ramp+-), at every tile edge of every route, against the float64 statement of the
operation -- on the f16 route against the model of its own arithmetic (split operands, float64 after).

Per case: one launch with B = 2, the launch name read from the detailed profile, the output finite, and two measures
(relative L2 over the tensor; the worst row, a row being one (item, position, head) slice of head_dim values) under
bars that are computed on the CPU: 4 x the distance between the float64 statement and its float32 stand-in, per case
and measure.  None is set by hand and none comes from a kernel.  Where the stand-in is exact (one key; two keys 50
apart in score) the bar is 0 and the kernel must be exact too.  Every case prints launch, model vs truth, kernel vs
model and the bars (pytest -s).

    route (launch)          precision  head_dim     L
    attention_mfma16        f16x3      128          1, 63, 64, 65, 130, 320
    attention_mfma64        f32        128          1, 63, 64, 65, 130, 320
    attention_mfma_flash    f32        128          321, 385
    attention_valu          f32        16, 48, 112  1, 15, 16, 17, 128, 129, 260
    relpos_attention_mfma   -          64           1, 63, 64, 65, 130, 200
    relpos_attention        -          16, 32       1, 16, 17, 64, 65, 130
    relpos_attention        -          64           1, 64, 65, 130        (ASW_RELPOS_VALU=1: a child process)
    inter_attention         -          16, 64       S = 1, 2, 27, 64 at L = 3
    inter_attention_groups  -          16, 64       groups 3, 0, 1, 6, 2 at L = 3

Bars and measured distances by family (ranges over a family's cases with more than one key; DESIGN.md has the table
by route):

    family        bar L2            bar row           kernel L2 / row (MI355X)
    flat          2.7e-07..2.1e-06  6.3e-07..8.0e-06  6.4e-08..5.2e-07 / 1.5e-07..1.4e-06
    peaked        5.4e-07..6.4e-06  2.9e-06..5.1e-05  7.7e-08..1.4e-06 / 3.2e-07..1.0e-05
    ramp          0.0e+00..3.3e-05  0.0e+00..1.4e-04  0.0e+00..8.9e-06 / 0.0e+00..3.7e-05
    neg_offset    9.1e-06..7.8e-05  3.6e-05..3.7e-04  1.5e-06..2.0e-05 / 6.7e-06..9.1e-05
    pos_offset    7.2e-06..8.7e-05  4.8e-05..4.1e-04  1.3e-06..1.9e-05 / 8.8e-06..9.2e-05
    rel_ramp+     4.7e-07..3.1e-05  8.0e-07..1.7e-04  1.2e-07..7.9e-06 / 2.2e-07..4.5e-05
    rel_ramp-     4.6e-07..3.2e-05  8.0e-07..2.5e-04  1.1e-07..9.4e-06 / 1.8e-07..5.2e-05

No kernel is above 0.56 of a bar.  The offset families are loose on purpose (a float32 score near 200 carries 1.5e-5 of
absolute error whoever computes it): they are there for NaN, a padded key in the maximum and a missing subtraction.
The f16 route's model is 2.2e-07..2.0e-06 / 3.6e-07..7.3e-06 from the truth, its kernel 4.0e-07..9.3e-06 from the model.

The stand-in adds its two products one k at a time, k ascending and descending, the larger distance counting
(attention_cases._mm).  A first sizing used numpy's float32 matmul: its BLAS adds 8 to 16 partial sums, chains a tenth as
long as any kernel's, and 5 of the 393 cases, all on exact-fp32 fmaf-chain kernels, then stood 1.1 to 1.5 x above the
worst-row bar while inside the L2 bar (DESIGN.md 7x has the figures).

Dispatch (bit for bit): "f16" is "f16x3" on attention_mfma16; "f16x3" past L = 320 and at other head dims is the f32
kernel; two runs of a call are equal on every route.

Isolation, through the C entry points with every pointer inside a larger allocation of the test's own: +inf / NaN in
the neighbouring batch items and NaN after the last one leave an item's output bit-equal to that of a call on the item
alone; NaN rows around P, bias_u and bias_v change nothing; the output is written in full (it is pre-filled with NaN)
and nothing around it is written.  At L = 65 and 130 (attention_mfma_flash: 321, the first length it takes).

Not tested, because no test-sized input reaches them: attention_valu<0, 128, false> at head_dim 128 (a sequence of 2^31
bytes and more) and the refusal of B or nhead above 65535.  ASW_NO_ATTN16 and ASW_ATTN_PF are measurement switches
over kernels the table reaches.  Needs an MI355X."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import attention_cases as ac          # noqa: E402
from tests import f16_model as fm                # noqa: E402

pytestmark = pytest.mark.gpu
PREC = {"f32": 0, "f16x3": 1, "f16": 2}
PAD = 64                                         # rows of NaN / sentinel around every buffer of the isolation tests


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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device(c):
    """the case's one launch -> device output"""
    from acousticswarms_speech_amd import ops
    inp = ac.inputs(c.id)
    if c.kind == "attn":
        return ops.attention(_dev(inp[0]), c.nhead, precision=c.precision)
    if c.kind == "relpos":
        return ops.relpos_attention(_dev(inp[0]), _dev(inp[1]), _dev(inp[2]), _dev(inp[3]), c.nhead, inp[4])
    x = _dev(inp[0])
    if c.route == "inter":
        S = c.counts[0]
        return ops.inter_attention(x.view(len(c.counts), S, c.L, 3 * c.d), c.nhead).view(-1, c.L, c.d)
    return ops.inter_attention_groups(x, list(c.counts), c.nhead)


def _figures(cid):
    """-> dict of what a case asserts on (JSON-able: the child process prints it)"""
    c = ac.all_cases()[cid]
    out, names = _launch_names(lambda: _device(c))
    finite = bool(torch.isfinite(out).all())
    s = ac.sizing(cid)
    l2, row = fm.measures(ac.rows(c, out.cpu().numpy()), ac.rows(c, s["model"])) if finite else (float("inf"), float("inf"))
    return dict(id=cid, names=names, finite=finite, l2=l2, row=row, bar_l2=s["bar_l2"], bar_row=s["bar_row"],
                truth=list(s["model_vs_truth"]))


def _check(f):
    c = ac.all_cases()[f["id"]]
    print(f"{f['id']}: {f['names']}  model vs truth {f['truth'][0]:.3e} / {f['truth'][1]:.3e}  kernel vs model "
          f"{f['l2']:.3e} / {f['row']:.3e}  bar {f['bar_l2']:.3e} / {f['bar_row']:.3e}")
    assert len(f["names"]) == 1 and c.name_ok(f["names"][0]), (f["names"], c.prefix)
    assert f["finite"], "non-finite output"
    assert f["l2"] <= f["bar_l2"], (f["l2"], f["bar_l2"])
    assert f["row"] <= f["bar_row"], (f["row"], f["bar_row"])


@pytest.mark.parametrize("cid", ac.case_ids())
def test_kernel_vs_statement(cid):
    _check(_figures(cid))


# ------------------------------------------------------------------------------------------------------- dispatch
def _attn(L, hd, precision, family="ramp"):
    from acousticswarms_speech_amd import ops
    x = _dev(ac.make_qkv(family, 2, L, ac.NHEAD, hd, seed=77))
    return _launch_names(lambda: ops.attention(x, ac.NHEAD, precision=precision))


def test_single_pass_f16_is_f16x3_in_attention():
    a, na = _attn(130, 128, "f16")
    b, nb = _attn(130, 128, "f16x3")
    assert len(na) == len(nb) == 1 and na[0].startswith("attention_mfma16") and nb[0].startswith("attention_mfma16"), (na, nb)
    assert torch.equal(a, b)


@pytest.mark.parametrize("L,hd,prefix", [(321, 128, "attention_mfma_flash"), (130, 48, "attention_valu")])
def test_f16x3_outside_the_f16_kernels_shapes_is_f32(L, hd, prefix):
    a, na = _attn(L, hd, "f16x3")
    b, nb = _attn(L, hd, "f32")
    assert len(na) == len(nb) == 1 and na[0].startswith(prefix) and nb[0].startswith(prefix), (na, nb)
    assert torch.equal(a, b)


TWICE = ["mfma16-hd128-L130-ramp", "mfma64-hd128-L130-ramp", "flash-hd128-L385-ramp", "valu-hd48-L260-ramp",
         "relpos_mfma-hd64-L130-ramp", "relpos_valu-hd32-L130-ramp", "inter-hd64-S27_27-ramp",
         "inter_groups-hd64-S3_0_1_6_2-ramp"]


@pytest.mark.parametrize("cid", TWICE)
def test_two_runs_are_equal(cid):
    c = ac.all_cases()[cid]
    assert torch.equal(_device(c), _device(c))


# ------------------------------------------------------------------------------------------------------ isolation
class _Op:
    """One operation at one shape for the isolation tests: an item is `rows` rows of 3d inputs and d outputs (the
    inter-speaker route: a group of 3 sequences of L = 3, the groups named by a table)."""

    def __init__(self, kind, hd, L, family, precision=None):
        self.kind, self.hd, self.L, self.precision = kind, hd, L, precision
        self.nhead, self.d = ac.NHEAD, ac.NHEAD * hd
        self.P = self.bu = self.bv = None
        self.scale = 0.0
        if kind == "attn":
            x = ac.make_qkv(family, 2, L, self.nhead, hd, seed=91)
        elif kind == "relpos":
            x, P, bu, bv, self.scale = ac.make_relpos(family, 2, L, self.nhead, hd, seed=91)
            self.P, self.bu, self.bv = _dev(P), _dev(bu), _dev(bv)
        else:
            x = ac.make_inter(family, (3, 3), L, self.nhead, hd, seed=91).reshape(2, 3 * L, 3 * self.d)
        self.items = _dev(x)                                   # [2][rows][3d]
        self.rows = self.items.shape[1]

    def launch(self, qkv, B, ctx, P=None, bu=None, bv=None):
        from acousticswarms_speech_amd.native import check, current_stream, lib, ptr
        if self.kind == "attn":
            check(lib().asw_attention_prec(ptr(qkv), B, self.L, self.d, self.nhead, PREC[self.precision], ptr(ctx), current_stream()))
        elif self.kind == "relpos":
            check(lib().asw_relpos_attention(ptr(qkv), ptr(self.P if P is None else P), ptr(self.bu if bu is None else bu),
                                             ptr(self.bv if bv is None else bv), B, self.L, self.d, self.nhead, float(self.scale),
                                             ptr(ctx), current_stream()))
        else:
            bounds = (ctypes.c_int32 * (B + 1))(*[3 * g for g in range(B + 1)])
            check(lib().asw_inter_attention_groups(ptr(qkv), bounds, B, self.L, self.d, self.nhead, ptr(ctx), current_stream()))

    def run(self, before, after_rows=PAD, **tables):
        """`before` [B][rows][3d] followed by after_rows rows of NaN in one allocation; the output lies between PAD rows
        of a NaN-free sentinel and starts as NaN.  Asserts the sentinel untouched and every output value written (finite,
        for finite items).  -> ctx [B][rows][d]"""
        B = before.shape[0]
        n_in = B * self.rows * 3 * self.d
        qbuf = torch.full((n_in + after_rows * 3 * self.d,), float("nan"), device="cuda")
        qbuf[:n_in] = before.reshape(-1)
        n_out, n_pad = B * self.rows * self.d, PAD * self.d
        sentinel = (torch.arange(n_out + 2 * n_pad, device="cuda") % 251).float() + 0.5
        cbuf = sentinel.clone()
        cbuf[n_pad:n_pad + n_out] = float("nan")
        self.launch(qbuf[:n_in], B, cbuf[n_pad:n_pad + n_out], **tables)
        torch.cuda.synchronize()
        assert torch.equal(cbuf[:n_pad], sentinel[:n_pad]) and torch.equal(cbuf[n_pad + n_out:], sentinel[n_pad + n_out:]), \
            "written outside the output"
        return cbuf[n_pad:n_pad + n_out].view(B, self.rows, self.d).clone()


def _isolation(kind, hd, L, family, precision=None):
    """-> list of what failed (empty: all held)"""
    op = _Op(kind, hd, L, family, precision)
    bad = []
    plain = op.run(op.items)
    if not bool(torch.isfinite(plain).all()):
        bad.append("output not written in full (NaN left) or not finite")
    alone = op.run(op.items[1:2])
    if not torch.equal(alone[0], plain[1]):
        bad.append("item 1 of B = 2 differs from the call on it alone")
    for name, poison in (("+inf", float("inf")), ("NaN", float("nan"))):
        p = torch.full_like(op.items[0], poison)
        out = op.run(torch.stack([p, op.items[1], p]))
        if not torch.equal(out[1], alone[0]):
            bad.append(f"{name} in the neighbouring items changes item 1")
        out = op.run(torch.stack([p, op.items[1]]))            # the last item: NaN rows follow it
        if not torch.equal(out[1], alone[0]):
            bad.append(f"{name} before and NaN after the last item change it")
    if kind == "relpos":
        def framed(t, n):                                      # t between n NaN values on either side
            buf = torch.full((t.numel() + 2 * n,), float("nan"), device="cuda")
            buf[n:n + t.numel()] = t.reshape(-1)
            return buf[n:n + t.numel()]
        out = op.run(op.items, P=framed(op.P, PAD * op.d), bu=framed(op.bu, PAD * op.d), bv=framed(op.bv, PAD * op.d))
        if not torch.equal(out, plain):
            bad.append("NaN rows around P / bias_u / bias_v change the output")
    return bad


ISOLATION = ([("attn", 128, L, f, p) for p in ("f16x3", "f32") for L in (65, 130) for f in ("ramp", "neg_offset")]
             + [("attn", 128, 321, f, "f32") for f in ("ramp", "neg_offset")]
             + [("attn", 48, L, f, "f32") for L in (65, 130) for f in ("ramp", "neg_offset")]
             + [("relpos", hd, L, f, None) for hd in (64, 32, 16) for L in (65, 130) for f in ("ramp", "neg_offset")]
             + [("inter", hd, 3, f, None) for hd in (16, 64) for f in ("ramp", "neg_offset")])
CHILD_ISOLATION = [("relpos", 64, L, f, None) for L in (65, 130) for f in ("ramp", "neg_offset")]


@pytest.mark.parametrize("kind,hd,L,family,precision", ISOLATION,
                         ids=[f"{k}-hd{h}-L{L}-{f}-{p}" for k, h, L, f, p in ISOLATION])
def test_neighbours_table_ends_and_output_bounds(kind, hd, L, family, precision):
    assert _isolation(kind, hd, L, family, precision) == []


# ------------------------------------------------------------------------------- the rel-pos VALU kernel at head_dim 64
def test_relpos_valu_kernel_at_head_dim_64():
    """attention_valu_kernel<64, 64, true> runs only under ASW_RELPOS_VALU, which is read once per process: a fresh
    child (a second or two on an MI355X; the limit of 300 s is for a cold start) runs L = 1, 64, 65, 130 on every family,
    two runs of one call and the isolation properties, and prints one line per figure."""
    env = dict(os.environ, ASW_RELPOS_VALU="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    figs = [f for f in lines if "id" in f]
    assert {f["id"] for f in figs} == set(ac.case_ids(child=True))
    for f in figs:
        _check(f)
    other = {f["what"]: f for f in lines if "what" in f}
    assert other["twice"]["equal"] is True
    assert set(other) == {"twice"} | {f"isolation-L{L}-{fam}" for _k, _h, L, fam, _p in CHILD_ISOLATION}
    for what, f in other.items():
        if what != "twice":
            assert f["bad"] == [], (what, f)


if __name__ == "__main__":
    assert os.environ.get("ASW_RELPOS_VALU") == "1"
    for cid in ac.case_ids(child=True):
        print(json.dumps(_figures(cid)), flush=True)
    c = ac.all_cases()["relpos_valu64-hd64-L130-ramp"]
    print(json.dumps(dict(what="twice", equal=bool(torch.equal(_device(c), _device(c))))), flush=True)
    for kind, hd, L, family, precision in CHILD_ISOLATION:
        print(json.dumps(dict(what=f"isolation-L{L}-{family}", bad=_isolation(kind, hd, L, family, precision))), flush=True)
