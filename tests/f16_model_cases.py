"""The cases of tests/test_gpu_f16_model.py: inputs, the launch each must make, the CPU model of its arithmetic
(tests/f16_model.py) and the device call.  Plain module: the host test sizes the bars from it without a GPU, and
`python -m tests.f16_model_cases` prints the whole bar table (model vs truth, stand-in distance, bar) for DESIGN.md.

Shapes are the smallest the suite already established for reaching each branch: the f16x3 rows of _DISPATCH in
tests/test_gpu_f16x3.py, the lengths of tests/test_gpu_resstack.py and the CASES of tests/test_gpu_up_fusion.py.
B = 256 rows repeat four distinct items (tests/test_gpu_residue_feed.py): the model is four items' worth, every
output is compared."""
import math
import zlib

import numpy as np

from tests import f16_model as fm

MODES = ("f16x3", "f16")
GLU_MR = np.array([[0.05, 0.9, -0.1, 1.2], [-0.02, 1.1, 0.07, 0.8], [0.03, 1.05, 0.02, 0.95]], dtype=np.float32)


def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def _randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _affine(rng, n):
    """bias, LayerNorm gamma, beta"""
    return _randn(rng, n, scale=0.1), (1 + _randn(rng, n, scale=0.1)).astype(np.float32), _randn(rng, n, scale=0.1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Case:
    """name; modes; expected launch name; chain = fused layers whose hand-over the one-term mode cannot protect;
    stats = chan_mod of the partial sums the kernel writes (0: none); rep = how often the distinct items repeat."""
    modes = MODES
    chain = 1
    stats = 0
    rep = 1
    x_scale = 1.0
    w_scale = 1.0

    def __init__(self, name, expected):
        self.name, self.expected = name, expected
        self._in = None

    @property
    def inp(self):
        if self._in is None:
            self._in = self.inputs()
        return self._in

    def fn(self, mode):
        """(acc, korder) -> model output, for fm.bars"""
        nterm = fm.NTERM[mode]
        return lambda acc, korder: self.model(nterm, acc=acc, korder=korder)

    def truth(self):
        return self.model(0)


class Gemm(Case):
    """the generic tiles and convgemm16p: x W^T + b, optionally (x + x2), * mul, partial sums; "ln": LN(ReLU(.) + x)"""

    def __init__(self, name, expected, B, M, N, K, form="plain", frag=True, x_scale=1.0, w_scale=1.0, sat=False):
        super().__init__(name, expected)
        self.B, self.M, self.N, self.K, self.form, self.frag = B, M, N, K, form, frag
        self.nd = 4 if B == 256 else B
        self.rep = B // self.nd
        self.stats = N if form.startswith("stats") else 0
        self.x_scale, self.w_scale, self.sat = x_scale, w_scale, sat

    def inputs(self):
        r = _rng("gemm", self.nd, self.M, self.N, self.K)
        d = dict(x=_randn(r, self.nd, self.M, self.K), x2=_randn(r, self.nd, self.M, self.K),
                 w=_randn(r, self.N, self.K, scale=1 / math.sqrt(self.K)), mul=_randn(r, self.nd, self.M, self.N))
        d["b"], d["g"], d["be"] = _affine(r, self.N)
        d["x"], d["w"] = d["x"] * np.float32(self.x_scale), d["w"] * np.float32(self.w_scale)
        if self.sat:
            d["x"][0, 0, 0] = 1e6                     # beyond fp16: the split saturates at 65504
        return d

    def model(self, nterm, acc="f64", korder=1):
        i, f = self.inp, self.form
        if f == "ln":
            return fm.conv_layer(i["x"], i["w"], nterm, bias=i["b"], act=1, resid=i["x"], ln=(i["g"], i["be"]), acc=acc, korder=korder)
        return fm.conv_layer(i["x"], i["w"], nterm, bias=i["b"], x2=i["x2"] if f == "stats+A2" else None,
                             mul=i["mul"] if f == "mul" else None, acc=acc, korder=korder)

    def device(self, ops, mode):
        i, f, R = self.inp, self.form, self.rep
        x, w, b = _dev(i["x"]).repeat(R, 1, 1), _dev(i["w"]), _dev(i["b"])
        if f == "ln":
            return ops.convgemm(x, w, self.M, self.N, self.K, bias=b, relu=True, resid=x, ln=(_dev(i["g"]), _dev(i["be"])),
                                precision=mode, use_fragments=False)
        return ops.convgemm(x, w, self.M, self.N, self.K, bias=b, precision=mode, use_fragments=self.frag,
                            stats_chan_mod=self.stats, A2=_dev(i["x2"]).repeat(R, 1, 1) if f == "stats+A2" else None,
                            mul=_dev(i["mul"]).repeat(R, 1, 1) if f == "mul" else None)


class Res(Case):
    """DilatedResidualLayer through resconv16, 7 taps: the residual is the LDS image's hi + lo at C = 64
    (csrc/resconv.hip, `if constexpr (C == 64)`) and the fp32 tensor above (csrc/gemm_epilogue.h, `p.resid + obase`).
    glu: the input is GLU(GroupNorm(2)(raw)) applied while staging; the fp32 tensor that gets split is the kernel's
    own side output (glu_out), itself held to fm.gn_glu."""

    def __init__(self, name, expected, C, T, dil, glu=False, x_scale=1.0, w_scale=1.0, sat=False):
        super().__init__(name, expected)
        self.C, self.T, self.dil, self.glu = C, T, dil, glu
        self.x_scale, self.w_scale, self.sat = x_scale, w_scale, sat
        self.side = None

    def inputs(self):
        C, T = self.C, self.T
        r = _rng("res", C, T, self.dil, self.glu)
        d = dict(w=_randn(r, C, 7 * C, scale=1 / math.sqrt(7 * C)) * np.float32(self.w_scale))
        d["b"], d["g"], d["be"] = _affine(r, C)
        if self.glu:
            d["raw"] = _randn(r, 2, T, 2 * C) * np.float32(1.7) + np.float32(0.3)
            d["gg"], d["gb"] = (1 + _randn(r, 2 * C, scale=0.2)).astype(np.float32), _randn(r, 2 * C, scale=0.1)
            d["x"] = fm.gn_glu(d["raw"], self.glu_mr(), d["gg"], d["gb"]).astype(np.float32)
        else:
            d["x"] = _randn(r, 2, T, C) * np.float32(self.x_scale)
        if self.sat:
            d["x"][0, T // 2, 5] = 1e6
        return d

    def glu_mr(self):
        return GLU_MR[:2]

    def model(self, nterm, acc="f64", korder=1):
        i = self.inp
        x = self.side if (self.side is not None and nterm) else i["x"]
        return fm.conv_layer(x, i["w"], nterm, taps=7, dil=self.dil, pad=3 * self.dil, bias=i["b"], act=1,
                             resid="image" if self.C == 64 else x, ln=(i["g"], i["be"]), acc=acc, korder=korder)

    def device(self, ops, mode):
        import torch
        i, C, T = self.inp, self.C, self.T
        kw = dict(taps=7, dil=self.dil, pad=3 * self.dil, bias=_dev(i["b"]), relu=True, ln=(_dev(i["g"]), _dev(i["be"])),
                  precision=mode)
        if self.glu:
            raw = _dev(i["raw"])
            side = torch.full((2, T, C), float("nan"), device="cuda")
            out = ops.convgemm(raw, _dev(i["w"]), T, C, C, resid=raw, a_batch_stride=T * C, a_len=T * C, B=2,
                               glu=(raw, _dev(self.glu_mr()), _dev(i["gg"]), _dev(i["gb"])), glu_out=side, **kw)
            self.side = side.cpu().numpy()
            return out
        x = _dev(i["x"])
        return ops.convgemm(x, _dev(i["w"]), T, C, C, resid=x, **kw)


class Down(Case):
    """downconv64: stride-2 convolution of a 64-channel tensor, with partial sums"""

    def __init__(self, name, expected, N, T):
        super().__init__(name, expected)
        self.N, self.T, self.stats = N, T, N

    def inputs(self):
        r = _rng("down", self.N, self.T)
        return dict(x=_randn(r, 2, self.T, 64), w=_randn(r, self.N, 7 * 64, scale=1 / math.sqrt(7 * 64)), b=_randn(r, self.N, scale=0.1))

    def model(self, nterm, acc="f64", korder=1):
        i = self.inp
        return fm.conv_layer(i["x"], i["w"], nterm, taps=7, stride=2, pad=3, M_out=(self.T + 1) // 2, bias=i["b"], acc=acc, korder=korder)

    def device(self, ops, mode):
        i = self.inp
        return ops.convgemm(_dev(i["x"]), _dev(i["w"]), (self.T + 1) // 2, self.N, 64, taps=7, stride=2, pad=3, bias=_dev(i["b"]),
                            stats_chan_mod=self.N, precision=mode)


def _stack_layers(r, dils, K, w_scale=1.0):
    out = []
    for d in dils:
        w = _randn(r, 64, K * 64, scale=1 / math.sqrt(64 * K)) * np.float32(w_scale)
        out.append((w,) + _affine(r, 64) + (d,))
    return out


class Stack(Case):
    """resstack64: one to three fused layers; B = 3 with item 1 a copy of item 0 (bit-equal outputs expected, the model
    is items 0 and 2).  The residual is the image's hi + lo in every form (csrc/resstack.hip, finish_rows).
    glu: GroupNorm + GLU on load with the side output, which is the tensor the model splits.
    up: the UpFeed tail (f16x3 only): raw rows and partial sums instead of the stack's output."""

    def __init__(self, name, expected, dils, K, T, glu=False, up=False, B=3, x_scale=1.0, w_scale=1.0, sat=False):
        super().__init__(name, expected)
        self.dils, self.K, self.T, self.glu, self.up, self.B = dils, K, T, glu, up, B
        self.chain = len(dils)
        self.x_scale, self.w_scale, self.sat = x_scale, w_scale, sat
        self.side = None
        if up:
            self.modes, self.stats = ("f16x3",), 128

    def inputs(self):
        T = self.T
        r = _rng("stack", *self.dils, self.K, T, self.glu, self.up)
        nd = self.B - 1 if self.B == 3 else self.B              # distinct items
        d = dict(layers=_stack_layers(r, self.dils, self.K, self.w_scale))
        if self.glu:
            d["raw"] = _randn(r, nd, T, 128)
            d["gg"], d["gb"] = (1 + _randn(r, 128, scale=0.1)).astype(np.float32), _randn(r, 128, scale=0.1)
            d["x"] = fm.gn_glu(d["raw"], self.glu_mr(), d["gg"], d["gb"]).astype(np.float32)
        else:
            d["x"] = _randn(r, nd, T, 64) * np.float32(self.x_scale)
        if self.sat:
            d["x"][0, T // 2, 5] = 1e6
        if self.up:
            d["skip"] = _randn(r, nd, T, 64)
            d["up_w"] = _randn(r, 256, 64, scale=1 / math.sqrt(64))
            d["up_b"] = (0.5 + _randn(r, 256, scale=0.1)).astype(np.float32)      # a mean away from zero (test_gpu_up_fusion.py)
        return d

    def glu_mr(self):
        """finalised statistics of the distinct items"""
        return GLU_MR[[0, 2]] if self.B == 3 else GLU_MR[:self.B]

    def _items(self, a):
        """distinct items -> the batch (item 1 = item 0)"""
        return a[[0, 0, 1]] if self.B == 3 else a

    def model(self, nterm, acc="f64", korder=1):
        i = self.inp
        x = self.side if (self.side is not None and nterm) else i["x"]
        y = fm.stack(x, i["layers"], nterm, taps=self.K, acc=acc, korder=korder)
        if self.up:
            y = fm.up_tail(y, i["skip"], i["up_w"], i["up_b"], nterm, acc=acc, korder=korder) if nterm else \
                fm.conv_layer(y + i["skip"].astype(np.float64), i["up_w"], 0, bias=i["up_b"])
        return y

    def one_term_chain_bar(self):
        i = self.inp
        x = self.side if self.side is not None else i["x"]
        return fm.chain_bar_one_term(x, i["layers"], self.K, self.model(1))

    def device(self, ops, mode):
        """-> out, or (raw, stats) with up.  The model's items are out[[0, 2]] when B == 3."""
        import torch
        i, T = self.inp, self.T
        layers = [(_dev(w), _dev(b), _dev(g), _dev(be), d) for w, b, g, be, d in i["layers"]]
        x, glu = None, None
        if self.glu:
            glu = (_dev(self._items(i["raw"])), _dev(self._items(self.glu_mr())), _dev(i["gg"]), _dev(i["gb"]))
            side = torch.full((self.B, T, 64), float("nan"), device="cuda")
            plain = ops.resstack(None, layers, taps=self.K, precision=mode, glu=glu, glu_out=side)
            self.side = side.cpu().numpy()[[0, 2] if self.B == 3 else slice(None)]
            if not self.up:
                return plain
        else:
            x = _dev(self._items(i["x"]))
        if self.up:
            return ops.resstack_up(x, layers, _dev(i["up_w"]), _dev(i["up_b"]), _dev(self._items(i["skip"])), taps=self.K, glu=glu)
        return ops.resstack(x, layers, taps=self.K, precision=mode)


class SrcPair(Case):
    """The source-fed pair (ops.resstack_src, f16x3 only): layer 0 runs on the 8-channel source planes u~ = (u_0 ..
    u_6, 1) with the composed weight (k = tap * 8 + channel, an eighth tap of zeros) and rebuilds its residual x0 =
    Wpre~ u~ with one more k-step on the 1x1 weight (csrc/resstack.hip, source_layer0); layer 1 is an ordinary
    handed-over layer.  The composed weights are the host library's (asw_compose_source_weights): inputs here."""
    modes = ("f16x3",)
    chain = 2

    def __init__(self, name, expected, T):
        super().__init__(name, expected)
        self.T = T

    def inputs(self):
        r = _rng("src", self.T)
        u = np.zeros((2, self.T, 8), dtype=np.float32)
        u[..., :7] = _randn(r, 2, self.T, 7)
        u[..., 7] = 1.0
        d = dict(u=u, pre_w=_randn(r, 64, 7, scale=1 / math.sqrt(7)), pre_b=_randn(r, 64), layers=_stack_layers(r, (1, 7), 7))
        return d

    def composed(self):
        """(comp [64][64], pre16 [64][16]) from the library's host function"""
        import ctypes
        from acousticswarms_speech_amd.native import check, lib
        i = self.inp
        wc = np.ascontiguousarray(i["layers"][0][0].reshape(64, 7, 64).transpose(0, 2, 1))       # torch layout [N][C][taps]
        comp, pre16 = np.empty((64, 64), dtype=np.float32), np.empty((64, 16), dtype=np.float32)
        check(lib().asw_compose_source_weights(ctypes.c_void_p(wc.ctypes.data), ctypes.c_void_p(i["pre_w"].ctypes.data),
                                               ctypes.c_void_p(i["pre_b"].ctypes.data), 7, 7, ctypes.c_void_p(comp.ctypes.data),
                                               ctypes.c_void_p(pre16.ctypes.data)))
        return comp, pre16

    def model(self, nterm, acc="f64", korder=1):
        i = self.inp
        comp, pre16 = self.composed()
        (w0, b0, g0, be0, _), l1 = i["layers"][0], i["layers"][1:]
        if nterm == 0:                                # from the definitions: x0 = Wpre u + bpre, then the two layers
            x0 = fm.conv_layer(i["u"][..., :7], i["pre_w"], 0, bias=i["pre_b"])
            return fm.stack(x0, i["layers"], 0)
        y = fm.conv_layer(i["u"], comp, 3, taps=8, pad=3, bias=b0, act=1, acc=acc, korder=korder)
        y = y + fm.conv_layer(i["u"], pre16, 3, taps=2, pad=0, acc=acc, korder=korder)           # second tap: zero weights
        x1 = fm.layer_norm(y, g0, be0, 1e-5).astype(np.float32)
        return fm.stack(x1, l1, 3, acc=acc, korder=korder)

    def device(self, ops, mode):
        import torch
        i = self.inp
        hi, lo = fm.split_act(i["u"], 3)
        layers = [(torch.from_numpy(np.ascontiguousarray(w.reshape(64, 7, 64).transpose(0, 2, 1))), _dev(b), _dev(g), _dev(be), d)
                  for w, b, g, be, d in i["layers"]]
        return ops.resstack_src(_dev(hi), _dev(lo), torch.from_numpy(i["pre_w"]), torch.from_numpy(i["pre_b"]), layers, taps=7)


# ---------------------------------------------------------------------------------------------------------- the table
def _dispatch_rows():
    """every f16x3 row of tests/test_gpu_f16x3.py::_DISPATCH (kind, arguments, launch name); the one-term instantiation
    of a branch is launched under the same name (asw::launch_pair picks it by the precision argument)"""
    from tests.test_gpu_f16x3 import _DISPATCH
    out = []
    for p in _DISPATCH:
        kind, kw, expected = p.values
        if kw.get("prec", "f16x3") != "f16x3":
            continue
        if kind == "ln":
            c = Gemm(p.id, expected, 2, 70, kw["N"], kw["N"], form="ln")
        elif kind == "res":
            c = Res(p.id, expected, kw["C"], kw["T"], kw["dil"], glu=kw.get("glu", False))
        elif kind == "down":
            c = Down(p.id, expected, kw["N"], kw["T"])
        else:
            c = Gemm(p.id, expected, kw["B"], kw["M"], kw["N"], kw["K"], form=kw["form"], frag=kw.get("frag", True))
        out.append(c)
    return out


def _stack_rows():
    S = Stack
    rows = [S("stack-d1-T37", "resstack64<1,4x2>[B3 M37 d1]", (1,), 7, 37),
            S("stack-d7-T777", "resstack64<1,4x2,poly2>[B3 M777 d7]", (7,), 7, 777),
            S("stack-d49-T100", "resstack64<1,4x2>[B3 M100 d49]", (49,), 7, 100),
            S("stack-d49-T2357", "resstack64<1,4x2,poly4>[B3 M2357 d49]", (49,), 7, 2357),
            S("stack-d49-T4737", "resstack64<1,4x2,poly2>[B3 M4737 d49]", (49,), 7, 4737),
            S("stack-d49-T10987", "resstack64<1,4x2,poly1>[B3 M10987 d49]", (49,), 7, 10987)]
    rows += [S(f"stack-d1.7-T{T}", f"resstack64<2,4x2>[B3 M{T} d1]", (1, 7), 7, T) for T in (5, 214, 215, 500)]
    rows += [S("stack-d1.2.4-K5-T233", "resstack64<3,4x2>[B3 M233 d1]", (1, 2, 4), 5, 233),
             S("stack-glu-d1.7-T500", "resstack64<2,4x2,glu>[B3 M500 d1]", (1, 7), 7, 500, glu=True)]
    # UpFeed: the six CASES of tests/test_gpu_up_fusion.py (B = 2)
    for nm, T, dils, glu, tag in (("poly", 4737, (49,), False, ",poly2"), ("contiguous", 300, (1,), False, ""),
                                  ("pair", 500, (1, 7), False, ""), ("pair-glu", 500, (1, 7), True, ",glu"),
                                  ("poly4", 2357, (49,), False, ",poly4"), ("poly1", 10987, (49,), False, ",poly1")):
        rows.append(S(f"up-{nm}", f"resstack64<{len(dils)},4x2{tag},up>[B2 M{T} d{dils[0]}]", dils, 7, T, glu=glu, up=True, B=2))
    rows.append(SrcPair("src-pair-T470", "resstack64<2,4x2,src>[B2 M470 d1]", 470))
    return rows


def _range_rows():
    """Range behaviour (the sweeps of test_wide_and_scaled_operands_f16x3): activations x 2^-10 and 2^6, weights x 1e-3
    and 30 -- the bars are recomputed at that scale -- and one activation of 1e6, which the split clamps at 65504 in
    both modes.  A generic tile with partial sums (the kernel of those sweeps) at every scale; the C = 64 halo layer
    (residual from the image) and a fused pair where the product still reaches the output.  Where it does not -- weights
    x 1e-3 in a residual + LayerNorm layer, activations x 2^-10 in a single one -- the output is LayerNorm of the input
    or of the bias alone: the stand-in's distance shrinks to the one rounding of a stored fp32 (2.6e-8) while the kernel's
    LayerNorm keeps its five fp32 roundings, which the stand-in leaves out by construction, so there is no product
    left to test and the bar does not apply.  (Measured once on the MI355X before these rows were taken out, kernel
    against bar, whole tensor / worst row: resconv16 x 2^-10 7.0e-8 / 1.4e-7 against 1.1e-7 / 1.6e-7, resconv16 w x 1e-3
    6.5e-8 / 1.5e-7 against 1.0e-7 / 1.4e-7, resstack64 w x 1e-3 1.2e-7 / 2.3e-7 against 1.0e-7 / 1.6e-7.)"""
    rows = []
    for tag, kw, ln_layers in (("x2^-10", dict(x_scale=2.0 ** -10), "stack"), ("x2^6", dict(x_scale=2.0 ** 6), "res stack"),
                               ("w1e-3", dict(w_scale=1e-3), ""), ("w30", dict(w_scale=30.0), "res stack"),
                               ("sat", dict(sat=True), "res stack")):
        rows.append(Gemm(f"range-gemm-{tag}", "convgemm16<128,128,32,stats>[B2 M300 N256 K128 s1]", 2, 300, 256, 128, form="stats", **kw))
        if "res" in ln_layers:
            rows.append(Res(f"range-res-{tag}", "resconv16<128,64,ph1>[B2 M300 N64 K448 d1]", 64, 300, 1, **kw))
        if "stack" in ln_layers:
            rows.append(Stack(f"range-stack-{tag}", "resstack64<2,4x2>[B3 M214 d1]", (1, 7), 7, 214, **kw))
    return rows


_ALL = {}


def all_cases():
    if not _ALL:
        for c in _dispatch_rows() + _stack_rows() + _range_rows():
            assert c.name not in _ALL, c.name
            _ALL[c.name] = c
    return _ALL


def case_ids():
    return [(n, m) for n, c in all_cases().items() for m in c.modes]


def sizing(case, mode):
    """-> dict(model, truth_l2, truth_row, standin (l2, row), bar_l2, bar_row or None, chain_row): the bars of a case in
    a mode, as the GPU test applies them"""
    model, (bl2, brow) = fm.bars(case.fn(mode))
    t = fm.measures(model, case.truth())
    out = dict(model=model, truth=t, standin=(bl2 / fm.BAR_FACTOR, brow / fm.BAR_FACTOR), bar_l2=bl2, bar_row=brow, chain_row=None)
    if mode == "f16" and case.chain > 1:
        out["bar_l2"], out["chain_row"] = case.one_term_chain_bar()
        out["bar_row"] = None
    return out


if __name__ == "__main__":
    print("| case | mode | model vs truth (L2 / row) | stand-in vs model (L2 / row) | bar L2 | bar row |")
    print("|---|---|---|---|---|---|")
    for name, mode in case_ids():
        s = sizing(all_cases()[name], mode)
        row = "reported only" if s["bar_row"] is None else f"{s['bar_row']:.2e}"
        print(f"| {name} | {mode} | {s['truth'][0]:.2e} / {s['truth'][1]:.2e} | {s['standin'][0]:.2e} / {s['standin'][1]:.2e} | "
              f"{s['bar_l2']:.2e} | {row} |", flush=True)
