"""Parity of the "f16x3" split-operand MFMA mode (csrc/convgemm.hip, pipegemm.hip, resconv.hip; precision 1) -- the
fast arithmetic of the GEMM-class layers.  Same references and same end-to-end bar as the
exact-f32 mode (>= 80 dB SNR against the reference's own outputs; north-star tolerance:
SI-SDR within 0.1 dB); per-kernel tolerance 2e-5 relative L2 (operands carry ~21 bits).
Needs an MI355X."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _log(msg):
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "diag_f16x3.txt"), "a") as f:
        f.write(msg + "\n")
    print(msg)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def snr_db(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return 10 * np.log10(np.sum(ref ** 2) / max(np.sum((got - ref) ** 2), 1e-300))


@pytest.mark.parametrize("frag", [True, False])
@pytest.mark.parametrize("C,T,dil", [(64, 1000, 1), (64, 900, 49), (64, 100, 49), (64, 777, 7), (128, 520, 7),
                                     (128, 300, 1), (256, 300, 49), (512, 130, 7), (512, 200, 49)])
def test_residual_layer_f16x3(C, T, dil, frag):
    """frag=True goes through the halo-staged kernel (resconv16), frag=False through the
    generic chunked kernel (convgemm16)."""
    from acousticswarms_speech_amd import ops
    B, K = 3, 7
    x = _rand(B, C, T, seed=3)
    w = _rand(C, C, K, seed=4, scale=1.0 / math.sqrt(C * K))
    b, g, be = _rand(C, seed=5, scale=0.1), 1 + _rand(C, seed=6, scale=0.1), _rand(C, seed=7, scale=0.1)
    want = F.layer_norm((F.relu(F.conv1d(x, w, b, dilation=dil, padding=3 * dil)) + x).transpose(1, 2), (C,), g, be)
    xc = x.transpose(1, 2).contiguous().cuda()
    out, _ = ops.convgemm(xc, ops.pack_conv_weight(w).cuda(), T, C, C, taps=K, dil=dil, pad=3 * dil, bias=b.cuda(),
                          relu=True, resid=xc, ln=(g.cuda(), be.cuda()), precision="f16x3", use_fragments=frag)
    r = _rel(out.cpu(), want)
    _log(f"f16x3 res C={C} T={T} dil={dil} frag={frag}: rel={r:.3e}")
    assert r < 2e-5


@pytest.mark.parametrize("Cout,T,K", [(64, 1000, 7), (128, 601, 7), (64, 37, 7), (128, 4100, 5), (64, 258, 5)])
def test_stride2_conv_of_64_channels_f16x3(Cout, T, K):
    """EncoderBlock tail of the two full-rate levels -- gate * x -> Conv1d(stride 2) -> GroupNorm(2) -> GLU
    (network.py:101-113) -- through the halo-staged stride-2 kernel (csrc/downconv.hip: even / odd row images,
    transposed accumulators) in f16x3 arithmetic, against torch fp32 and against the generic GEMM (which the
    fragment-free call reaches: the stride-2 kernel needs fragment-order weights)."""
    from acousticswarms_speech_amd import ops
    B, Cin = 3, 64
    x = _rand(B, Cin, T, seed=8)
    w = _rand(2 * Cout, Cin, K, seed=9, scale=1.0 / math.sqrt(Cin * K))
    b = _rand(2 * Cout, seed=10, scale=0.1)
    gate = 0.5 + _rand(Cin, seed=11, scale=0.2)
    gg, gb = 1 + _rand(2 * Cout, seed=12, scale=0.1), _rand(2 * Cout, seed=13, scale=0.1)
    raw = F.conv1d(gate.view(1, -1, 1) * x, w, b, stride=2, padding=K // 2)
    want = F.glu(F.group_norm(raw, 2, gg, gb, 1e-5), dim=1).transpose(1, 2)
    To = raw.shape[-1]
    wt = ops.pack_conv_weight(w * gate.view(1, -1, 1)).cuda()
    xc = x.transpose(1, 2).contiguous().cuda()
    r, st = ops.convgemm(xc, wt, To, 2 * Cout, Cin, taps=K, stride=2, pad=K // 2, bias=b.cuda(), stats_chan_mod=2 * Cout,
                         precision="f16x3")
    r0, st0 = ops.convgemm(xc, wt, To, 2 * Cout, Cin, taps=K, stride=2, pad=K // 2, bias=b.cuda(), stats_chan_mod=2 * Cout,
                           precision="f16x3", use_fragments=False)
    rel_raw, rel_gen = _rel(r.cpu(), raw.transpose(1, 2)), _rel(r.cpu(), r0.cpu())
    out = ops.gn_glu(r, st, gg.cuda(), gb.cuda())
    out0 = ops.gn_glu(r0, st0, gg.cuda(), gb.cuda())
    rel = _rel(out.cpu(), want)
    _log(f"f16x3 down 64->{Cout} K={K} T={T}: raw rel {rel_raw:.3e}, vs generic kernel {rel_gen:.3e}, glu rel {rel:.3e}, "
         f"glu vs generic {_rel(out.cpu(), out0.cpu()):.3e}")
    assert rel_raw < 2e-5 and rel < 2e-5 and rel_gen < 3e-6


def test_wide_and_scaled_operands_f16x3():
    """Plain / stats tiles; operands far from unit scale (tiny weights, large activations,
    values beyond the fp16 range saturate instead of turning into inf/NaN)."""
    from acousticswarms_speech_amd import ops
    B, T, Cin, N = 2, 300, 128, 256
    for wscale, xscale in ((1e-3, 1.0), (1.0, 300.0), (30.0, 1e-2)):
        x = _rand(B, T, Cin, seed=8, scale=xscale)
        w = _rand(N, Cin, seed=9, scale=wscale / math.sqrt(Cin))
        want = F.linear(x, w)
        out, st = ops.convgemm(x.cuda(), w.cuda(), T, N, Cin, stats_chan_mod=N, precision="f16x3")
        r = _rel(out.cpu(), want)
        _log(f"f16x3 wide wscale={wscale} xscale={xscale}: rel={r:.3e}")
        assert r < 2e-5
        s = st.cpu().double().sum(1)
        np.testing.assert_allclose(s[:, 0].numpy(), want[..., :N // 2].double().sum((1, 2)).numpy(), rtol=1e-3, atol=1e-2)
    x = _rand(1, 256, 64, seed=10)
    x[0, 0, 0] = 1e6                                   # beyond fp16: saturates to 65504
    out, _ = ops.convgemm(x.cuda(), _rand(64, 64, seed=11).cuda(), 256, 64, 64, precision="f16x3")
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("M,N,K,skip", [(500, 1024, 256, True), (500, 512, 512, True), (500, 512, 1024, False)])
def test_pipelined_wide_tiles_f16x3(M, N, K, skip):
    """The 256-column pipelined GEMM (convgemm16p) in both forms -- eight waves on 256 rows (K >= 896) and two 4-wave
    workgroups of 128 rows per CU (K <= 512, the decoder's transposed convolutions) -- at a batch that fills >= 512
    tiles, i.e. the shapes the dispatcher sends there: output and GroupNorm partial sums against torch in float64,
    with the skip operand added on load."""
    from acousticswarms_speech_amd import ops
    B = 512 // (2 * (N // 256))                        # two row tiles per item (500 rows: the 256-row form, not 192)
    x = _rand(B, M, K, seed=31)
    x2 = _rand(B, M, K, seed=32) if skip else None
    w = _rand(N, K, seed=33, scale=1 / math.sqrt(K))
    bias = _rand(N, seed=34, scale=0.1)
    want = F.linear(((x + x2) if skip else x).double(), w.double(), bias.double())
    import ctypes
    import json
    from acousticswarms_speech_amd import native
    L = native.lib()
    L.asw_profile_enable(2)
    out, st = ops.convgemm(x.cuda(), w.cuda(), M, N, K, bias=bias.cuda(), stats_chan_mod=N,
                           A2=(x2.cuda() if skip else None), precision="f16x3")
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    native.check(L.asw_profile_report(buf, len(buf)))
    L.asw_profile_enable(0)
    names = list(json.loads(buf.value.decode()))
    r = _rel(out.cpu().double(), want)
    _log(f"pipelined wide tile M={M} N={N} K={K} skip={skip} B={B}: rel={r:.3e} via {names}")
    assert any(n.startswith("convgemm16p<128," if K <= 512 else "convgemm16p<256,") for n in names), names
    assert r < 2e-6
    s = st.cpu().double().sum(1)
    np.testing.assert_allclose(s[:, 0].numpy(), want[..., :N // 2].sum((1, 2)).numpy(), rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(s[:, 1].numpy(), (want[..., :N // 2] ** 2).sum((1, 2)).numpy(), rtol=1e-5)
    np.testing.assert_allclose(s[:, 3].numpy(), (want[..., N // 2:] ** 2).sum((1, 2)).numpy(), rtol=1e-5)


# ---- which kernel a shape is sent to.  (arguments -> launch name in the detailed profile), the names recorded from the
# dispatcher as it stood before its launch functions and its variant cascade were folded into shared helpers.
_DISPATCH = []


def _row(kind, expected, **kw):
    _DISPATCH.append(pytest.param(kind, kw, expected, id=kind + "-" + "-".join(f"{k}{v}" for k, v in kw.items())))


for _N in (64, 128, 256, 512, 1024):                    # LayerNorm epilogue on the generic tiles (one tap: no halo kernel)
    _bk = 32 if _N <= 256 else 16
    _bm = {64: 256, 128: 128, 256: 64, 512: 64, 1024: 32}[_N]
    _row("ln", f"convgemm<{_bm},{_N},{_bk},ln>[B2 M70 N{_N} K{_N} s1]", N=_N, prec="f32")
    _row("ln", f"convgemm16<{_bm},{_N},{_bk},ln>[B2 M70 N{_N} K{_N} s1]", N=_N, prec="f16x3")
for _C, _T, _d, _nm in ((64, 300, 1, "128,64,ph1"), (64, 777, 7, "128,64,poly1"), (64, 4800, 49, "128,64,poly1"),
                        (64, 2400, 49, "128,64,poly2"), (64, 1800, 49, "128,64,poly4"), (64, 900, 49, "128,64,ph1"),
                        (64, 100, 49, "128,64,ph1"), (128, 520, 7, "128,128,ph1,q2"), (128, 2400, 49, "128,128,poly2,q2"),
                        (256, 300, 7, "64,256,ph1,q2"), (512, 200, 1, "64,512,ph1,q2"), (512, 200, 49, "64,512,ph1")):
    _row("res", f"resconv16<{_nm}>[B2 M{_T} N{_C} K{7 * _C} d{_d}]", C=_C, T=_T, dil=_d)      # halo kernel, 7 taps
_row("res", "resconv16<128,64,ph1,glu>[B2 M300 N64 K448 d1]", C=64, T=300, dil=1, glu=True)
_row("down", "downconv64<128x128,stats>[B2 M129 N128 K448 s2]", N=128, T=258)
# wide tiles need B x tiles >= 512; M = 500: two 256-row tiles per item, M = 300: one 192-row tile and a half
for _K, _forms in ((256, ("plain", "stats", "stats+A2")), (1024, ("plain", "stats", "stats+A2", "mul"))):
    for _f in _forms:
        _ep = "plain" if _f in ("plain", "mul") else "stats"
        _m = "m" if _f == "mul" else ""
        _row("gemm", f"convgemm16p{_m}<{128 if _K <= 512 else 256},256,32,{_ep}>[B256 M500 N256 K{_K} s1]",
             B=256, M=500, N=256, K=_K, prec="f16x3", form=_f)
        _row("gemm", f"convgemm16{_m}<256,256,32,{_ep}>[B256 M500 N256 K{_K} s1]",
             B=256, M=500, N=256, K=_K, prec="f16x3", form=_f, frag=False)
_row("gemm", "convgemm16<192,256,32,plain>[B256 M300 N256 K256 s1]", B=256, M=300, N=256, K=256, prec="f16x3", form="plain")
_row("gemm", "convgemm16m<192,256,32,plain>[B256 M300 N256 K256 s1]", B=256, M=300, N=256, K=256, prec="f16x3", form="mul")
for _prec, _k in (("f32", "convgemm"), ("f16x3", "convgemm16")):
    for _f in ("plain", "stats", "stats+A2", "mul"):                                      # 128 x 128
        _nm = f"{_k}{'' if _f != 'mul' else '_m' if _prec == 'f32' else 'm'}<128,128,32,{'plain' if _f in ('plain', 'mul') else 'stats'}>"
        _row("gemm", _nm + "[B2 M300 N256 K128 s1]", B=2, M=300, N=256, K=128, prec=_prec, form=_f)
    for _f in ("plain", "stats"):                                                         # 256 x 64
        _row("gemm", f"{_k}<256,64,32,{_f}>[B2 M300 N192 K128 s1]", B=2, M=300, N=192, K=128, prec=_prec, form=_f)


def _grand(*shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda") * scale


_gemm_cache = {}


def _gemm_case(B, M, N, K):
    """Inputs and float64 references of one GEMM shape, shared by the rows of that shape (one shape kept at a time)."""
    key = (B, M, N, K)
    if key not in _gemm_cache:
        _gemm_cache.clear()
        x, x2 = _grand(B, M, K, seed=41), _grand(B, M, K, seed=42)
        w, bias, mul = _grand(N, K, seed=43, scale=1 / math.sqrt(K)), _grand(N, seed=44, scale=0.1), _grand(B, M, N, seed=45)
        want = F.linear(x.double(), w.double(), bias.double())
        want2 = F.linear(x.double() + x2.double(), w.double(), bias.double())
        _gemm_cache[key] = dict(x=x, x2=x2, w=w, bias=bias, mul=mul, want=want, want2=want2)
    return _gemm_cache[key]


@pytest.mark.parametrize("kind,kw,expected", _DISPATCH)
def test_convgemm_dispatch_table(kind, kw, expected):
    """Every branch of asw_convgemm_f32's dispatch at the smallest shape that reaches it: the launch it makes (read
    from the detailed profile) and its output against torch in float64, at the bounds this file and
    test_gpu_kernels.py use per kernel: 2e-5 relative L2 for f16x3 (operands carry ~21 bits), 2e-6 for exact f32."""
    import ctypes
    import json
    from acousticswarms_speech_amd import native, ops
    prec = kw.get("prec", "f16x3")
    if kind == "ln":                                   # LN(ReLU(x W^T + b) + x), one tap
        N = kw["N"]
        x = _grand(2, 70, N, seed=51)
        w, b = _grand(N, N, seed=52, scale=1 / math.sqrt(N)), _grand(N, seed=53, scale=0.1)
        g, be = 1 + _grand(N, seed=54, scale=0.1), _grand(N, seed=55, scale=0.1)
        want = F.layer_norm(F.relu(F.linear(x.double(), w.double(), b.double())) + x.double(), (N,), g.double(), be.double())
        call = lambda: ops.convgemm(x, w, 70, N, N, bias=b, relu=True, resid=x, ln=(g, be), precision=prec, use_fragments=False)
    elif kind == "res":                                # DilatedResidualLayer, 7 taps, fragment-order weights
        C, T, dil = kw["C"], kw["T"], kw["dil"]
        w = _grand(C, C, 7, seed=62, scale=1 / math.sqrt(7 * C))
        b, g, be = _grand(C, seed=63, scale=0.1), 1 + _grand(C, seed=64, scale=0.1), _grand(C, seed=65, scale=0.1)
        args = dict(taps=7, dil=dil, pad=3 * dil, bias=b, relu=True, ln=(g, be), precision=prec)
        if kw.get("glu"):                              # the input is GLU(GroupNorm(2)(raw)), applied while staging
            raw = _grand(2, T, 2 * C, seed=61) * 1.7 + 0.3
            gg, gb = 1 + _grand(2 * C, seed=66, scale=0.2), _grand(2 * C, seed=67, scale=0.1)
            r = raw.double()
            stats = torch.stack([r[..., :C].sum((1, 2)), (r[..., :C] ** 2).sum((1, 2)), r[..., C:].sum((1, 2)),
                                 (r[..., C:] ** 2).sum((1, 2))], dim=1).float().view(2, 1, 4).contiguous()
            mr = ops.gn_finalize(stats, T, C)
            xd = F.glu(F.group_norm(r.transpose(1, 2), 2, gg.double(), gb.double(), 1e-5), dim=1)      # [B, C, T]
            call = lambda: ops.convgemm(raw, ops.pack_conv_weight(w), T, C, C, resid=raw, a_batch_stride=T * C, a_len=T * C,
                                        B=2, glu=(raw, mr, gg, gb), **args)
        else:
            x = _grand(2, T, C, seed=61)
            xd = x.double().transpose(1, 2)
            call = lambda: ops.convgemm(x, ops.pack_conv_weight(w), T, C, C, resid=x, **args)
        want = F.layer_norm((F.relu(F.conv1d(xd, w.double(), b.double(), dilation=dil, padding=3 * dil)) + xd).transpose(1, 2),
                            (C,), g.double(), be.double())
    elif kind == "down":                               # stride-2 convolution of a 64-channel tensor, with partial sums
        N, T = kw["N"], kw["T"]
        x = _grand(2, T, 64, seed=71)
        w, b = _grand(N, 64, 7, seed=72, scale=1 / math.sqrt(7 * 64)), _grand(N, seed=73, scale=0.1)
        want = F.conv1d(x.double().transpose(1, 2), w.double(), b.double(), stride=2, padding=3).transpose(1, 2)
        call = lambda: ops.convgemm(x, ops.pack_conv_weight(w), want.shape[1], N, 64, taps=7, stride=2, pad=3, bias=b,
                                    stats_chan_mod=N, precision=prec)
    else:                                              # plain GEMM tiles: x W^T + b, optionally (x + x2), * mul, partial sums
        B, M, N, K, form = kw["B"], kw["M"], kw["N"], kw["K"], kw["form"]
        c = _gemm_case(B, M, N, K)
        want = c["want2"] if form == "stats+A2" else c["want"] * c["mul"].double() if form == "mul" else c["want"]
        call = lambda: ops.convgemm(c["x"], c["w"], M, N, K, bias=c["bias"], precision=prec, use_fragments=kw.get("frag", True),
                                    stats_chan_mod=N if form.startswith("stats") else 0,
                                    A2=c["x2"] if form == "stats+A2" else None, mul=c["mul"] if form == "mul" else None)
    L = native.lib()
    L.asw_profile_enable(2)
    out, _ = call()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    native.check(L.asw_profile_report(buf, len(buf)))
    L.asw_profile_enable(0)
    names = list(json.loads(buf.value.decode()))
    r = float((out.double() - want).norm() / want.norm())
    _log(f"dispatch {kind} {kw}: {names} rel={r:.3e}")
    assert names == [expected]
    assert r < (2e-6 if prec == "f32" else 2e-5)


def _model(cfg, seed, batch=32):
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    return SpotModel(cfg, make_spot_state_dict(cfg, seed), batch_size=batch, precision="f16x3").to("cuda")


def test_forward_full_f16x3_vs_reference_golden(golden):
    from acousticswarms_speech_amd.config import FULL
    g = golden("g3_spot_full")
    m = _model(FULL, 5)
    rng = np.random.default_rng(31)
    x = torch.from_numpy(rng.standard_normal((2, 7, 12288)).astype(np.float32))
    y = m.forward(x, torch.tensor([[0.0, 1.0]] * 2)).cpu().numpy()
    s = snr_db(y, g["y"])
    _log(f"f16x3 full forward: SNR vs reference {s:.1f} dB")
    for k in ["bottleneck", "dec4"]:
        probe, idx = g[f"{k}_probe"], g[f"{k}_idx"]
        tap = m.get_tap(k).cpu().numpy().reshape(2, -1, probe.shape[1])
        _log(f"f16x3 tap {k}: probe SNR {snr_db(tap[:, idx, :].transpose(0, 2, 1), probe):.1f} dB")
    assert s > 80.0


def test_shift_and_sep_full_f16x3_vs_reference_golden(golden):
    from acousticswarms_speech_amd.config import FULL
    from acousticswarms_speech_amd.scenes import make_scene
    from oracle import spot_ref
    g = golden("g4b_shift_and_sep_full")
    m = _model(FULL, 5, batch=4)
    mix = torch.from_numpy(make_scene(2, 3, 7, 6000).mix)
    for strict in (0, 1):
        y = m.shift_and_sep(mix, list(g["offsets"]), Strict=strict)
        ref = g[f"y_strict{strict}"]
        per = [snr_db(y[i], ref[i]) for i in range(y.shape[0])]
        _log(f"f16x3 shift_and_sep strict={strict}: per-candidate SNR {np.round(per, 1)}")
        assert min(per) > 80.0
        en = m.shift_and_score(mix, list(g["offsets"]), Strict=strict, window=1500)
        np.testing.assert_allclose(en, spot_ref.candidate_energies(ref, 1500), rtol=1e-4)
    m.set_precision("f32")
    y32 = m.shift_and_sep(mix, list(g["offsets"]), Strict=1)
    assert min(snr_db(y32[i], g["y_strict1"][i]) for i in range(5)) > 100.0


@pytest.mark.parametrize("T", [1000, 128, 77])
def test_groupnorm_glu_on_load_is_bit_identical(T):
    """The first residual layer of a 64-channel decoder block can take its input as the un-normalised
    2 x 64-channel tensor and apply GroupNorm(2) + GLU while it stages its rows (asw_convgemm_args.glu_raw):
    same bits as asw_gn_glu followed by the plain layer, including the zero padding at both ends."""
    from acousticswarms_speech_amd import ops
    B, C, K = 3, 64, 7
    raw = (_rand(B, T, 2 * C, seed=70) * 1.7 + 0.3).cuda()
    gamma, beta = (1 + 0.2 * _rand(2 * C, seed=71)).cuda(), (0.1 * _rand(2 * C, seed=72)).cuda()
    w = _rand(C, C, K, seed=73, scale=1 / math.sqrt(C * K))
    bias, lg, lb = _rand(C, seed=74, scale=0.1).cuda(), (1 + 0.1 * _rand(C, seed=75)).cuda(), (0.1 * _rand(C, seed=76)).cuda()
    r = raw.double()
    stats = torch.stack([r[..., :C].sum((1, 2)), (r[..., :C] ** 2).sum((1, 2)), r[..., C:].sum((1, 2)),
                         (r[..., C:] ** 2).sum((1, 2))], dim=1).float().view(B, 1, 4).contiguous()
    g = ops.gn_glu(raw, stats, gamma, beta)
    Wt = ops.pack_conv_weight(w).cuda()
    kw = dict(taps=K, pad=3, bias=bias, relu=True, ln=(lg, lb), precision="f16x3")
    want, _ = ops.convgemm(g, Wt, T, C, C, resid=g, **kw)
    mr = ops.gn_finalize(stats, T, C)
    got, _ = ops.convgemm(raw, Wt, T, C, C, resid=raw, a_batch_stride=T * C, a_len=T * C, B=B,
                          glu=(raw, mr, gamma, beta), **kw)
    assert torch.equal(got, want)
    with pytest.raises(RuntimeError):                # any other layer shape refuses instead of ignoring the request
        ops.convgemm(raw, Wt, T, C, C, resid=raw, a_batch_stride=T * C, a_len=T * C, B=B, dil=7, glu=(raw, mr, gamma, beta),
                     **dict(kw, pad=21))


@pytest.mark.parametrize("C,T", [(64, 333), (128, 1000), (128, 77), (256, 300), (256, 3008), (512, 200), (512, 64)])
def test_groupnorm_glu_on_load_wide_blocks_and_side_output(C, T):
    """The same at 128 / 256 / 512 channels (the image holds one 64-channel slice at a time): the layer also writes
    the normalised rows of its own output range to glu_out -- the encoder's skip connection -- and reads its residual
    back from there.  Output and side tensor equal asw_gn_glu + the plain layer bit for bit."""
    from acousticswarms_speech_amd import ops
    B, K = (5 if T == 3008 else 2), 7                 # 256 channels: the 128-row tile needs >= 512 workgroups, else 64 rows
    raw = (_rand(B, T, 2 * C, seed=170) * 1.3 - 0.2).cuda()
    gamma, beta = (1 + 0.2 * _rand(2 * C, seed=171)).cuda(), (0.1 * _rand(2 * C, seed=172)).cuda()
    w = _rand(C, C, K, seed=173, scale=1 / math.sqrt(C * K))
    bias, lg, lb = _rand(C, seed=174, scale=0.1).cuda(), (1 + 0.1 * _rand(C, seed=175)).cuda(), (0.1 * _rand(C, seed=176)).cuda()
    r = raw.double()
    stats = torch.stack([r[..., :C].sum((1, 2)), (r[..., :C] ** 2).sum((1, 2)), r[..., C:].sum((1, 2)),
                         (r[..., C:] ** 2).sum((1, 2))], dim=1).float().view(B, 1, 4).contiguous()
    g = ops.gn_glu(raw, stats, gamma, beta)
    Wt = ops.pack_conv_weight(w).cuda()
    kw = dict(taps=K, pad=3, bias=bias, relu=True, ln=(lg, lb), precision="f16x3")
    want, _ = ops.convgemm(g, Wt, T, C, C, resid=g, **kw)
    mr = ops.gn_finalize(stats, T, C)
    side = torch.full((B, T, C), float("nan"), device="cuda")
    got, _ = ops.convgemm(raw, Wt, T, C, C, resid=raw, a_batch_stride=T * C, a_len=T * C, B=B,
                          glu=(raw, mr, gamma, beta), glu_out=side, **kw)
    _log(f"glu-on-load C={C} T={T}: out max diff {float((got - want).abs().max()):.2e}, side max diff {float((side - g).abs().max()):.2e}")
    assert torch.equal(side, g)
    assert torch.equal(got, want)
    if C > 64:
        with pytest.raises(RuntimeError):            # no place for the residual: refused
            ops.convgemm(raw, Wt, T, C, C, resid=raw, a_batch_stride=T * C, a_len=T * C, B=B, glu=(raw, mr, gamma, beta), **kw)


def test_single_pass_f16_mode_vs_reference_golden(golden):
    """precision="f16": one MFMA per product on round-to-nearest fp16 halves (the reference's own half-precision
    switch, `use_fp16`, is bf16 autocast and hard-wired off).  An OPTIONAL mode, never the headline: against the
    reference's outputs the FULL network stays above 40 dB (47 measured; north-star tolerance 0.1 dB SI-SDR needs
    ~35), per-layer error 2e-3 instead of 2e-5."""
    from acousticswarms_speech_amd import ops
    from acousticswarms_speech_amd.config import FULL
    from acousticswarms_speech_amd.scenes import make_scene
    g = golden("g4b_shift_and_sep_full")
    m = _model(FULL, 5, batch=4)
    m.set_precision("f16")
    mix = torch.from_numpy(make_scene(2, 3, 7, 6000).mix)
    y = m.shift_and_sep(mix, list(g["offsets"]), Strict=1)
    per = [snr_db(y[i], g["y_strict1"][i]) for i in range(y.shape[0])]
    _log(f"single-pass f16 shift_and_sep: per-candidate SNR vs reference {np.round(per, 1)}")
    assert min(per) > 40.0
    C, T, K = 128, 520, 7
    x = _rand(2, T, C, seed=90).cuda()
    w = _rand(C, C, K, seed=91, scale=1 / math.sqrt(C * K))
    b, lg, lb = _rand(C, seed=92, scale=0.1).cuda(), (1 + 0.1 * _rand(C, seed=93)).cuda(), (0.1 * _rand(C, seed=94)).cuda()
    Wt = ops.pack_conv_weight(w).cuda()
    kw = dict(taps=K, dil=7, pad=21, bias=b, relu=True, resid=x, ln=(lg, lb))
    want, _ = ops.convgemm(x, Wt, T, C, C, precision="f32", **kw)
    got, _ = ops.convgemm(x, Wt, T, C, C, precision="f16", **kw)
    rel = _rel(got.cpu(), want.cpu())
    _log(f"single-pass f16 residual layer rel={rel:.2e}")
    assert rel < 2e-3


def test_fused_mask_path_matches_three_gemm_path(golden):
    """f16x3 runs the mask path as one launch by default (asw_mask_path_f16x3: no latent in memory); the
    three-GEMM path stays selectable.  Both against the reference's own output (g4b) and against each
    other; the "latent" tap exists on the three-GEMM path only; the fused path keeps the range guard."""
    from acousticswarms_speech_amd import ops
    from acousticswarms_speech_amd.config import FULL
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    from acousticswarms_speech_amd.spot import SpotModel
    g = golden("g4b_shift_and_sep_full")
    m = _model(FULL, 5, batch=4)
    mix = torch.from_numpy(make_scene(2, 3, 7, 6000).mix)
    y_fused = m.shift_and_sep(mix, list(g["offsets"]), Strict=1)
    with pytest.raises(RuntimeError):
        m.get_tap("latent")
    m.set_fused_mask(False)
    y_three = m.shift_and_sep(mix, list(g["offsets"]), Strict=1)
    assert m.get_tap("latent").numel() > 0
    ref = g["y_strict1"]
    per_f = [snr_db(y_fused[i], ref[i]) for i in range(ref.shape[0])]
    per_t = [snr_db(y_three[i], ref[i]) for i in range(ref.shape[0])]
    both = [snr_db(y_fused[i], y_three[i]) for i in range(ref.shape[0])]
    _log(f"mask path fused {np.round(per_f, 1)} dB, three GEMMs {np.round(per_t, 1)} dB vs reference; "
         f"fused vs three {np.round(both, 1)} dB")
    assert min(per_f) > 80.0 and min(per_t) > 80.0 and min(both) > 90.0
    sd = make_spot_state_dict(FULL, 5)
    big = dict(sd)
    big["mask_encoder.weight"] = sd["mask_encoder.weight"] * 3.0e3
    big["reference_bypass.weight"] = sd["reference_bypass.weight"] * 3.0e3
    ops.f16x3_overflow_count(reset=True)
    SpotModel(FULL, big, batch_size=2, precision="f16x3").to("cuda").shift_and_sep(mix, list(g["offsets"])[:2], Strict=1)
    assert ops.f16x3_overflow_count(reset=True) > 0


def test_f16x3_range_guard_counts_saturating_activations():
    """The f16x3 mode splits activations to fp16 halves that saturate at +-65504.  The plain GEMM
    epilogue counts un-normalised outputs beyond that range (asw_f16x3_overflow_count): zero for
    the seeded network, non-zero once the mask path is scaled so that the latent exceeds it -- and
    the exact-f32 mode of the same weights is not flagged."""
    from acousticswarms_speech_amd import ops
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    mix = torch.from_numpy(make_scene(7, 2, 7, 4000).mix)
    offs = [np.array([0, 0, 0, 0, 0, 0]), np.array([3, -5, 8, -13, 21, -34])]
    sd = make_spot_state_dict(SMALL, seed=3)
    ops.f16x3_overflow_count(reset=True)
    SpotModel(SMALL, sd, batch_size=4, precision="f16x3").to("cuda").shift_and_sep(mix, offs, Strict=1)
    assert ops.f16x3_overflow_count(reset=True) == 0
    big = dict(sd)
    big["mask_encoder.weight"] = sd["mask_encoder.weight"] * 3.0e3
    big["reference_bypass.weight"] = sd["reference_bypass.weight"] * 3.0e3
    SpotModel(SMALL, big, batch_size=4, precision="f32").to("cuda").shift_and_sep(mix, offs, Strict=1)
    assert ops.f16x3_overflow_count(reset=True) == 0          # the exact mode has no such limit
    SpotModel(SMALL, big, batch_size=4, precision="f16x3").to("cuda").shift_and_sep(mix, offs, Strict=1)
    assert ops.f16x3_overflow_count(reset=True) > 0


def test_f16x3_range_guard_counts_in_both_translation_units():
    """The counter behind asw_f16x3_overflow_count exists once per translation unit that writes it: pipegemm.hip
    (convgemm16p, the mask path) and convgemm.hip (the two-barrier kernels).  One shape of the dispatch table reaches
    either file with and without fragment-order weights: each file counts, each is cleared by a reset, and the
    call returns the sum of the two."""
    import ctypes
    import json
    from acousticswarms_speech_amd import native, ops
    B, M, N, K = 256, 500, 256, 256
    unit = _gemm_case(B, M, N, K)
    # output standard deviation near 1e6, far beyond 65504, from inputs that fp16 still holds (|x|, |w| < 1e4)
    big_x, big_w = _grand(B, M, K, seed=46, scale=1e3), _grand(N, K, seed=47, scale=1e3 / math.sqrt(K))
    names = {True: "convgemm16p<128,256,32,plain>[B256 M500 N256 K256 s1]",        # pipegemm.hip
             False: "convgemm16<256,256,32,plain>[B256 M500 N256 K256 s1]"}        # convgemm.hip
    L = native.lib()

    def run(x, w, bias, frag):
        L.asw_profile_enable(2)
        ops.convgemm(x, w, M, N, K, bias=bias, precision="f16x3", use_fragments=frag)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        native.check(L.asw_profile_report(buf, len(buf)))
        L.asw_profile_enable(0)
        assert list(json.loads(buf.value.decode())) == [names[frag]]

    ops.f16x3_overflow_count(reset=True)
    single = {}
    for frag in (True, False):
        run(unit["x"], unit["w"], unit["bias"], frag)
        assert ops.f16x3_overflow_count(reset=False) == 0
        run(big_x, big_w, None, frag)
        single[frag] = ops.f16x3_overflow_count(reset=True)
        _log(f"range guard frag={frag}: {single[frag]} threads")
        assert single[frag] > 0
        assert ops.f16x3_overflow_count(reset=True) == 0
    run(big_x, big_w, None, True)
    run(big_x, big_w, None, False)
    assert ops.f16x3_overflow_count(reset=False) == single[True] + single[False]
    assert ops.f16x3_overflow_count(reset=True) == single[True] + single[False]          # (this call clears both)
    assert ops.f16x3_overflow_count(reset=True) == 0
