"""precision="f16x3_safe" (ABI value 3): the f16x3 kernels wherever a GEMM reads a normalised tensor, the exact f32
kernels where it reads an un-normalised one (attention context, feed-forward hidden layer, masked latent), and the
one-launch mask path with a per-frame power-of-two scale (asw_mask_path_f16x3_scaled).  The rule is Trunk::site in
csrc/model_common.h.  Needs an MI355X.

1. parity on the reference's own outputs at the project's bars (>= 80 dB, energies to 1e-4, range guard 0);
2. function-preserving rescalings (tests/safe_precision_cases.py; exactness shown on the CPU by
   test_rescaling_oracle_host.py): f16x3 trips the guard, f32 and f16x3_safe keep >= 80 dB, f16x3_safe with guard 0;
3. the scaled mask-path kernel alone against a float64 numpy statement of the formula in include/asw_hip.h, on both
   feeds (ASW_NO_RESIDUE_FEED=1 is read once per process: a fresh child);
4. the site plan read from the launch profiler;
5. switching the mode leaves no state behind.

Notes on the cases.
 * The g4_shift_and_sep fixture is the reference's output for the TINY network (8 channels), which the MFMA tiles do
   not accept; the SMALL spot network is therefore held to the reference's own SMALL outputs, g2b_spot_small
   (Network.forward), and its shift_and_sep to the oracle in the rescaling case.
 * 3(a): asw_pack_fragments_f16 bounds a weight tensor's power-of-two pre-scale to +-24, so over k = -20 .. 40 the
   fp16 images of enc_w * 2**k are the same bits only if the weights need no lo half at the coarsest placement: enc_w
   carries 8 significant bits there.  The activations, the biases and the latent keep full fp32 mantissas, and the
   latent's scaling is what the case is about.
 * 3(c): the kernel splits its two activation inputs (x and the reference rows) to fp16 unscaled -- they are
   normalised tensors by contract -- so the frames' magnitudes are driven with inputs inside the fp16 range: a block of
   frames whose x window is silent (mask = the encoder bias, 2**-20 |r|), a block at unit scale, and a block with x
   and the reference rows both times 2**12 (latent times 2**24).
"""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.safe_precision_cases import S, SPOT_OFFSETS, rescale_sep, rescale_spot   # noqa: E402

pytestmark = pytest.mark.gpu

BAR_DB = 80.0            # end to end against the reference's own outputs
BAR_KERNEL = 5e-6        # per kernel, relative L2


def _log(msg):
    print(msg)


def snr_db(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return 10 * np.log10(np.sum(ref ** 2) / max(np.sum((got - ref) ** 2), 1e-300))


def _guard(reset=True):
    from acousticswarms_speech_amd import ops
    return ops.f16x3_overflow_count(reset=reset)


_models = {}


def _spot(cfg_name, seed, rescaled=False, batch=4):
    """one device model per (network, weights), shared by the tests; every test sets the precision it wants"""
    key = ("spot", cfg_name, seed, rescaled)
    if key not in _models:
        from acousticswarms_speech_amd import config
        from acousticswarms_speech_amd.spot import SpotModel
        from acousticswarms_speech_amd.weights import make_spot_state_dict
        cfg = getattr(config, cfg_name)
        sd = make_spot_state_dict(cfg, seed)
        if rescaled:
            sd = rescale_spot(sd, cfg)
        _models[key] = SpotModel(cfg, sd, batch_size=batch, precision="f16x3").to("cuda")
    return _models[key]


def _sep(seed, rescaled=False):
    key = ("sep", seed, rescaled)
    if key not in _models:
        from acousticswarms_speech_amd.config import SEP_SMALL
        from acousticswarms_speech_amd.sep import SepModel
        from acousticswarms_speech_amd.weights import make_sep_state_dict
        sd = make_sep_state_dict(SEP_SMALL, seed)
        if rescaled:
            sd = rescale_sep(sd, SEP_SMALL)
        _models[key] = SepModel(SEP_SMALL, sd, precision="f16x3").to("cuda")
    return _models[key]


# ------------------------------------------------------------------ 1. parity on the reference's own outputs
def test_spot_full_vs_reference_golden(golden):
    from acousticswarms_speech_amd.scenes import make_scene
    from oracle import spot_ref
    g = golden("g4b_shift_and_sep_full")
    m = _spot("FULL", 5)
    mix = torch.from_numpy(make_scene(2, 3, 7, 6000).mix)
    offs = list(g["offsets"])
    assert len(offs) == 5
    for strict in (0, 1):
        ref = g[f"y_strict{strict}"]
        worst = {}
        for prec in ("f16x3", "f16x3_safe"):
            m.set_precision(prec)
            _guard()
            y = m.shift_and_sep(mix, offs, Strict=strict)
            en = m.shift_and_score(mix, offs, Strict=strict, window=1500)
            count = _guard()
            per = [snr_db(y[i], ref[i]) for i in range(5)]
            worst[prec] = min(per)
            _log(f"spot FULL strict={strict} {prec}: per-candidate SNR {np.round(per, 1)} dB, guard {count}")
            if prec == "f16x3_safe":
                assert min(per) > BAR_DB
                np.testing.assert_allclose(en, spot_ref.candidate_energies(ref, 1500), rtol=1e-4)
                assert count == 0
        _log(f"spot FULL strict={strict}: worst candidate f16x3 {worst['f16x3']:.1f} dB, f16x3_safe {worst['f16x3_safe']:.1f} dB")


def test_spot_small_vs_reference_golden(golden):
    g = golden("g2b_spot_small")
    m = _spot("SMALL", 21)
    for T in (4800, 5000):
        rng = np.random.default_rng(200 + T)
        x = torch.from_numpy(rng.standard_normal((3, 7, T)).astype(np.float32))
        for wi, w in enumerate(([1.0, 0.0], [0.0, 1.0])):
            ref = g[f"y_T{T}_w{wi}"]
            fig = {}
            for prec in ("f16x3", "f16x3_safe"):
                m.set_precision(prec)
                _guard()
                y = m.forward(x, torch.tensor([w] * 3)).cpu().numpy()
                fig[prec] = (snr_db(y, ref), _guard())
            _log(f"spot SMALL forward T={T} w={wi}: f16x3 {fig['f16x3'][0]:.1f} dB, f16x3_safe {fig['f16x3_safe'][0]:.1f} dB "
                 f"(guard {fig['f16x3_safe'][1]})")
            assert fig["f16x3_safe"][0] > BAR_DB and fig["f16x3_safe"][1] == 0


def test_sep_small_vs_reference_golden(golden):
    from acousticswarms_speech_amd.scenes import make_scene
    ga, gb = golden("g11a_sep_forward_small"), golden("g11b_sep_infer_small")
    m = _sep(31)
    for t in (2048, 2100):                                   # g11a: Network.forward
        rng = np.random.default_rng(500 + t)
        x = torch.from_numpy(rng.standard_normal((2, 21, t)).astype(np.float32))
        fig = {}
        for prec in ("f16x3", "f16x3_safe"):
            m.set_precision(prec)
            _guard()
            fig[prec] = (snr_db(m(x, torch.tensor([[3], [3]])).cpu().numpy(), ga[f"y_t{t}"]), _guard())
        _log(f"sep SMALL forward t={t}: f16x3 {fig['f16x3'][0]:.1f} dB, f16x3_safe {fig['f16x3_safe'][0]:.1f} dB")
        assert fig["f16x3_safe"][0] > BAR_DB and fig["f16x3_safe"][1] == 0
    mix = torch.from_numpy(make_scene(4, 3, 7, 4000).mix)
    for i in range(3):                                       # g11b: infer_sample, 2 / 3 / 6 speakers
        fig = {}
        for prec in ("f16x3", "f16x3_safe"):
            m.set_precision(prec)
            _guard()
            fig[prec] = (snr_db(m.infer_sample(mix, list(gb[f"samples{i}"])), gb[f"y{i}"]), _guard())
        _log(f"sep SMALL infer_sample case {i} (S={gb[f'y{i}'].shape[0]}): f16x3 {fig['f16x3'][0]:.1f} dB, "
             f"f16x3_safe {fig['f16x3_safe'][0]:.1f} dB")
        assert fig["f16x3_safe"][0] > BAR_DB and fig["f16x3_safe"][1] == 0


# ------------------------------------------------------------------ 2. function-preserving rescalings
def _rescaled_spot_case(m, mix, offs, strict, ref, what, energy_window):
    from oracle import spot_ref
    m.set_precision("f16x3")
    _guard()
    m.shift_and_sep(mix, offs, Strict=strict)
    tripped = _guard()
    _log(f"{what} rescaled by 2**20, f16x3: guard {tripped}")
    assert tripped > 0                                       # the witness: these inputs really leave the fp16 range
    m.set_precision("f32")
    y32 = m.shift_and_sep(mix, offs, Strict=strict)
    per32 = [snr_db(y32[i], ref[i]) for i in range(len(offs))]
    m.set_precision("f16x3_safe")
    _guard()
    y = m.shift_and_sep(mix, offs, Strict=strict)
    en = m.shift_and_score(mix, offs, Strict=strict, window=energy_window)
    count = _guard()
    per = [snr_db(y[i], ref[i]) for i in range(len(offs))]
    _log(f"{what} rescaled by 2**20: f32 {np.round(per32, 1)} dB, f16x3_safe {np.round(per, 1)} dB, guard {count}")
    assert min(per32) > BAR_DB
    assert count == 0
    assert min(per) > BAR_DB
    np.testing.assert_allclose(en, spot_ref.candidate_energies(ref, energy_window), rtol=1e-4)


def test_rescaled_spot_small():
    """SMALL (three-GEMM mask path: 128 encoder channels fit no 256-column tile): the oracle on the ORIGINAL weights is
    the expected output (the rescaled network computes the same function bit for bit)."""
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    from oracle import spot_ref
    mix = torch.from_numpy(make_scene(7, 2, 7, 4000).mix)
    ref = spot_ref.shift_and_sep(make_spot_state_dict(SMALL, 3), SMALL, mix, SPOT_OFFSETS, strict=1)
    _rescaled_spot_case(_spot("SMALL", 3, rescaled=True), mix, SPOT_OFFSETS, 1, ref, "spot SMALL", 1500)


def test_rescaled_spot_full(golden):
    """FULL (the one-launch mask path): the fixture g4b itself is the expected output"""
    from acousticswarms_speech_amd.scenes import make_scene
    g = golden("g4b_shift_and_sep_full")
    mix = torch.from_numpy(make_scene(2, 3, 7, 6000).mix)
    _rescaled_spot_case(_spot("FULL", 5, rescaled=True), mix, list(g["offsets"]), 1, g["y_strict1"], "spot FULL", 1500)


def test_rescaled_sep_small(golden):
    """inter-speaker feed-forward pairs and the mask path times 2**20: the fixture g11b is the expected output"""
    from acousticswarms_speech_amd.scenes import make_scene
    g = golden("g11b_sep_infer_small")
    m = _sep(31, rescaled=True)
    mix = torch.from_numpy(make_scene(4, 3, 7, 4000).mix)
    for i in range(3):
        samples, ref = list(g[f"samples{i}"]), g[f"y{i}"]
        m.set_precision("f16x3")
        _guard()
        m.infer_sample(mix, samples)
        tripped = _guard()
        m.set_precision("f32")
        s32 = snr_db(m.infer_sample(mix, samples), ref)
        m.set_precision("f16x3_safe")
        _guard()
        s = snr_db(m.infer_sample(mix, samples), ref)
        count = _guard()
        _log(f"sep SMALL rescaled by 2**20 case {i}: f16x3 guard {tripped}; f32 {s32:.1f} dB, f16x3_safe {s:.1f} dB, guard {count}")
        assert tripped > 0
        assert s32 > BAR_DB
        assert count == 0 and s > BAR_DB


# ------------------------------------------------------------------ 3. the scaled mask-path kernel alone
EK, ES, PAD = 33, 16, 16
KERNEL_CASES = [(E, C, Fr) for E in (256, 512) for C in (32, 64) for Fr in (130, 257)]
KS = (-20, 10, 20, 40)


def _rand(*shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _profile_names(fn):
    """fn() under the detailed launch profile -> (its result, {launch name: launches})"""
    from acousticswarms_speech_amd import native
    L = native.lib()
    L.asw_profile_enable(2)
    try:
        out = fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 18)
        native.check(L.asw_profile_report(buf, len(buf)))
    finally:
        L.asw_profile_enable(0)
    return out, {k: v["launches"] for k, v in json.loads(buf.value.decode()).items()}


def _mask_want(x, refx, enc_w, enc_b, byp_w, byp_b, dec_w, frames):
    """float64: taps[c][b][f][j] = sum_{e in column tile c} relu(enc(x)[b][f][e] + bias_e) * relu(byp(ref)[b][f][e] + byp_bias_e) * D[e][j]
    x [B][Tp][C], refx [B][RL] (frame f reads refx[b][f*ES + k]), enc_w [E][C][EK], byp_w / dec_w [E][1][EK]"""
    B, Tp, C = x.shape
    E = enc_w.shape[0]
    xp = np.zeros((B, Tp + 2 * PAD + ES, C))
    xp[:, PAD:PAD + Tp] = x
    idx = np.arange(frames)[:, None] * ES + np.arange(EK)[None, :]
    wm = enc_w.astype(np.float64).transpose(0, 2, 1).reshape(E, EK * C)           # [e][k*C + c]
    mask = xp[:, idx].reshape(B, frames, EK * C) @ wm.T + (0.0 if enc_b is None else enc_b.astype(np.float64))
    byp = refx.astype(np.float64)[:, idx] @ byp_w[:, 0].astype(np.float64).T
    byp = byp + (0.0 if byp_b is None else byp_b.astype(np.float64))
    lat = (np.maximum(mask, 0.0) * np.maximum(byp, 0.0)).reshape(B, frames, E // 256, 256)
    wd = dec_w[:, 0].astype(np.float64).reshape(E // 256, 256, EK)
    return np.stack([lat[:, :, c] @ wd[c] for c in range(E // 256)])


def _frame_err(parts, want):
    """per-frame relative L2 over a frame's partial taps, worst frame (frames whose expected value is zero excluded)"""
    got = parts[..., :EK].astype(np.float64)
    num = np.sqrt(((got - want) ** 2).sum(axis=(0, 3)))
    den = np.sqrt((want ** 2).sum(axis=(0, 3)))
    return float((num[den > 0] / den[den > 0]).max())


def _kernel_figures(E, C, frames):
    from acousticswarms_speech_amd import ops
    B, Tp = 2, frames * ES
    RL = ((PAD + Tp + 48 + 64) + 3) & ~3
    seed = 1000 + E + 7 * C + frames
    x = _rand(B, Tp, C, seed=seed)
    refx = np.zeros((B, RL), np.float32)
    refx[:, PAD:PAD + Tp] = _rand(B, Tp, seed=seed + 1)
    enc_w, enc_b = _rand(E, C, EK, seed=seed + 2, scale=1 / math.sqrt(C * EK)), _rand(E, seed=seed + 3, scale=0.1)
    byp_w, byp_b = _rand(E, 1, EK, seed=seed + 4, scale=0.2), _rand(E, seed=seed + 5, scale=0.1)
    dec_w = _rand(E, 1, EK, seed=seed + 6, scale=1 / math.sqrt(E))
    t = torch.from_numpy

    def run(xa, ra, ew, eb, bb, scaled):
        _guard()
        parts, names = _profile_names(lambda: ops.mask_path(
            t(xa).cuda(), t(ra).cuda(), ES, t(ew), None if eb is None else t(eb).cuda(), t(byp_w),
            None if bb is None else t(bb).cuda(), t(dec_w), frames, ES, PAD, scaled=scaled))
        assert parts.shape == (E // 256, B, frames, 64)
        return parts.cpu().numpy(), names, _guard()

    fig = {}
    # (a) homogeneity: enc_w with 8 significant bits (module docstring), everything else as drawn
    q = np.clip(np.rint(enc_w * 2.0 ** 12 * (0.02 * math.sqrt(C * EK))), -255, 255).astype(np.float32) * np.float32(2.0 ** -12)
    base, names, g0 = run(x, refx, q, enc_b, byp_b, True)
    fig["names"] = sorted(names)
    fig["guard_k0"] = g0
    fig["homog"] = {}
    for k in KS:
        s = np.float32(2.0 ** k)
        got, _n, gk = run(x, refx, q * s, enc_b * s, byp_b, True)
        fig["homog"][str(k)] = bool(np.isfinite(got).all() and np.array_equal(got, base * s) and gk == 0)
    # (b) accuracy in range, against the unscaled kernel on the same data
    want = _mask_want(x, refx, enc_w, enc_b, byp_w, byp_b, dec_w, frames)
    ps, _n, gs = run(x, refx, enc_w, enc_b, byp_b, True)
    pu, names_u, gu = run(x, refx, enc_w, enc_b, byp_b, False)
    fig["names_unscaled"] = sorted(names_u)
    fig["acc_scaled"], fig["acc_unscaled"], fig["acc_guards"] = _frame_err(ps, want), _frame_err(pu, want), [gs, gu]
    # (c) mixed magnitudes in one tile: blocks of frames with the latent at 2**-20 (silent x window: mask = bias), 1, 2**24
    xm, rm = x.copy(), refx.copy()
    third = frames // 3
    xm[:, :third * ES] = 0.0
    xm[:, 2 * third * ES:] *= np.float32(2.0 ** 12)
    rm[:, PAD + 2 * third * ES:] *= np.float32(2.0 ** 12)
    eb = np.abs(enc_b) * np.float32(2.0 ** -20)
    wantm = _mask_want(xm, rm, enc_w, eb, byp_w, None, dec_w, frames)
    pm, _n, gm = run(xm, rm, enc_w, eb, None, True)
    _pu, _n, gmu = run(xm, rm, enc_w, eb, None, False)
    mag = np.sqrt((wantm ** 2).sum(axis=(0, 3)))
    fig["mixed"], fig["mixed_guards"] = _frame_err(pm, wantm), [gm, gmu]
    fig["mixed_span_log2"] = float(np.log2(mag.max() / mag[mag > 0].min()))
    # (d) a silent item, and one inf in the encoder bias
    rz = refx.copy()
    rz[0] = 0.0
    pz, _n, gz = run(x, rz, enc_w, enc_b, None, True)
    fig["silent"] = bool(np.all(pz[:, 0] == 0.0) and np.isfinite(pz).all() and gz == 0)
    ebi = enc_b.copy()
    ebi[E // 2] = np.inf
    _pi, _n, fig["inf_guard"] = run(x, refx, enc_w, ebi, byp_b, True)
    return fig


def _check_kernel(fig, what):
    _log(f"scaled mask path {what}: " + json.dumps(fig))
    want_res = "ASW_NO_RESIDUE_FEED" not in os.environ
    for names, prefix in ((fig["names"], "maskpath16ps<256,256,32>["), (fig["names_unscaled"], "maskpath16p<256,256,32>[")):
        assert len(names) == 1 and names[0].startswith(prefix), names
        assert names[0].endswith(" res]") == want_res, (names, want_res)
    assert fig["guard_k0"] == 0
    assert all(fig["homog"].values()) and set(fig["homog"]) == {str(k) for k in KS}, fig["homog"]
    assert fig["acc_guards"] == [0, 0]
    assert fig["acc_scaled"] <= 1.25 * fig["acc_unscaled"], fig
    assert fig["acc_scaled"] < BAR_KERNEL, fig
    assert fig["mixed_span_log2"] > 40.0, fig              # the frames of one tile really span 2**-20 .. 2**24
    assert fig["mixed"] < BAR_KERNEL, fig
    assert fig["mixed_guards"][0] == 0 and fig["mixed_guards"][1] > 0, fig
    assert fig["silent"], fig
    assert fig["inf_guard"] > 0, fig


@pytest.mark.parametrize("E,C,frames", KERNEL_CASES)
def test_scaled_mask_path_kernel(E, C, frames):
    _check_kernel(_kernel_figures(E, C, frames), f"E={E} C={C} frames={frames}")


def test_scaled_mask_path_kernel_on_the_chunk_per_tap_feed():
    env = dict(os.environ, ASW_NO_RESIDUE_FEED="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    figs = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(figs) == {f"{E}-{C}-{Fr}" for E, C, Fr in KERNEL_CASES}
    os.environ["ASW_NO_RESIDUE_FEED"] = "1"                  # (for _check_kernel's reading of the launch names only)
    try:
        for what, fig in figs.items():
            _check_kernel(fig, what + " [chunk-per-tap feed]")
    finally:
        del os.environ["ASW_NO_RESIDUE_FEED"]


# ------------------------------------------------------------------ 4. the site plan, read from the launch profiler
def _tag(name):
    return name[name.index("["):] if "[" in name else ""


def _site_diff(fast, safe, gemm_shapes, n_gemm, n_attention, n_mask, what):
    """fast / safe: {launch name: launches} of the same call in f16x3 and in f16x3_safe"""
    left = {k: fast[k] - safe.get(k, 0) for k in fast if fast[k] > safe.get(k, 0)}
    came = {k: safe[k] - fast.get(k, 0) for k in safe if safe[k] > fast.get(k, 0)}
    _log(f"site plan {what}: left {left}; arrived {came}")
    assert sum(fast.values()) == sum(safe.values())
    gl = {k: v for k, v in left.items() if k.startswith("convgemm16")}
    gc = {k: v for k, v in came.items() if k.startswith("convgemm<") or k.startswith("convgemm_m<")}
    al = {k: v for k, v in left.items() if k.startswith("attention_mfma16")}
    ac = {k: v for k, v in came.items() if k.startswith("attention_mfma") and not k.startswith("attention_mfma16")}
    ml = {k: v for k, v in left.items() if k.startswith("maskpath16p<")}
    mc = {k: v for k, v in came.items() if k.startswith("maskpath16ps<")}
    assert set(left) == set(gl) | set(al) | set(ml) and set(came) == set(gc) | set(ac) | set(mc)      # nothing else moved
    assert sum(gl.values()) == sum(gc.values()) == n_gemm
    assert sum(al.values()) == sum(ac.values()) and sum(al.values()) in n_attention
    assert sum(ml.values()) == sum(mc.values()) == n_mask
    if n_mask:
        assert {_tag(k) for k in ml} == {_tag(k) for k in mc}
    by_tag_l, by_tag_c = {}, {}
    for d, o in ((gl, by_tag_l), (gc, by_tag_c)):
        for k, v in d.items():
            o[_tag(k)] = o.get(_tag(k), 0) + v
    assert by_tag_l == by_tag_c                              # shape for shape, the f32 kernels took the sites over
    for tag in by_tag_l:
        n, k = int(tag.split(" N")[1].split()[0]), int(tag.split(" K")[1].split()[0])
        assert (n, k) in gemm_shapes, tag


def _spot_plan(cfg_name, seed, fused):
    from acousticswarms_speech_amd import config
    from acousticswarms_speech_amd.scenes import make_scene
    cfg = getattr(config, cfg_name)
    m = _spot(cfg_name, seed)
    m.set_fused_mask(fused)
    mix = torch.from_numpy(make_scene(2, 3, 7, 6000).mix)
    offs = [np.zeros(6), np.array([4, -8, 12, -16, 20, -24])]
    out = {}
    try:
        for prec in ("f16x3", "f16x3_safe"):
            m.set_precision(prec)
            _y, out[prec] = _profile_names(lambda: m.shift_and_sep(mix, offs, Strict=1))
    finally:
        m.set_fused_mask(True)
    return cfg, out


def test_site_plan_spot_small():
    cfg, p = _spot_plan("SMALL", 21, True)                   # 128 encoder channels: the three-GEMM mask path either way
    d, nl = cfg.bottleneck_channels, cfg.num_transformer_layers
    _site_diff(p["f16x3"], p["f16x3_safe"], {(d, d), (d, cfg.ffw_dim), (64, cfg.encoder_channels)}, 2 * nl + 1, (0,), 0, "spot SMALL")


@pytest.mark.parametrize("fused", [True, False])
def test_site_plan_spot_full(fused):
    cfg, p = _spot_plan("FULL", 5, fused)
    d, nl = cfg.bottleneck_channels, cfg.num_transformer_layers
    shapes = {(d, d), (d, cfg.ffw_dim)} | (set() if fused else {(64, cfg.encoder_channels)})
    _site_diff(p["f16x3"], p["f16x3_safe"], shapes, 2 * nl + (0 if fused else 1), (nl,), 1 if fused else 0, f"spot FULL fused={fused}")
    has_scaled = any(k.startswith("maskpath16ps<") for k in p["f16x3_safe"])
    assert has_scaled == fused and not any(k.startswith("maskpath16p") for k in p["f16x3_safe"] if not fused)


def test_site_plan_sep_small(golden):
    from acousticswarms_speech_amd.config import SEP_SMALL as cfg
    from acousticswarms_speech_amd.scenes import make_scene
    g = golden("g11b_sep_infer_small")
    m = _sep(31)
    mix = torch.from_numpy(make_scene(4, 3, 7, 4000).mix)
    p = {}
    for prec in ("f16x3", "f16x3_safe"):
        m.set_precision(prec)
        _y, p[prec] = _profile_names(lambda: m.infer_sample(mix, list(g["samples1"])))
    d = cfg.channels * int(cfg.growth) ** (len(cfg.stride_list) - 1)
    # per bottleneck layer: the Conformer's two second feed-forward linears and out_proj, the inter-speaker layer's
    # out_proj and linear2; the rel-pos and inter-speaker attention kernels are fp32 in both modes
    _site_diff(p["f16x3"], p["f16x3_safe"], {(d, d), (d, cfg.ffw_dim)}, 5 * cfg.bottleneck_layers, (0,), 1, "sep SMALL")


# ------------------------------------------------------------------ 5. mode switching
def test_mode_switching_leaves_no_state():
    from acousticswarms_speech_amd.scenes import make_scene
    mix = torch.from_numpy(make_scene(7, 2, 7, 4000).mix)
    m = _spot("SMALL", 21)
    ys = []
    for prec in ("f16x3", "f16x3_safe", "f16x3"):
        m.set_precision(prec)
        ys.append(m.shift_and_sep(mix, SPOT_OFFSETS, Strict=1))
    assert np.array_equal(ys[0], ys[2])
    assert not np.array_equal(ys[0], ys[1])                  # (the exact sites round differently: the mode did run)
    s = _sep(31)
    smix = torch.from_numpy(make_scene(4, 3, 7, 4000).mix)
    samples = [np.zeros(6), np.array([3, -5, 8, -13, 21, -34])]
    zs = []
    for prec in ("f16x3", "f16x3_safe", "f16x3"):
        s.set_precision(prec)
        zs.append(s.infer_sample(smix, samples))
    assert np.array_equal(zs[0], zs[2])


if __name__ == "__main__":
    assert os.environ.get("ASW_NO_RESIDUE_FEED") == "1"
    print(json.dumps({f"{E}-{C}-{Fr}": _kernel_figures(E, C, Fr) for E, C, Fr in KERNEL_CASES}))
