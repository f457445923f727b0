"""The 1x1 preproc convolution folded into the first residual layer of encoder block 0 (csrc/resstack.hip, SRC;
csrc/prep_kernels.hip, src_planes_kernel): the front end writes the 8-channel network input u~ = (u_0 .. u_6, 1) as
fp16 hi / lo planes, the fused pair's first layer runs on it with the composed weights Wc_k [Wpre | bpre] and rebuilds
its residual with one more k-step; the 64-channel preproc output is never written.

Bars (those of tests/test_gpu_resstack.py): relative L2 <= 3e-6 against the separate preproc pass followed by the plain
fused pair (two f16x3 executions of the same layers), <= 2e-5 against a float64 statement of the definitions -- on the
whole tensor AND separately on the first eight rows, the last eight and the eight rows around the left-pad boundary,
where a wrong edge row would vanish in a whole-tensor norm.  Needs an MI355X."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, M, K = 64, 7, 7
DILS = (1, 7)


def _log(msg):
    print(msg)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


_WEIGHTS = {}


def _weights(dils=DILS):
    """preproc (bias x10: a boundary mistake is large) and the two residual layers, torch layout, made once"""
    if not _WEIGHTS:
        _WEIGHTS["pre_w"] = _rand(C, M, seed=401, scale=1.0 / math.sqrt(M))
        _WEIGHTS["pre_b"] = _rand(C, seed=402, scale=0.1) * 10
        _WEIGHTS["layers"] = [(_rand(C, C, K, seed=410 + 10 * i, scale=1.0 / math.sqrt(C * K)), _rand(C, seed=411 + 10 * i, scale=0.1),
                               1 + _rand(C, seed=412 + 10 * i, scale=0.1), _rand(C, seed=413 + 10 * i, scale=0.1)) for i in range(2)]
    return _WEIGHTS["pre_w"], _WEIGHTS["pre_b"], [ly + (d,) for ly, d in zip(_WEIGHTS["layers"], dils)]


OFFSETS = np.array([[0, 0, 0, 0, 0, 0], [3, -5, 8, -13, 21, -34], [-40, 30, -20, 10, -5, 2]], dtype=np.int32)


def _reference_f64(mix, offsets, mean, std, pad, circular, pre_w, pre_b, layers):
    """shift, int16 quantisation, normalisation, left pad, 1x1 convolution, two residual layers: float64, from the
    definitions.  mean / std are the arguments the kernels under test receive.  -> (out [B][Tp][C], refn [B][Tp])"""
    Mm, T = mix.shape
    B = offsets.shape[0]
    u = torch.zeros(B, Mm, pad + T, dtype=torch.float64)
    t = torch.arange(T)
    for n in range(B):
        for m in range(Mm):
            o = 0 if m == 0 else int(offsets[n, m - 1])
            i = t + o
            if circular:
                x = mix[m, i % T].double()
            else:
                ok = (i >= 0) & (i < T)
                x = torch.where(ok, mix[m, i.clamp(0, T - 1)].double(), torch.zeros((), dtype=torch.float64))
            q = torch.round(x.float() * 32768.0).double() / 32768.0          # the quantisation itself is exact in fp32
            u[n, m, pad:] = (q - float(mean[n])) / float(std[n])
    x = F.conv1d(u, pre_w.double().unsqueeze(-1), pre_b.double())
    for w, b, g, be, d in layers:
        y = F.relu(F.conv1d(x, w.double(), b.double(), dilation=d, padding=d * (K - 1) // 2)) + x
        x = F.layer_norm(y.transpose(1, 2), (C,), g.double(), be.double(), 1e-5).transpose(1, 2)
    return x.transpose(1, 2).contiguous(), u[:, 0].contiguous()


def _run_both(ops, mix_d, off_d, Tp, circular, pre_w, pre_b, layers):
    mean, std = ops.shift_stats(mix_d, off_d, circular)
    hi, lo, refn = ops.shift_norm_src(mix_d, off_d, mean, std, Tp, circular)
    got = ops.resstack_src(hi, lo, pre_w, pre_b, [(w, b.cuda(), g.cuda(), be.cuda(), d) for w, b, g, be, d in layers], taps=K)
    return mean, std, refn, got


@pytest.mark.parametrize("circular", [True, False])
@pytest.mark.parametrize("pad", [0, 37])
@pytest.mark.parametrize("Tp", [214, 215, 470])
def test_source_fed_pair_vs_separate_preproc_and_float64(Tp, pad, circular):
    """Tp = 214: exactly one tile; 215: a second tile of one row; 470: three tiles, ragged last fragment."""
    from acousticswarms_speech_amd import ops
    pre_w, pre_b, layers = _weights()
    T = Tp - pad
    mix = _rand(M, T, seed=7 + Tp + pad, scale=0.3)
    mix_d, off_d = mix.cuda(), torch.from_numpy(OFFSETS).cuda()
    mean, std, refn, got = _run_both(ops, mix_d, off_d, Tp, circular, pre_w, pre_b, layers)
    assert torch.isfinite(got).all()
    # (a) the separate preproc pass and the plain fused pair
    x0, refn_a = ops.shift_norm_preproc(mix_d, off_d, mean, std, pre_w.cuda(), pre_b.cuda(), Tp, circular)
    dev_layers = [(ops.pack_conv_weight(w).cuda(), b.cuda(), g.cuda(), be.cuda(), d) for w, b, g, be, d in layers]
    want_a = ops.resstack(x0, dev_layers, taps=K)
    # (b) float64 from the definitions
    want_b, refn_b = _reference_f64(mix, OFFSETS, mean.cpu(), std.cpu(), pad, circular, pre_w, pre_b, layers)
    spans = {"all": (0, Tp), "head": (0, 8), "tail": (Tp - 8, Tp)}
    if pad:
        spans["pad boundary"] = (pad - 4, pad + 4)
    for name, (r0, r1) in spans.items():
        ra = _rel(got[:, r0:r1].cpu(), want_a[:, r0:r1].cpu())
        rb = _rel(got[:, r0:r1].cpu(), want_b[:, r0:r1])
        _log(f"src pair Tp={Tp} pad={pad} circular={circular} rows {name}: rel vs preproc + pair {ra:.3e}, vs float64 {rb:.3e}")
        assert ra <= 3e-6 and rb <= 2e-5, (name, ra, rb)
    assert torch.equal(refn, refn_a)
    assert float((refn.cpu().double() - refn_b).abs().max()) <= 1e-5
    # run to run, and wherever the candidate sits in the batch
    _, _, refn2, again = _run_both(ops, mix_d, off_d, Tp, circular, pre_w, pre_b, layers)
    assert torch.equal(got, again) and torch.equal(refn, refn2)
    perm = [2, 0, 1]
    _, _, refn_p, got_p = _run_both(ops, mix_d, torch.from_numpy(OFFSETS[perm].copy()).cuda(), Tp, circular, pre_w, pre_b, layers)
    assert torch.equal(got_p, got[perm]) and torch.equal(refn_p, refn[perm])


def test_source_fed_pair_of_one_tile_per_run():
    """the pair (1, 9): its 2 x 27 shared layer-0 rows exceed the 48 the carrying registers hold, so every tile of 202
    rows is a run of its own (image 278 rows); Tp = 405 is two full tiles and one row.  Against the separate preproc
    pass + staged pair."""
    from acousticswarms_speech_amd import ops
    from tests.test_gpu_resstack import _one_tile_per_run, _profiled
    pre_w, pre_b, layers = _weights((1, 9))
    Tp = 405
    mix_d, off_d = _rand(M, Tp, seed=7 + Tp, scale=0.3).cuda(), torch.from_numpy(OFFSETS).cuda()
    (mean, std, _, got), names = _profiled(lambda: _run_both(ops, mix_d, off_d, Tp, True, pre_w, pre_b, layers))
    assert any(n.startswith("resstack64<2,4x2,src>") for n in names) and _one_tile_per_run(names), names
    x0, _ = ops.shift_norm_preproc(mix_d, off_d, mean, std, pre_w.cuda(), pre_b.cuda(), Tp, True)
    want = ops.resstack(x0, [(ops.pack_conv_weight(w).cuda(), b.cuda(), g.cuda(), be.cuda(), d) for w, b, g, be, d in layers], taps=K)
    assert torch.isfinite(got).all()
    for name, (r0, r1) in {"all": (0, Tp), "head": (0, 8), "tail": (Tp - 8, Tp), "tile boundary": (198, 206)}.items():
        ra = _rel(got[:, r0:r1].cpu(), want[:, r0:r1].cpu())
        _log(f"src pair (1, 9) Tp={Tp} rows {name}: rel vs preproc + pair {ra:.3e}")
        assert ra <= 3e-6, (name, ra)


def test_source_fed_form_refuses_other_shapes():
    """anything but the fused pair (here: one layer) is refused instead of silently taking another path"""
    from acousticswarms_speech_amd import ops
    pre_w, pre_b, layers = _weights()
    mix_d, off_d = _rand(M, 300, seed=3, scale=0.3).cuda(), torch.from_numpy(OFFSETS).cuda()
    mean, std = ops.shift_stats(mix_d, off_d, True)
    hi, lo, _ = ops.shift_norm_src(mix_d, off_d, mean, std, 300, True)
    dl = [(w, b.cuda(), g.cuda(), be.cuda(), d) for w, b, g, be, d in layers]
    with pytest.raises(RuntimeError, match="source-fed"):
        ops.resstack_src(hi, lo, pre_w, pre_b, dl[:1], taps=K)


# ---- the model -------------------------------------------------------------------------------------------------------
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


def _snr(y, ref):
    y, ref = y.astype(np.float64), ref.astype(np.float64)
    return 10 * np.log10(np.sum(ref ** 2) / np.sum((y - ref) ** 2))


@pytest.fixture(scope="module")
def small_scene():
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    from oracle import spot_ref
    sd = make_spot_state_dict(SMALL, seed=13)
    model = SpotModel(SMALL, sd, batch_size=2, precision="f16x3").to("cuda")
    mix = torch.from_numpy(make_scene(11, 3, 7, 3000).mix)
    offs = [np.array(o) for o in ([0, 0, 0, 0, 0, 0], [3, -5, 8, -13, 21, -34], [-40, 30, -20, 10, -5, 2],
                                  [1, 2, 3, 4, 5, 6], [-7, 0, 7, -1, 0, 1])]
    want = {s: spot_ref.shift_and_sep(sd, SMALL, mix, offs, strict=s) for s in (0, 1)}
    return model, mix, offs, want


@pytest.mark.parametrize("strict", [0, 1])
def test_model_source_path_vs_oracle_and_switch(small_scene, strict):
    """SMALL network, f16x3, 5 candidates at internal batch 2 (a ragged last batch): the source-fed path against the
    oracle at the project's 80 dB, the energies at rtol 1e-4, and the switch reproduces the parent's launches."""
    from oracle import spot_ref
    model, mix, offs, want = small_scene
    model.set_source_stack(True)
    y_on, names_on = _names(lambda: model.shift_and_sep(mix, offs, Strict=strict))
    en = model.shift_and_score(mix, offs, Strict=strict, window=1000)
    model.set_source_stack(False)
    y_off, names_off = _names(lambda: model.shift_and_sep(mix, offs, Strict=strict))
    model.set_source_stack(True)
    per = [_snr(y_on[i], want[strict][i]) for i in range(len(offs))]
    on_off = [_snr(y_on[i], y_off[i]) for i in range(len(offs))]
    _log(f"model strict={strict}: source path vs oracle {np.round(per, 1)} dB; on vs off {np.round(on_off, 1)} dB")
    _log(f"  launches on: {sorted(names_on)}")
    _log(f"  launches off: {sorted(names_off)}")
    assert min(per) > 80.0
    np.testing.assert_allclose(en, spot_ref.candidate_energies(want[strict], 1000), rtol=1e-4)
    assert any(n.startswith("resstack64<2,4x2,src>") for n in names_on) and "preproc_src" in names_on
    assert "preproc" not in names_on and not any(n.startswith("resstack64<2,4x2>") for n in names_on)
    assert any(n.startswith("resstack64<2,4x2>") for n in names_off) and "preproc" in names_off
    assert "preproc_src" not in names_off and not any(",src>" in n for n in names_off)


def test_preproc_tap_exists_only_where_the_tensor_does(small_scene):
    model, mix, offs, _ = small_scene
    model.set_source_stack(True)
    model.shift_and_sep(mix, offs, Strict=1)
    with pytest.raises(RuntimeError, match="no activation named preproc"):
        model.get_tap("preproc")
    assert model.get_tap("enc0").numel() > 0
    x = _rand(2, 7, 1000, seed=5)
    model.forward(x, torch.tensor([[0.0, 1.0]] * 2))
    assert model.get_tap("preproc").numel() == 2 * model.cfg.padded_length(1000) * 64
