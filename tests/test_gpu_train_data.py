"""GPU: the training-batch ops (csrc/augment_kernels.hip) against the float64 statements of
acousticswarms_speech_amd/train_data.py -- never against the kernels themselves (tests/test_train_data_host.py holds the
statements to the reference's recorded outputs and to the published Philox vectors).  Needs an MI355X.

Bars.  Every float64 device output: max abs difference <= 1e-12 x max abs value of the statement's row, the bar DESIGN.md
7t and 7u hold this family to (a Bluestein transform through numpy's FFTs measures 7.6e-16 of the peak at T = 48 000 and
144 000).  Losses: 1e-9 dB for the logarithmic terms and 1e-12 relative for L1 -- the differences of float32 inputs are
exact in float64, what remains is the order of the sums.  Every test prints its largest figure before it asserts
(DESIGN.md 7v quotes them).
"""
import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import native, ops
from acousticswarms_speech_amd import train_data as td
from tests import train_data_cases as cases

pytestmark = pytest.mark.gpu

BAR = 1e-12
DEV = "cuda:0"


def check(label, got, want):
    err = float(np.max(cases.row_errors(got, want)))
    print(f"{label}: {err:.3e}")
    assert err <= BAR, (label, err)


@pytest.mark.parametrize("T,rows,per_pass", cases.NOISE_CASES)
def test_colored_noise_against_the_statement(T, rows, per_pass):
    want = cases.noise_statement(T, rows)
    with torch.cuda.device(DEV):
        y = ops.colored_noise(cases.NOISE_KEY, rows, T, max_rows_per_pass=per_pass)
    assert y.dtype == torch.float64 and tuple(y.shape) == (rows, T) and y.device == torch.device(DEV)
    check(f"colored_noise T={T} rows={rows} per_pass={per_pass}", y.cpu().numpy(), want)
    # a second run into a poisoned buffer, in passes of the default size: identical bytes, every sample written
    again = ops.colored_noise(cases.NOISE_KEY, rows, T, out=torch.full_like(y, float("nan")))
    assert torch.equal(again, y)


def test_colored_noise_rows_keys_and_the_torch_op():
    """Rows are addressed by (key, row index), not by their place in the call; an exponent other than 1."""
    T = 1023
    full = cases.noise_statement(T, 3)
    keys, ids = [5, cases.NOISE_KEY, 5, cases.NOISE_KEY], [1, 2, 0, 0]
    want = np.stack([td.colored_noise_f64(5, [1], T)[0], full[2], td.colored_noise_f64(5, [0], T)[0], full[0]])
    with torch.cuda.device(DEV):
        y = ops.colored_noise(keys, ids, T)
        signed = [k - 2 ** 64 if k >= 2 ** 63 else k for k in keys]
        z = native.torch_ops().colored_noise(signed, ids, T)
        b = ops.colored_noise(3, 2, T, exponent=2.0)
    check("colored_noise per-row keys", y.cpu().numpy(), want)
    assert torch.equal(y, z)
    check("colored_noise exponent 2", b.cpu().numpy(), td.colored_noise_f64(3, 2, T, exponent=2.0))


def device_batch(s_max, noisy, dtype, mix=None):
    it = cases.batch_items(s_max, noisy)
    n = len(it["item_mix"])
    mix = torch.from_numpy(np.array(cases.batch_mix() if mix is None else mix, dtype=np.float32)).to(DEV)
    pink = None
    if noisy:
        rows = s_max * cases.M
        keys = [k for k in it["pink_key"] for _ in range(rows)]
        pink = ops.colored_noise(keys, list(range(rows)) * n, cases.T, device=DEV).reshape(n, rows, cases.T)
    return ops.train_batch(mix, it["item_mix"], it["shifts"], it["counts"], it["pink_level"], it["white_level"], it["white_key"],
                           pink=pink, dtype=dtype)


@pytest.mark.parametrize("s_max", (1, 3))
def test_train_batch_levels_zero_is_the_roll(s_max):
    it = cases.batch_items(s_max, False)
    want = np.zeros((len(it["counts"]), s_max * cases.M, cases.T), dtype=np.float32)
    for i, c in enumerate(it["counts"]):
        for s in range(c):
            want[i, s * cases.M:(s + 1) * cases.M] = td.roll_rows(cases.batch_mix()[it["item_mix"][i]], it["shifts"][i, s])
    assert any(c == s_max for c in it["counts"]) and 0 in it["counts"]
    got = device_batch(s_max, False, torch.float32)
    assert got.dtype == torch.float32 and got.device == torch.device(DEV)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert want.tobytes() == cases.batch_statement(s_max, False, True).tobytes()
    got64 = device_batch(s_max, False, torch.float64)
    assert got64.dtype == torch.float64 and np.array_equal(got64.cpu().numpy(), want.astype(np.float64))


@pytest.mark.parametrize("s_max", (1, 3))
def test_train_batch_with_noise(s_max):
    want64, want32 = cases.batch_statement(s_max, True, False), cases.batch_statement(s_max, True, True)
    got64 = device_batch(s_max, True, torch.float64)
    got32 = device_batch(s_max, True, torch.float32)
    check(f"train_batch float64 S_max={s_max}", got64.cpu().numpy(), want64)
    assert torch.equal(got32, got64.float())                       # one rounding of the same float64 sum
    g32 = got32.cpu().numpy()
    ulps = float(np.max(np.abs(g32.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)))
    print(f"train_batch float32 S_max={s_max}: {ulps:.1f} ulp, {int(np.sum(g32 != want32))} of {g32.size} samples differ")
    assert ulps <= 1.0
    # blocks of talkers beyond counts[i] are noise only: they do not depend on the mixture
    it = cases.batch_items(s_max, True)
    other = device_batch(s_max, True, torch.float64, mix=cases.batch_mix()[::-1] * 3.0)
    for i, c in enumerate(it["counts"]):
        assert torch.equal(other[i, c * cases.M:], got64[i, c * cases.M:])
        if c:
            assert not torch.equal(other[i, :c * cases.M], got64[i, :c * cases.M])
    i = it["counts"].index(0)
    noise = td.perturb_f64(np.zeros((s_max * cases.M, cases.T), np.float32), it["pink_level"][i], it["white_level"][i],
                           it["pink_key"][i], it["white_key"][i], rounded=False)
    check(f"train_batch pure noise S_max={s_max}", got64[i].cpu().numpy(), noise)


def test_train_losses():
    est, gt = cases.loss_rows()
    want = td.row_losses_f64(est, gt)
    e, g = torch.from_numpy(np.array(est)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV)
    rows = ops.train_losses(e, g)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (5, 4)
    assert torch.equal(native.torch_ops().train_losses(e, g), rows)
    assert torch.equal(ops.train_losses(e, g, out=torch.full_like(rows, float("nan"))), rows)
    got = rows.cpu().numpy()
    l1 = float(np.max(np.abs(got[:, 0] - want[:, 0]) / np.where(want[:, 0] > 0, want[:, 0], 1.0)))      # est == gt: exactly 0
    db = float(np.max(np.abs(got[:, 1:3] - want[:, 1:3])))
    print(f"train_losses: L1 {l1:.3e} relative, logarithmic terms {db:.3e} dB; the statement's rows:\n{want}")
    assert l1 <= 1e-12 and db <= 1e-9
    assert np.array_equal(got[:, 3], want[:, 3]) and got[0, 3] == 0.0
    est3, gt3 = est[:, None, :], gt[:, None, :]
    for name in cases.LOSS_NAMES:
        a, b = td.loss_from_rows(got, name), td.loss_f64(est3, gt3, name)
        # a weight of at most 1 on a logarithmic term, of at most 500 (snr_w_scaled_neg) on an L1 term
        tol = 1e-9 + 500 * 1e-12 * float(np.max(want[:, 0]))
        print(f"loss {name}: {a!r} against {b!r}")
        assert abs(a - b) <= tol, (name, a, b)


# ---- the datasets on the device ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    return cases.rebuild_dataset(tmp_path_factory.mktemp("g18"))


@pytest.mark.parametrize("name", ("loc_train", "loc_test", "sep_train", "sep_test"))
def test_device_batches_against_the_host_backend_and_the_statement(dataset_dir, name):
    import random
    ds = cases.make_sets(dataset_dir)[name]
    seed, worst, noisy = 9, 0.0, 0
    dev = list(ds.batches(2, seed=seed, backend="device", device=DEV))
    host = list(ds.batches(2, seed=seed, backend="host"))
    assert len(dev) == len(host) == 1
    (data, gt, extra), (hdata, hgt, hextra) = dev[0], host[0]
    assert data.device == gt.device == extra.device == torch.device(DEV)
    assert data.dtype == hdata.dtype == torch.float32 and data.shape == hdata.shape
    assert gt.dtype == hgt.dtype and extra.dtype == hextra.dtype
    assert torch.equal(gt.cpu(), hgt) and torch.equal(extra.cpu(), hextra)           # the same decisions under the same seeds
    got = data.cpu().numpy()
    for pos in range(2):
        random.seed(td.item_seed(seed, pos))
        np.random.seed(td.item_seed(seed, pos))
        dec = ds.decide(pos, "device")                                               # the draws batches() made for this item
        S, M = dec.shifts.shape
        rolled = np.zeros((S * M, dec.mix.shape[-1]), dtype=np.float32)
        for s in range(dec.count):
            rolled[s * M:(s + 1) * M] = td.roll_rows(dec.mix, dec.shifts[s])
        if dec.noise is None:
            assert got[pos].tobytes() == rolled.tobytes() == hdata[pos].numpy().tobytes()
            continue
        pink_level, pink_key, white_level, white_key = dec.noise
        noisy += 1
        # data minus the rolled mixture is the statement's noise for the keys drawn: within one float32 unit of the sum
        want = td.perturb_f64(rolled, pink_level, white_level, pink_key, white_key)
        ulps = float(np.max(np.abs(got[pos].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)))
        worst = max(worst, ulps)
        assert pink_level > 0 and white_level > 0 and not np.array_equal(got[pos], rolled)
    print(f"batches(device) {name}: {noisy} perturbed items, {worst:.1f} ulp of float32 from the statement")
    assert worst <= 1.0 and noisy == (2 if name.endswith("train") else 0)


@pytest.mark.parametrize("kind", ("spot", "sep"))
def test_validate_is_the_statements_on_the_same_forward_output(tmp_path, monkeypatch, kind):
    from acousticswarms_speech_amd.config import SEP_SMALL, SMALL
    from acousticswarms_speech_amd.sep import SepModel
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict
    from tests.golden import make_golden_training as mg
    mg.write_dataset(str(tmp_path), n_samples=4, T=4000)
    if kind == "spot":
        model = SpotModel(SMALL, make_spot_state_dict(SMALL, seed=3), batch_size=4).to(DEV)
        ds = td.LocalizationDataset(str(tmp_path), "test", **mg.LOC_TEST)
    else:
        model = SepModel(SEP_SMALL, make_sep_state_dict(SEP_SMALL, seed=31)).to(DEV)
        ds = td.SeparationDataset(str(tmp_path), "test", **dict(mg.SEP_TEST, n_speakers=SEP_SMALL.max_speakers))
    forward_batch, outputs = td.forward_batch, []

    def recorded(*args):                                           # keep what validate's forward returned
        outputs.append(forward_batch(*args))
        return outputs[-1]
    monkeypatch.setattr(td, "forward_batch", recorded)
    for name in cases.LOSS_NAMES:
        outputs.clear()
        res = td.validate(model, ds, loss=name, batch_size=3, backend="device")
        gts = [gt for _data, gt, _extra in ds.batches(3, seed=td.VAL_SEED, backend="host")]
        assert len(outputs) == len(gts) == 2 and len(res["batch_losses"]) == 2
        want = [td.loss_f64(o.cpu().numpy(), g.numpy(), name) for o, g in zip(outputs, gts)]
        l1 = max(float(np.max(td.row_losses_f64(o.cpu().numpy().reshape(-1, 4000), g.numpy().reshape(-1, 4000))[:, 0])) for o, g in zip(outputs, gts))
        print(f"validate {kind} {name}: {res['loss']!r} against {float(np.mean(want))!r}")
        if np.isnan(want).any():                                   # sisdr over a batch without a positive row, as in the reference
            assert np.array_equal(np.isnan(want), np.isnan(res["batch_losses"]))
            continue
        assert max(abs(a - b) for a, b in zip(res["batch_losses"], want)) <= 1e-9 + 500 * 1e-12 * l1
        assert abs(res["loss"] - float(np.mean(want))) <= 1e-9 + 500 * 1e-12 * l1
        n_pos = sum(int((g.abs().amax(dim=-1) > 0).sum()) for g in gts)
        assert len(res["input_si_sdr"]) == len(res["output_si_sdr"]) == n_pos and n_pos > 0
    assert td.validate(model, ds, loss="snr", batch_size=3, backend="host")["loss"] == pytest.approx(
        td.validate(model, ds, loss="snr", batch_size=3, backend="device")["loss"], abs=1e-6)


def test_validate_command_ranks_checkpoints(tmp_path, capsys):
    """``python -m acousticswarms_speech_amd.validate EXP --all`` in process: one line per checkpoint, the best named."""
    import json
    import os
    from acousticswarms_speech_amd import validate
    from acousticswarms_speech_amd.config import SMALL
    from acousticswarms_speech_amd.experiment import load_model_from_exp
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    from tests.golden import make_golden_training as mg
    data, exp = tmp_path / "data", tmp_path / "exp"
    mg.write_dataset(str(data), n_samples=2, T=4000)
    os.makedirs(exp / "checkpoints")
    desc = {"model_name": "SpeakerLocalization", "sr": 48000,
            "model_params": {"stride_list": list(SMALL.stride_list), "channels": SMALL.channels,
                             "encoder_channels": SMALL.encoder_channels, "ffw_dim": SMALL.ffw_dim},
            "training_params": {"loss": "snr", "batch_size": 2},
            "test_set_params": dict({k: v for k, v in mg.LOC_TEST.items() if k != "sr"}, input_dir=str(data))}
    with open(exp / "description.json", "w") as f:
        json.dump(desc, f)
    for epoch, seed in ((0, 3), (1, 4)):
        sd = {k: torch.from_numpy(v) for k, v in make_spot_state_dict(SMALL, seed=seed).items()}
        torch.save(sd, exp / "checkpoints" / f"exp_{epoch}.pt")
    results = validate.main([str(exp), "--all", "--device", DEV])
    out = capsys.readouterr().out
    assert sorted(results) == [0, 1] and f"best: checkpoint {min(results, key=results.get)}" in out
    assert out.count("checkpoint 0: loss") == 1 and out.count("checkpoint 1: loss") == 1
    model = load_model_from_exp(str(exp), mode="last").to(DEV)
    ds = td.LocalizationDataset(dataset_type="test", sr=48000, **desc["test_set_params"])
    assert td.validate(model, ds, loss="snr", batch_size=2)["loss"] == pytest.approx(results[1], abs=1e-6)
    assert validate.main([str(exp), "--checkpoint", "0", "--device", DEV, "--backend", "host"])[0] == pytest.approx(results[0], abs=1e-6)
