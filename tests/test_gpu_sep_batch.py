"""GPU: the joint separation of a batch of mixtures with a talker count per mixture (``asw_sep_infer_batch``) -- the
two ragged kernels against the statements and the single-group kernels of tests/test_gpu_sep.py, the network against
the reference's own fixture (g11b) and the oracle, item by item, and ``localize_batch(..., separate=True)`` against
``JointModel.forward``.  SEP_SMALL, T = 4000 except for the whole path.  Needs an MI355X."""
import io
import math
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T = 4000


def _log(msg):
    print(msg)


def _relerr(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _snr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return 10 * np.log10(np.sum(want ** 2) / max(np.sum((got - want) ** 2), 1e-300))


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


@pytest.fixture(scope="module")
def ops():
    from acousticswarms_speech_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return o


# ---------------------------------------------------------------- kernels
# at head_dim 64 a wave's LDS region is 1036 bytes per sequence of the widest group: four regions fit the 160 KB up to
# 39 sequences, two beyond.  [39, 25] / [40, 24] are the two sides of that boundary, [64] is the largest group
@pytest.mark.parametrize("counts", [[1], [1, 3, 2], [6, 1, 1, 5], [38, 26], [39, 25], [40, 24], [64]])
@pytest.mark.parametrize("d,H", [(128, 8), (512, 8)])
def test_inter_attention_groups(ops, d, H, counts):
    L, hd, N = 5, d // H, sum(counts)
    qkv = _rand(N, L, 3 * d, seed=15, scale=0.7)
    out = torch.empty((N, L, d * 4), dtype=torch.uint8).fill_(0xFF).view(torch.float32).cuda()
    assert bool(torch.isnan(out).all())
    got = ops.inter_attention_groups(qkv.cuda(), counts, H, out=out).cpu()
    assert not bool(torch.isnan(got).any())                            # every row of every group was written
    n0 = 0
    for S in counts:                                                    # the statement of test_inter_attention, per group
        q, k, v = [t.permute(1, 0, 2).reshape(L, S, H, hd).transpose(1, 2) for t in qkv[n0:n0 + S].split(d, dim=-1)]
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
        want = (att @ v).transpose(1, 2).reshape(L, S, d).permute(1, 0, 2)
        assert _relerr(got[n0:n0 + S], want) < 2e-6, (counts, n0)
        n0 += S


@pytest.mark.parametrize("d,H", [(128, 8), (512, 8)])
def test_inter_attention_groups_of_one_size_write_the_bytes_of_the_single_size_kernel(ops, d, H):
    qkv = _rand(2, 3, 5, 3 * d, seed=16, scale=0.7).cuda()
    want = ops.inter_attention(qkv, H)
    got = ops.inter_attention_groups(qkv.view(6, 5, 3 * d), [3, 3], H)
    np.testing.assert_array_equal(got.view(2, 3, 5, d).cpu().numpy(), want.cpu().numpy())
    # an empty item between them never reaches the device
    got = ops.inter_attention_groups(qkv.view(6, 5, 3 * d), [3, 0, 3], H)
    np.testing.assert_array_equal(got.view(2, 3, 5, d).cpu().numpy(), want.cpu().numpy())


def test_joint_shift_stats_groups(ops):
    from acousticswarms_speech_amd.scenes import make_scene
    from oracle import spot_ref
    mixes = [torch.from_numpy(make_scene(seed, 3, 7, T).mix) for seed in (4, 5, 6)]
    offs = np.array([[0, 0, 0, 0, 0, 0], [131, -131, 7, -7, 64, -64], [2500, -2500, 3999, -3999, 4000, -4100],
                     [17, -3, 8, 0, -12, 40]], dtype=np.int32)           # test_joint_shift_stats': shifts beyond T included
    items = [offs[:1], offs[:4], offs[1:3]]
    counts = [len(o) for o in items]
    stack = torch.stack(mixes).cuda()
    mean, std = ops.joint_shift_stats_groups(stack, _i32(np.concatenate(items)), counts)
    assert mean.shape == std.shape == (sum(counts),)
    n0 = 0
    for k, o in enumerate(items):
        S = len(o)
        data = torch.cat([spot_ref.roll_channels(mixes[k], row, circular=False) for row in o], dim=0).unsqueeze(0)
        _dn, mu, sg = spot_ref.normalize_input(data)
        m, s = mean[n0:n0 + S].cpu(), std[n0:n0 + S].cpu()
        assert torch.all(m == m[0]) and torch.all(s == s[0])            # one value per item, on each of its sequences
        np.testing.assert_allclose(m[0].item(), mu.item(), rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(s[0].item(), sg.item(), rtol=2e-6)
        m1, s1 = ops.joint_shift_stats(stack[k], _i32(o))               # same partition, same order of the sums
        np.testing.assert_array_equal(m.numpy(), m1.cpu().numpy())
        np.testing.assert_array_equal(s.numpy(), s1.cpu().numpy())
        n0 += S
    # an item with no sequence is left out of the table
    mean0, std0 = ops.joint_shift_stats_groups(stack, _i32(np.concatenate([items[0], items[2]])), [1, 0, 2])
    np.testing.assert_array_equal(mean0.cpu().numpy(), torch.cat([mean[:1], mean[5:]]).cpu().numpy())
    np.testing.assert_array_equal(std0.cpu().numpy(), torch.cat([std[:1], std[5:]]).cpu().numpy())


# ---------------------------------------------------------------- the network
_MODELS = {}


def _model(precision):
    """SEP_SMALL, weights seed 31 (the fixtures'), one model per arithmetic for the whole module"""
    if precision not in _MODELS:
        from acousticswarms_speech_amd.config import SEP_SMALL
        from acousticswarms_speech_amd.sep import SepModel
        from acousticswarms_speech_amd.weights import make_sep_state_dict
        sd = make_sep_state_dict(SEP_SMALL, 31)
        _MODELS[precision] = (SepModel(SEP_SMALL, sd, precision=precision).to("cuda"), sd)
    return _MODELS[precision]


@pytest.fixture(scope="module")
def scenes():
    from acousticswarms_speech_amd.scenes import make_scene
    return [make_scene(seed, 3, 7, T) for seed in (4, 5, 6)]


def _oracle(sd, mix, offs):
    from acousticswarms_speech_amd.config import SEP_SMALL
    from oracle import sep_ref
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return sep_ref.infer_sample(sd, SEP_SMALL, torch.as_tensor(mix), list(offs))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_reference_fixture_ragged_in_one_call(golden, scenes, precision):
    """g11b: the reference's own infer_sample on make_scene(4, 3, 7, 4000) with 2, 3 and 6 talkers.  Here the three
    cases are the three items of ONE call.  An implementation that pads the items to the widest count lets zero
    sequences into the inter-speaker attention (and into the joint statistics) of the first two and cannot pass."""
    g = golden("g11b_sep_infer_small")
    model, _sd = _model(precision)
    samples = [list(g[f"samples{i}"]) for i in range(3)]
    assert [len(s) for s in samples] == [2, 3, 6]
    out = model.infer_batch([scenes[0].mix] * 3, samples)
    for i, y in enumerate(out):
        assert y.shape == g[f"y{i}"].shape and y.dtype == np.float32
        snr = _snr(y, g[f"y{i}"])
        _log(f"sep infer_batch SMALL {precision} item {i} (S={y.shape[0]}): {snr:.1f} dB vs reference")
        assert snr > 80.0


def test_different_mixtures_vs_oracle(scenes):
    model, sd = _model("f16x3")
    counts = (3, 1, 2)
    samples = [list(sc.tdoa_samples())[:c] for sc, c in zip(scenes, counts)]
    out = model.infer_batch([sc.mix for sc in scenes], samples)
    for k, (sc, y) in enumerate(zip(scenes, out)):
        assert y.shape == (counts[k], T)
        snr = _snr(y, _oracle(sd, sc.mix, samples[k]))
        _log(f"sep infer_batch SMALL f16x3, own mixture per item, item {k} (S={counts[k]}): {snr:.1f} dB vs oracle")
        assert snr > 80.0


def _device_args(scenes, samples):
    from acousticswarms_speech_amd.sep import rounded_offsets
    stack = torch.stack([torch.from_numpy(sc.mix) for sc in scenes]).cuda()
    offs = [rounded_offsets(s, 6) for s in samples]
    return stack, offs


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_bytes(scenes, precision):
    model, _sd = _model(precision)
    samples = [list(sc.tdoa_samples()) for sc in scenes]
    stack, offs = _device_args(scenes, samples)
    # one mixture: the call is infer_device
    one = model.infer_batch_device(stack[1:2], _i32(offs[1]), [3])
    assert one.shape == (3, T) and one.dtype == torch.float32 and one.is_cuda
    np.testing.assert_array_equal(one.cpu().numpy(), model.infer_device(stack[1], _i32(offs[1])).cpu().numpy())
    # an item without talkers adds no row and changes none
    got = model.infer_batch_device(stack, _i32(np.concatenate([offs[0][:2], offs[2]])), [2, 0, 3])
    want = model.infer_batch_device(stack[[0, 2]].contiguous(), _i32(np.concatenate([offs[0][:2], offs[2]])), [2, 3])
    assert got.shape == (5, T)
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    # every item is what infer_device computes for it
    np.testing.assert_array_equal(got[:2].cpu().numpy(), model.infer_device(stack[0], _i32(offs[0][:2])).cpu().numpy())
    np.testing.assert_array_equal(got[2:].cpu().numpy(), model.infer_device(stack[2], _i32(offs[2])).cpu().numpy())
    none = model.infer_batch_device(stack, _i32(np.zeros((0, 6))), [0, 0, 0])
    assert none.shape == (0, T)
    assert [y.shape for y in model.infer_batch([sc.mix for sc in scenes], [[], [], []])] == [(0, T)] * 3


def test_more_than_64_sequences_go_out_in_two_calls(golden, scenes, monkeypatch):
    """13 items of 6 talkers: 78 sequences, so ten items in the first device call and three in the second."""
    from acousticswarms_speech_amd.sep import SepModel, rounded_offsets
    model, sd = _model("f16x3")
    base = np.stack(list(golden("g11b_sep_infer_small")["samples2"]))
    assert base.shape == (6, 6)
    mixes = [scenes[k % 3].mix for k in range(13)]
    samples = [list(base + (k - 6)) for k in range(13)]                  # every item its own offsets
    calls = []
    inner = SepModel.infer_batch_device

    def counted(self, stack, offs, counts):
        calls.append(list(counts))
        return inner(self, stack, offs, counts)
    monkeypatch.setattr(SepModel, "infer_batch_device", counted)
    out = model.infer_batch(mixes, samples)
    monkeypatch.undo()
    assert calls == [[6] * 10, [6] * 3] and [y.shape for y in out] == [(6, T)] * 13
    stack = torch.stack([torch.from_numpy(m) for m in mixes]).cuda()
    offs = [rounded_offsets(s, 6) for s in samples]
    packs = [model.infer_batch_device(stack[a:b], _i32(np.concatenate(offs[a:b])), [6] * (b - a)).cpu().numpy()
             for a, b in ((0, 10), (10, 13))]
    for k in range(13):
        rows = packs[0][6 * k:6 * k + 6] if k < 10 else packs[1][6 * (k - 10):6 * (k - 10) + 6]
        np.testing.assert_array_equal(out[k], rows)
    for k in (1, 11):                                                    # one item of each call
        snr = _snr(out[k], _oracle(sd, mixes[k], samples[k]))
        _log(f"sep infer_batch SMALL f16x3, 13 x 6 talkers, item {k}: {snr:.1f} dB vs oracle")
        assert snr > 80.0


def test_refusals(scenes):
    model, _sd = _model("f32")
    stack = torch.stack([torch.from_numpy(sc.mix) for sc in scenes]).cuda()

    def offs(n):
        return _i32(np.zeros((n, 6)))
    with pytest.raises(RuntimeError, match="65 sequences"):
        model.infer_batch_device(stack, offs(65), [30, 30, 5])
    with pytest.raises(RuntimeError, match="holds 65 speakers"):
        model.infer_batch_device(stack, offs(65), [65, 0, 0])
    with pytest.raises(RuntimeError, match="holds -1 speakers"):
        model.infer_batch_device(stack, offs(3), [2, -1, 2])
    with pytest.raises(RuntimeError, match="2 counts for 3 mixtures"):
        model.infer_batch_device(stack, offs(3), [1, 2])
    with pytest.raises(RuntimeError, match="sum"):
        model.infer_batch_device(stack, offs(4), [1, 1, 1])
    with pytest.raises(RuntimeError, match="Float"):
        model.infer_batch_device(stack.double(), offs(3), [1, 1, 1])
    with pytest.raises(RuntimeError, match="Int"):
        model.infer_batch_device(stack, offs(3).long(), [1, 1, 1])
    with pytest.raises(RuntimeError):
        model.infer_batch_device(stack.cpu(), offs(3), [1, 1, 1])       # a host tensor
    with pytest.raises(RuntimeError, match="contiguous"):
        model.infer_batch_device(stack.transpose(1, 2).contiguous().transpose(1, 2), offs(3), [1, 1, 1])
    with pytest.raises(RuntimeError, match="channels"):
        model.infer_batch_device(stack[:, :6].contiguous(), _i32(np.zeros((3, 5))), [1, 1, 1])
    # the model still works after every refusal
    assert model.infer_batch_device(stack, offs(3), [1, 1, 1]).shape == (3, T)


# ---------------------------------------------------------------- the whole path
def test_localize_batch_with_separation():
    """Four mixtures (the scene of the four-mixture batch tests: seeds 2000-2003, 5 talkers, 7 mics, 24 000 samples, one
    array) through ``localize_batch(..., separate=True)`` in the batched form against ``JointModel.forward`` per mixture.
    Both audio paths are the same network on the same talkers, each within 80 dB of the oracle (the tests above), so
    they lie within twice that error of each other: 80 dB - 20 log10(2) = 74 dB."""
    from acousticswarms_speech_amd.config import FULL, SEP_SMALL
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.sep import SepModel
    from acousticswarms_speech_amd.shard import localize_batch
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict
    first = make_scene(2000, 5, 7, 24000)
    scs = [make_scene(2000 + k, 5, 7, 24000, mic_positions=first.mic_positions) for k in range(4)]
    mixes = [torch.from_numpy(s.mix) for s in scs]
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")
    sep = SepModel(SEP_SMALL, make_sep_state_dict(SEP_SMALL, 31), precision="f16x3").to("cuda")
    jm = JointModel(spot, sep, device="cuda")
    with redirect_stdout(io.StringIO()):
        jm.setup(first.mic_positions, first.speaker_range)
        plain = localize_batch(jm, mixes, concurrent=2)
        got = localize_batch(jm, mixes, concurrent=2, separate=True)
        fwd = [jm.forward(m) for m in mixes]
    assert len(got) == len(plain) == 4 and all("audio" not in r for r in plain)
    n_talkers = 0
    for k in range(4):
        r, p = got[k], plain[k]
        assert set(r) == set(p) | {"audio"}
        # the search is the one without separate= (two runs of the batched form share their launches differently:
        # the bar of test_config3_mixture_batch_equals_plain_loop)
        assert list(r["names"]) == list(p["names"]) and int(r["spot_times"]) == int(p["spot_times"])
        np.testing.assert_allclose(r["centres"], p["centres"], atol=1e-6)
        assert r["audio"].dtype == np.float32 and r["audio"].shape == (len(r["names"]), 24000)
        patches, _al, audio, _d0, _d1, _st = fwd[k]
        assert [q[3] for q in patches] == list(r["names"])
        if len(patches):
            snr = _snr(r["audio"], audio)
            _log(f"localize_batch separate=True, mixture {k}: {len(patches)} talkers, {snr:.1f} dB vs forward()")
            assert snr >= 74.0
        n_talkers += len(patches)
    assert n_talkers >= 4                                                # the test is about audio: there must be some
    # the plain loop hands out forward's audio
    with redirect_stdout(io.StringIO()):
        loop = localize_batch(jm, mixes[:1], concurrent=1, separate=True)
    if fwd[0][2] is not None:
        np.testing.assert_array_equal(loop[0]["audio"], fwd[0][2])
