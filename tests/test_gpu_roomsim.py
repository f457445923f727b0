"""GPU: the room simulator on the device (csrc/room_kernels.hip) against the float64 statements of
acousticswarms_speech_amd/roomsim.py -- never against the kernels themselves (tests/test_roomsim_host.py holds the
statements to numpy.convolve, to reciprocity and to the reference's recipe).  Needs an MI355X.

The bar of every device comparison: max abs difference <= 1e-12 x max abs value of the statement's row (one response,
one premix or mix signal), the bar DESIGN.md 7t holds this float64 family to; a row of zeros must be met exactly.  The
device floors every image delay as the statement does (the file is compiled without fused multiply-adds), so what is
left between the two responses is a few ulps of sin and of the order of the sum, about 1e-15; a delay that floored the
other way would move a tap window and show as 1e-5.  The convolution goes through two float64 transforms of 2048 points
per partition, relative error of order 1e-15 each.  Every test prints its largest figure before it asserts (DESIGN.md 7u
quotes them).
"""
import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import native, ops, room_scenes, roomsim
from acousticswarms_speech_amd import oracle_masks as om
from acousticswarms_speech_amd.patch import FS
from tests.oracle_masks_cases import transform_rows
from tests.roomsim_cases import (CONV_SIZES, SEGMENT, conv_case, conv_statement, largest_batch, pair_delays, rir_case,
                                 row_errors)

pytestmark = pytest.mark.gpu

BAR = 1e-12
DEV = "cuda:0"


def check(label, got, want, rows):
    err = float(np.max(row_errors(got, want, rows)))
    print(f"{label}: {err:.3e}")
    assert err <= BAR, (label, err)


def device_rir(case, **kw):
    rooms, absorptions, orders, src, mics, counts, fs, length, _want = case
    args = dict(rooms=rooms, absorptions=absorptions, orders=list(orders), src=src, mics=mics, counts=list(counts), length=length)
    args.update(kw)
    with torch.cuda.device(DEV):
        host = [torch.from_numpy(np.array(args[k], dtype=np.float64)) for k in ("rooms", "absorptions", "src", "mics")]
        return native.torch_ops().room_rir(host[0], host[1], args["orders"], host[2], host[3], args["counts"], float(fs), args["length"])


@pytest.mark.parametrize("name", ("a", "b", "c", "d"))
def test_room_rir_against_the_statement(name):
    case = rir_case(name)
    rooms, absorptions, orders, src, mics, counts, fs, length, want = case
    if name == "a":
        # what the case is for: images skipped, a tap window cut by the end, and no boundary on a segment's edge
        ip = np.concatenate([pair_delays(case, s, m)[0] for s in range(src.shape[0]) for m in range(mics.shape[1])])
        assert (ip >= length).any() and ((ip < length) & (ip + 80 >= length)).any()
        direct = [int(d[len(d) // 2]) for d in (pair_delays(case, s, 0)[0] for s in (0, 1))]       # image (0, 0, 0): the middle one
        assert length % SEGMENT and all(d % SEGMENT for d in direct)
    if name == "b":
        assert roomsim.image_count(15) == 4991 and length > 3 * SEGMENT
    if name == "c":
        f = np.concatenate([pair_delays(case, s, 0)[1] for s in range(3)])
        assert int(np.sum(np.minimum(f, 1.0 - f) < 1e-9)) >= 2                 # delays within 1e-9 of an integer
    if name == "d":
        assert largest_batch(case) > 2 * 1024                                  # three accumulation rounds for one batch of columns
    h = device_rir(case)
    assert h.dtype == torch.float64 and tuple(h.shape) == want.shape and h.device == torch.device(DEV)
    check(f"room_rir ({name})", h.cpu().numpy(), want, 2)
    # a second run, into a poisoned buffer through the C ABI wrapper: identical bytes, every sample written
    again = ops.room_rir(rooms, absorptions, orders, src, mics, counts, fs, length, out=torch.full_like(h, float("nan")))
    assert torch.equal(again, h)


def test_room_rir_lengths_around_a_segment():
    """One sample, the last sample of a segment, the first of the next: the head of the longer response each time."""
    case = rir_case("a")
    want = case[-1]
    for length in (1, SEGMENT - 1, SEGMENT, SEGMENT + 1):
        h = device_rir(case, length=length).cpu().numpy()
        check(f"room_rir length={length}", h, want[:, :, :length], 2)


@pytest.mark.parametrize("T,length,counts,kind", tuple(c + ("statement",) for c in CONV_SIZES)
                         + ((2500, 1, (1,), "noise"), (1025, 3000, (1,), "noise")))
def test_room_convolve_against_the_statement(T, length, counts, kind):
    dry, rir, _c = conv_case(T, length, counts, kind)
    want_premix, want_mix = conv_statement(T, length, counts, kind)
    d, r = torch.tensor(dry, device=DEV), torch.tensor(rir, device=DEV)
    premix, mix = native.torch_ops().room_convolve(d, r, list(counts))
    assert premix.dtype == mix.dtype == torch.float64
    assert tuple(premix.shape) == want_premix.shape and tuple(mix.shape) == want_mix.shape
    check(f"room_convolve premix T={T} length={length} counts={counts} {kind}", premix.cpu().numpy(), want_premix, 2)
    check(f"room_convolve mix T={T} length={length} counts={counts} {kind}", mix.cpu().numpy(), want_mix, 2)
    # the mixture is the ordered sum of the premix rows, exactly
    acc, row = torch.zeros_like(mix), 0
    for k, c in enumerate(counts):
        for s in range(c):
            acc[k] = acc[k] + premix[row + s]
        row += c
    assert torch.equal(acc, mix)
    again = ops.room_convolve(d, r, list(counts), out=(torch.full_like(premix, float("nan")), torch.full_like(mix, float("nan"))))
    assert torch.equal(again[0], premix) and torch.equal(again[1], mix)


def test_room_convolve_a_scene_without_sources():
    dry, rir, _c = conv_case(2500, 1025, (1, 3))
    want_premix, want_mix = conv_statement(2500, 1025, (1, 3))
    premix, mix = native.torch_ops().room_convolve(torch.tensor(dry, device=DEV), torch.tensor(rir, device=DEV), [1, 0, 3])
    check("room_convolve counts=(1, 0, 3) premix", premix.cpu().numpy(), want_premix, 2)
    check("room_convolve counts=(1, 0, 3) mix", mix.cpu().numpy()[[0, 2]], want_mix, 2)
    assert not mix[1].any()


def test_workspace_queries():
    L = native.lib()
    assert L.asw_room_rir_workspace_bytes(2, 7, 4) >= 2 * 32 + 4 * 32 + 2 * 7 * 24 + 2 * 151 * 8 + 81 * 8
    c = (native.c_int32 * 2)(1, 3)
    blocks, parts = 3, 2                                                      # T = 2500, length = 1025
    assert L.asw_room_convolve_workspace_bytes(c, 2, 7, 1025, 2500) >= (4 * blocks + 4 * 7 * parts) * 1025 * 16


def test_refusals_carry_the_library_message():
    case = rir_case("c")
    rooms, absorptions, orders, src, mics, counts, fs, length, _want = case
    for kw, text in ((dict(orders=[151]), "max_order 151 outside 0..150"), (dict(orders=[-1]), "max_order -1 outside 0..150"),
                     (dict(absorptions=np.array([0.0])), r"absorption 0 outside \(0, 1\]"),
                     (dict(absorptions=np.array([1.25])), r"absorption 1.25 outside \(0, 1\]"),
                     (dict(src=src + np.array([9.0, 0.0, 0.0])), "source 0 lies outside the room"),
                     (dict(mics=mics * np.array([1.0, 1.0, 3.0])), "microphone 0 lies outside the room"),
                     (dict(mics=src[1][None, None, :].copy()), "source 1 sits at microphone 0"),
                     (dict(length=0), "length = 0 outside"), (dict(length=(1 << 25) + 1), "outside 1..2")):
        with pytest.raises(RuntimeError, match=text):
            device_rir(case, **kw)
    with pytest.raises(RuntimeError, match="libasw_hip.*max_order 200 outside 0..150"):
        ops.room_rir(rooms, absorptions, [200], src, mics, counts, fs, length, device=DEV)
    with pytest.raises(RuntimeError, match="65 sources outside 0..64"):
        ops.room_convolve(torch.zeros((65, 1100), device=DEV), torch.zeros((65, 1, 10), dtype=torch.float64, device=DEV), [65])
    with pytest.raises(RuntimeError, match="outside 0..64"):
        native.torch_ops().room_convolve(torch.zeros((65, 1100), device=DEV), torch.zeros((65, 1, 10), dtype=torch.float64, device=DEV),
                                         [65])


def test_simulate_rooms_device_against_host():
    rng = np.random.RandomState(21)
    specs = [room_scenes.make_room_spec(rng, n, n_mics=4, T=4096, max_order=3) for n in (2, 3)]
    host = room_scenes.simulate_rooms(specs, backend="host")
    dev = room_scenes.simulate_rooms(specs, backend="device", device=DEV)
    worst = 0.0
    for h, d in zip(host, dev):
        assert d.mix.dtype == d.sources.dtype == np.float32 and d.mix.shape == h.mix.shape and d.sources.shape == h.sources.shape
        for a, b in ((h.mix, d.mix), (h.sources, d.sources)):
            ulp = float(np.spacing(np.float32(np.max(np.abs(a)))))
            worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) / ulp)
        np.testing.assert_array_equal(d.mic_positions, h.mic_positions)
    print(f"simulate_rooms device against host: {worst:.2f} float32 ulps of the peak")
    assert worst <= 2.0
    one = room_scenes.make_room_scene(21, 2, n_mics=4, T=4096, max_order=3, backend="device", device=DEV)
    np.testing.assert_array_equal(one.mix, dev[0].mix)                         # a scene alone equals the scene in a batch


def test_the_shared_transform_left_the_stft_alone():
    """The smallest case of tests/test_gpu_oracle_masks.py through the stft op, at that file's bar: the transform now
    lives in a header that room_kernels.hip includes too."""
    x = transform_rows(2048 + 1, 1, 2048)
    t = native.torch_ops()
    z = t.stft(torch.from_numpy(x).to(DEV))
    got, want = z.cpu().numpy(), om.stft_f64(x)
    err = float(np.max(row_errors(got, want, 1)))
    print(f"stft N=2048 R=1 after the move: {err:.3e}")
    assert err <= BAR
    assert torch.equal(t.stft(torch.from_numpy(x).to(DEV)), z)
