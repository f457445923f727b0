"""GPU: the voice preparation on the device (csrc/voice_kernels.hip; ``torch.ops.asw.voice_resample`` / ``voice_trim``,
DESIGN.md section 7w) against the float64 statements of acousticswarms_speech_amd/voiceprep.py -- never against the
kernels themselves (tests/test_voiceprep_host.py holds the statements to scipy and to the restated librosa split).  Needs
an MI355X.

The bar of every comparison is equality of bytes: the kernels add the statement's terms in the statement's order, each
product and sum rounded on its own, so the float64 resampler output, its one rounding to float32, the trim bounds, the
peak frame value and the variance must be the statement's to the last bit.  Shapes are the smallest that reach every
path: rows shorter than one filter, rows of 1 and 2 samples, more than one workgroup per row (3000 samples at 640/147
are 13 workgroups), the LDS limit max(up, down) = 640, rows packed at odd offsets, and for the trim a row of 100 000
samples (196 blocks, 391 passes of the variance loop).

``test_generate_device_equals_host``: the room simulator's two backends agree to 1e-15 of the peak, not to the bit
(tests/test_gpu_roomsim.py), and where no sound has arrived both write the rounding noise of their transforms.  The
generator therefore runs prepared voices with ``simulate_rooms(exact_silence=True)``, which writes those samples as zeros.
Measured on an MI355X: without it 16 of 16 wav files differed, in 5355 samples of about 1e-18; with it none.  The test
prints how many files and samples differ before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import generate, native, ops, room_scenes
from acousticswarms_speech_amd import voiceprep as vp
from tests.voiceprep_cases import (DEVICE_RATIOS, GENERATE_ARGS, RAGGED_LENGTHS, long_row, make_corpus, packed, resampled, tree,
                                   trim_cases, trim_statement)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def full_rows(up, down, dtype, lengths=RAGGED_LENGTHS, via_torch_op=False):
    x, offs, _rows = packed(lengths)
    n_out = [vp.resampled_length(n, up, down) for n in lengths]
    xd = torch.from_numpy(x).to(DEV)
    if via_torch_op:
        h = ops.voice_filter(up, down, xd.device)
        y = native.torch_ops().voice_resample(xd, offs, list(lengths), up, down, h, [0] * len(lengths), n_out, max(n_out) + 5,
                                              dtype == torch.float64)
    else:
        y = ops.voice_resample(xd, offs, lengths, up, down, [0] * len(lengths), n_out, max(n_out) + 5, dtype=dtype)
    return y.cpu().numpy(), n_out


@pytest.mark.parametrize("up,down", DEVICE_RATIOS)
def test_resample_equals_the_statement(up, down):
    want = resampled(RAGGED_LENGTHS, up, down)
    got64, n_out = full_rows(up, down, torch.float64)
    got32, _ = full_rows(up, down, torch.float32, via_torch_op=True)
    assert got64.dtype == np.float64 and got32.dtype == np.float32 and got64.shape == (len(RAGGED_LENGTHS), max(n_out) + 5)
    for r, w in enumerate(want):
        assert w.shape == (n_out[r],)
        row = np.concatenate([w, np.zeros(got64.shape[1] - n_out[r])])          # zeros past the row's end
        assert same_bytes(got64[r], row), (up, down, r, float(np.max(np.abs(got64[r] - row))))
        assert same_bytes(got32[r], row.astype(np.float32)), (up, down, r)      # the one rounding of the float64 value
    if (up, down) == (640, 147):
        assert vp.resample_filter(up, down).nbytes == 102408                    # the LDS limit, beyond the default 64 KB
    if (up, down) == (1, 1):
        assert same_bytes(got32[4][:3000], packed(RAGGED_LENGTHS)[2][4])        # a windowed copy


def test_resample_windows():
    up, down = 160, 147
    lengths = (3000, 3000, 3000, 1025, 63)
    x, offs, _rows = packed(lengths)
    want = resampled(lengths, up, down)
    n_out = [w.shape[0] for w in want]
    T = 700
    begin = [0, 1500, n_out[2] - 100, 400, 10_000_000]          # from the start, inside, past the end, a window of 0, far beyond
    length = [700, 700, 700, 0, 50]
    xd = torch.from_numpy(x).to(DEV)
    for dtype in (torch.float64, torch.float32):
        got = ops.voice_resample(xd, offs, lengths, up, down, begin, length, T, dtype=dtype).cpu().numpy()
        for r in range(5):
            row = vp.window_f64(want[r], begin[r], length[r], T)
            assert same_bytes(got[r], row.astype(got.dtype)), (dtype, r)
        full = ops.voice_resample(xd, offs, lengths, up, down, [0] * 5, n_out, max(n_out), dtype=dtype).cpu().numpy()
        assert same_bytes(got[1], full[1][1500:2200]) and same_bytes(got[2][:100], full[2][n_out[2] - 100:n_out[2]])
        assert not got[2][100:].any() and not got[3].any() and not got[4].any() and got[1].any()


def test_resample_refusals_carry_the_library_message():
    x = torch.zeros(100, device=DEV)
    h = torch.ones(1, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match=r"beyond max\(up, down\) <= 640"):
        ops.voice_resample(x, [0], [100], 641, 1, [0], [10], 10, h=torch.ones(12821, dtype=torch.float64, device=DEV))
    t = native.torch_ops()
    with pytest.raises(RuntimeError, match=r"beyond max\(up, down\) <= 640"):
        t.voice_resample(x, [0], [100], 641, 1, torch.ones(12821, dtype=torch.float64, device=DEV), [0], [10], 10, False)
    with pytest.raises(RuntimeError, match="leaves x"):
        t.voice_resample(x, [50], [51], 1, 1, h, [0], [10], 10, False)
    with pytest.raises(RuntimeError, match="win_len"):
        t.voice_resample(x, [0], [100], 1, 1, h, [0], [11], 10, False)
    with pytest.raises(RuntimeError, match="the other tables do not"):
        t.voice_resample(x, [0, 1], [100], 1, 1, h, [0], [10], 10, False)
    with pytest.raises(RuntimeError, match="must be Float"):
        t.voice_resample(x.double(), [0], [100], 1, 1, h, [0], [10], 10, False)
    with pytest.raises(RuntimeError, match="1 dimensions"):
        t.voice_resample(x.reshape(10, 10), [0], [100], 1, 1, h, [0], [10], 10, False)
    with pytest.raises(RuntimeError, match="taps"):
        t.voice_resample(x, [0], [100], 3, 1, h, [0], [10], 10, False)
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.voice_resample(x.cpu(), [0], [100], 1, 1, h, [0], [10], 10, False)
    with pytest.raises(RuntimeError, match="leaves x"):
        t.voice_trim(x, [0], [101], 18.0)
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.voice_trim(x.cpu(), [0], [100], 18.0)
    assert t.voice_resample(x, [], [], 3, 1, ops.voice_filter(3, 1, x.device), [], [], 10, False).shape == (0, 10)
    b, s = t.voice_trim(x, [], [], 18.0)
    assert b.shape == (0, 2) and s.shape == (0, 2)


def _trim_batch():
    names = sorted(trim_cases()) + ["long_row"]
    rows = [long_row() if k == "long_row" else trim_cases()[k] for k in names]
    return names, rows


def test_trim_equals_the_statement():
    names, rows = _trim_batch()
    lens = [r.shape[0] for r in rows]
    # packed with one sample between the rows: odd offsets, no row 16-byte aligned by design
    pieces, offs, pos = [], [], 0
    for r in rows:
        offs.append(pos)
        pieces += [r, np.full(1, 0.9, dtype=np.float32)]
        pos += r.shape[0] + 1
    x = torch.from_numpy(np.concatenate(pieces)).to(DEV)
    bounds, stats = ops.voice_trim(x, offs, lens)
    tb, ts = native.torch_ops().voice_trim(x, offs, lens, 18.0)
    assert torch.equal(bounds, tb) and same_bytes(stats.cpu().numpy(), ts.cpu().numpy())
    bounds, stats = bounds.cpu().numpy(), stats.cpu().numpy()
    for r, name in enumerate(names):
        begin, end, peak, var = trim_statement(name)
        assert (int(bounds[r, 0]), int(bounds[r, 1])) == (begin, end), (name, bounds[r], begin, end)
        assert same_bytes(stats[r], np.array([peak, var])), (name, stats[r], peak, var)
    # the same rows as a padded matrix
    T_max = max(lens)
    mat = np.zeros((len(rows), T_max), dtype=np.float32)
    for r, row in enumerate(rows):
        mat[r, :lens[r]] = row
    b2, s2 = ops.voice_trim(torch.from_numpy(mat).to(DEV).reshape(-1), [r * T_max for r in range(len(rows))], lens)
    assert same_bytes(b2.cpu().numpy(), bounds) and same_bytes(s2.cpu().numpy(), stats)


def test_two_runs_give_the_same_bytes():
    x, offs, _rows = packed(RAGGED_LENGTHS)
    xd = torch.from_numpy(x).to(DEV)
    n_out = [vp.resampled_length(n, 160, 147) for n in RAGGED_LENGTHS]
    outs = []
    for fill in (0.0, float("nan")):
        out = torch.full((len(n_out), max(n_out) + 3), fill, dtype=torch.float32, device=DEV)
        ops.voice_resample(xd, offs, RAGGED_LENGTHS, 160, 147, [0] * 5, n_out, max(n_out) + 3, out=out)
        outs.append(out.cpu().numpy())
    assert same_bytes(*outs)
    _names, rows = _trim_batch()
    xs = torch.from_numpy(np.concatenate(rows)).to(DEV)
    lens = [r.shape[0] for r in rows]
    offs = [int(v) for v in np.concatenate([[0], np.cumsum(lens)])[:-1]]
    res = []
    for fill in (0, -1):
        out = (torch.full((len(rows), 2), fill, dtype=torch.int32, device=DEV), torch.full((len(rows), 2), float(fill), dtype=torch.float64, device=DEV))
        ops.voice_trim(xs, offs, lens, out=out)
        res.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
    assert same_bytes(res[0][0], res[1][0]) and same_bytes(res[0][1], res[1][1])


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return make_corpus(str(tmp_path_factory.mktemp("voices")))


def test_index_and_fetch_equal_the_host(corpus):
    files = room_scenes.list_voices(corpus)
    audio = [room_scenes.read_voice(f, 48000, resample=True) for f in files]
    signals, rates = [a for a, _ in audio], [s for _, s in audio]
    host = vp.prepare(signals, rates, 48000, backend="host")
    dev = vp.prepare(signals, rates, 48000, backend="device", device=DEV)
    assert dev == host and len({e[1:3] for e in host}) > 3
    picks = [(files[0], 0, 24000), (files[4], 9000, 24000), (files[7], 50000, 20000), (files[9], 100, 0), (files[16], 2048, 24000)]
    want = vp.fetch(picks, 24000, 48000, backend="host")
    got = vp.fetch(picks, 24000, 48000, backend="device", device=DEV)
    assert got.is_cuda and same_bytes(got.cpu().numpy(), want) and want[1].any() and not want[3].any()


def test_generate_device_equals_host(corpus, tmp_path):
    flags = ["--voices", corpus, "--voice_prep", "reference", "--generate_dereverb"] + GENERATE_ARGS
    assert generate.main([str(tmp_path / "host"), "--backend", "host"] + flags) == 0
    assert generate.main([str(tmp_path / "device"), "--backend", "device"] + flags) == 0
    h, d = tree(tmp_path / "host"), tree(tmp_path / "device")
    assert sorted(h) == sorted(d) and any(f.endswith("_dereverb.wav") for f in h)
    from scipy.io import wavfile
    worst, files, samples = 0.0, 0, 0
    for f in sorted(h):
        if f.endswith(".wav") and h[f] != d[f]:
            a, b = wavfile.read(os.path.join(tmp_path / "host", f))[1], wavfile.read(os.path.join(tmp_path / "device", f))[1]
            files, samples = files + 1, samples + int(np.count_nonzero(a != b))
            worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b)) / np.spacing(np.float32(np.max(np.abs(a))))))
    print(f"generate device against host: {files} of {sum(f.endswith('.wav') for f in h)} wav files differ, in {samples} samples, "
          f"by at most {worst:.2f} float32 ulps of the file's peak")
    for f in sorted(h):
        if f.endswith("metadata.json"):
            assert json.loads(h[f]) == json.loads(d[f]), f
    assert all(h[f] == d[f] for f in h if f.endswith(".wav")), (files, samples, worst)
