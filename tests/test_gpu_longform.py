"""GPU: a recording of any length -- ``asw_frame_blocks`` and ``asw_stitch_blocks`` against their float64 statements
(acousticswarms_speech_amd/longform.py), ``SepModel.infer_long`` and ``JointModel.forward_long`` against the same path
composed on the host from the per-block calls.  Needs an MI355X.

The stitch bound: the kernel accumulates in float64 (about 1e-16 of the result) and rounds once to float32, at most
2^-24 |out| with |out| <= max_k |x_k| over the blocks that cover the sample (a weighted mean); a contracted
multiply-add can move that rounding by one unit.  Hence |got - stitch_f64| <= 2^-22 max_k |x_k| per sample, with a
floor of 1e-30 where every cover is silent."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import longform

pytestmark = pytest.mark.gpu

# (M, T, hop, Ttot): a shifted last block with a triple cover (starts 0, 48, 53), a recording shorter than a block, the
# shape of the network tests (0, 3000, 6000, 6500: more than one workgroup per row, triple cover 6500 .. 6999), and
# tables beyond one launch's kernel arguments (frame: more than 960 blocks; stitch: 42 blocks x 40 tracks in two runs of
# blocks, 3 blocks x 130 tracks in three runs of tracks)
SHAPES = [(7, 64, 48, 117), (7, 64, 48, 40), (3, 4000, 3000, 10500)]
FRAME_SHAPES = SHAPES + [(2, 8, 4, 4 * 1000 + 8)]
STITCH_SHAPES = [(sh, 4) for sh in SHAPES] + [((1, 64, 48, 64 + 48 * 40 + 5), 40), ((1, 64, 48, 117), 130)]


def _nan_filled(*shape):
    out = torch.empty(shape, dtype=torch.uint8).fill_(0xFF).view(torch.float32).cuda()     # last dimension: bytes
    assert bool(torch.isnan(out).all())
    return out


def _cover_max(rows, starts, row_of, Ttot, T):
    """max_k |x_k[s][t - a_k]| over the blocks that cover t, [S, Ttot]"""
    row_of = np.asarray(row_of).reshape(len(starts), -1)
    out = np.zeros((row_of.shape[1], Ttot))
    for k, a in enumerate(starts):
        n = min(T, Ttot - int(a))
        for s, r in enumerate(row_of[k]):
            if r >= 0:
                out[s, a:a + n] = np.maximum(out[s, a:a + n], np.abs(rows[r, :n].astype(np.float64)))
    return out


def _check_stitch(got, rows, starts, row_of, Ttot, T, V, what):
    want = longform.stitch_f64(rows, starts, row_of, Ttot, T, V)
    assert got.shape == want.shape and got.dtype == np.float32
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} samples not written"
    err, scale = np.abs(got.astype(np.float64) - want), _cover_max(rows, starts, row_of, Ttot, T)
    ratio = float(np.max(err[scale > 0] / (2.0 ** -22 * scale[scale > 0]))) if (scale > 0).any() else 0.0
    print(f"{what}: largest |got - stitch_f64| / (2^-22 max|x|) = {ratio:.4f}")
    assert np.all(err <= 2.0 ** -22 * scale + 1e-30), what
    return want


@pytest.fixture(scope="module")
def ops():
    from acousticswarms_speech_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return o


# ---------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("M,T,hop,Ttot", FRAME_SHAPES)
def test_frame_blocks(ops, M, T, hop, Ttot):
    from acousticswarms_speech_amd import native
    mix = np.random.default_rng(Ttot).standard_normal((M, Ttot)).astype(np.float32)
    starts = longform.block_starts(Ttot, T, hop)
    want = longform.frame_f64(mix, starts, T)
    out = _nan_filled(len(starts), M, T * 4)
    got = ops.frame_blocks(torch.from_numpy(mix).cuda(), starts, T, out=out).cpu().numpy()
    assert not np.isnan(got).any()                                      # every sample of every block was written
    assert got.astype(np.float64).tobytes() == want.tobytes()
    via_op = native.torch_ops().frame_blocks(torch.from_numpy(mix).cuda(), [int(a) for a in starts], T)
    assert via_op.shape == (len(starts), M, T) and via_op.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("shape,S", STITCH_SHAPES)
def test_stitch_blocks(ops, shape, S):
    from acousticswarms_speech_amd import native
    _M, T, hop, Ttot = shape
    rng = np.random.default_rng(Ttot + S)
    starts = longform.block_starts(Ttot, T, hop)
    K, V = len(starts), T - hop
    rows = (rng.standard_normal((K * (S - 1), T)) * rng.uniform(0.01, 10.0, (K * (S - 1), 1))).astype(np.float32)
    row_of = np.full((K, S), -1, dtype=np.int64)                        # the last track is absent everywhere
    row_of[:, :S - 1] = rng.permutation(K * (S - 1)).reshape(K, S - 1)
    row_of[K // 2, 0] = -1                                              # track 0 is absent from a middle block
    row_of[K - 1, S - 2] = -1 if K > 1 else row_of[K - 1, S - 2]        # and one from the shifted last block
    taper = torch.from_numpy(longform.taper(T, V)).cuda()
    out = _nan_filled(S, Ttot * 4)
    got = ops.stitch_blocks(torch.from_numpy(rows).cuda(), taper, starts, row_of.tolist(), Ttot, out=out).cpu().numpy()
    _check_stitch(got, rows, starts, row_of, Ttot, T, V, f"stitch_blocks T={T} hop={hop} Ttot={Ttot} S={S}")
    np.testing.assert_array_equal(got[S - 1], 0.0)
    via_op = native.torch_ops().stitch_blocks(torch.from_numpy(rows).cuda(), taper, [int(a) for a in starts],
                                              [int(r) for r in row_of.reshape(-1)], Ttot)
    assert via_op.cpu().numpy().tobytes() == got.tobytes()


def test_the_ops_refuse_with_the_entries_own_messages():
    from acousticswarms_speech_amd import native
    t = native.torch_ops()
    mix, rows = torch.zeros(7, 117).cuda(), torch.zeros(6, 64).cuda()
    taper = torch.ones(64, dtype=torch.float64).cuda()
    with pytest.raises(RuntimeError, match="frame_blocks: block 2 starts at 117"):
        t.frame_blocks(mix, [0, 48, 117], 64)
    with pytest.raises(RuntimeError, match="Float"):
        t.frame_blocks(mix.double(), [0, 48, 53], 64)
    with pytest.raises(RuntimeError, match="stitch_blocks: block 1 starts at 65 after 0"):
        t.stitch_blocks(rows, taper, [0, 65, 70], [0, 1, 2, 3, 4, 5], 117)
    with pytest.raises(RuntimeError, match="row_of.1..1. = 6"):
        t.stitch_blocks(rows, taper, [0, 48, 53], [0, 1, 2, 6, 4, 5], 117)
    with pytest.raises(RuntimeError, match="K x S"):
        t.stitch_blocks(rows, taper, [0, 48, 53], [0, 1, 2, 3, 4], 117)
    with pytest.raises(RuntimeError, match="taper must be"):
        t.stitch_blocks(rows, taper[:63].contiguous(), [0, 48, 53], [0, 1, 2, 3, 4, 5], 117)
    with pytest.raises(RuntimeError, match="Double"):
        t.stitch_blocks(rows, taper.float(), [0, 48, 53], [0, 1, 2, 3, 4, 5], 117)
    assert t.stitch_blocks(rows, taper, [0, 48, 53], [], 117).shape == (0, 117)


# ---------------------------------------------------------------- SepModel.infer_long
BLOCK, HOP, TTOT = 4000, 3000, 10500


@pytest.fixture(scope="module")
def sep_small():
    """SEP_SMALL, weights seed 31, f16x3: the model of tests/test_gpu_sep_batch.py"""
    from acousticswarms_speech_amd.config import SEP_SMALL
    from acousticswarms_speech_amd.sep import SepModel
    from acousticswarms_speech_amd.weights import make_sep_state_dict
    return SepModel(SEP_SMALL, make_sep_state_dict(SEP_SMALL, 31), precision="f16x3").to("cuda")


@pytest.fixture(scope="module")
def recording():
    from acousticswarms_speech_amd.scenes import make_scene
    sc = make_scene(4, 3, 7, TTOT)
    return sc.mix, list(sc.tdoa_samples())


def test_infer_long(sep_small, recording):
    mix, samples = recording
    starts = longform.block_starts(TTOT, BLOCK, HOP)
    assert starts.tolist() == [0, 3000, 6000, 6500]
    got = sep_small.infer_long(mix, samples, hop=HOP, block=BLOCK)
    blocks = longform.frame_f64(mix, starts, BLOCK, np.float32)
    # the same device path, block by block: the difference is the stitch's alone
    rows = np.concatenate(sep_small.infer_batch(list(blocks), [samples] * 4))
    row_of = np.arange(12).reshape(4, 3)
    _check_stitch(got, rows, starts, row_of, TTOT, BLOCK, BLOCK - HOP, "infer_long vs infer_batch rows")
    # against the single call per block: tests/test_gpu_sep_batch.py::test_bytes holds the packed call to the bytes of
    # the single one (assert_array_equal), so the rows are the same rows and the bound is the same bound
    single = np.concatenate([sep_small.infer_sample(b, samples) for b in blocks])
    np.testing.assert_array_equal(single, rows)
    _check_stitch(got, single, starts, row_of, TTOT, BLOCK, BLOCK - HOP, "infer_long vs infer_sample rows")
    assert float(np.abs(got).max()) > 1e-3                              # there is audio to compare


def test_infer_long_of_less_than_a_block_and_of_no_talker(sep_small, recording):
    mix, samples = recording
    short = np.ascontiguousarray(mix[:, :2500])
    got = sep_small.infer_long(short, samples, hop=HOP, block=BLOCK)
    assert got.shape == (3, 2500) and got.dtype == np.float32
    padded = longform.frame_f64(short, [0], BLOCK, np.float32)[0]      # one block, zero past the recording
    rows = sep_small.infer_sample(padded, samples)
    _check_stitch(got, rows, [0], [[0, 1, 2]], 2500, BLOCK, BLOCK - HOP, "infer_long of 2500 samples")
    none = sep_small.infer_long(mix, [], hop=HOP, block=BLOCK)
    assert none.shape == (0, TTOT) and none.dtype == np.float32


# ---------------------------------------------------------------- JointModel.forward_long
LBLOCK, LTOT = 24000, 50000                                            # starts 0, 21000, 26000 at the default hop


@pytest.fixture(scope="module")
def joint(sep_small):
    """The models and the block length of tests/test_gpu_sep_batch.py::test_localize_batch_with_separation (the spot
    network FULL with weights seed 5, scene seed 2000 with 5 talkers and 7 mics, 24 000 samples per search), on a
    recording of three blocks.  With random weights the "talkers" the search finds are arbitrary: these tests pin how
    the pieces are composed, not the quality of what comes out."""
    from acousticswarms_speech_amd.config import FULL
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.scenes import make_scene
    from acousticswarms_speech_amd.spot import SpotModel
    from acousticswarms_speech_amd.weights import make_spot_state_dict
    sc = make_scene(2000, 5, 7, LTOT)
    spot = SpotModel(FULL, make_spot_state_dict(FULL, 5), batch_size=64, precision="f16x3").to("cuda")
    jm = JointModel(spot, sep_small, device="cuda")
    with redirect_stdout(io.StringIO()):
        jm.setup(sc.mic_positions, sc.speaker_range)
    return jm, sc.mix


def test_forward_long_every(joint):
    from acousticswarms_speech_amd.shard import localize_batch
    jm, mix = joint
    starts = longform.block_starts(LTOT, LBLOCK, LBLOCK - LBLOCK // 8)
    assert starts.tolist() == [0, 21000, 26000]
    frames = longform.frame_f64(mix, starts, LBLOCK, np.float32)
    with redirect_stdout(io.StringIO()):
        res = jm.forward_long(mix, block=LBLOCK, localize="every")
        again = localize_batch(jm, [torch.from_numpy(f) for f in frames], details=True)
    np.testing.assert_array_equal(res["starts"], starts)
    blocks = res["blocks"]
    assert len(blocks) == 3
    for r, p in zip(blocks, again):         # the searches are those of localize_batch on the framed blocks, at the bar
        assert list(r["names"]) == list(p["names"])                     # two runs of the batched form are held to
        np.testing.assert_allclose(r["centres"], p["centres"], atol=1e-6)
    # the same composition on the host, from the searches the call returns
    det_of, per_block = longform.link_tracks([r["centres"] for r in blocks], 0.25)
    n_tracks = det_of.shape[1]
    assert n_tracks >= 1                                                # the test is about audio: there must be some
    np.testing.assert_array_equal(res["detection"], det_of.T)
    np.testing.assert_array_equal(res["present"], det_of.T >= 0)
    assert res["present"].dtype == bool and res["present"].any(axis=1).all()
    np.testing.assert_array_equal(res["positions"]["per_block"], per_block)
    np.testing.assert_allclose(res["positions"]["mean"], np.nanmean(per_block, axis=1))
    for s in range(n_tracks):
        for k in range(3):
            d = res["detection"][s, k]
            if d >= 0:
                np.testing.assert_array_equal(res["positions"]["per_block"][s, k], blocks[k]["centres"][d])
    counts = [len(r["names"]) for r in blocks]
    rows = np.concatenate(jm.sep_model.infer_batch(list(frames), [list(r["offsets"]) for r in blocks]))
    assert rows.shape == (sum(counts), LBLOCK)
    print(f"forward_long every: talkers per block {counts}, {n_tracks} tracks, present\n{res['present'].astype(int)}")
    _check_stitch(res["audio"], rows, starts, longform.rows_of(det_of, counts), LTOT, LBLOCK, LBLOCK // 8,
                  "forward_long every vs the host composition")


def test_forward_long_first(joint):
    jm, mix = joint
    with redirect_stdout(io.StringIO()):
        res = jm.forward_long(mix, block=LBLOCK, localize="first")
    assert len(res["blocks"]) == 1
    n = len(res["blocks"][0]["names"])
    assert n >= 1 and res["audio"].shape == (n, LTOT) and res["present"].shape == (n, 3) and res["present"].all()
    np.testing.assert_array_equal(res["detection"], np.tile(np.arange(n)[:, None], (1, 3)))
    np.testing.assert_allclose(res["positions"]["mean"], res["blocks"][0]["centres"], rtol=1e-15)
    want = jm.sep_model.infer_long(mix, list(res["blocks"][0]["offsets"]), block=LBLOCK)
    np.testing.assert_array_equal(res["audio"], want)                   # the same calls on the same talkers
