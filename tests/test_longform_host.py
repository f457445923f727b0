"""CPU-only: the statements of the long-form path (acousticswarms_speech_amd/longform.py) -- block starts, taper,
normalised overlap-add, framing, the linking of talkers across blocks -- and the host-side refusals of the two C entries
and their ops.  No device call is made."""
import ctypes

import numpy as np
import pytest

from acousticswarms_speech_amd import longform, native

# (Ttot, T, hop): shorter than a block, exactly one, one sample more, an exact fit of the grid, a shifted last block
# that starts 5 < V = 16 samples after its neighbour (three blocks cover 53 .. 63), and the shape of the network test
# (three blocks cover 6500 .. 6999)
CASES = {(40, 64, 48): [0], (64, 64, 48): [0], (65, 64, 48): [0, 1], (160, 64, 48): [0, 48, 96],
         (117, 64, 48): [0, 48, 53], (10500, 4000, 3000): [0, 3000, 6000, 6500]}


# ---------------------------------------------------------------- block_starts
@pytest.mark.parametrize("case", sorted(CASES))
def test_block_starts(case):
    Ttot, T, hop = case
    starts = longform.block_starts(Ttot, T, hop)
    assert starts.tolist() == CASES[case]
    assert np.all(np.diff(starts) > 0)
    assert starts[-1] + T == max(Ttot, T)                              # the last block ends with the recording
    cover = np.zeros(Ttot, dtype=int)
    for a in starts:
        cover[a:a + T] += 1
    assert cover.min() >= 1 and cover.max() == (3 if case in ((117, 64, 48), (10500, 4000, 3000)) else min(2, len(starts)))


@pytest.mark.parametrize("T,hop", [(64, 64), (64, 65), (64, 31), (64, 0), (7, 3), (1, 1)])
def test_block_starts_refuses_an_overlap_outside_1_to_half_a_block(T, hop):
    with pytest.raises(ValueError):
        longform.block_starts(1000, T, hop)


def test_block_starts_takes_the_largest_and_the_smallest_overlap():
    assert longform.block_starts(200, 64, 32).tolist() == [0, 32, 64, 96, 128, 136]
    assert longform.block_starts(200, 64, 63).tolist() == [0, 63, 126, 136]
    with pytest.raises(ValueError):
        longform.block_starts(0, 64, 48)


# ---------------------------------------------------------------- taper
@pytest.mark.parametrize("T,V", [(64, 16), (64, 32), (64, 1), (4000, 1000), (48000, 6000), (7, 3)])
def test_taper(T, V):
    w = longform.taper(T, V)
    assert w.shape == (T,) and w.dtype == np.float64
    assert np.all(w > 0) and np.all(w <= 1)
    np.testing.assert_array_equal(w, w[::-1])
    np.testing.assert_array_equal(w[V:T - V], 1.0)
    assert np.max(np.abs(w[:V] + w[:V][::-1] - 1.0)) <= 1e-15          # two ramps that meet on the grid sum to 1
    assert np.all(np.diff(w[:V]) > 0)


# ---------------------------------------------------------------- frame_f64 / stitch_f64
@pytest.mark.parametrize("case", sorted(CASES))
def test_stitching_windows_of_one_signal_returns_the_signal(case):
    """The property that makes the normalised form right everywhere: single, double and triple covers, the first and
    the last block and the zero-filled one all go through one formula."""
    Ttot, T, hop = case
    rng = np.random.default_rng(Ttot)
    sig = rng.standard_normal((3, Ttot))
    starts = longform.block_starts(Ttot, T, hop)
    blocks = longform.frame_f64(sig, starts, T)
    assert blocks.shape == (len(starts), 3, T) and blocks.dtype == np.float64
    for k, a in enumerate(starts):
        n = min(T, Ttot - a)
        np.testing.assert_array_equal(blocks[k, :, :n], sig[:, a:a + n])
        np.testing.assert_array_equal(blocks[k, :, n:], 0.0)
    row_of = np.arange(len(starts) * 3).reshape(len(starts), 3)
    out = longform.stitch_f64(blocks.reshape(-1, T), starts, row_of, Ttot, T, T - hop)
    assert out.shape == (3, Ttot)
    assert np.max(np.abs(out - sig) / np.abs(sig)) <= 1e-15


def test_an_absent_row_fades_over_the_seam():
    T, hop, Ttot = 64, 48, 160
    V = T - hop
    starts = longform.block_starts(Ttot, T, hop)                       # 0, 48, 96
    w = longform.taper(T, V)
    x = np.random.default_rng(1).standard_normal(Ttot)
    rows = longform.frame_f64(x[None], starts, T).reshape(-1, T)
    out = longform.stitch_f64(rows, starts, [[0], [-1], [2]], Ttot, T, V)[0]      # the talker is not in block 1
    np.testing.assert_allclose(out[:48], x[:48], rtol=1e-15)           # block 0 alone
    j = np.arange(V)
    np.testing.assert_allclose(out[48:64], x[48:64] * w[48 + j] / (w[48 + j] + w[j]), rtol=1e-15)
    np.testing.assert_array_equal(out[64:96], 0.0)                     # silence where only block 1 covers
    np.testing.assert_allclose(out[96:112], x[96:112] * w[j] / (w[j] + w[48 + j]), rtol=1e-15)
    np.testing.assert_allclose(out[112:], x[112:], rtol=1e-15)
    assert np.all(np.abs(out[48:64]) <= np.abs(x[48:64])) and abs(out[63]) < 0.01 * abs(x[63])


# ---------------------------------------------------------------- link_tracks
A, B, C = np.array([1.0, 0.5, 0.0]), np.array([-0.8, 1.2, 0.1]), np.array([0.2, -1.5, 0.0])


def _jit(p, seed):
    return p + np.random.default_rng(seed).uniform(-0.03, 0.03, 3)


def test_two_talkers_keep_their_tracks_whatever_the_order_of_the_detections():
    blocks = [np.stack([_jit(A, 0), _jit(B, 1)]), np.stack([_jit(B, 2), _jit(A, 3)]), np.stack([_jit(A, 4), _jit(B, 5)])]
    det_of, pos = longform.link_tracks(blocks)
    assert det_of.tolist() == [[0, 1], [1, 0], [0, 1]]
    assert pos.shape == (2, 3, 3)
    for k in range(3):
        np.testing.assert_array_equal(pos[0, k], blocks[k][det_of[k, 0]])
        assert np.linalg.norm(pos[0, k] - A) < 0.06 and np.linalg.norm(pos[1, k] - B) < 0.06


def test_a_new_talker_opens_a_track_and_an_empty_block_leaves_every_track_absent():
    blocks = [np.stack([A, B]), np.zeros((0, 3)), np.stack([C, B, A])]
    det_of, pos = longform.link_tracks(blocks)
    assert det_of.tolist() == [[0, 1, -1], [-1, -1, -1], [2, 1, 0]]
    assert np.all(np.isnan(pos[:, 1])) and np.all(np.isnan(pos[2, 0]))
    np.testing.assert_array_equal(pos[2, 2], C)
    det_of, pos = longform.link_tracks([np.zeros((0, 3)), []])
    assert det_of.shape == (2, 0) and pos.shape == (0, 2, 3)
    det_of, pos = longform.link_tracks([])
    assert det_of.shape == (0, 0) and pos.shape == (0, 0, 3)


def test_a_talker_rejoins_its_track_only_within_the_radius_of_where_it_was_last_seen():
    near, far = A + [0.2, 0.0, 0.0], A + [0.3, 0.0, 0.0]
    det_of, _ = longform.link_tracks([np.stack([A, B]), B[None], np.stack([B, near])])
    assert det_of.tolist() == [[0, 1], [-1, 0], [1, 0]]
    det_of, _ = longform.link_tracks([np.stack([A, B]), B[None], np.stack([B, far])])
    assert det_of.tolist() == [[0, 1, -1], [-1, 0, -1], [-1, 0, 1]]
    # the track stands where it was detected LAST: a slow walk of 0.2 m per block is followed, 0.4 m from the start
    det_of, _ = longform.link_tracks([A[None], near[None], (A + [0.4, 0.0, 0.0])[None]])
    assert det_of.tolist() == [[0], [0], [0]]
    det_of, _ = longform.link_tracks([A[None], near[None]], radius=0.1)
    assert det_of.tolist() == [[0, -1], [-1, 0]]


def test_two_detections_within_the_radius_of_one_track_are_resolved_by_total_distance():
    # tracks at x = 0 and x = 0.3; detections at 0.2 (within 0.25 of both) and 0.05 (within 0.25 of both as well):
    # 0.2 -> 0.3 and 0.05 -> 0 costs 0.15, the other pairing 0.45
    t0, t1 = np.zeros(3), np.array([0.3, 0.0, 0.0])
    d0, d1 = np.array([0.2, 0.0, 0.0]), np.array([0.05, 0.0, 0.0])
    det_of, _ = longform.link_tracks([np.stack([t0, t1]), np.stack([d0, d1])])
    assert det_of.tolist() == [[0, 1], [1, 0]]
    # one more pair beats a shorter total: the detection at 0.1 is nearest to track 0, which is the only track within
    # reach of the one at -0.2; taking the nearest pair first would leave that one without a track
    det_of, _ = longform.link_tracks([np.stack([t0, t1]), np.stack([np.array([0.1, 0.0, 0.0]), np.array([-0.2, 0.0, 0.0])])])
    assert det_of.tolist() == [[0, 1], [1, 0]]
    # an exact tie (one detection midway between two tracks): one of them takes it, the other is absent
    det_of, _ = longform.link_tracks([np.stack([t0, t1]), np.array([[0.15, 0.0, 0.0]])])
    assert sorted(det_of[1].tolist()) == [-1, 0] and det_of.shape == (2, 2)


def test_rows_of():
    det_of = np.array([[0, 1, -1], [-1, -1, -1], [2, 1, 0]])
    assert longform.rows_of(det_of, [2, 0, 3]).tolist() == [[0, 1, -1], [-1, -1, -1], [4, 3, 2]]
    assert longform.rows_of(det_of, [2, 0, 3]).dtype == np.int32


# ---------------------------------------------------------------- the C entries and the ops, on the host
def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_frame_blocks_refusals():
    L = native.lib()
    p = ctypes.c_void_p(np.zeros(64).ctypes.data)                      # never dereferenced: every call below is refused
    ok = dict(mix=p, M=7, Ttot=117, starts=_i32(0, 48, 53), K=3, T=64, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.asw_frame_blocks(a["mix"], a["M"], a["Ttot"], a["starts"], a["K"], a["T"], a["out"], None)
    for name in ("mix", "starts", "out"):
        assert call(**{name: None}) == -1 and b"frame_blocks: null pointer" in L.asw_last_error(), name
    for kw in (dict(M=0), dict(M=65536), dict(Ttot=0), dict(K=0), dict(T=0), dict(T=(1 << 30) + 1), dict(Ttot=(1 << 30) + 1)):
        assert call(**kw) == -1 and b"frame_blocks: bad shape" in L.asw_last_error(), kw
    assert call(starts=_i32(0, 48, 117)) == -1 and b"frame_blocks: block 2 starts at 117" in L.asw_last_error()
    assert call(starts=_i32(0, -1, 53)) == -1 and b"frame_blocks: block 1 starts at -1" in L.asw_last_error()


def test_stitch_blocks_refusals():
    L = native.lib()
    p = ctypes.c_void_p(np.zeros(64).ctypes.data)
    ok = dict(rows=p, N=6, taper=p, starts=_i32(0, 48, 53), row_of=_i32(0, 1, 2, -1, 4, 5), K=3, S=2, T=64, Ttot=117, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.asw_stitch_blocks(a["rows"], a["N"], a["taper"], a["starts"], a["row_of"], a["K"], a["S"], a["T"], a["Ttot"],
                                   a["out"], None)
    for name in ("rows", "taper", "starts", "row_of", "out"):
        assert call(**{name: None}) == -1 and b"stitch_blocks: null pointer" in L.asw_last_error(), name
    for kw in (dict(N=0), dict(K=0), dict(S=0), dict(T=0), dict(Ttot=0), dict(Ttot=(1 << 30) + 1)):
        assert call(**kw) == -1 and b"stitch_blocks: bad shape" in L.asw_last_error(), kw
    assert call(starts=_i32(1, 48, 53)) == -1 and b"block 0 starts at 1, not at 0" in L.asw_last_error()
    assert call(starts=_i32(0, 53, 48)) == -1 and b"block 2 starts at 48 after 53" in L.asw_last_error()
    assert call(starts=_i32(0, 48, 48)) == -1 and b"block 2 starts at 48 after 48" in L.asw_last_error()
    assert call(starts=_i32(0, 65, 70)) == -1 and b"block 1 starts at 65 after 0" in L.asw_last_error()        # a gap
    assert call(starts=_i32(0, 48, 117)) == -1 and b"block 2 starts at 117" in L.asw_last_error()
    assert call(starts=_i32(0, 40, 50)) == -1 and b"the last block ends at 114" in L.asw_last_error()
    assert call(row_of=_i32(0, 1, 2, 6, 4, 5)) == -1 and b"row_of[1][1] = 6 outside -1..5" in L.asw_last_error()
    assert call(row_of=_i32(0, 1, -2, 3, 4, 5)) == -1 and b"row_of[1][0] = -2" in L.asw_last_error()
    # a launch's table takes 15 blocks beside 63 tracks: sixteen blocks one sample apart all cover sample 15
    assert call(starts=_i32(*range(16)), K=16, Ttot=79, S=63, row_of=_i32(*([0] * (16 * 63)))) == -1
    assert b"the 16 blocks that cover sample 15 outgrow one launch's table" in L.asw_last_error()


def test_the_ops_refuse_host_tensors():
    import torch
    ops = native.torch_ops()
    assert hasattr(ops, "frame_blocks") and hasattr(ops, "stitch_blocks")
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.frame_blocks(torch.zeros(7, 117), [0, 48, 53], 64)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.stitch_blocks(torch.zeros(6, 64), torch.ones(64, dtype=torch.float64), [0, 48, 53], [0, 1, 2, 3, 4, 5], 117)


def test_the_models_refuse_before_any_device_work():
    """No model is loaded and there is no device here: each of these raises on the host checks alone."""
    from acousticswarms_speech_amd.config import SEP_SMALL
    from acousticswarms_speech_amd.joint import JointModel
    from acousticswarms_speech_amd.sep import SepModel
    sep = SepModel(SEP_SMALL)
    mix = np.zeros((7, 10500), dtype=np.float32)
    with pytest.raises(ValueError, match="overlap"):
        sep.infer_long(mix, [np.zeros(6)], hop=4000, block=4000)
    with pytest.raises(ValueError, match="overlap"):
        sep.infer_long(mix, [np.zeros(6)], hop=1000, block=4000)
    with pytest.raises(RuntimeError, match="65 speakers"):
        sep.infer_long(mix, [np.zeros(6)] * 65, block=4000)
    out = sep.infer_long(mix, [], block=4000)                          # no talker: no device work
    assert out.shape == (0, 10500) and out.dtype == np.float32
    with pytest.raises(RuntimeError, match="separation model"):
        JointModel(object()).forward_long(mix, block=4000)
    with pytest.raises(ValueError, match="localize"):
        JointModel(object(), sep).forward_long(mix, block=4000, localize="all")


# ---------------------------------------------------------------- the command
def test_the_separate_command_writes_one_wav_per_track_and_tracks_json(tmp_path):
    import json
    from acousticswarms_speech_amd import evalkit, separate
    args = separate.build_parser().parse_args(["rec", "--spot_experiment_dir", "a", "--sep_experiment_dir", "b", "--out", "o"])
    assert (args.block, args.hop, args.localize, args.link_radius) == (48000, None, "every", 0.25)
    with pytest.raises(SystemExit):
        separate.main(["rec", "--spot_experiment_dir", "a"])           # refused before anything is loaded
    audio = np.random.default_rng(0).standard_normal((2, 300)).astype(np.float32) * 0.1
    per_block = np.array([[A, A + 0.01, A], [[np.nan] * 3, B, B]])
    result = {"audio": audio, "present": np.array([[True, True, True], [False, True, True]]),
              "positions": {"per_block": per_block, "mean": np.nanmean(per_block, axis=1)}, "starts": np.array([0, 100, 172])}
    doc = separate.write_tracks(result, str(tmp_path / "out"), 48000, {"block": 128, "hop": 100, "localize": "every"})
    assert json.load(open(tmp_path / "out" / "tracks.json")) == doc
    assert doc["starts"] == [0, 100, 172] and doc["block"] == 128 and [t["file"] for t in doc["tracks"]] == ["track00.wav", "track01.wav"]
    assert doc["tracks"][1]["present"] == [False, True, True] and doc["tracks"][1]["positions"][0] is None
    assert doc["tracks"][1]["positions"][1] == B.tolist() and doc["tracks"][0]["position"] == np.nanmean(per_block[0], axis=0).tolist()
    for s in range(2):                                                 # float32 wav, read back by the reader of get_items
        np.testing.assert_array_equal(evalkit._read_wav(str(tmp_path / "out" / f"track{s:02d}.wav")), audio[s])
