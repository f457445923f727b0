"""CPU only: the float64 statements of the voice preparation (acousticswarms_speech_amd/voiceprep.py)
which ``asw_voice_resample`` and ``asw_voice_trim`` reproduce bit for bit on the GPU (tests/test_gpu_voiceprep.py), the
draws of ``get_voices`` and of the three desks against the reference's own functions (tests/golden/g19_voice_recipe.npz),
the host-side refusals of the two entry points, and the generator's new options on the host backend.

Bars.  The resampler against ``scipy.signal.resample_poly``: equal lengths and max |difference| <= 1e-13 of the peak --
both sum the same at most 61 products of the same float64 table, in different orders, so they differ by a few ulps of
the peak (measured: 8.2e-16).  The trim against ``hostdsp.nonsilent_intervals`` (the project's restatement of
``librosa.effects.split``): equal bounds on waveforms whose every frame is at least 1e-6 dB from the threshold."""
import ctypes
import json
import os

import numpy as np
import pytest

from acousticswarms_speech_amd import generate, hostdsp, native, room_scenes, roomsim
from acousticswarms_speech_amd import voiceprep as vp
from tests.voiceprep_cases import (GENERATE_ARGS, HOST_LENGTHS, HOST_RATIOS, MARGIN_DB, long_row, make_corpus, signal, tree,
                                   trim_cases, trim_margin_db, trim_statement)


# ---- the resampler ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", HOST_RATIOS)
def test_resample_against_scipy(up, down):
    from scipy.signal import resample_poly
    worst = 0.0
    for n in HOST_LENGTHS:
        x = signal(n, n).astype(np.float64)
        got, want = vp.resample_poly_f64(x, up, down), resample_poly(x, up, down)
        assert got.shape == want.shape == (vp.resampled_length(n, up, down),) and got.dtype == np.float64
        worst = max(worst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    print(f"resample_poly_f64 {up}/{down} against scipy: {worst:.2e} of the peak")
    assert worst <= 1e-13


def test_resample_reduces_the_ratio_and_the_identity_is_exact():
    x = signal(777, 3)
    np.testing.assert_array_equal(vp.resample_poly_f64(x, 48000, 44100), vp.resample_poly_f64(x, 160, 147))
    np.testing.assert_array_equal(vp.resample_poly_f64(x, 5, 5), x.astype(np.float64))
    assert vp.reduced(48000, 16000) == (3, 1) and vp.resample_filter(7, 7).tolist() == [1.0]
    h = vp.resample_filter(48000, 44100)
    assert h.shape == (2 * 10 * 160 + 1,) and h.dtype == np.float64
    np.testing.assert_array_equal(h, h[::-1])                                 # a symmetric design
    with pytest.raises(ValueError):
        vp.reduced(0, 3)


def test_window_of_a_resampled_row():
    y = vp.resample_poly_f64(signal(100, 1), 3, 2)
    np.testing.assert_array_equal(vp.window_f64(y, 10, 20, 32), np.concatenate([y[10:30], np.zeros(12)]))
    np.testing.assert_array_equal(vp.window_f64(y, 140, 20, 20), np.concatenate([y[140:150], np.zeros(10)]))
    np.testing.assert_array_equal(vp.window_f64(y, 500, 20, 20), np.zeros(20))
    np.testing.assert_array_equal(vp.window_f64(y, 0, 0, 8), np.zeros(8))


# ---- the trim -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(trim_cases()) + ["long_row"])
def test_trim_against_the_restated_split(name):
    x = long_row() if name == "long_row" else trim_cases()[name]
    begin, end, peak, var = trim_statement(name)
    T = x.shape[0]
    if T == 0:
        assert (begin, end, peak, var) == (0, 0, 0.0, 0.0)
        return
    margin = trim_margin_db(x)
    print(f"{name}: T {T}, kept [{begin}, {end}), margin {margin:.3g} dB")
    assert margin >= MARGIN_DB
    iv = hostdsp.nonsilent_intervals(x, top_db=18, frame_length=2048, hop_length=512)
    assert (begin, end) == (int(iv[0, 0]), int(iv[-1, 1]))
    assert 0 <= begin <= end <= T and begin % 512 == 0
    ms, _level = vp.trim_levels(x)
    assert ms.shape == (1 + T // 512,) and peak == float(np.max(ms))
    # the fixed order of additions computes the plain quantities
    np.testing.assert_allclose(ms, hostdsp.frame_rms(x.astype(np.float64), 2048, 512)[0] ** 2, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(var, np.var(x[begin:end].astype(np.float64)), rtol=1e-11, atol=1e-300)


def test_trim_edge_rows():
    cases = trim_cases()
    assert trim_statement("zeros") == (0, 3000, 0.0, 0.0)                     # all zero: non-silent everywhere
    assert trim_statement("below_one_block")[:2] == (0, 300)
    assert trim_statement("silence_first")[0] > 0 and trim_statement("silence_first")[1] == cases["silence_first"].shape[0]
    assert trim_statement("silence_last")[0] == 0 and trim_statement("silence_last")[1] < cases["silence_last"].shape[0]
    b, e = trim_statement("burst")[:2]
    assert b <= 5300 and e >= 6000 and e - b <= 700 + 2 * 1024                # the burst and the frames that touch it
    assert trim_statement("peak_in_the_partial_block")[1] == 512 * 9 + 100
    assert vp.span_var_f64(cases["both_ends"], 5, 5) == 0.0


def test_accept_is_condition_one():
    assert vp.accept(0, 24001, 4.1e-8, 48000) and not vp.accept(0, 24000, 1.0, 48000) and not vp.accept(0, 48000, 4e-8, 48000)
    assert vp.accept(100, 8200, 1e-3, 16000) and not vp.accept(100, 8100, 1e-3, 16000)


# ---- the draws against the reference ------------------------------------------------------------------------------------
class TableIndex:
    """The index of the fixture's table: what ``make_golden_voices.py`` answered ``glob``, ``load`` and ``trim`` from."""

    def __init__(self, g):
        self.names = [str(f) for f in g["files"]]
        self.rows = {f: g["entries"][i] for i, f in enumerate(self.names)}
        self.fs = int(g["sr"])

    def files(self, directory):
        return [f for f in self.names if os.path.dirname(f) == directory]

    def entry(self, path):
        n, begin, end, std = self.rows[path]
        return {"n": int(n), "begin": int(begin), "end": int(end), "ok": vp.accept(int(begin), int(end), float(std) ** 2, self.fs)}


def test_get_voices_equals_the_reference(golden):
    g = golden("g19_voice_recipe")
    index = TableIndex(g)
    dirs = [str(d) for d in g["dirs"]]
    kinds = set()
    for c, (seed, n, duration) in enumerate(g["voice_cases"]):
        T = int(round(duration * index.fs))
        rng = np.random.RandomState(int(seed))
        picks, ids = vp.get_voices(rng, dirs, int(n), T, index.fs, index)
        want = g[f"v{c}_picks"]
        assert [index.names.index(p) for p, _b, _n in picks] == want[:, 0].tolist(), (c, picks)
        assert [b for _p, b, _n in picks] == want[:, 1].tolist() and [m for _p, _b, m in picks] == want[:, 2].tolist()
        assert ids == [str(i) for i in g[f"v{c}_ids"]]
        assert rng.uniform() == float(g[f"v{c}_after"])                       # as many draws as the reference made
        kinds |= {"short" if m < T else "full" for _p, _b, m in picks}
    assert kinds == {"short", "full"}
    assert not all(index.entry(f)["ok"] for f in index.names)                 # the table holds rejected files


def test_clip_voice_draws_only_when_it_cuts():
    rng = np.random.RandomState(0)
    state = (rng.get_state()[1].copy(), rng.get_state()[2])
    assert vp.clip_voice(rng, 30000, 2000, 29000, 48000, 48000) == (0, 30000)          # shorter: padded by the caller
    assert vp.clip_voice(rng, 48000, 100, 47000, 48000, 48000) == (0, 48000)           # equal: no draw
    assert vp.clip_voice(rng, 100000, 20000, 40000, 48000, 48000) == (10400, 39200)    # the 0.2 s pad on both sides
    assert np.array_equal(rng.get_state()[1], state[0]) and rng.get_state()[2] == state[1]
    b, n = vp.clip_voice(rng, 200000, 9000, 150000, 48000, 48000)
    assert n == 48000 and 0 <= b < 159600 - 48000
    assert not (np.array_equal(rng.get_state()[1], state[0]) and rng.get_state()[2] == state[1])


def test_three_desks_equal_the_reference(golden):
    g = golden("g19_voice_recipe")
    assert max(int(g[f"d{s}_redraws"]) for s in g["desk_seeds"]) >= 1
    for s in (int(v) for v in g["desk_seeds"]):
        rng = np.random.RandomState(s)
        room = room_scenes.draw_room(rng)
        absorption = rng.uniform(low=room_scenes.ABSORPTION[0], high=room_scenes.ABSORPTION[1])
        arrays, desks, wall = vp.draw_three_desks(rng, 7, room)
        np.testing.assert_array_equal(room, g[f"d{s}_room"])
        assert absorption == float(g[f"d{s}_absorption"]) and wall == int(g[f"d{s}_wall"])
        np.testing.assert_array_equal(np.stack(arrays), g[f"d{s}_mics"])
        np.testing.assert_array_equal(np.array(desks), g[f"d{s}_sizes"])
        assert rng.uniform() == float(g[f"d{s}_after"])


def test_colocated_array_is_a_circle():
    rng, twin = np.random.RandomState(4), np.random.RandomState(4)
    mics = vp.colocated_array(rng, np.array([3.0, 2.0, 0.02]), 7)
    phi0 = twin.uniform(0, 2 * np.pi)
    assert mics.shape == (7, 3) and rng.uniform() == twin.uniform()           # one draw
    np.testing.assert_allclose(np.hypot(mics[:, 0] - 3.0, mics[:, 1] - 2.0), 0.05, rtol=1e-12)
    np.testing.assert_array_equal(mics[:, 2], 0.02)
    np.testing.assert_allclose(mics[0, :2], [3.0 + 0.05 * np.cos(phi0), 2.0 + 0.05 * np.sin(phi0)], rtol=1e-15)
    np.testing.assert_allclose(np.diff(np.unwrap(np.arctan2(mics[:, 1] - 2.0, mics[:, 0] - 3.0))), 2 * np.pi / 7, rtol=1e-9)


# ---- the library's refusals, which happen before any launch -------------------------------------------------------------
def test_library_refusals_need_no_gpu():
    L = native.lib()
    x = np.zeros(64, dtype=np.float32)
    off, wb = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    ln, wl = np.array([10, 20], dtype=np.int32), np.array([4, 4], dtype=np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                              # noqa: E731  (never dereferenced: every call is refused)

    def resample(up=3, down=1, h_len=61, T_out=8, n=2, off=off, ln=ln, wb=wb, wl=wl, ws=p(x), ws_bytes=64, x_len=64):
        return L.asw_voice_resample(p(x), x_len, p(off), p(ln), n, up, down, p(x), h_len, p(wb), p(wl), T_out, p(x), 0, ws, ws_bytes, None)

    for kw, msg in ((dict(up=641, h_len=12821), b"beyond max(up, down) <= 640"), (dict(up=1, down=1282, h_len=12821), b"beyond max"),
                    (dict(up=0), b"must be positive"), (dict(h_len=60), b"has 61 taps, got 60"), (dict(T_out=0), b"T_out = 0"),
                    (dict(n=-1), b"n = -1"), (dict(n=70000), b"n = 70000"), (dict(ln=np.array([10, 70], dtype=np.int32)), b"leaves x"),
                    (dict(off=np.array([0, -1], dtype=np.int64)), b"leaves x"), (dict(wb=np.array([0, -1], dtype=np.int64)), b"win_begin[1]"),
                    (dict(wl=np.array([4, 9], dtype=np.int32)), b"win_len[1] = 9"), (dict(ws=None), b"null pointer"),
                    (dict(ws_bytes=8), b"too small"), (dict(up=6, down=2, h_len=60), b"filter of 3/1")):
        assert resample(**kw) == -1 and msg in L.asw_last_error(), (kw, L.asw_last_error())
    assert resample(n=0) == 0                                                  # nothing to do: no launch
    assert L.asw_voice_resample_workspace_bytes(3) == 3 * 24 and L.asw_voice_resample_workspace_bytes(-1) == 0

    def trim(n=2, max_len=20, thr=0.1, ln=ln, ws=p(x), ws_bytes=256):
        return L.asw_voice_trim(p(x), 64, p(off), p(ln), n, max_len, thr, p(x), p(x), ws, ws_bytes, None)

    for kw, msg in ((dict(max_len=15), b"row_len[1] = 20 outside 0..15"), (dict(thr=float("nan")), b"not a number"),
                    (dict(ws=None), b"null pointer"), (dict(ws_bytes=16), b"too small"), (dict(n=-2), b"n = -2"),
                    (dict(max_len=-1), b"max_len = -1")):
        assert trim(**kw) == -1 and msg in L.asw_last_error(), (kw, L.asw_last_error())
    assert trim(n=0) == 0
    assert L.asw_voice_trim_workspace_bytes(2, 1025) == 2 * (24 + 3 * 8) and L.asw_voice_trim_workspace_bytes(2, -1) == 0
    assert L.asw_abi_version() == 3


# ---- the generator on the host backend ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return make_corpus(str(tmp_path_factory.mktemp("voices")))


def run(out, corpus, *flags):
    assert generate.main([str(out), "--voices", corpus, "--backend", "host"] + GENERATE_ARGS + list(flags)) == 0
    return str(out)


def _wav(path):
    from scipy.io import wavfile
    return wavfile.read(path)[1]


def test_read_voice_resample_flag(corpus):
    path = os.path.join(corpus, "p001", "u1.wav")
    with pytest.raises(ValueError, match="resample the voices beforehand"):
        room_scenes.read_voice(path, 48000)
    x, sr = room_scenes.read_voice(path, 48000, resample=True)
    assert sr == 44100 and x.dtype == np.float32 and x.ndim == 1
    y, sr16 = room_scenes.read_voice(os.path.join(corpus, "p002", "u1.wav"), 48000, resample=True)      # the int16 file
    assert sr16 == 16000 and y.dtype == np.float32 and np.max(np.abs(y)) < 1.0


def test_generate_reference_voices_equal_the_statements(corpus, tmp_path):
    out = run(tmp_path / "ref", corpus, "--voice_prep", "reference", "--voice_index", str(tmp_path / "index.json"), "--max_order", "0")
    # the same draws again, and the dry voices from the statements alone
    rng = np.random.RandomState(0)
    index = vp.VoiceIndex(48000, "host")
    voices = room_scenes.list_voices(corpus)
    rates = set()
    for i in range(2):
        n = rng.randint(2, 4)
        spec = room_scenes.make_room_spec(rng, n, 4, 24000, 0, None, 48000, voices, prep="reference", index=index)
        assert isinstance(spec.dry, room_scenes.VoicePicks) and spec.dry.shape == (n, 24000)
        dry = np.zeros((n, 24000), dtype=np.float32)
        for r, (path, begin, length) in enumerate(spec.dry.picks):
            x, sr = room_scenes.read_voice(path, 48000, resample=True)
            rates.add(sr)
            y = vp.resample_poly_f64(x, 48000, sr).astype(np.float32)
            e = index.entry(path)
            assert e["ok"] and (e["n"], e["begin"], e["end"]) == (y.shape[0],) + vp.trim_f64(y)[:2]
            dry[r, :length] = y[begin:begin + length]
        spec.meta["dry_len"] = [length for _p, _b, length in spec.dry.picks]
        spec.dry = dry
        scene = room_scenes.simulate_rooms([spec], backend="host", exact_silence=True)[0]
        plain = room_scenes.simulate_rooms([spec], backend="host")[0]
        # exact_silence only replaces the transforms' rounding noise where no sound has arrived by zeros
        for a, b in ((scene.mix, plain.mix), (scene.sources, plain.sources)):
            changed = a != b
            assert changed.any() and not a[changed].any() and np.max(np.abs(b[changed])) < 1e-12 * np.max(np.abs(b))
            first = np.argmax(a != 0, axis=1)
            assert first.min() > 100 and not ((np.abs(a) < 1e-12 * np.max(np.abs(b))) & (a != 0)).any()
        d = os.path.join(out, f"{i:05d}")
        for s in range(n):
            np.testing.assert_array_equal(_wav(os.path.join(d, f"mic00_voice{s:02d}.wav")), scene.sources[s])
        np.testing.assert_array_equal(_wav(os.path.join(d, "mic02_mixed.wav")), scene.mix[2])
        with open(os.path.join(d, "metadata.json")) as f:
            meta = json.load(f)
        assert [meta[f"voice{s:02d}"]["speaker_id"] for s in range(n)] == spec.meta["speaker_id"]
        assert all(i.startswith("p0") for i in spec.meta["speaker_id"]) and len(set(spec.meta["speaker_id"])) == n
    assert rates == {16000, 44100}
    with open(tmp_path / "index.json") as f:
        stored = json.load(f)
    assert stored["fs"] == 48000 and stored["files"] and all(f.startswith(corpus) for f in stored["files"])
    again = vp.VoiceIndex(48000, "host", path=str(tmp_path / "index.json"))
    assert all(again._fresh(f) for f in stored["files"])                       # read back, not computed again
    silent = os.path.join(corpus, "p001", "u0.wav")
    assert not again.entry(silent)["ok"] and again.entry(os.path.join(corpus, "p001", "u1.wav"))["ok"]


def test_generate_dereverb_is_the_order_zero_simulation(corpus, tmp_path):
    plain = run(tmp_path / "plain", corpus, "--voice_prep", "reference")
    out = run(tmp_path / "dereverb", corpus, "--voice_prep", "reference", "--generate_dereverb")
    zero = run(tmp_path / "zero", corpus, "--voice_prep", "reference", "--max_order", "0")
    a, b, z = tree(plain), tree(out), tree(zero)
    extra = sorted(set(b) - set(a))
    assert extra and all(f.endswith("_dereverb.wav") for f in extra) and all(a[f] == b[f] for f in a if f != "args.json")
    for f in extra:
        got, want = _wav(os.path.join(out, f)), _wav(os.path.join(zero, f.replace("_dereverb", "")))
        # the same float64 response through a transform of another length, rounded to float32: within one float32 ulp of
        # the peak of the row
        assert np.max(np.abs(got - want)) <= np.spacing(np.float32(np.max(np.abs(want))))
        assert np.max(np.abs(want)) > 1e-3
    with open(os.path.join(out, "args.json")) as f:
        assert json.load(f)["generate_dereverb"] is True


def test_generate_colocated_writes_a_second_tree(corpus, tmp_path):
    out = run(tmp_path / "main", corpus, "--voice_prep", "reference", "--generate_colocated")
    plain = run(tmp_path / "plain", corpus, "--voice_prep", "reference")
    side = out + "_colocated"
    assert sorted(os.listdir(side)) == ["00000", "00001"]
    for name in ("00000", "00001"):
        with open(os.path.join(out, name, "metadata.json")) as f:
            main_meta = json.load(f)
        with open(os.path.join(side, name, "metadata.json")) as f:
            meta = json.load(f)
        mics = np.array([meta[f"mic{m:02d}"]["position"] for m in range(4)])
        centre = np.mean([main_meta[f"mic{m:02d}"]["position"] for m in range(4)], axis=0)
        np.testing.assert_allclose(np.hypot(*(mics[:, :2] - centre[:2]).T), 0.05, rtol=1e-9)
        assert meta["voice00"]["position"] == main_meta["voice00"]["position"] and meta["Room_dimensions"] == main_meta["Room_dimensions"]
        offsets = room_scenes.sample_offsets(mics, np.array(meta["voice00"]["position"]), 48000)
        assert meta["voice00"]["shifts"] == np.round(offsets).astype(int).tolist() and max(map(abs, meta["voice00"]["shifts"])) <= 15
        assert meta["voice00"]["speaker_id"] == main_meta["voice00"]["speaker_id"]
    # the first scene is the scene of a run without the option; the circle's one draw moves the later ones
    first = {f: v for f, v in tree(out).items() if f.startswith("00000")}
    assert first == {f: v for f, v in tree(plain).items() if f.startswith("00000")}


def test_generate_size_writes_three_trees(corpus, tmp_path):
    out = run(tmp_path / "size", corpus, "--voice_prep", "reference", "--generate_size")
    assert sorted(os.listdir(out)) == ["args.json", "large", "middle", "small"]
    metas = {}
    for size in ("large", "middle", "small"):
        assert sorted(os.listdir(os.path.join(out, size))) == ["00000", "00001"]
        with open(os.path.join(out, size, "00000", "metadata.json")) as f:
            metas[size] = json.load(f)
    lo = {"large": (1.9, 1.1), "middle": (1.4, 0.8), "small": (1.0, 0.5)}
    for size, m in metas.items():
        assert lo[size][0] <= m["Desk_size"][0] <= lo[size][0] + 0.1 and lo[size][1] <= m["Desk_size"][1] <= lo[size][1] + 0.1
        assert m["voice01"] ["position"] == metas["large"]["voice01"]["position"] and m["Pick_wall"] == metas["large"]["Pick_wall"]
        assert m["mic00"]["position"] == metas["large"]["mic00"]["position"]                   # the desks share microphone 0
        mics = np.array([m[f"mic{k:02d}"]["position"] for k in range(4)])
        offsets = room_scenes.sample_offsets(mics, np.array(m["voice01"]["position"]), 48000)
        assert m["voice01"]["shifts"] == np.round(offsets).astype(int).tolist()
    assert metas["small"]["mic03"]["position"] != metas["large"]["mic03"]["position"]
    assert tree(os.path.join(out, "small"))["00000/mic01_mixed.wav"] != tree(os.path.join(out, "large"))["00000/mic01_mixed.wav"]


def test_generate_defaults_are_todays_path(corpus, tmp_path):
    """Without the new flags the scenes are those of a run with the flags at their defaults, and ``draw_voices`` keeps its
    order of draws: files chosen as they are, after the geometry."""
    at16k = str(tmp_path / "at48k")
    os.makedirs(os.path.join(at16k, "a"))
    from scipy.io import wavfile
    for k in range(4):
        wavfile.write(os.path.join(at16k, "a", f"v{k}.wav"), 48000, signal(30000 + 9000 * k, k))
    base = [str(tmp_path / "d0"), "--voices", at16k, "--backend", "host"] + GENERATE_ARGS
    assert generate.main(base) == 0
    assert generate.main([str(tmp_path / "d1")] + base[1:] + ["--voice_prep", "none"]) == 0
    a, b = tree(tmp_path / "d0"), tree(tmp_path / "d1")
    assert sorted(a) == sorted(b) and all(a[f] == b[f] for f in a if f != "args.json")
    rng = np.random.RandomState(0)
    n = rng.randint(2, 4)
    spec = room_scenes.make_room_spec(rng, n, 4, 24000, 2, None, 48000, room_scenes.list_voices(at16k))
    scene = room_scenes.simulate_rooms([spec], backend="host")[0]
    np.testing.assert_array_equal(_wav(os.path.join(tmp_path / "d0", "00000", "mic01_mixed.wav")), scene.mix[1])
    with open(tmp_path / "d0" / "args.json") as f:
        args = json.load(f)
    assert args["voice_prep"] == "none" and args["voice_index"] is None
    assert not (args["generate_dereverb"] or args["generate_colocated"] or args["generate_size"])


@pytest.mark.parametrize("flags,match", [
    (["--generate_size", "--generate_rt60"], "generate_size"), (["--generate_size", "--sample_rt60"], "generate_size"),
    (["--generate_size", "--generate_colocated"], "generate_size"), (["--generate_colocated", "--generate_rt60"], "generate_colocated"),
    (["--voice_index", "x.json"], "voice_index")])
def test_generate_refuses_what_the_reference_cannot_reach(tmp_path, flags, match):
    with pytest.raises(SystemExit, match=match):
        generate.main([str(tmp_path / "o"), "--n_outputs", "1", "--backend", "host"] + flags)


def test_reference_prep_needs_voices(tmp_path):
    with pytest.raises(SystemExit, match="needs --voices"):
        generate.main([str(tmp_path / "o"), "--n_outputs", "1", "--backend", "host", "--voice_prep", "reference"])
    with pytest.raises(ValueError, match="neither"):
        room_scenes.draw_voices(np.random.RandomState(0), 2, 100, prep="librosa")
    with pytest.raises(ValueError, match="still picks"):
        room_scenes._cat_dry([room_scenes.VoicePicks([], 10, 48000)])
    assert roomsim.MAX_ORDER == 150
