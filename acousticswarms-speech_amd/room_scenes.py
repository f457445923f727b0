"""Reverberant scenes: the reference's dataset recipe (datasets/generate_dataset.py) over the shoebox simulator of
``roomsim`` -- on the device through ``torch.ops.asw.room_rir`` / ``room_convolve``, or on the host through the float64
statements.

The recipe is restated over a ``numpy.random.RandomState`` drawn in the reference's order, so that a seed gives the
room, desk, robot fan and talkers that ``np.random.seed`` gives the reference (tests/golden/g17_room_recipe.npz):
room and ceiling, absorption, the desk with its robots fanned from microphone 0 and pushed against one wall
(``get_random_mic_positions_desk``), then the talkers inside the pick-up range with the desk keep-out and 0.51 m between
any two (``get_random_speaker_positions``).  What the reference leaves to pyroomacoustics is ``roomsim``'s statement:
parity with pyroomacoustics is unpinned.  ``scenes.make_scene`` and everything that calls it are untouched.
"""
import json
import os
from dataclasses import dataclass, field

import numpy as np

from . import roomsim
from .patch import FS, SPEED_OF_SOUND
from .scenes import Scene, _speech_like

# generate_dataset.py:19-63
FG_VOL = (0.2, 0.5)
SPEAKER_HEIGHT = (0.1, 0.7)            # lowest height, and the span above it
MIN_SPEAKER_DIST = 0.51
MIC_HEIGHT = 0.02
ABSORPTION = (0.1, 0.99)
ROOM_SIDES = ((6, 8), (6, 8), (2, 2.5))             # length, width, ceiling of generate_sample
ROOM_SIDES_RT60 = ((4, 4.2), (4, 4.2), (1.6, 1.7))  # of generate_sample_rt60
DESK_LENGTH = (1.2, 2)
DESK_WIDTH = (0.6, 1.2)
WALL_KEEPOUT = 0.5
SPK_RANGE = (3, 4.5)                   # half width along the wall, depth into the room
SPK_RANGE_RT60 = (1.6, 2.4)
EXPAND_MAX_DEV = 0.08
THETA_MAX_DEV = np.deg2rad(6)
RT60_BANDS = ((0.08, 0.2), (0.2, 0.4), (0.4, 0.6), (0.6, 0.8))
RT60_SAMPLED = (0.08, 0.7)
ORDER_CAP = roomsim.MAX_ORDER


def draw_room(rng, sides=ROOM_SIDES):
    """[length, width, ceiling], drawn in that order."""
    return [rng.uniform(low=lo, high=hi) for lo, hi in sides]


def _fan_mics(rng, n_mics, length, width):
    """The robots of one desk before it is placed, [n_mics, 2]: microphone 0 at the origin, the others driven away from it
    at angles fanned over the half plane, each off by up to 6 degrees, until 4 cm before the edge they reach, and stopped
    up to 8 cm off."""
    corner = np.arctan(length / 2 / width)
    fan = np.linspace(0, np.pi, n_mics - 1) - np.pi / 2
    xy = np.zeros((n_mics, 2))
    for i in range(n_mics - 1):
        angle = fan[i] + rng.uniform(low=-THETA_MAX_DEV, high=THETA_MAX_DEV)
        if -corner < angle < corner:
            reach = width / np.cos(angle)                 # the far long edge
        elif angle > corner:
            reach = length / 2 / np.sin(angle)
        else:
            reach = length / 2 / np.sin(-angle)
        reach = reach - 0.04
        px = reach * np.cos(angle) + rng.uniform(low=-EXPAND_MAX_DEV, high=EXPAND_MAX_DEV)
        py = reach * np.sin(angle) + rng.uniform(low=-EXPAND_MAX_DEV, high=EXPAND_MAX_DEV)
        xy[i + 1] = np.array([px, py])
    return xy


def _place_desk(rng, room, length):
    """(wall, rotation [2, 2], centre [2]) of a desk of that length against one wall: at most 35 cm from it and at least
    1.8 m from the side walls, turned by up to pi / 8 as far as its corners allow."""
    left, right, bottom, top = 0, room[0], 0, room[1]
    wall = rng.choice(4)
    min_x, max_x, min_y, max_y = left + 0.1, right - 0.1, bottom + 0.1, top - 0.1
    near, side, max_rot = 0.35, 1.8, np.pi / 8
    if wall in (0, 2):
        x_range = [min_x, min_x + near] if wall == 0 else [max_x - near, max_x]
        y_range = [min_y + side, max_y - side]
    else:
        y_range = [min_y, min_y + near] if wall == 1 else [max_y - near, max_y]
        x_range = [min_x + side, max_x - side]
    cx = rng.uniform(low=x_range[0], high=x_range[1])
    cy = rng.uniform(low=y_range[0], high=y_range[1])
    slack = (cx - min_x, cy - min_y, max_x - cx, max_y - cy)[wall]
    facing = (0.0, np.pi / 2, np.pi, -np.pi / 2)[wall]
    if slack >= length / 2:
        # the reference leaves the turn by pi out here for the right wall
        centre = 0.0 if wall == 2 else facing
        theta = rng.uniform(low=-max_rot + centre, high=max_rot + centre)
    else:
        bound = np.arcsin(slack / (length / 2))
        if bound > max_rot:
            theta = rng.uniform(low=-max_rot + facing, high=max_rot + facing)
        else:
            theta = rng.uniform(low=-bound + facing, high=bound + facing)
    rot = np.array([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]])
    return int(wall), rot, np.array([cx, cy])


def _off_the_walls(xy, room):
    """No microphone within 6 cm of a wall (``is_valid_mic_array``)."""
    edge = 0.06
    return not np.any((xy[:, 0] <= edge) | (xy[:, 0] >= room[0] - edge) | (xy[:, 1] <= edge) | (xy[:, 1] >= room[1] - edge))


def draw_desk_mics(rng, n_mics, room):
    """The robots on the desk -> (mic_positions [n_mics, 3], [desk length, desk width], wall 0..3 = left, bottom, right,
    top).  Microphone 0 sits at the middle of the desk's wall-side edge; the others drive away from it at angles fanned
    over the half plane, each off by up to 6 degrees, until 4 cm before the edge they reach, and stop up to 8 cm off.  The
    desk is then put against one wall, at most 35 cm from it and at least 1.8 m from the side walls, and turned by up to
    pi / 8 as far as its corners allow.  An array with a microphone within 6 cm of a wall is drawn again."""
    while True:
        length = rng.uniform(low=DESK_LENGTH[0], high=DESK_LENGTH[1])
        width = rng.uniform(low=DESK_WIDTH[0], high=DESK_WIDTH[1])
        xy = _fan_mics(rng, n_mics, length, width)
        wall, rot, centre = _place_desk(rng, room, length)
        xy = xy.dot(rot) + centre
        if _off_the_walls(xy, room):
            mics = np.concatenate([xy, MIC_HEIGHT * np.ones((n_mics, 1))], axis=1)
            return mics, [length, width], wall


def sample_offsets(mics, pos, fs=FS):
    """TDoA of ``pos`` at microphones 1.. against microphone 0, in samples (``calculate_sample_offset``)."""
    return np.array([(np.linalg.norm(pos - mics[i]) - np.linalg.norm(pos - mics[0])) / SPEED_OF_SOUND * fs
                     for i in range(1, mics.shape[0])])


def draw_talkers(rng, n_voices, mics, wall, room, spk_range=SPK_RANGE, fs=FS):
    """-> (positions [n_voices, 3], offsets [n_voices, M-1] in samples, ROI).  The pick-up range reaches ``spk_range[0]`` to
    either side of microphone 0 along the desk's wall and from 25 cm to ``spk_range[1]`` into the room, 0.5 m off every
    wall; a point inside the microphones' bounding box widened by 25 cm is drawn again, and so is a talker closer than
    0.51 m to an earlier one."""
    left, right, down, up = 0, room[0], 0, room[1]
    keepout = 0.25
    box_x, box_y = np.min(mics[:, 0]), np.min(mics[:, 1])
    h = np.max(mics[:, 1]) - box_y
    w = np.max(mics[:, 0]) - box_x
    h = h + 2 * keepout
    w = w + 2 * keepout
    box_x -= keepout
    box_y -= keepout
    c = mics[0]
    half, depth = spk_range
    lo_x, hi_x, lo_y, hi_y = c[0] - half, c[0] + half, c[1] - half, c[1] + half
    if wall == 0:
        lo_x, hi_x = c[0] + keepout, c[0] + depth
    elif wall == 1:
        lo_y, hi_y = c[1] + keepout, c[1] + depth
    elif wall == 2:
        lo_x, hi_x = c[0] - depth, c[0] - keepout
    else:
        lo_y, hi_y = c[1] - depth, c[1] - keepout
    min_x, max_x = max([lo_x, left + WALL_KEEPOUT]), min([hi_x, right - WALL_KEEPOUT])
    min_y, max_y = max([lo_y, down + WALL_KEEPOUT]), min([hi_y, up - WALL_KEEPOUT])
    roi = [min_x - 0.1, max_x + 0.1, min_y - 0.1, max_y + 0.1, SPEAKER_HEIGHT[0] - 0.1, SPEAKER_HEIGHT[0] + SPEAKER_HEIGHT[1] + 0.1]
    voices, offsets = [], []
    for _ in range(n_voices):
        while True:
            while True:
                x = rng.uniform(low=min_x, high=max_x)
                y = rng.uniform(low=max_y, high=min_y)        # from the far end down, as the reference passes them
                if not (x >= box_x and x - box_x <= w and y >= box_y and y - box_y <= h):
                    break
            z = rng.random_sample() * SPEAKER_HEIGHT[1] + SPEAKER_HEIGHT[0]
            pos = np.array([x, y, z])
            if all(np.linalg.norm(q - pos) >= MIN_SPEAKER_DIST for q in voices):
                break
        voices.append(pos)
        offsets.append(sample_offsets(mics, pos, fs))
    return np.array(voices), np.array(offsets), [float(v) for v in roi]


def draw_geometry(rng, n_voices, n_mics=7, rt60_room=False, fs=FS):
    """Room, absorption, desk and talkers in the reference's order of draws (``generate_sample``; with ``rt60_room`` the
    small room and short pick-up range of ``generate_sample_rt60``, which draws no absorption)."""
    room = draw_room(rng, ROOM_SIDES_RT60 if rt60_room else ROOM_SIDES)
    absorption = None if rt60_room else rng.uniform(low=ABSORPTION[0], high=ABSORPTION[1])
    mics, desk, wall = draw_desk_mics(rng, n_mics, room)
    voices, offsets, roi = draw_talkers(rng, n_voices, mics, wall, room, SPK_RANGE_RT60 if rt60_room else SPK_RANGE, fs)
    return {"room": [float(v) for v in room], "absorption": absorption, "mics": mics, "desk": [float(v) for v in desk], "wall": wall,
            "voices": voices, "offsets": offsets, "roi": roi}


def rt60_to_absorption(rt60, room):
    """(rt60, absorption, max_order): ``roomsim.inverse_sabine`` with the reference's retry -- an rt60 too short for the
    room grows by 20 ms until it is not -- and its cap of the order at 150."""
    while True:
        try:
            absorption, order = roomsim.inverse_sabine(rt60, room)
            return float(rt60), absorption, min(order, ORDER_CAP)
        except ValueError:
            rt60 = rt60 + 0.02


@dataclass
class RoomSpec:
    """One scene for ``simulate_rooms``."""
    room: list                       # [Lx, Ly, Lz]
    absorption: float
    max_order: int
    mics: np.ndarray                 # [M, 3]
    sources: np.ndarray              # [S, 3]
    dry: np.ndarray                  # [S, T] float32
    roi: list = None
    fs: int = FS
    meta: dict = field(default_factory=dict)       # what the dataset writer adds: Desk_size, Pick_wall, rt60, shifts, ids


def _cat_dry(rows):
    """The dry voices of the specs of one call as one [sum S, T] float32 array -- or, when ``fetch_voices`` left them on the
    device, as one tensor there."""
    if any(isinstance(d, VoicePicks) for d in rows):
        raise ValueError("the voices of a spec are still picks: call fetch_voices on the specs first")
    if not any(hasattr(d, "is_cuda") for d in rows):
        return np.ascontiguousarray(np.concatenate([np.asarray(d, dtype=np.float32) for d in rows]))
    import torch
    dev = next(d.device for d in rows if hasattr(d, "is_cuda"))
    return torch.cat([d if hasattr(d, "is_cuda") else torch.from_numpy(np.asarray(d, dtype=np.float32)).to(dev) for d in rows])


def _pack(specs):
    M, T, fs = specs[0].mics.shape[0], specs[0].dry.shape[1], specs[0].fs
    for sp in specs:
        if sp.mics.shape != (M, 3) or sp.dry.shape[1] != T or sp.fs != fs or sp.dry.shape[0] != np.asarray(sp.sources).reshape(-1, 3).shape[0]:
            raise ValueError("the specs of one call share the number of microphones, the length and the rate")
    rooms = np.array([sp.room for sp in specs], dtype=np.float64)
    if rooms.ndim != 2 or rooms.shape[1] != 3:
        raise ValueError(f"only 3-D shoebox rooms: got dimensions of shape {rooms.shape}")
    absorption = np.array([sp.absorption for sp in specs], dtype=np.float64)
    orders = [int(sp.max_order) for sp in specs]
    counts = [int(sp.dry.shape[0]) for sp in specs]
    src = np.concatenate([np.asarray(sp.sources, dtype=np.float64).reshape(-1, 3) for sp in specs])
    mics = np.stack([np.asarray(sp.mics, dtype=np.float64) for sp in specs])
    dry = _cat_dry([sp.dry for sp in specs])
    length = max(roomsim.rir_length(sp.room, sp.max_order, fs, T) for sp in specs)
    return rooms, absorption, orders, src, mics, counts, dry, fs, length, M, T


def _silence(sp, length, T):
    """(first [S, M], last [S]): the samples of a scene that no sound reaches.  Before ``first[s, m]``, one past the floored
    delay of the direct image, the response of source s at microphone m is exactly zero (every other image is farther, the
    tap window starts at the floored delay and its first weight, the Hann window's, is zero); from ``last[s]`` on, the voice's last sample (``meta["dry_len"]``, else T) has left
    a response of ``length`` samples behind."""
    src = np.asarray(sp.sources, dtype=np.float64).reshape(-1, 3)
    first = np.array([[int(roomsim.image_delays_f64(sp.room, sp.absorption, 0, s, m, sp.fs)[0][0]) + 1 for m in np.asarray(sp.mics)] for s in src],
                     dtype=np.int64).reshape(src.shape[0], -1)
    lens = sp.meta.get("dry_len") or [T] * src.shape[0]
    return first, np.minimum(np.asarray(lens, dtype=np.int64) + length, T)


def simulate_rooms(specs, backend="device", device="cuda:0", exact_silence=False):
    """The specs -> a list of ``Scene`` (mix [M, T] and the sources as received at microphone 0, float32; rounded from the
    float64 simulation only here).  ``backend="device"`` sends all specs of one (M, T, fs) in one ``room_rir`` and one
    ``room_convolve`` call, with one upload of the dry voices and one read-back; ``"host"`` runs the float64 statements.
    The response length is the largest ``roomsim.rir_length`` of the group.

    The convolution goes through transforms, so a sample that no sound reaches -- before the direct sound arrives, after
    the last response has died -- comes out as rounding noise of about 1e-18, another on each backend.
    ``exact_silence`` writes those samples as the zeros they are (``_silence``); the default leaves every byte as it was."""
    if backend not in ("device", "host"):
        raise ValueError(f"backend {backend!r} is neither 'device' nor 'host'")
    specs = list(specs)
    scenes = [None] * len(specs)
    groups = {}
    for i, sp in enumerate(specs):
        groups.setdefault((sp.mics.shape[0], sp.dry.shape[1], sp.fs), []).append(i)
    for idx in groups.values():
        rooms, absorption, orders, src, mics, counts, dry, fs, length, M, T = _pack([specs[i] for i in idx])
        if backend == "host":
            rir = roomsim.rir_f64(rooms, absorption, orders, src, mics, counts, fs, length)
            premix, mix = roomsim.convolve_f64(dry if isinstance(dry, np.ndarray) else dry.cpu().numpy(), rir, counts)
            gt, mix = premix[:, 0].astype(np.float32), mix.astype(np.float32)
        else:
            import torch
            from . import native
            t = native.torch_ops()
            with torch.cuda.device(device):
                rir = t.room_rir(torch.from_numpy(rooms), torch.from_numpy(absorption), orders, torch.from_numpy(src),
                                 torch.from_numpy(mics), counts, float(fs), length)
                premix, dmix = t.room_convolve(native.to_device(dry, rir.device) if isinstance(dry, np.ndarray) else dry, rir, counts)
                gt, mix = native.read_back(premix[:, 0].to(torch.float32), dmix.to(torch.float32))
        row = 0
        for k, i in enumerate(idx):
            sp = specs[i]
            roi = sp.roi if sp.roi is not None else [0.0, float(sp.room[0]), 0.0, float(sp.room[1]), 0.0, float(sp.room[2])]
            scene_mix, scene_gt = np.ascontiguousarray(mix[k]), np.ascontiguousarray(gt[row:row + counts[k]])
            if exact_silence and counts[k]:
                first, last = _silence(sp, length, T)
                for s in range(counts[k]):
                    scene_gt[s, :first[s, 0]] = 0
                    scene_gt[s, last[s]:] = 0
                for m in range(M):
                    scene_mix[m, :first[:, m].min()] = 0
                scene_mix[:, last.max():] = 0
            scenes[i] = Scene(np.asarray(sp.mics, dtype=np.float64), np.asarray(sp.sources, dtype=np.float64).reshape(-1, 3), list(roi),
                              scene_mix, scene_gt, sp.fs)
            row += counts[k]
    return scenes


def read_voice(path, fs, resample=False):
    """A wav file as float32 mono, at ``fs`` already: there is no resampling here, a file at another rate raises.  With
    ``resample`` the answer is (x, its rate) whatever the rate is: the caller resamples (``voiceprep``)."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if sr != fs and not resample:
        raise ValueError(f"{path} is at {sr} Hz, the scene at {fs} Hz: resample the voices beforehand")
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    elif x.dtype == np.int32:
        x = x.astype(np.float32) / 2147483648.0
    x = x.astype(np.float32)
    x = x.mean(axis=1).astype(np.float32) if x.ndim == 2 else x
    return (x, int(sr)) if resample else x


def list_voices(voices_dir):
    """The wav files below ``voices_dir``, sorted; a file's speaker is the directory that holds it."""
    found = []
    for base, _dirs, files in sorted(os.walk(voices_dir)):
        found += [os.path.join(base, f) for f in sorted(files) if f.lower().endswith(".wav")]
    if not found:
        raise ValueError(f"no wav files below {voices_dir}")
    return found


@dataclass
class VoicePicks:
    """The voices of a scene before their audio is fetched: [(file, win_begin, win_len)] at ``fs`` and the length T."""
    picks: list
    T: int
    fs: int

    @property
    def shape(self):
        return (len(self.picks), self.T)


def speaker_dirs(voices):
    """The directories that hold the wav files of ``list_voices``, sorted: one speaker each."""
    return sorted({os.path.dirname(f) for f in voices})


def draw_voices(rng, n_voices, T, fs=FS, voices=None, prep="none", index=None, backend="device"):
    """(dry [n_voices, T] float32, speaker ids).  Without ``voices`` the dry signals are ``scenes._speech_like`` at a peak
    drawn from 0.2..0.5; with a list of wav files, distinct files are chosen, zero-padded at the end or cut at a random
    start to T samples, and taken at the level they have (no trimming of silence: librosa is not available).

    ``prep="reference"`` draws as the reference's ``get_voices`` does (``voiceprep.get_voices``): distinct speakers, a
    file of each that has half a second of activity after the trim, resampled to ``fs``, clipped to the activity and cut
    or padded to T.  The draws only need the ``index`` (a ``voiceprep.VoiceIndex``; one on ``backend`` is made when none
    is given), so the answer holds ``VoicePicks`` in place of the audio: ``fetch_voices`` fetches the audio of many scenes
    at once."""
    if prep not in ("none", "reference"):
        raise ValueError(f"prep {prep!r} is neither 'none' nor 'reference'")
    if prep == "reference":
        from . import voiceprep
        if voices is None:
            raise ValueError('prep="reference" prepares voice files: it needs voices')
        if index is None:
            index = voiceprep.VoiceIndex(fs, backend)
        picks, ids = voiceprep.get_voices(rng, speaker_dirs(voices), n_voices, T, fs, index)
        return VoicePicks(picks, T, fs), ids
    dry = np.zeros((n_voices, T), dtype=np.float32)
    if voices is None:
        for s in range(n_voices):
            dry[s] = (_speech_like(rng, T, fs) * rng.uniform(FG_VOL[0], FG_VOL[1])).astype(np.float32)
        return dry, [f"synthetic{s:02d}" for s in range(n_voices)]
    if len(voices) < n_voices:
        raise ValueError(f"{n_voices} talkers need as many voice files, {len(voices)} found")
    ids = []
    for s, path in enumerate(rng.choice(voices, n_voices, replace=False)):
        x = read_voice(path, fs)
        if x.shape[0] > T:
            begin = rng.choice(x.shape[0] - T)
            x = x[begin:begin + T]
        dry[s, :x.shape[0]] = x
        ids.append(os.path.basename(os.path.dirname(os.path.abspath(path))))
    return dry, ids


def fetch_voices(specs, backend="device", device="cuda:0"):
    """Replace the ``VoicePicks`` of the specs by their audio, all of them in one ``voiceprep.fetch`` (one resample call per
    distinct source rate on the device, where the result stays): specs that share their picks share the rows."""
    from . import voiceprep
    todo = {}
    for sp in specs:
        if isinstance(sp.dry, VoicePicks):
            todo.setdefault(id(sp.dry), sp.dry)
    if not todo:
        return
    groups = {}
    for vp in todo.values():
        groups.setdefault((vp.T, vp.fs), []).append(vp)
    rows_of = {}
    for (T, fs), vps in groups.items():
        dry = voiceprep.fetch([p for vp in vps for p in vp.picks], T, fs, backend, device)
        row = 0
        for vp in vps:
            rows_of[id(vp)] = dry[row:row + len(vp.picks)]
            row += len(vp.picks)
    for sp in specs:
        if isinstance(sp.dry, VoicePicks):
            sp.meta["dry_len"] = [n for _p, _b, n in sp.dry.picks]       # zeros from there on (simulate_rooms(exact_silence=))
            sp.dry = rows_of[id(sp.dry)]


def make_room_spec(rng, n_speakers, n_mics=7, T=48000, max_order=15, rt60=None, fs=FS, voices=None, rt60_room=False,
                   prep="none", index=None, geometry=draw_geometry):
    """One scene of the recipe from ``rng`` (a ``numpy.random.RandomState``): the geometry, then the voices.  ``rt60``
    replaces the drawn absorption and ``max_order`` by those of ``rt60_to_absorption``.  The RT60 room draws no
    absorption: without ``rt60`` its spec is anechoic (absorption 1) until ``with_rt60`` gives it a reverberation time.
    ``prep="reference"`` (``draw_voices``) draws the voices before the geometry, as the reference does, and leaves
    ``VoicePicks`` in ``dry`` for ``fetch_voices``."""
    if prep == "reference":
        dry, ids = draw_voices(rng, n_speakers, T, fs, voices, prep, index)
        g = geometry(rng, n_speakers, n_mics, rt60_room, fs)
    else:
        g = geometry(rng, n_speakers, n_mics, rt60_room, fs)
        dry, ids = draw_voices(rng, n_speakers, T, fs, voices)
    meta = {"Desk_size": g["desk"], "Pick_wall": g["wall"], "shifts": np.round(g["offsets"]).astype(np.int32).tolist(), "speaker_id": ids}
    if "desks" in g:
        meta["desks"], meta["desks_mics"] = g["desks"], g["desks_mics"]         # for with_mics: the writer leaves them out
    absorption, order = g["absorption"], int(max_order)
    if rt60 is not None:
        meta["rt60"], absorption, order = rt60_to_absorption(rt60, g["room"])
    elif absorption is None:
        absorption = 1.0
    return RoomSpec(g["room"], float(absorption), order, g["mics"], g["voices"], dry, g["roi"], fs, meta)


def with_mics(spec, mics, desk=None):
    """The same room, talkers and voices on another array, with that array's offsets and shifts (the colocated array and
    the desk sizes)."""
    meta = {k: v for k, v in spec.meta.items() if k not in ("desks", "desks_mics")}
    offsets = np.array([sample_offsets(mics, pos, spec.fs) for pos in np.asarray(spec.sources).reshape(-1, 3)])
    meta["shifts"] = np.round(offsets).astype(np.int32).reshape(-1, mics.shape[0] - 1).tolist()
    if desk is not None:
        meta["Desk_size"] = [float(v) for v in desk]
    return RoomSpec(spec.room, spec.absorption, spec.max_order, mics, spec.sources, spec.dry, spec.roi, spec.fs, meta)


def with_order(spec, max_order):
    """The same scene at another order of reflections (order 0: the dereverberated ground truth)."""
    return RoomSpec(spec.room, spec.absorption, int(max_order), spec.mics, spec.sources, spec.dry, spec.roi, spec.fs, dict(spec.meta))


def draw_geometry_three_desks(rng, n_voices, n_mics=7, rt60_room=False, fs=FS):
    """``draw_geometry`` of ``generate_sample_size``: three desks of falling size in one place (``voiceprep.draw_three_desks``)
    and the talkers drawn against the large one.  ``mics`` is the large desk's array, ``desks_mics`` and ``desks`` hold
    all three."""
    from .voiceprep import draw_three_desks
    room = draw_room(rng, ROOM_SIDES)
    absorption = rng.uniform(low=ABSORPTION[0], high=ABSORPTION[1])
    arrays, desks, wall = draw_three_desks(rng, n_mics, room)
    voices, offsets, roi = draw_talkers(rng, n_voices, arrays[0], wall, room, SPK_RANGE, fs)
    return {"room": [float(v) for v in room], "absorption": absorption, "mics": arrays[0], "desk": [float(v) for v in desks[0]],
            "wall": wall, "voices": voices, "offsets": offsets, "roi": roi, "desks_mics": arrays, "desks": desks}


def with_rt60(spec, rt60):
    """The same geometry and voices under another reverberation time (the RT60 sweep)."""
    meta = dict(spec.meta)
    meta["rt60"], absorption, order = rt60_to_absorption(rt60, spec.room)
    return RoomSpec(spec.room, absorption, order, spec.mics, spec.sources, spec.dry, spec.roi, spec.fs, meta)


def make_room_scene(seed, n_speakers, n_mics=7, T=48000, max_order=15, rt60=None, fs=FS, voices=None, backend="device",
                    device="cuda:0"):
    """A reverberant ``Scene`` of the reference's recipe, seeded like ``np.random.seed(seed)``."""
    spec = make_room_spec(np.random.RandomState(seed), n_speakers, n_mics, T, max_order, rt60, fs, voices)
    return simulate_rooms([spec], backend, device)[0]


def write_room_scene_dir(scene, spec, path):
    """``evalkit.write_scene_dir`` plus the reference's metadata keys (``save_scenario``): Room_dimensions, Desk_size,
    Pick_wall, absorption, rt60 when the scene has one, and shifts and speaker_id per voice."""
    from .evalkit import write_scene_dir
    write_scene_dir(scene, path)
    meta_path = os.path.join(path, "metadata.json")
    with open(meta_path) as f:
        meta = json.load(f)
    shifts, ids = spec.meta.get("shifts"), spec.meta.get("speaker_id")
    for s in range(scene.speaker_positions.shape[0]):
        if shifts is not None:
            meta[f"voice{s:02d}"]["shifts"] = [int(v) for v in shifts[s]]
        if ids is not None:
            meta[f"voice{s:02d}"]["speaker_id"] = ids[s]
    if "rt60" in spec.meta:
        meta["rt60"] = float(spec.meta["rt60"])
    meta["Room_dimensions"] = [float(v) for v in spec.room]
    meta["Desk_size"] = spec.meta.get("Desk_size")
    meta["Pick_wall"] = spec.meta.get("Pick_wall")
    meta["absorption"] = float(spec.absorption)
    with open(meta_path, "w") as f:
        json.dump(meta, f, indent=1)


def write_dereverb(scene, path):
    """The ground truth of the order-0 simulation beside the reverberant one: ``mic00_voiceNN_dereverb.wav``, which
    ``train_data.LocalizationDataset(use_dereverb=True)`` reads."""
    from scipy.io import wavfile
    for s in range(scene.sources.shape[0]):
        wavfile.write(os.path.join(path, f"mic00_voice{s:02d}_dereverb.wav"), scene.fs, scene.sources[s].astype(np.float32))
