"""Inputs shared by the room simulator tests (host and GPU): the scenes of the response cases, the sizes of the
convolution cases and their seeded dry signals, each made once and read-only.  No GPU, nothing of the reference."""
import functools

import numpy as np

from acousticswarms_speech_amd import roomsim
from acousticswarms_speech_amd.patch import FS, SPEED_OF_SOUND

SEGMENT = 1024                                     # samples a workgroup of room_rir owns


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _mics(room, M, seed):
    """M microphones a few centimetres above a desk height, spread over the middle of the floor."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.3, 0.7, (M, 2)) * np.asarray(room[:2])
    return np.concatenate([xy, np.full((M, 1), 0.77)], axis=1)


def _sources(room, S, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 0.9, (S, 3)) * np.asarray(room)


@functools.lru_cache(maxsize=None)
def rir_case(name):
    """(rooms [K,3], absorptions [K], max_orders, src [sum S,3], mics [K,M,3], counts, fs, length, statement [sum S,M,length])"""
    if name == "a":                                 # two scenes, S = 1 and 3, M = 7, orders 0 and 3; the end cuts a tap window
        room = [6.3, 7.1, 2.4]
        rooms, absorptions, orders, counts, length = [room, room], [0.35, 0.2], [0, 3], [1, 3], 1500
        src = np.concatenate([_sources(room, 1, 1), _sources(room, 3, 2)])
        mics = np.stack([_mics(room, 7, 3), _mics(room, 7, 4)])
    elif name == "b":                               # order 15
        room = [6.3, 7.1, 2.4]
        rooms, absorptions, orders, counts, length = [room], [0.3], [15], [2], 4096
        src, mics = _sources(room, 2, 5), _mics(room, 2, 6)[None]
    elif name == "c":                               # delays on, a hair above and a hair below an integer
        rooms, absorptions, orders, counts, length = [[9.0, 4.0, 3.0]], [0.25], [2], [3], 2100
        src = np.array([[1.0 + k * SPEED_OF_SOUND / FS, 1.0, 1.0] for k in (100, 257, 1000)])
        mics = np.array([[[1.0, 1.0, 1.0]]])
    elif name == "d":                               # a small room at order 40: more hits per batch of columns than one round holds
        room = [1.1, 1.3, 0.9]
        rooms, absorptions, orders, counts, length = [room], [0.05], [40], [1], 4096
        src, mics = np.array([[0.3, 0.9, 0.5]]), np.array([[[0.7, 0.4, 0.35]]])
    else:
        raise KeyError(name)
    rooms, absorptions, src, mics = (np.asarray(v, dtype=np.float64) for v in (rooms, absorptions, src, mics))
    want = roomsim.rir_f64(rooms, absorptions, orders, src, mics, counts, FS, length)
    _frozen(rooms, absorptions, src, mics, want)
    return rooms, absorptions, tuple(orders), src, mics, tuple(counts), FS, length, want


def pair_delays(case, s, m):
    """``roomsim.image_delays_f64`` of source row s at microphone m of a case."""
    rooms, absorptions, orders, src, mics, counts, fs, _length, _want = case
    k = int(np.searchsorted(np.cumsum(counts), s, side="right"))
    return roomsim.image_delays_f64(rooms[k], absorptions[k], orders[k], src[s], mics[k, m], fs)


def largest_batch(case, s=0, m=0, columns=256):
    """The most images that one batch of ``columns`` consecutive (nx, ny) columns sends into one segment, for source row s
    at microphone m: what the kernel has to hold between two accumulation rounds."""
    _rooms, _a, orders, _src, _mics, counts, _fs, length, _want = case
    N = orders[int(np.searchsorted(np.cumsum(counts), s, side="right"))]
    n = roomsim._lattice(N)
    ip = pair_delays(case, s, m)[0]
    batch = ((n[:, 0] + N) * (2 * N + 1) + (n[:, 1] + N)) // columns
    worst = 0
    for t0 in range(0, length, SEGMENT):
        hit = (ip >= t0 - (roomsim.TAPS - 1)) & (ip <= min(t0 + SEGMENT, length) - 1)
        if hit.any():
            worst = max(worst, int(np.bincount(batch[hit]).max()))
    return worst


# (T, response length, counts): the block boundary of the dry signal, one and two partitions and their boundary, a
# response longer than the signal, and two scenes of one and three sources
CONV_SIZES = ((1025, 1, (1,)), (1025, 1024, (1,)), (1025, 1025, (1,)), (1025, 3000, (1,)),
              (2500, 1, (1,)), (2500, 1024, (1,)), (2500, 1025, (1,)), (2500, 3000, (1,)), (2500, 1025, (1, 3)))
CONV_M = 2


@functools.lru_cache(maxsize=None)
def conv_case(T, length, counts, kind="statement"):
    """(dry [sum S,T] float32, rir [sum S,M,length] float64, counts).  ``kind="statement"``: the responses of
    ``roomsim.rir_f64`` for sources 0.3 to 1 m from two microphones (order 2; a response of one sample is all zero, its
    only tap carries the window's zero).  ``kind="noise"``: decaying Gaussian responses, no sample zero."""
    NS = sum(counts)
    rng = np.random.default_rng(1000 * T + length + NS)
    dry = rng.standard_normal((NS, T)).astype(np.float32)
    if kind == "noise":
        rir = rng.standard_normal((NS, CONV_M, length)) * np.exp(-np.arange(length) / 700.0)
    else:
        room = [3.1, 2.7, 2.2]
        mics = np.array([[1.5, 1.3, 1.0], [1.62, 1.3, 1.0]])
        src = mics[0] + rng.uniform(0.2, 0.55, (NS, 3))
        K = len(counts)
        rir = roomsim.rir_f64([room] * K, [0.3] * K, [2] * K, src, np.stack([mics] * K), counts, FS, length)
    _frozen(dry, rir)
    return dry, rir, counts


@functools.lru_cache(maxsize=None)
def conv_statement(T, length, counts, kind="statement"):
    dry, rir, _c = conv_case(T, length, counts, kind)
    return _frozen(*roomsim.convolve_f64(dry, rir, counts))


def row_errors(got, want, rows):
    """max abs difference over max abs value of the statement per row (the leading ``rows`` axes); a row of zeros must be
    met exactly."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    n = int(np.prod(want.shape[:rows]))
    got, want = got.reshape(n, -1), want.reshape(n, -1)
    top = np.max(np.abs(want), axis=1)
    diff = np.max(np.abs(got - want), axis=1)
    assert not diff[top == 0].any()
    return diff / np.where(top == 0, 1.0, top)
