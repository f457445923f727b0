"""The shoebox room simulator as a float64 statement (numpy only, no torch): image-source impulse responses and their
convolution with the dry voices.  It is what ``csrc/room_kernels.hip`` is held to.

The reference hands this arithmetic to pyroomacoustics 0.5.0 (datasets/generate_dataset.py); that library is not
available here, so the statement is written from the published image-source method and parity with pyroomacoustics is
unpinned.

Room: an axis-aligned box [Lx, Ly, Lz] with one corner at the origin and one energy absorption ``a`` on all six walls,
amplitude reflection r = sqrt(1 - a).  Images: all integer triples n with |nx| + |ny| + |nz| <= max_order, in the order
nx, then ny, then nz ascending; along an axis image n lies at n L + s for even n and (n + 1) L - s for odd n.  An image
at distance d arrives after t = d / c * fs samples with gain r^(|nx|+|ny|+|nz|) / (4 pi d) and adds an 81-tap
Hann-windowed sinc centred at 40 + t, so a response carries a lead-in of 40 samples.

The distance and delay arithmetic below is explicit ``+ - * / sqrt floor`` in one order: the device repeats it operation
by operation, so that floor(t) comes out the same for every image.
"""
import numpy as np

from .patch import SPEED_OF_SOUND

TAPS = 81            # taps of the fractional-delay filter
LEAD = 40            # its centre: the lead-in of every response
MAX_ORDER = 150      # what the dataset generator caps the order at, and the device accepts
MAX_LENGTH = 1 << 25


def image_count(max_order: int) -> int:
    """Number of integer triples with |nx| + |ny| + |nz| <= max_order."""
    N = int(max_order)
    return (2 * N + 1) * (2 * N * N + 2 * N + 3) // 3


def _lattice(max_order: int) -> np.ndarray:
    """The triples [I, 3] in canonical order: nx ascending, then ny, then nz."""
    N = int(max_order)
    r = np.arange(-N, N + 1)
    nx, ny = (v.ravel() for v in np.meshgrid(r, r, indexing="ij"))
    rem = N - np.abs(nx) - np.abs(ny)                       # the (nx, ny) columns and the |nz| each one allows
    nx, ny, rem = nx[rem >= 0], ny[rem >= 0], rem[rem >= 0]
    height = 2 * rem + 1
    first = np.cumsum(height) - height
    nz = np.arange(int(height.sum())) - np.repeat(first + rem, height)
    return np.stack([np.repeat(nx, height), np.repeat(ny, height), nz], axis=1).astype(np.int64)


def _check_room(room):
    room = np.asarray(room, dtype=np.float64)
    if room.shape != (3,):
        raise ValueError(f"only 3-D shoebox rooms: got dimensions of shape {room.shape}")
    if not np.all(room > 0):
        raise ValueError(f"room sides must be positive, got {room}")
    return room


def shoebox_images(room, src, max_order):
    """-> (n [I, 3] int64, positions [I, 3] float64) of the images of ``src`` in canonical order."""
    room = _check_room(room)
    src = np.asarray(src, dtype=np.float64)
    n = _lattice(max_order)
    pos = np.empty(n.shape, dtype=np.float64)
    for a in range(3):
        na = n[:, a]
        even = na * room[a] + src[a]
        odd = (na + 1) * room[a] - src[a]
        pos[:, a] = np.where(na % 2 == 0, even, odd)
    return n, pos


def _check_scene(room, absorption, max_order, src, mics):
    room = _check_room(room)
    if not 0.0 < absorption <= 1.0:
        raise ValueError(f"absorption {absorption} outside (0, 1]")
    if not 0 <= int(max_order) <= MAX_ORDER:
        raise ValueError(f"max_order {max_order} outside 0..{MAX_ORDER}")
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    mics = np.asarray(mics, dtype=np.float64).reshape(-1, 3)
    for name, p in (("source", src), ("microphone", mics)):
        if not (np.all(p > 0) and np.all(p < room)):
            raise ValueError(f"a {name} lies outside the room {room}")
    if np.any(np.all(src[:, None, :] == mics[None, :, :], axis=2)):
        raise ValueError("a source sits at a microphone's position")
    return room, src, mics


def image_delays_f64(room, absorption, max_order, src, mic, fs):
    """(ip int64 [I], f [I], gain [I]) of the images of ``src`` at ``mic``, in canonical order: the delay
    t = d / c * fs split into floor and fraction, and r^order / (4 pi d)."""
    n, pos = shoebox_images(room, src, max_order)
    mic = np.asarray(mic, dtype=np.float64)
    dx = pos[:, 0] - mic[0]
    dy = pos[:, 1] - mic[1]
    dz = pos[:, 2] - mic[2]
    d = np.sqrt(dx * dx + dy * dy + dz * dz)
    t = d / SPEED_OF_SOUND * float(fs)
    ip = np.floor(t)
    f = t - ip
    r = np.sqrt(1.0 - float(absorption))
    order = np.abs(n[:, 0]) + np.abs(n[:, 1]) + np.abs(n[:, 2])
    gain = r ** order / (4 * np.pi * d)
    return ip.astype(np.int64), f, gain


def rir_length(room, max_order, fs, T):
    """min(T, floor(fs / c * (max_order + 1) * |L|_2) + 81): every image lies within (max_order + 1) L_d of the microphone
    on each axis, which bounds every delay; nothing past the clip length T is ever heard."""
    room = _check_room(room)
    diag = np.sqrt(room[0] * room[0] + room[1] * room[1] + room[2] * room[2])
    return int(min(int(T), int(np.floor(float(fs) / SPEED_OF_SOUND * (int(max_order) + 1) * diag)) + TAPS))


_WINDOW = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(TAPS) / (TAPS - 1))
_IMAGE_CHUNK = 1 << 15


def _pair_rir(room, absorption, max_order, src, mic, fs, length):
    ip, f, gain = image_delays_f64(room, absorption, max_order, src, mic, fs)
    keep = ip < length
    ip, f, gain = ip[keep], f[keep], gain[keep]
    h = np.zeros(length + TAPS, dtype=np.float64)
    j = np.arange(TAPS)
    for a in range(0, ip.shape[0], _IMAGE_CHUNK):
        sl = slice(a, a + _IMAGE_CHUNK)
        taps = gain[sl, None] * _WINDOW[None, :] * np.sinc((j[None, :] - LEAD) - f[sl, None])
        h += np.bincount((ip[sl, None] + j[None, :]).ravel(), weights=taps.ravel(), minlength=length + TAPS)
    return h[:length]


def _check_counts(counts, rows):
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts) or sum(counts) != rows:
        raise ValueError(f"counts {counts} do not describe {rows} packed sources")
    return counts


def rir_f64(rooms, absorptions, max_orders, src, mics, counts, fs, length):
    """Impulse responses [sum S, M, length] of K scenes: rooms [K, 3], absorptions [K], max_orders [K], the packed sources
    src [sum S, 3] with counts [K] of them per scene, and mics [K, M, 3]."""
    rooms = np.asarray(rooms, dtype=np.float64)
    if rooms.ndim != 2 or rooms.shape[1] != 3:
        raise ValueError(f"only 3-D shoebox rooms: rooms must be [K, 3], got {rooms.shape}")
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    mics = np.asarray(mics, dtype=np.float64)
    K = rooms.shape[0]
    counts = _check_counts(counts, src.shape[0])
    if not (len(counts) == K == len(absorptions) == len(max_orders) and mics.ndim == 3 and mics.shape[0] == K and mics.shape[2] == 3):
        raise ValueError("rooms, absorptions, max_orders, counts and mics do not describe the same scenes")
    length = int(length)
    if not 1 <= length <= MAX_LENGTH:
        raise ValueError(f"length {length} outside 1..2^25")
    M = mics.shape[1]
    out = np.zeros((src.shape[0], M, length), dtype=np.float64)
    row = 0
    for k in range(K):
        room, s_k, m_k = _check_scene(rooms[k], float(absorptions[k]), max_orders[k], src[row:row + counts[k]], mics[k])
        for s in range(counts[k]):
            for m in range(M):
                out[row + s, m] = _pair_rir(room, float(absorptions[k]), int(max_orders[k]), s_k[s], m_k[m], fs, length)
        row += counts[k]
    return out


def convolve_f64(dry, rir, counts):
    """premix[s, m, t] = sum_k dry[s, t - k] rir[s, m, k] for t < T, and mix[k, m] the sum of scene k's premix rows in
    source order -> (premix [sum S, M, T], mix [K, M, T]).  ``dry`` holds float32 values, widened exactly."""
    dry = np.asarray(dry)
    rir = np.asarray(rir, dtype=np.float64)
    if dry.ndim != 2 or rir.ndim != 3 or rir.shape[0] != dry.shape[0]:
        raise ValueError(f"dry {dry.shape} and rir {rir.shape} do not describe the same sources")
    counts = _check_counts(counts, dry.shape[0])
    T, length = dry.shape[1], rir.shape[2]
    if not (1 <= T <= MAX_LENGTH and 1 <= length <= MAX_LENGTH):
        raise ValueError(f"T {T} or length {length} outside 1..2^25")
    x = dry.astype(np.float32).astype(np.float64)
    n = 1 << int(np.ceil(np.log2(T + length - 1))) if T + length > 2 else 2
    X = np.fft.rfft(x, n, axis=1)
    premix = np.fft.irfft(X[:, None, :] * np.fft.rfft(rir, n, axis=2), n, axis=2)[:, :, :T]
    M = rir.shape[1]
    mix = np.zeros((len(counts), M, T), dtype=np.float64)
    row = 0
    for k, c in enumerate(counts):
        for s in range(c):
            mix[k] = mix[k] + premix[row + s]
        row += c
    return np.ascontiguousarray(premix), mix


def inverse_sabine(rt60, room):
    """(energy absorption, max_order) that give a shoebox ``room`` the reverberation time ``rt60`` by Sabine's formula:
    e_abs = 24 ln(10) V / (c S rt60) and max_order = ceil(c rt60 / min(R) - 1) with R the l1 l2 / sqrt(l1^2 + l2^2) of
    the three pairs of sides.  The caller caps the order."""
    room = _check_room(room)
    V = room[0] * room[1] * room[2]
    S = 2.0 * (room[0] * room[1] + room[0] * room[2] + room[1] * room[2])
    e_abs = 24.0 * np.log(10.0) * V / (SPEED_OF_SOUND * S * float(rt60))
    if e_abs > 1.0:
        raise ValueError(f"rt60 = {rt60} s is too short for room {room}: it would need an absorption of {e_abs:.3f} > 1")
    R = [room[a] * room[b] / np.sqrt(room[a] * room[a] + room[b] * room[b]) for a, b in ((0, 1), (0, 2), (1, 2))]
    max_order = int(np.ceil(SPEED_OF_SOUND * float(rt60) / min(R) - 1))
    return float(e_abs), max_order
