"""CPU only: the host side of the UpFeed of a 64-channel residual stack (csrc/resstack.hip, UP): the K order in which
the last layer hands its LayerNorm rows to the matrix unit (``asw_up_feed_kperm``), the up-convolution weight packed in
that order (``asw_pack_up_feed_f16``, csrc/asw_common.cpp) and the row-tile count that sizes the partial sums
(``asw_resstack_tiles``).  Every bound is equality."""
import ctypes

import numpy as np
import pytest

from acousticswarms_speech_amd.native import lib
from tests.test_weight_pack_host import _call, _weights, split_np


def acc_row(r, h):
    """row of a 32 x 32 accumulator block that register r of a lane in half h holds (csrc/mfma_util.h)"""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def test_kperm_is_the_accumulator_order_and_a_bijection_per_kstep():
    perm = [lib().asw_up_feed_kperm(k) for k in range(16)]
    assert sorted(perm) == list(range(16))
    # as an MFMA operand, element j of lane half h is k = 8 h + j of its k-step; k-step s of a 32-channel block is made
    # of the accumulator registers 8 s .. 8 s + 7, which hold the block's channels acc_row(8 s + j, h)
    for s in range(2):
        for h in range(2):
            for j in range(8):
                assert 16 * s + perm[8 * h + j] == acc_row(8 * s + j, h)
    assert [perm[perm[k]] for k in range(16)] == list(range(16))       # bits 2 and 3 exchanged: its own inverse


def unpack(fh, fl, N, K):
    """fragment order -> [N][K] in the channel order the kernel's operand has: lane l of fragment (ks, nt) holds row
    nt 32 + (l & 31), and its element j multiplies channel ks 16 + kperm(8 (l >> 5) + j)"""
    perm = np.array([lib().asw_up_feed_kperm(k) for k in range(16)])
    NT = N // 32
    ks, nt, l, j = np.meshgrid(np.arange(K // 16), np.arange(NT), np.arange(64), np.arange(8), indexing="ij")
    src = (((ks * NT + nt) * 64 + l) * 8 + j).ravel()
    dst = ((nt * 32 + (l & 31)) * K + ks * 16 + perm[8 * (l >> 5) + j]).ravel()
    assert sorted(dst.tolist()) == list(range(N * K))
    hi, lo = np.empty(N * K, dtype=np.uint16), np.empty(N * K, dtype=np.uint16)
    hi[dst], lo[dst] = fh[src], fl[src]
    return hi, lo


@pytest.mark.parametrize("N,K,seed", [(256, 64, 5), (32, 16, 6)])
def test_packed_up_weights_unpack_to_the_original(N, K, seed):
    # (a) any weights: the halves of the original matrix, element for element
    w = _weights(N, K, seed)
    rc, fh, fl, sh = _call(lib().asw_pack_up_feed_f16, w, N, K)
    wh, wl, wsh = split_np(w)
    assert rc == 0 and sh == wsh
    hi, lo = unpack(fh, fl, N, K)
    assert hi.tobytes() == wh.tobytes() and lo.tobytes() == wl.tobytes()
    # (b) weights that fp16 holds exactly: the matrix itself
    rng = np.random.default_rng(seed)
    wi = rng.integers(-1000, 1001, size=(N, K)).astype(np.float32)
    rc, fh, fl, sh = _call(lib().asw_pack_up_feed_f16, wi, N, K)
    assert rc == 0
    hi, lo = unpack(fh, fl, N, K)
    back = (hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)) * 2.0 ** -sh
    assert np.array_equal(back.reshape(N, K), wi.astype(np.float64))


def test_pack_refuses_a_k_that_is_no_multiple_of_16():
    w = np.zeros((32, 24), dtype=np.float32)
    rc, *_ = _call(lib().asw_pack_up_feed_f16, w, 32, 24)
    assert rc != 0


def _tiles(T, taps, dils, glu):
    d = (ctypes.c_int32 * 3)(*(list(dils) + [1] * (3 - len(dils))))
    return lib().asw_resstack_tiles(T, taps, len(dils), d, int(glu))


def test_row_tiles_of_the_launches_the_decoder_makes():
    # one polyphase layer, dilation 49: ceil(ceil(T / 49) / (256 / PH)) * ceil(49 / PH), PH by the rows per phase
    assert _tiles(24064, 7, [49], 0) == 2 * 49            # 491 rows per phase: PH = 1
    assert _tiles(4737, 7, [49], 0) == 1 * 25             # 96 rows per phase: PH = 2
    assert _tiles(2400, 7, [49], 0) == 1 * 13             # 48 rows per phase: PH = 4
    # contiguous tiles: 256 rows less the later layers' halo on both sides
    assert _tiles(300, 7, [1], 0) == 2
    assert _tiles(500, 7, [1, 7], 0) == -(-500 // (256 - 42))
    assert _tiles(2000, 7, [49], 0) == -(-2000 // 256)   # 40 rows per phase: too few for row sets
    assert _tiles(4737, 7, [49], 1) == -(-4737 // 256)   # GroupNorm + GLU on load: contiguous
    assert _tiles(500, 7, [1, 49], 0) < 0                 # the halo of dilation 49 leaves no tile
