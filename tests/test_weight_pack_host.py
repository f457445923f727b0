"""CPU only: the host weight preparation of the f16x3 kernels (``asw_split_weights_f16``, ``asw_pack_fragments_f16``
in csrc/asw_common.cpp) against a numpy statement of it.  Every bound is equality of every output byte."""
import ctypes

import numpy as np
import pytest

from acousticswarms_speech_amd.native import lib
from tests.f16_model import split_np      # the numpy statement of the split (shared with the kernels' CPU model)


def pack_np(w, N, K):
    """dst = ((ks NT + nt) 64 + l) 8  <-  src = (nt 32 + (l & 31)) K + ks 16 + 8 (l >> 5), eight halves each"""
    hi, lo, shift = split_np(w)
    NT = N // 32
    ks, nt, l, j = np.meshgrid(np.arange(K // 16), np.arange(NT), np.arange(64), np.arange(8), indexing="ij")
    dst = (((ks * NT + nt) * 64 + l) * 8 + j).ravel()
    src = ((nt * 32 + (l & 31)) * K + ks * 16 + 8 * (l >> 5) + j).ravel()
    fh, fl = np.empty_like(hi), np.empty_like(lo)
    fh[dst], fl[dst] = hi[src], lo[src]
    return fh, fl, shift


def _call(fn, w, *dims):
    w = np.ascontiguousarray(w, dtype=np.float32)
    hi = np.full(w.size, 0xAAAA, dtype=np.uint16)
    lo = np.full(w.size, 0xAAAA, dtype=np.uint16)
    sh = ctypes.c_int32(99)
    rc = fn(ctypes.c_void_p(w.ctypes.data), *dims, ctypes.c_void_p(hi.ctypes.data), ctypes.c_void_p(lo.ctypes.data),
            ctypes.byref(sh))
    return rc, hi, lo, sh.value


def split_lib(w):
    return _call(lib().asw_split_weights_f16, w, np.asarray(w).size)


def pack_lib(w, N, K):
    return _call(lib().asw_pack_fragments_f16, w, N, K)


def _weights(N, K, seed):
    # seeded, a spread of magnitudes so that lo parts are normal, subnormal and zero
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, K)) * np.exp2(rng.integers(-12, 3, size=(N, K)))).astype(np.float32)


@pytest.mark.parametrize("N,K,seed", [(32, 16, 11), (64, 48, 12)])
def test_split_and_pack_match_the_statement(N, K, seed):
    w = _weights(N, K, seed)
    rc, hi, lo, sh = split_lib(w)
    wh, wl, wsh = split_np(w)
    assert rc == 0 and sh == wsh
    assert hi.tobytes() == wh.tobytes() and lo.tobytes() == wl.tobytes()
    rc, fh, fl, fsh = pack_lib(w, N, K)
    ph, pl, psh = pack_np(w, N, K)
    assert rc == 0 and fsh == psh == wsh
    assert fh.tobytes() == ph.tobytes() and fl.tobytes() == pl.tobytes()
    assert sorted(fh.tolist()) == sorted(hi.tolist())          # a permutation of the split, nothing else


def test_all_zero_weights_shift_zero():
    w = np.zeros((32, 16), dtype=np.float32)
    rc, hi, lo, sh = split_lib(w)
    assert rc == 0 and sh == 0 and not hi.any() and not lo.any()
    rc, fh, fl, sh = pack_lib(w, 32, 16)
    assert rc == 0 and sh == 0 and not fh.any() and not fl.any()


def test_huge_weights_clamp_the_shift_and_saturate():
    w = _weights(32, 16, 13)
    w[3, 5], w[4, 6] = 1e30, -1e30
    rc, hi, lo, sh = split_lib(w)
    wh, wl, wsh = split_np(w)
    assert rc == 0 and sh == wsh == -24
    assert hi.tobytes() == wh.tobytes() and lo.tobytes() == wl.tobytes()
    big = np.float16(65504.0).view(np.uint16)
    assert hi.reshape(32, 16)[3, 5] == big and hi.reshape(32, 16)[4, 6] == big | 0x8000      # saturated, not inf
    assert lo.reshape(32, 16)[3, 5] == 0 and lo.reshape(32, 16)[4, 6] in (0, 0x8000)


def test_tiny_weights_clamp_the_shift():
    w = _weights(32, 16, 14)
    w = (w / np.max(np.abs(w)) * np.float32(5e-31)).astype(np.float32)
    w[0, 0] = 1e-30
    assert np.max(np.abs(w)) == np.float32(1e-30)
    rc, hi, lo, sh = split_lib(w)
    wh, wl, wsh = split_np(w)
    assert rc == 0 and sh == wsh == 24
    assert hi.tobytes() == wh.tobytes() and lo.tobytes() == wl.tobytes()


def test_nan_weight_is_refused():
    w = _weights(32, 16, 15)
    w[7, 3] = np.nan
    for rc in (split_lib(w)[0], pack_lib(w, 32, 16)[0]):
        assert rc == -1
        assert b"non-finite" in lib().asw_last_error()


@pytest.mark.parametrize("N,K", [(48, 16), (32, 8)])
def test_packer_refuses_shapes_that_are_no_whole_fragments(N, K):
    rc = pack_lib(_weights(N, K, 16), N, K)[0]
    assert rc == -1 and b"pack_fragments" in lib().asw_last_error()
