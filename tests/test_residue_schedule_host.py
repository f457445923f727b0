"""The residue-image A feed of the pipelined f16x3 tiles, as the library enumerates it on the host
(asw_residue_schedule, csrc/asw_common.cpp; the device loop of csrc/pipegemm.hip goes through the same formulae,
asw::ResidueFeed): every k-step once, every image row the input row its taps expect, image heights, and the shapes the
feed does not apply to.  Host code only: no GPU."""
import pytest

from acousticswarms_speech_amd import native

BK, BM = 32, 256
CASES = [(33, 16, 2), (7, 4, 4), (7, 4, 8), (7, 4, 16), (5, 4, 4), (5, 2, 4), (7, 2, 2)]      # (taps, stride, Cin / BK)


@pytest.mark.parametrize("taps,stride,cpb", CASES)
@pytest.mark.parametrize("m0", [0, 768])
def test_schedule_covers_every_kstep_once_and_maps_rows(taps, stride, cpb, m0):
    pad = taps // 2
    got = native.residue_schedule(taps, stride, cpb * BK, BK=BK, BM=BM, m0=m0, pad=pad)
    assert got is not None
    stages, max_shift = got
    KS = BK // 16
    assert len(stages) == stride * cpb and max_shift == (taps - 1) // stride
    seen = []
    for s, st in enumerate(stages):
        r, c = st["residue"], st["chunk"]
        assert s == r * cpb + c and 0 <= r < stride and 0 <= c < cpb          # residue-major, channel chunk inner
        assert st["rows"] == BM + (taps - 1 - r) // stride                   # image height
        assert [t for t, _, _ in st["taps"]] == list(range(r, taps, stride))  # all taps of the residue, in order
        for tap, shift, k0 in st["taps"]:
            assert tap % stride == r and 0 <= shift and BM - 1 + shift < st["rows"]
            # the packed weights are untouched: k-step ks of (tap, chunk c) is ((tap * cpb + c) * KS + ks)
            assert k0 == (tap * cpb + c) * KS
            seen += [k0 + ks for ks in range(KS)]
            # image row i is input row first_row + i * stride; frame m0 + i reads image row i + shift for this tap
            for i in (0, 1, BM // 2, BM - 1):
                image_row = i + shift
                assert st["first_row"] + image_row * stride == (m0 + i) * stride - pad + tap
    assert sorted(seen) == list(range(taps * cpb * KS))                      # every (tap, chunk, k-step) exactly once


@pytest.mark.parametrize("taps,stride,dil,cin,skip", [
    (4, 4, 1, 128, False), (1, 1, 1, 256, False), (3, 4, 1, 128, False), (7, 1, 1, 128, False),   # taps <= stride, stride 1
    (7, 4, 2, 128, False), (7, 2, 7, 128, False),                                                  # dilated
    (7, 4, 1, 48, False),                                                                          # Cin % BK != 0
    (7, 4, 1, 128, True)])                                                                         # skip operand
def test_shapes_the_feed_does_not_apply_to(taps, stride, dil, cin, skip):
    assert native.residue_schedule(taps, stride, cin, BK=BK, BM=BM, dil=dil, pad=taps // 2, has_skip=skip) is None


def test_kernel_limit_on_the_row_shift():
    """The kernels' ring has ASW_RESIDUE_MAX_SHIFT = 2 rows beyond BM per image: the shapes of both networks fit,
    (7, 2) -- four taps on one image -- is enumerated but stays on the chunk-per-tap feed."""
    for taps, stride, cpb in CASES:
        _, max_shift = native.residue_schedule(taps, stride, cpb * BK, BK=BK, BM=BM, pad=taps // 2)
        assert (max_shift <= 2) == ((taps, stride) != (7, 2))
