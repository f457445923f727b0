"""GPU: ``scorer.DeviceScorer`` on its own, without any spot network -- each of its nine helpers returns the bytes the
same method returns when it is called on a ``SpotModel``, and the three ways into the segment SI-SDR op agree."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 3, 4096


def _bytes(out):
    """one result (an ndarray, a tensor, or a tuple of them) as a tuple of (dtype, shape, bytes)"""
    items = out if isinstance(out, tuple) else (out,)
    arrays = [t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in items]
    return tuple((str(a.dtype), a.shape, a.tobytes()) for a in arrays)


def _calls(s, waves):
    """the nine helpers on one scorer, by name"""
    seg_tab, cnt = s.voiced_segments(waves)
    cnt_host = cnt.cpu().numpy()
    lists = [[tuple(int(v) for v in ab) for ab in row[:c]] for row, c in zip(seg_tab.cpu().numpy(), cnt_host)]
    full = s.pair_sisdr_device(waves)
    seg_res = s.segment_sisdr_resident(waves, seg_tab, cnt)
    w64 = waves.double()
    en = torch.stack([(w64 * w64).sum(dim=1), (w64 * w64).mean(dim=1).sqrt()], dim=1).contiguous()
    en_host = en.cpu().numpy()
    gate = np.full(N, 0.25 * en_host[:, 0].max())
    dis1 = torch.tensor([1.0, 1.5, 2.0], dtype=torch.float64, device=waves.device)
    out = {
        "voiced_segments": (seg_tab, cnt),
        "pair_sisdr": s.pair_sisdr(waves),
        "pair_sisdr_device": full,
        "segment_sisdr": s.segment_sisdr(waves, lists),
        "segment_sisdr_device": s.segment_sisdr_device(waves, seg_tab, cnt),
        "segment_sisdr_resident": seg_res,
        "fine_clusters": s.fine_clusters(waves, [0, N], en, gate, [0.25 * en_host[:, 0].max()], 0.5),
        "global_clusters": s.global_clusters(full, seg_res, cnt, np.eye(N, dtype=np.uint8)),
        "coarse_select": s.coarse_select(en, dis1, thr1=0.5, cap=4),
    }
    return out, cnt_host


def test_device_scorer_alone_returns_the_bytes_of_the_spot_model():
    from acousticswarms_speech_amd.config import TINY
    from acousticswarms_speech_amd.scorer import DeviceScorer
    from acousticswarms_speech_amd.spot import SpotModel

    rows = torch.randn(N, T, generator=torch.Generator().manual_seed(17))
    rows[1] = 0.0                                            # a silent row: no voiced segment, a NaN-only slice
    waves = rows.cuda()
    scorer = DeviceScorer("cuda")
    assert scorer.device == torch.device("cuda") and not hasattr(scorer, "shift_and_sep")
    got, cnt = _calls(scorer, waves)
    # (no handle is made: the library builds no network as narrow as TINY, and the helpers ask for none -- they run
    # where the tensors they are given live)
    want, _ = _calls(SpotModel(TINY), waves)
    assert set(got) == set(DeviceScorer.HELPERS) and len(DeviceScorer.HELPERS) == 9
    for name in DeviceScorer.HELPERS:
        assert _bytes(got[name]) == _bytes(want[name]), name
    # the silent row has no segment, and its slice of the segment tensor is NaN only
    assert cnt[1] == 0 and cnt[0] >= 1 and cnt[2] >= 1
    seg_host, cnt_host = got["segment_sisdr_device"]
    assert np.all(np.isnan(seg_host[1])) and np.array_equal(cnt_host, cnt)
    # host lists cut from the device table, the table itself, and the resident form: one op
    assert _bytes(got["segment_sisdr"]) == _bytes(got["segment_sisdr_device"])
    kmax = seg_host.shape[2]
    resident = got["segment_sisdr_resident"].cpu().numpy()
    assert kmax == max(1, int(cnt.max())) and np.array_equal(resident[:, :, :kmax], seg_host, equal_nan=True)
    assert np.all(np.isnan(resident[:, :, kmax:]))
    assert got["pair_sisdr_device"].cpu().numpy().tobytes() == got["pair_sisdr"].tobytes()
